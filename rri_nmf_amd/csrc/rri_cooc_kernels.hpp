// rri_cooc_kernels.hpp -- k_cooc_masks and k_cooc_count: document and co-document frequencies of groups of words over a CSR
// pattern, in two launches per row chunk (DESIGN "Co-document counts"; the request, the membership table, the packing of its
// entries, the pair test and the row chunks are rri_cooc.hpp's).
//
// k_cooc_masks, the pass over the corpus.  A 256-thread workgroup takes a tile of COOC_TILE_ROWS = 32 rows and keeps a word per
// (group, row of the tile) in LDS, [group][row].  LPS lanes share a row (8: the 32 rows at once; 64: a wave takes 8 rows one
// after the other -- cooc_lps, the rule of spx_scale_lps), stride over its column indices, look each column up in the
// membership table and OR bit `slot` into the row's word of `group`: an integer LDS OR, so the word does not depend on which
// lane came first.  Most columns are in no group and cost the two reads of ptr.  After a barrier the words leave group-major,
// masks[group * rows_pad + row of the chunk]: 32 consecutive words per group and tile, and every word of the array is written
// (rows beyond the chunk's last: 0), so nothing needs to be cleared first.
//
// k_cooc_count<PPT>.  Grid (pieces of COOC_COUNT_ROWS mask words, group); a wave takes a quarter of the piece, 64 consecutive
// words per step.  Lane l owns the pairs of slots a <= b with triangular index l + 64 i, i < PPT (cooc_count_ppt: 1, 2, 4 or 9 for
// the group_size (group_size + 1) / 2 <= 528 pairs; the other half of codf is the mirror image).  Most words are 0 -- a document
// rarely holds one of a topic's ten words -- and are never looked at: a ballot finds the non-zero ones, each is broadcast by a
// lane read (v_readlane: no LDS, no barrier anywhere in the kernel) and every lane asks cooc_pair of its pairs.  A lane's int32
// counts (at most COOC_COUNT_ROWS / 4) leave by one 64-bit integer atomic add per pair with a non-zero count, two off the
// diagonal: integer sums are exact, so the totals do not depend on the order of arrival, and two calls give the same bits.
// No floating point anywhere.
#pragma once

#include "rri_cooc.hpp"

namespace rri {

template <int LPS>
__global__ __launch_bounds__(256) void k_cooc_masks(const i64* __restrict__ indptr, const int* __restrict__ indices,
                                                    const int* __restrict__ mptr, const int* __restrict__ ment, i64 r0, i64 r1,
                                                    int n_groups, i64 rows_pad, unsigned* __restrict__ masks) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned* word = reinterpret_cast<unsigned*>(smem);                    // [n_groups][COOC_TILE_ROWS]
    const int tid = threadIdx.x;
    const int nw = n_groups * COOC_TILE_ROWS;
    for (int w = tid; w < nw; w += 256) word[w] = 0u;
    __syncthreads();
    constexpr int SUBS = 256 / LPS;                                        // rows in flight
    const int sub = tid / LPS, sl = tid % LPS;
    const i64 t0 = (i64)blockIdx.x * COOC_TILE_ROWS;                       // the tile's first row inside the chunk
    for (int rl = sub; rl < COOC_TILE_ROWS; rl += SUBS) {
        const i64 row = r0 + t0 + rl;
        if (row >= r1) break;
        const i64 p1 = indptr[row + 1];
        for (i64 p = indptr[row] + sl; p < p1; p += LPS) {
            const int j = indices[p];
            const int q1 = mptr[j + 1];
            for (int q = mptr[j]; q < q1; ++q) {
                const int e = ment[q];
                atomicOr(&word[cooc_group(e) * COOC_TILE_ROWS + rl], 1u << cooc_slot(e));
            }
        }
    }
    __syncthreads();
    for (int w = tid; w < nw; w += 256) {
        const int g = w / COOC_TILE_ROWS, rl = w % COOC_TILE_ROWS;
        masks[(i64)g * rows_pad + t0 + rl] = word[w];
    }
}

template <int PPT>
__global__ __launch_bounds__(256) void k_cooc_count(const unsigned* __restrict__ masks, i64 rows_pad, int group_size,
                                                    unsigned long long* __restrict__ codf) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = blockIdx.y;
    const unsigned* mrow = masks + (i64)g * rows_pad;
    const int npairs = group_size * (group_size + 1) / 2;
    int pa[PPT], pb[PPT], cnt[PPT];
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        int p = lane + 64 * i, a = 0;
        if (p < npairs) {
            while (p >= group_size - a) { p -= group_size - a; ++a; }         // row a of the triangle holds the pairs (a, a .. group_size - 1)
        } else {
            p = 0;
        }
        pa[i] = a;
        pb[i] = a + p;
        cnt[i] = 0;
    }
    constexpr int WAVE_ROWS = COOC_COUNT_ROWS / 4;
    const i64 w0 = (i64)blockIdx.x * COOC_COUNT_ROWS + (i64)wave * WAVE_ROWS;
    const i64 w1 = w0 + WAVE_ROWS < rows_pad ? w0 + WAVE_ROWS : rows_pad;
#pragma unroll 4
    for (i64 base = w0; base < w1; base += 64) {
        const unsigned m = base + lane < w1 ? mrow[base + lane] : 0u;
        unsigned long long nz = __ballot(m != 0u);
        while (nz) {                                                          // uniform: the wave's non-zero words, in row order
            const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)nz) - 1);
            nz &= nz - 1ull;
            const unsigned mm = (unsigned)__builtin_amdgcn_readlane((int)m, src);
#pragma unroll
            for (int i = 0; i < PPT; ++i) cnt[i] += (int)cooc_pair(mm, pa[i], pb[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < PPT; ++i)
        if (lane + 64 * i < npairs && cnt[i] > 0) {
            atomicAdd(&codf[((i64)g * group_size + pa[i]) * group_size + pb[i]], (unsigned long long)cnt[i]);
            if (pa[i] != pb[i]) atomicAdd(&codf[((i64)g * group_size + pb[i]) * group_size + pa[i]], (unsigned long long)cnt[i]);
        }
}

}  // namespace rri
