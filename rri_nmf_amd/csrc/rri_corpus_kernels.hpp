// rri_corpus_kernels.hpp -- the ingest of a raw CSR matrix into a resident canonical one (DESIGN "A corpus on the device"; the
// semantics, the key, the classes and the pad are rri_corpus.hpp's).
//
// k_corpus_check, the one pass over the raw arrays.  It reads indptr, indices and values BY POSITION ONLY -- 0 .. n_rows and
// 0 .. nnz - 1, grid-stride -- so nothing a caller wrote is an address or a loop bound in it.  The smallest offending position
// of each of rules 0 .. 4 leaves by a 64-bit integer minimum (err[rule], ~0 where the rule holds): the verdict does not depend on
// which workgroup came first.  The same pass leaves two bits per entry, a ballot word per 64 entries: ZERO (the value is 0) and
// DESC (the column does not exceed the one stored in front of it, whatever row that one belongs to).  Nothing else runs before
// the host has read err.
// k_corpus_rows (the check has passed: indptr is monotone inside [0, nnz]) turns the marks into a flag per row -- a ZERO bit in
// [lo, hi) or a DESC bit in [lo + 1, hi) -- and writes indptr as int64 and the stored length of every row.  A matrix without a
// flagged row is ingested by k_corpus_copy, the converting copy, and nothing else.
// Otherwise the copy fills a staging pair (int32, float64) at the raw offsets, and every flagged row is sorted by
// (column, position) and merged into the staging at its own raw offset, shorter or as long as it was:
//   k_corpus_sort_wave   rows of up to 64 entries, four per workgroup: a key per lane, a bitonic network of 21 lane exchanges,
//                        the run of a column summed by its first lane in stored order, places by a ballot;
//   k_corpus_sort_block  one workgroup per row, the keys in LDS (launched per padded length, so a short row does not pay for
//                        the LDS of a long one) or, for the rare row beyond CORPUS_LDS_MAX, in a global buffer: the same
//                        in-place network with a barrier per stage, then every thread takes a contiguous share of the sorted
//                        row, sums the runs that begin in it sequentially in stored order, and a scan of the threads' counts
//                        gives the places.
// The rows' canonical lengths go to the host, which takes the prefix sum, and k_corpus_compact writes the final arrays once: a
// thread per canonical entry finds its row by bisection of the canonical indptr.  The counters (duplicates, zeros, negatives)
// are integer atomics.  No floating-point sum crosses a thread, so two ingests of one matrix give the same bytes.
#pragma once

#include "rri_corpus.hpp"

namespace rri {

typedef unsigned long long u64;

enum { CORPUS_STAT_DUP = 8, CORPUS_STAT_ZERO = 9, CORPUS_STAT_NEG = 10, CORPUS_STAT_WORDS = 16 };    // words of the ingest's counters; 0 .. 4: err

__device__ inline u64 corpus_shfl_xor(u64 v, int m) {
    const int lo = __shfl_xor((int)(unsigned)(v & 0xffffffffull), m), hi = __shfl_xor((int)(unsigned)(v >> 32), m);
    return ((u64)(unsigned)hi << 32) | (u64)(unsigned)lo;
}
__device__ inline double corpus_shfl(double v, int src) {
    const long long b = __double_as_longlong(v);
    const int lo = __shfl((int)(unsigned)((u64)b & 0xffffffffull), src), hi = __shfl((int)(unsigned)((u64)b >> 32), src);
    return __longlong_as_double((long long)(((u64)(unsigned)hi << 32) | (u64)(unsigned)lo));
}

// the two sorting networks, shared with the builder of the blocked store (rri_spbuild_kernels.hpp), whose key has the same shape.
// A wave's 64 keys, one per lane, ascending by lane: a bitonic network of 21 lane exchanges
__device__ inline u64 corpus_sort_wave_key(u64 key, int lane) {
    for (int k = 2; k <= 64; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            const u64 other = corpus_shfl_xor(key, j);
            const bool take_min = ((lane & k) == 0) == ((lane & j) == 0);
            key = take_min ? (key < other ? key : other) : (key < other ? other : key);
        }
    return key;
}
// P keys (a power of two; LDS or global), ascending, by the nt threads of one workgroup: the same network in place, a barrier per
// stage.  The keys are written and a barrier has passed before the call; a barrier has passed when it returns
__device__ inline void corpus_sort_keys(u64* keys, i64 P, int tid, int nt) {
    for (i64 k = 2; k <= P; k <<= 1)
        for (i64 j = k >> 1; j > 0; j >>= 1) {
            for (i64 t = tid; t < (P >> 1); t += nt) {
                const i64 i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), m = i | j;        // a pair that differs in bit j
                const u64 a = keys[i], b = keys[m];
                if ((a > b) == ((i & k) == 0)) {
                    keys[i] = b;
                    keys[m] = a;
                }
            }
            __syncthreads();
        }
}

__global__ __launch_bounds__(256) void k_corpus_check(const void* __restrict__ indptr, int pdt, const void* __restrict__ indices,
                                                      int idt, const void* __restrict__ values, int vdt, i64 n_rows, i64 n_cols,
                                                      i64 nnz, u64* __restrict__ err, u64* __restrict__ zero_bits,
                                                      u64* __restrict__ desc_bits) {
    const i64 gid = (i64)blockIdx.x * 256 + threadIdx.x, stride = (i64)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    for (i64 r = gid; r <= n_rows; r += stride) {
        const i64 a = corpus_idx(indptr, pdt, r);
        if (r == 0 && a != 0) atomicMin(&err[0], (u64)0);
        if (r > 0 && a < corpus_idx(indptr, pdt, r - 1)) atomicMin(&err[1], (u64)r);
        if (r == n_rows && a != nnz) atomicMin(&err[2], (u64)r);
    }
    for (i64 base = gid - lane; base < nnz; base += stride) {       // uniform per wave: 64 consecutive entries, one ballot word
        const i64 p = base + lane;
        const bool in = p < nnz;
        const i64 col = in ? corpus_idx(indices, idt, p) : 0;
        const i64 prev = in && p > 0 ? corpus_idx(indices, idt, p - 1) : -1;
        const double v = in ? corpus_val(values, vdt, p) : 1.0;
        if (in && (col < 0 || col >= n_cols)) atomicMin(&err[3], (u64)p);
        if (in && !corpus_finite(v)) atomicMin(&err[4], (u64)p);
        const u64 zb = __ballot(in && v == 0.0), db = __ballot(in && col <= prev);
        if (lane == 0) {
            zero_bits[base >> 6] = zb;
            desc_bits[base >> 6] = db;
        }
    }
}

// is a bit of [a, b) set?
__device__ inline bool corpus_bits_any(const u64* __restrict__ w, i64 a, i64 b) {
    if (a >= b) return false;
    const i64 w0 = a >> 6, w1 = (b - 1) >> 6;
    for (i64 i = w0; i <= w1; ++i) {
        u64 m = w[i];
        if (i == w0) m &= ~0ull << (a & 63);
        if (i == w1 && ((b & 63) != 0)) m &= ~0ull >> (64 - (b & 63));
        if (m) return true;
    }
    return false;
}

__global__ __launch_bounds__(256) void k_corpus_rows(const void* __restrict__ indptr, int pdt, i64 n_rows,
                                                     const u64* __restrict__ zero_bits, const u64* __restrict__ desc_bits,
                                                     i64* __restrict__ ptr64, unsigned char* __restrict__ flag, i64* __restrict__ clen) {
    const i64 stride = (i64)gridDim.x * 256;
    for (i64 r = (i64)blockIdx.x * 256 + threadIdx.x; r <= n_rows; r += stride) {
        const i64 lo = corpus_idx(indptr, pdt, r);
        ptr64[r] = lo;
        if (r == n_rows) break;
        const i64 hi = corpus_idx(indptr, pdt, r + 1);
        flag[r] = (unsigned char)(corpus_bits_any(zero_bits, lo, hi) || corpus_bits_any(desc_bits, lo + 1, hi));
        clen[r] = hi - lo;
    }
}

// a wave's count, added to a counter by one lane
__device__ inline void corpus_count(u64* counter, bool mine) {
    const u64 b = __ballot(mine);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(counter, (u64)__popcll(b));
}

__global__ __launch_bounds__(256) void k_corpus_copy(const void* __restrict__ indices, int idt, const void* __restrict__ values, int vdt,
                                                     i64 nnz, int* __restrict__ out_idx, double* __restrict__ out_val,
                                                     u64* __restrict__ negatives) {
    const i64 gid = (i64)blockIdx.x * 256 + threadIdx.x, stride = (i64)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    for (i64 base = gid - lane; base < nnz; base += stride) {
        const i64 p = base + lane;
        double v = 0.0;
        if (p < nnz) {
            v = corpus_val(values, vdt, p);
            out_idx[p] = (int)corpus_idx(indices, idt, p);
            out_val[p] = v;
        }
        if (negatives) corpus_count(negatives, v < 0.0);
    }
}

__global__ __launch_bounds__(256) void k_corpus_sort_wave(const i64* __restrict__ rows, i64 n_list, const i64* __restrict__ ptr64,
                                                          const void* __restrict__ indices, int idt, const void* __restrict__ values,
                                                          int vdt, int* __restrict__ out_idx, double* __restrict__ out_val,
                                                          i64* __restrict__ clen, u64* __restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const i64 item = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= n_list) return;                                      // a whole wave
    const i64 r = rows[item], lo = ptr64[r];
    const int len = (int)(ptr64[r + 1] - lo);                        // 1 .. CORPUS_WAVE_MAX
    u64 key = lane < len ? corpus_key(corpus_idx(indices, idt, lo + lane), lane) : CORPUS_KEY_PAD;
    key = corpus_sort_wave_key(key, lane);
    const bool valid = lane < len;                                   // the real keys stand below the pad
    const int col = (int)corpus_key_col(key);
    const double v = valid ? corpus_val(values, vdt, lo + corpus_key_pos(key)) : 0.0;
    const int before = __shfl(col, lane > 0 ? lane - 1 : 0);
    const bool head = valid && (lane == 0 || col != before);
    double sum = v;
    for (int s = 1; s < 64; ++s) {                                   // uniform: the entries s places behind, while any run goes on
        const int src = lane + s < 64 ? lane + s : 63;
        const int c2 = __shfl(col, src);
        const double v2 = corpus_shfl(v, src);
        const bool in_run = head && lane + s < len && c2 == col;
        if (!__ballot(in_run)) break;
        if (in_run) sum += v2;
    }
    const bool keep = head && sum != 0.0;
    const u64 hm = __ballot(head), km = __ballot(keep);
    if (keep) {
        const i64 o = lo + __popcll(km & ((1ull << lane) - 1ull));
        out_idx[o] = col;
        out_val[o] = sum;
    }
    if (lane == 0) {
        const int heads = __popcll(hm), kept = __popcll(km);
        clen[r] = kept;
        if (len > heads) atomicAdd(&stats[CORPUS_STAT_DUP], (u64)(len - heads));
        if (heads > kept) atomicAdd(&stats[CORPUS_STAT_ZERO], (u64)(heads - kept));
    }
}

// One workgroup per listed row.  IN_LDS: the P keys live in dynamic LDS (P is the launch's padded length); otherwise in
// keybuf + keyoff[item], corpus_pad(len) of them.
template <bool IN_LDS>
__global__ __launch_bounds__(1024) void k_corpus_sort_block(const i64* __restrict__ rows, const i64* __restrict__ keyoff,
                                                            u64* __restrict__ keybuf, i64 P_lds, const i64* __restrict__ ptr64,
                                                            const void* __restrict__ indices, int idt, const void* __restrict__ values,
                                                            int vdt, int* __restrict__ out_idx, double* __restrict__ out_val,
                                                            i64* __restrict__ clen, u64* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int cnt[1024];
    __shared__ int tot[2];
    const int tid = threadIdx.x, nt = blockDim.x;
    const i64 item = blockIdx.x;
    const i64 r = rows[item], lo = ptr64[r], len = ptr64[r + 1] - lo;
    const i64 P = IN_LDS ? P_lds : corpus_pad(len);
    u64* keys = IN_LDS ? reinterpret_cast<u64*>(smem) : keybuf + keyoff[item];
    if (tid < 2) tot[tid] = 0;
    for (i64 i = tid; i < P; i += nt) keys[i] = i < len ? corpus_key(corpus_idx(indices, idt, lo + i), i) : CORPUS_KEY_PAD;
    __syncthreads();
    corpus_sort_keys(keys, P, tid, nt);
    // every thread takes a contiguous share of the sorted row and the runs that begin in it
    const i64 share = (len + nt - 1) / nt;
    const i64 a0 = (i64)tid * share < len ? (i64)tid * share : len, a1 = a0 + share < len ? a0 + share : len;
    int heads = 0, kept = 0;
    for (int pass = 0; pass < 2; ++pass) {
        i64 o = 0;
        if (pass == 1) {
            cnt[tid] = kept;
            __syncthreads();
            for (int off = 1; off < nt; off <<= 1) {
                const int t = tid >= off ? cnt[tid - off] : 0;
                __syncthreads();
                cnt[tid] += t;
                __syncthreads();
            }
            o = lo + cnt[tid] - kept;
        }
        for (i64 i = a0; i < a1; ++i) {
            const unsigned col = corpus_key_col(keys[i]);
            if (i > 0 && corpus_key_col(keys[i - 1]) == col) continue;
            double s = corpus_val(values, vdt, lo + corpus_key_pos(keys[i]));
            for (i64 e = i + 1; e < len && corpus_key_col(keys[e]) == col; ++e) s += corpus_val(values, vdt, lo + corpus_key_pos(keys[e]));
            if (pass == 0) {
                heads += 1;
                kept += s != 0.0;
            } else if (s != 0.0) {
                out_idx[o] = (int)col;
                out_val[o] = s;
                ++o;
            }
        }
    }
    if (heads) atomicAdd(&tot[0], heads);
    if (kept) atomicAdd(&tot[1], kept);
    __syncthreads();
    if (tid == 0) {
        clen[r] = tot[1];
        if (len > tot[0]) atomicAdd(&stats[CORPUS_STAT_DUP], (u64)(len - tot[0]));
        if (tot[0] > tot[1]) atomicAdd(&stats[CORPUS_STAT_ZERO], (u64)(tot[0] - tot[1]));
    }
}

// canonical entry q belongs to the last row r with cptr[r] <= q; it stands in the staging at ptr64[r] + (q - cptr[r])
__global__ __launch_bounds__(256) void k_corpus_compact(const i64* __restrict__ cptr, const i64* __restrict__ ptr64, i64 n_rows, i64 nnz,
                                                        const int* __restrict__ st_idx, const double* __restrict__ st_val,
                                                        int* __restrict__ out_idx, double* __restrict__ out_val, u64* __restrict__ negatives) {
    const i64 gid = (i64)blockIdx.x * 256 + threadIdx.x, stride = (i64)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    for (i64 base = gid - lane; base < nnz; base += stride) {
        const i64 q = base + lane;
        double v = 0.0;
        if (q < nnz) {
            i64 a = 0, b = n_rows;                   // cptr[a] <= q < cptr[b]
            while (b - a > 1) {
                const i64 m = a + ((b - a) >> 1);
                if (cptr[m] <= q) a = m;
                else b = m;
            }
            const i64 src = ptr64[a] + (q - cptr[a]);
            v = st_val[src];
            out_idx[q] = st_idx[src];
            out_val[q] = v;
        }
        corpus_count(negatives, v < 0.0);
    }
}

}  // namespace rri
