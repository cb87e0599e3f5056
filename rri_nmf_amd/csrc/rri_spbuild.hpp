// rri_spbuild.hpp -- the blocked store of a CSR handle built from arrays that are on the device already (rri_upload_X_corpus;
// DESIGN 4.13).  The specification of the store is build_sp_copy (rri_layout.hpp), the host's stable counting sort: this builder
// leaves the same bytes -- segptr, idx, perm, the work items -- for the same canonical matrix, whatever the scheduling.
//
// Input: the canonical arrays of an rri_corpus -- int64 indptr, int32 indices strictly ascending in every row, float64 values.
// Per copy (which = 0: rows as segments, cut into column blocks of bw; 1: columns as segments, cut into row blocks of bw):
//   1 COUNT   cnt[b][s + 1] = stored entries of segment s inside block b; cnt[b][0] = 0.
//             Copy 0: the entries of one (row, block) are contiguous in the canonical row, so the count is the distance of two
//             bisections of the row -- no atomic.  Copy 1: an integer histogram; its result does not depend on arrival order.
//   2 SCAN    segptr = the inclusive prefix sum, over the flat [nblk][nseg + 1] array, of the counts rounded up to a multiple of
//             4 (k_sp_blk moves quads).  Because cnt[b][0] = 0, segptr[b][0] is the end of block b - 1, as the host leaves it.
//   3 CLAIM   every stored entry takes a slot of its segment.  Copy 0: slot = segptr[b][r] + (p - first position of the row
//             inside block b), again by bisection: the slot IS the stable order.  Copy 1: slots are handed out by an integer
//             counter per segment, in arrival order, and the entry leaves the key (p << 32 | offset inside the block) there;
//   4 SORT    ... so every segment of copy 1 is then sorted by that key.  p, the position in the canonical CSR, is unique and is
//             the high half, so the sorted segment is the one the stable counting sort leaves; the low half carries idx along.
//             A segment holds at most bw <= spx_block_cap() = 15296 entries: its keys fit the LDS of one workgroup.  The key
//             is corpus_key (rri_corpus.hpp) with the position in the column's place, the pad is CORPUS_KEY_PAD, which sorts
//             behind every entry: the padding of a segment falls out of the same sort.
// Pads: idx = bw (the zero slot of the factor tables), perm = -1; both arrays have max(count, 4) entries.
// The work items are cut on the host from the downloaded segptr by sp_cut_work, the cutter of the host route.
//
// spbuild_copy_plain restates the four steps as a host loop that claims in ANY order (tests/c/spbuild_main.cpp shuffles it);
// spbuild_check_corpus is the argument check of rri_upload_X_corpus.  Host-only, nothing here needs HIP.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rri_corpus.hpp"
#include "rri_layout.hpp"

namespace rri {

// the key an entry leaves in its claimed slot: position in the canonical CSR (below 2^31) above the offset inside the block
RRI_TOPN_FN unsigned long long spbuild_key(int64_t pos, int64_t off) { return corpus_key(pos, off); }
RRI_TOPN_FN int spbuild_key_pos(unsigned long long key) { return (int)corpus_key_col(key); }
RRI_TOPN_FN unsigned short spbuild_key_off(unsigned long long key) { return (unsigned short)corpus_key_pos(key); }

// how a segment of `len` padded entries is sorted: one wave in registers, or a workgroup in LDS on corpus_pad(len) keys
RRI_TOPN_FN bool spbuild_wave_sorted(int64_t len) { return len <= CORPUS_WAVE_MAX; }

// The argument check of rri_upload_X_corpus, after the handle's own refusals: TOPN_REQ_OK, TOPN_REQ_INVALID or
// TOPN_REQ_UNSUPPORTED and the text.  alive: the corpus is one that rri_corpus_create made and rri_corpus_destroy has not seen.
inline int spbuild_check_corpus(bool alive, int64_t c_rows, int64_t c_cols, int64_t c_nnz, int c_device, int64_t n, int64_t d,
                                int device, char* msg, size_t msg_len) {
    if (!alive) {
        snprintf(msg, msg_len, "the corpus is NULL or has been destroyed");
        return TOPN_REQ_INVALID;
    }
    if (c_device != device) {
        snprintf(msg, msg_len, "the corpus lives on device %d, the handle on device %d", c_device, device);
        return TOPN_REQ_INVALID;
    }
    if (c_rows != n || c_cols != d) {
        snprintf(msg, msg_len, "the corpus is %lld x %lld, the handle %lld x %lld", (long long)c_rows, (long long)c_cols, (long long)n,
                 (long long)d);
        return TOPN_REQ_INVALID;
    }
    if (c_nnz >= 2147483647LL) {
        snprintf(msg, msg_len, "more than 2^31-1 stored entries");
        return TOPN_REQ_UNSUPPORTED;
    }
    return TOPN_REQ_OK;
}

// One blocked copy by count, padded scan, claim and sort.  claim_order: the stored positions 0 .. nnz - 1 in the order in which
// they arrive at the claim (any permutation; NULL: ascending).  Leaves segptr, idx, perm and count of SpCopyHost; the work items
// and lps are sp_cut_work's and sp_lanes_per_segment's, as on both routes.
inline SpCopyHost spbuild_copy_plain(const int64_t* indptr, const int32_t* indices, i64 n, i64 nnz, int which, const SpDims& cp,
                                     int target_items, const int64_t* claim_order) {
    SpCopyHost out;
    const i64 nseg = cp.nseg, stride = nseg + 1;
    std::vector<i64> row_of((size_t)nnz);
    for (i64 r = 0; r < n; ++r) {
        out.longest_row = std::max<i64>(out.longest_row, (i64)(indptr[r + 1] - indptr[r]));
        for (i64 p = indptr[r]; p < indptr[r + 1]; ++p) row_of[(size_t)p] = r;
    }
    auto place = [&](i64 p, i64& b, i64& sgm, i64& off) {
        const i64 r = row_of[(size_t)p], j = indices[p];
        const i64 g = which == 0 ? j : r;
        sgm = which == 0 ? r : j;
        b = g / cp.bw;
        off = g - b * cp.bw;
    };
    // 1 count
    std::vector<i64>& sp = out.segptr;
    sp.assign((size_t)cp.nblk * stride, 0);
    for (i64 p = 0; p < nnz; ++p) {
        i64 b, sgm, off;
        place(p, b, sgm, off);
        sp[(size_t)(b * stride + sgm + 1)] += 1;
    }
    // 2 padded inclusive scan over the flat array
    i64 run = 0;
    for (size_t i = 0; i < sp.size(); ++i) {
        run += (sp[i] + 3) / 4 * 4;
        sp[i] = run;
    }
    out.count = run;
    const size_t cntp = (size_t)std::max<i64>(run, 4);
    // 3 claim, in arrival order
    std::vector<unsigned long long> keys(cntp, CORPUS_KEY_PAD);
    std::vector<i64> fill((size_t)cp.nblk * nseg, 0);
    for (i64 a = 0; a < nnz; ++a) {
        const i64 p = claim_order ? claim_order[a] : a;
        i64 b, sgm, off;
        place(p, b, sgm, off);
        const i64 q = sp[(size_t)(b * stride + sgm)] + fill[(size_t)(b * nseg + sgm)]++;
        keys[(size_t)q] = spbuild_key(p, off);
    }
    // 4 sort every padded segment by key; the pads stay behind
    out.idx.assign(cntp, (unsigned short)cp.bw);
    out.perm.assign(cntp, -1);
    for (int b = 0; b < cp.nblk; ++b)
        for (i64 s = 0; s < nseg; ++s) {
            const i64 lo = sp[(size_t)(b * stride + s)], hi = sp[(size_t)(b * stride + s + 1)];
            std::sort(keys.begin() + (std::ptrdiff_t)lo, keys.begin() + (std::ptrdiff_t)hi);
            for (i64 q = lo; q < hi; ++q)
                if (keys[(size_t)q] != CORPUS_KEY_PAD) {
                    out.idx[(size_t)q] = spbuild_key_off(keys[(size_t)q]);
                    out.perm[(size_t)q] = spbuild_key_pos(keys[(size_t)q]);
                }
        }
    sp_cut_work(sp.data(), cp, which, target_items, out.work);
    out.lps = sp_lanes_per_segment(nnz, cp);
    return out;
}

}  // namespace rri
