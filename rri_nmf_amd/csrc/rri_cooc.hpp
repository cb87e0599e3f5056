// rri_cooc.hpp -- document and co-document frequencies of groups of words, written once (DESIGN "Co-document counts").
//
// The CORPUS is a CSR pattern: indptr (n_rows + 1 entries, from 0, monotone) and indices (strictly ascending inside every row,
// inside [0, n_cols)).  A stored entry means "the word occurs in the document"; there are no values.  The GROUPS are `words`,
// n_groups x group_size, row-major: each entry a column in [0, n_cols) or -1 for an empty slot, empty slots anywhere, a column at
// most once inside one group and in any number of groups; 1 <= group_size <= RRI_MAX_COOC_WORDS (one bit per slot of a 32-bit
// word), 1 <= n_groups <= RRI_MAX_K.  The answer:
//   df[g, a]       the number of rows that contain words[g, a];
//   codf[g, a, b]  the number of rows that contain both words[g, a] and words[g, b]: symmetric, codf[g, a, a] = df[g, a];
// a -1 slot has 0 in its row and its column.  Integers throughout, so the answer does not depend on how the work is split.
//
// How it is counted, here and on the device: a row's MASK for group g is the 32-bit word whose bit a says that the row contains
// words[g, a]; the column -> (group, slot) MEMBERSHIP table turns a row's column indices into its masks, and codf[g, a, b] is the
// number of rows whose mask for g has bits a and b.  The kernels (rri_cooc_kernels.hpp), the entry point
// (rri_cooccurrence_counts) and the stand-alone CPU test (tests/c/cooc_main.cpp) take the request check, the membership table,
// the packing of its entries, the pair test and the row chunks from here.  Plain inline functions; nothing in this file needs HIP.
#pragma once

#include <cstdint>
#include <cstdio>
#include <vector>

#include "rri_layout.hpp"
#include "rri_topn.hpp"

namespace rri {

constexpr int COOC_TILE_ROWS = 32;        // rows whose masks a workgroup of k_cooc_masks forms at a time; row chunks are whole tiles
constexpr int COOC_COUNT_ROWS = 4096;     // mask words of one group that a workgroup of k_cooc_count counts: 1024 per wave
// The mask array of a row chunk is rows x n_groups x 4 bytes (20 MB at 100000 x 50, 4 GB at 1 M x 1024): at most this much of it
// exists at a time.  A quarter of the Infinity Cache, so that the counting launch finds on the die what the mask launch wrote.
constexpr i64 COOC_MASK_BUDGET = 64ll << 20;

// an entry of the membership table: group and slot in one word (group < RRI_MAX_K <= 2^26, slot < 32)
RRI_TOPN_FN int32_t cooc_pack(int group, int slot) { return (int32_t)((group << 5) | slot); }
RRI_TOPN_FN int cooc_group(int32_t e) { return (int)(e >> 5); }
RRI_TOPN_FN int cooc_slot(int32_t e) { return (int)(e & 31); }
// does a row with mask m count for the pair of slots (a, b)?
RRI_TOPN_FN unsigned cooc_pair(unsigned m, int a, int b) { return (m >> a) & (m >> b) & 1u; }

// the words of a request whose sizes are in range: every one a column or -1, none twice in its group
inline int cooc_check_words(int64_t n_cols, const int32_t* words, int32_t n_groups, int32_t group_size, char* msg, size_t msg_len) {
    auto say = [&](int code, const char* what, long long a, long long b) {
        if (msg && msg_len) snprintf(msg, msg_len, what, a, b);
        return code;
    };
    for (int g = 0; g < n_groups; ++g) {
        const int32_t* w = words + (size_t)g * group_size;
        for (int a = 0; a < group_size; ++a) {
            if (w[a] == -1) continue;
            if (w[a] < 0 || w[a] >= n_cols) return say(TOPN_REQ_INVALID, "word %lld of group %lld is out of range", (long long)w[a], (long long)g);
            for (int b = 0; b < a; ++b)
                if (w[b] == w[a]) return say(TOPN_REQ_INVALID, "word %lld stands twice in group %lld", (long long)w[a], (long long)g);
        }
    }
    return TOPN_REQ_OK;
}

// ---- a request, checked on the host before anything is copied -------------------------------------------------------------------
// Returns TOPN_REQ_OK, TOPN_REQ_INVALID or TOPN_REQ_UNSUPPORTED (a group_size or n_groups outside its limits: a shape this
// library does not count) and writes the first broken rule to msg.
inline int cooc_check_request(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_cols, const int32_t* words,
                              int32_t n_groups, int32_t group_size, char* msg, size_t msg_len) {
    auto say = [&](int code, const char* what, long long a, long long b) {
        if (msg && msg_len) snprintf(msg, msg_len, what, a, b);
        return code;
    };
    if (n_rows < 0) return say(TOPN_REQ_INVALID, "n_rows %lld is negative", (long long)n_rows, 0);
    if (n_cols < 0 || n_cols > 0x7fffffffLL) return say(TOPN_REQ_INVALID, "n_cols %lld outside 0 .. 2^31 - 1", (long long)n_cols, 0);
    if (n_groups < 0) return say(TOPN_REQ_INVALID, "n_groups %lld is negative", (long long)n_groups, 0);
    if (group_size < 0) return say(TOPN_REQ_INVALID, "group_size %lld is negative", (long long)group_size, 0);
    if (group_size < 1 || group_size > RRI_MAX_COOC_WORDS)
        return say(TOPN_REQ_UNSUPPORTED, "group_size %lld outside 1 .. %lld", (long long)group_size, (long long)RRI_MAX_COOC_WORDS);
    if (n_groups < 1 || n_groups > RRI_MAX_K) return say(TOPN_REQ_UNSUPPORTED, "n_groups %lld outside 1 .. %lld", (long long)n_groups, (long long)RRI_MAX_K);
    if (!indptr) return say(TOPN_REQ_INVALID, "indptr is NULL", 0, 0);
    if (!words) return say(TOPN_REQ_INVALID, "words is NULL", 0, 0);
    const int64_t nnz = indptr[n_rows];
    if (nnz > 0 && !indices) return say(TOPN_REQ_INVALID, "indices is NULL with %lld entries", (long long)nnz, 0);
    // a pattern has no values: csr_check is shown the indices in their place
    const std::string bad = csr_check(indptr, indices, indices, nnz, RRI_F32, n_rows, n_cols, CSR_INCREASING);
    if (!bad.empty()) {
        if (msg && msg_len) snprintf(msg, msg_len, "%s", bad.c_str());
        return TOPN_REQ_INVALID;
    }
    return cooc_check_words(n_cols, words, n_groups, group_size, msg, msg_len);
}
// ... and the groups alone, against a corpus that is resident and canonical already (rri_corpus_cooccurrence_counts): the rules
// of the request above that do not read the pattern, in the same order
inline int cooc_check_groups(int64_t n_cols, const int32_t* words, int32_t n_groups, int32_t group_size, char* msg, size_t msg_len) {
    auto say = [&](int code, const char* what, long long a, long long b) {
        if (msg && msg_len) snprintf(msg, msg_len, what, a, b);
        return code;
    };
    if (n_groups < 0) return say(TOPN_REQ_INVALID, "n_groups %lld is negative", (long long)n_groups, 0);
    if (group_size < 0) return say(TOPN_REQ_INVALID, "group_size %lld is negative", (long long)group_size, 0);
    if (group_size < 1 || group_size > RRI_MAX_COOC_WORDS)
        return say(TOPN_REQ_UNSUPPORTED, "group_size %lld outside 1 .. %lld", (long long)group_size, (long long)RRI_MAX_COOC_WORDS);
    if (n_groups < 1 || n_groups > RRI_MAX_K) return say(TOPN_REQ_UNSUPPORTED, "n_groups %lld outside 1 .. %lld", (long long)n_groups, (long long)RRI_MAX_K);
    if (!words) return say(TOPN_REQ_INVALID, "words is NULL", 0, 0);
    return cooc_check_words(n_cols, words, n_groups, group_size, msg, msg_len);
}

// ---- the membership table -----------------------------------------------------------------------------------------------------
// ent[ptr[j] .. ptr[j + 1]) holds cooc_pack(group, slot) of every slot that names column j, groups ascending (a counting sort,
// stable); a -1 slot is in nobody's list.  ptr has n_cols + 1 entries, ent at most n_groups * group_size.
struct CoocMemb {
    std::vector<int32_t> ptr, ent;
};
inline CoocMemb cooc_build_memb(const int32_t* words, int32_t n_groups, int32_t group_size, int64_t n_cols) {
    CoocMemb m;
    m.ptr.assign((size_t)n_cols + 1, 0);
    const size_t slots = (size_t)n_groups * group_size;
    for (size_t s = 0; s < slots; ++s)
        if (words[s] >= 0) m.ptr[(size_t)words[s] + 1] += 1;
    for (int64_t j = 0; j < n_cols; ++j) m.ptr[(size_t)j + 1] += m.ptr[(size_t)j];
    m.ent.assign((size_t)m.ptr[(size_t)n_cols], 0);
    std::vector<int32_t> fill(m.ptr.begin(), m.ptr.end() - 1);
    for (int g = 0; g < n_groups; ++g)
        for (int a = 0; a < group_size; ++a) {
            const int32_t j = words[(size_t)g * group_size + a];
            if (j >= 0) m.ent[(size_t)fill[(size_t)j]++] = cooc_pack(g, a);
        }
    return m;
}

// ---- row chunks ---------------------------------------------------------------------------------------------------------------
// Rows per chunk: the most whole tiles whose masks (4 bytes per row and group) fit `budget` bytes, at least one tile
inline i64 cooc_chunk_rows(int32_t n_groups, i64 budget) {
    const i64 rows = budget / (4 * (i64)std::max<int32_t>(n_groups, 1));
    return std::max<i64>(COOC_TILE_ROWS, rows / COOC_TILE_ROWS * COOC_TILE_ROWS);
}
// chunk c holds the rows [r0, r1); its mask array has rows_pad = r1 - r0 rounded up to whole tiles words per group
struct CoocChunk {
    i64 r0, r1, rows_pad;
};
// the number of chunks of n_rows rows; out (NULL: count only) takes them.  No row, no chunk.
inline i64 cooc_cut_rows(i64 n_rows, int32_t n_groups, i64 budget, std::vector<CoocChunk>* out) {
    const i64 per = cooc_chunk_rows(n_groups, budget);
    i64 nc = 0;
    for (i64 r0 = 0; r0 < n_rows; r0 += per, ++nc)
        if (out) {
            const i64 r1 = std::min(n_rows, r0 + per);
            out->push_back(CoocChunk{r0, r1, round_up(r1 - r0, COOC_TILE_ROWS)});
        }
    return nc;
}
// lanes that share a row in k_cooc_masks: 8, a whole wave from 64 entries per row on (the rule of spx_scale_lps)
inline int cooc_lps(i64 nnz, i64 n_rows) { return spx_scale_lps(nnz, n_rows); }
// pairs of slots a <= b per lane of k_cooc_count: group_size (group_size + 1) / 2 pairs over the 64 lanes of a wave, in the four
// instantiations that exist (group_size <= 10, 15, 22, 32)
inline int cooc_count_ppt(int32_t group_size) {
    const int need = (group_size * (group_size + 1) / 2 + 63) / 64;
    return need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : 9;
}
// LDS of k_cooc_masks: a word per (group, row of the tile)
inline size_t cooc_mask_lds_bytes(int32_t n_groups) { return (size_t)n_groups * COOC_TILE_ROWS * sizeof(unsigned); }

// ---- the plain counter --------------------------------------------------------------------------------------------------------
// df (n_groups x group_size) and codf (n_groups x group_size x group_size) of a checked request, row by row through the masks
inline void cooc_reference(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_cols, const int32_t* words,
                           int32_t n_groups, int32_t group_size, int64_t* df, int64_t* codf) {
    const CoocMemb memb = cooc_build_memb(words, n_groups, group_size, n_cols);
    const size_t M = (size_t)group_size;
    std::fill(df, df + (size_t)n_groups * M, (int64_t)0);
    std::fill(codf, codf + (size_t)n_groups * M * M, (int64_t)0);
    std::vector<unsigned> mask((size_t)n_groups, 0u);
    std::vector<int> touched;
    for (int64_t r = 0; r < n_rows; ++r) {
        touched.clear();
        for (int64_t p = indptr[r]; p < indptr[r + 1]; ++p) {
            const int32_t j = indices[p];
            for (int32_t q = memb.ptr[(size_t)j]; q < memb.ptr[(size_t)j + 1]; ++q) {
                const int g = cooc_group(memb.ent[(size_t)q]);
                if (!mask[(size_t)g]) touched.push_back(g);
                mask[(size_t)g] |= 1u << cooc_slot(memb.ent[(size_t)q]);
            }
        }
        for (int g : touched) {
            const unsigned m = mask[(size_t)g];
            mask[(size_t)g] = 0u;
            for (int a = 0; a < group_size; ++a)
                for (int b = 0; b < group_size; ++b) codf[((size_t)g * M + a) * M + b] += cooc_pair(m, a, b);
        }
    }
    for (int g = 0; g < n_groups; ++g)
        for (int a = 0; a < group_size; ++a) df[(size_t)g * M + a] = codf[((size_t)g * M + a) * M + a];
}

}  // namespace rri
