// Stand-alone check of rri_nmf_amd/csrc/rri_cooc.hpp (own main, host compiler, sanitizers): the request check rule by rule, the
// membership table, the row chunks at their borders, and the plain counter on seeded corpora whose rows, words and counts are
// printed for tests/test_cooc_cpu.py to hold against numpy on the dense 0/1 form.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rri_cooc.hpp"

using namespace rri;

static unsigned long long g_state = 0x9e3779b97f4a7c15ull;
static unsigned rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(g_state >> 33);
}

struct Req {
    std::vector<int64_t> indptr{0, 2, 2, 5};
    std::vector<int32_t> indices{0, 3, 1, 2, 4};
    int64_t n_rows = 3, n_cols = 5;
    std::vector<int32_t> words{0, 3, -1, 4, -1, 1};
    int32_t n_groups = 2, group_size = 3;
    bool null_indptr = false, null_indices = false, null_words = false;
};
static void req(const char* name, const Req& r) {
    char msg[200] = "";
    const int code = cooc_check_request(r.null_indptr ? nullptr : r.indptr.data(), r.null_indices ? nullptr : r.indices.data(), r.n_rows,
                                        r.n_cols, r.null_words ? nullptr : r.words.data(), r.n_groups, r.group_size, msg, sizeof msg);
    printf("req %s : %d : %s\n", name, code, msg);
}

static void memb(const char* name, const std::vector<int32_t>& words, int n_groups, int group_size, int64_t n_cols) {
    const CoocMemb m = cooc_build_memb(words.data(), n_groups, group_size, n_cols);
    printf("memb %s :", name);
    for (int32_t p : m.ptr) printf(" %d", p);
    printf(" |");
    for (int32_t e : m.ent) {
        if (cooc_pack(cooc_group(e), cooc_slot(e)) != e) { printf("\npacking of %d does not round-trip\n", e); exit(1); }
        printf(" %d.%d", cooc_group(e), cooc_slot(e));
    }
    printf("\n");
}

static void cut(const char* name, int64_t n_rows, int32_t n_groups, int64_t budget) {
    std::vector<CoocChunk> ch;
    const i64 nc = cooc_cut_rows(n_rows, n_groups, budget, &ch);
    if (nc != (i64)ch.size() || nc != cooc_cut_rows(n_rows, n_groups, budget, nullptr)) { printf("chunk count of %s\n", name); exit(1); }
    printf("cut %s %lld :", name, (long long)cooc_chunk_rows(n_groups, budget));
    for (const CoocChunk& c : ch) printf(" %lld:%lld:%lld", (long long)c.r0, (long long)c.r1, (long long)c.rows_pad);
    printf("\n");
}

static void corpus(int id, int n_rows, int n_cols, int n_groups, int group_size, int percent, int empty_slots) {
    std::vector<int64_t> indptr{0};
    std::vector<int32_t> indices;
    for (int r = 0; r < n_rows; ++r) {
        const bool all = r % 7 == 3, none = r % 7 == 5;
        for (int j = 0; j < n_cols; ++j)
            if (!none && (all || (int)(rnd() % 100) < percent)) indices.push_back(j);
        indptr.push_back((int64_t)indices.size());
    }
    std::vector<int32_t> words((size_t)n_groups * group_size, -1);
    for (int g = 0; g < n_groups; ++g) {
        std::vector<int32_t> pool((size_t)n_cols);
        for (int j = 0; j < n_cols; ++j) pool[(size_t)j] = j;
        int left = n_cols;
        for (int a = 0; a < group_size && left > 0; ++a) {
            if (empty_slots && rnd() % 4 == 0) continue;
            if (empty_slots == 2 && g == 1) continue;          // a group made only of empty slots
            const int pick = (int)(rnd() % (unsigned)left);
            words[(size_t)g * group_size + a] = pool[(size_t)pick];
            pool[(size_t)pick] = pool[(size_t)--left];
        }
    }
    char msg[200] = "";
    if (cooc_check_request(indptr.data(), indices.data(), n_rows, n_cols, words.data(), n_groups, group_size, msg, sizeof msg) != TOPN_REQ_OK) {
        printf("corpus %d is refused: %s\n", id, msg);
        exit(1);
    }
    std::vector<int64_t> df((size_t)n_groups * group_size, -1), codf((size_t)n_groups * group_size * group_size, -1);
    cooc_reference(indptr.data(), indices.data(), n_rows, n_cols, words.data(), n_groups, group_size, df.data(), codf.data());
    printf("corpus %d : %d %d %d %d\n", id, n_rows, n_cols, n_groups, group_size);
    printf("indptr %d :", id);
    for (int64_t p : indptr) printf(" %lld", (long long)p);
    printf("\nindices %d :", id);
    for (int32_t j : indices) printf(" %d", j);
    printf("\nwords %d :", id);
    for (int32_t w : words) printf(" %d", w);
    printf("\ndf %d :", id);
    for (int64_t v : df) printf(" %lld", (long long)v);
    printf("\ncodf %d :", id);
    for (int64_t v : codf) printf(" %lld", (long long)v);
    printf("\n");
}

int main() {
    // ---- the request check: every rule has its own text
    req("fine", Req());
    { Req r; r.n_rows = 0; r.indptr = {0}; r.indices.clear(); r.null_indices = true; req("no_rows", r); }
    { Req r; r.indptr = {0, 0, 0, 0}; r.indices.clear(); r.null_indices = true; req("no_entries", r); }
    { Req r; r.words = {-1, -1, -1, -1, -1, -1}; req("only_empty_slots", r); }
    { Req r; r.words = {0, 3, 1, 0, 3, 1}; req("same_words_in_two_groups", r); }
    { Req r; r.n_rows = -1; req("negative_rows", r); }
    { Req r; r.n_cols = -1; req("negative_cols", r); }
    { Req r; r.n_groups = -1; req("negative_groups", r); }
    { Req r; r.group_size = -1; req("negative_group_size", r); }
    { Req r; r.group_size = 0; r.words.clear(); r.words.push_back(0); req("group_size_0", r); }
    { Req r; r.n_groups = 0; req("no_groups", r); }
    { Req r; r.n_cols = 40; r.n_groups = 1; r.group_size = 32; r.words.resize(32); for (int a = 0; a < 32; ++a) r.words[(size_t)a] = a; req("group_size_32", r); }
    { Req r; r.n_cols = 40; r.n_groups = 1; r.group_size = 33; r.words.resize(33); for (int a = 0; a < 33; ++a) r.words[(size_t)a] = a; req("group_size_33", r); }
    { Req r; r.n_groups = RRI_MAX_K; r.group_size = 1; r.words.assign((size_t)RRI_MAX_K, 2); req("groups_max_k", r); }
    { Req r; r.n_groups = RRI_MAX_K + 1; r.group_size = 1; r.words.assign((size_t)RRI_MAX_K + 1, 2); req("groups_max_k_plus_1", r); }
    { Req r; r.null_indptr = true; req("indptr_null", r); }
    { Req r; r.null_words = true; req("words_null", r); }
    { Req r; r.null_indices = true; req("indices_null", r); }
    { Req r; r.indptr = {1, 2, 2, 5}; req("indptr_not_from_zero", r); }
    { Req r; r.indptr = {0, 2, 1, 5}; req("indptr_decreases", r); }
    { Req r; r.indptr = {0, 2, 2, -1}; req("negative_nnz", r); }
    { Req r; r.indices = {0, 5, 1, 2, 4}; req("column_n_cols", r); }
    { Req r; r.indices = {-1, 3, 1, 2, 4}; req("column_negative", r); }
    { Req r; r.indices = {0, 3, 2, 2, 4}; req("column_twice", r); }
    { Req r; r.indices = {3, 0, 1, 2, 4}; req("columns_descend", r); }
    { Req r; r.words[1] = 5; req("word_n_cols", r); }
    { Req r; r.words[1] = -2; req("word_below_minus_one", r); }
    { Req r; r.words = {0, 3, 0, 4, -1, 1}; req("word_twice_in_a_group", r); }

    // ---- the membership table: column 0 in no group, 1 in one, 2 in every group; empty slots at the front and in the middle
    memb("mixed", {2, 1, -1, -1, 2, 4, 3, -1, 2}, 3, 3, 6);
    memb("only_empty_slots", {-1, -1, -1, -1}, 2, 2, 3);
    memb("one_column", {0, 0, 0}, 3, 1, 1);
    memb("slot_31", std::vector<int32_t>{-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
                                         -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 1}, 1, 32, 2);

    // ---- the row chunks at their borders: budget / (4 n_groups) rows, whole tiles of 32, at least one tile
    cut("none", 0, 50, 1 << 20);
    cut("one_row", 1, 50, 1 << 20);
    cut("budget_below_a_tile", 70, 1024, 1000);              // 0 rows fit: one tile per chunk all the same
    cut("exactly_one_chunk", 64, 2, 512);                    // 64 rows fit
    cut("one_row_more", 65, 2, 512);
    cut("not_whole_tiles", 100, 2, 600);                     // 75 rows fit: 64 per chunk
    cut("max_k", 16385, RRI_MAX_K, COOC_MASK_BUDGET);        // the first n_rows with two chunks at n_groups = RRI_MAX_K
    cut("max_k_one_chunk", 16384, RRI_MAX_K, COOC_MASK_BUDGET);
    cut("fifty_topics", 100000, 50, COOC_MASK_BUDGET);

    // ---- pairs per lane of the counting kernel: the instantiation a group size takes
    printf("ppt :");
    for (int M = 1; M <= RRI_MAX_COOC_WORDS; ++M) printf(" %d", cooc_count_ppt(M));
    printf("\n");

    // ---- the plain counter on seeded corpora (rows with every column and with none among them)
    int id = 0;
    corpus(id++, 1, 1, 1, 1, 100, 0);
    corpus(id++, 9, 1, 2, 1, 50, 0);
    corpus(id++, 40, 12, 3, 5, 30, 1);
    corpus(id++, 33, 33, 4, 32, 50, 1);
    corpus(id++, 70, 40, 5, 31, 20, 2);
    corpus(id++, 25, 7, 65, 2, 40, 1);
    corpus(id++, 12, 64, 2, 10, 0, 0);                       // no entry besides the full rows
    corpus(id++, 3, 5, 2, 3, 0, 0);                          // no entry at all: words that occur in no document
    printf("ok %d corpora\n", id);
    return 0;
}
