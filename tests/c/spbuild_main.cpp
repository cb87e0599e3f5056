// spbuild_main.cpp -- rri_spbuild.hpp alone, with the host compiler under sanitizers (tests/test_spbuild_cpu.py).
//
// stdin: any number of
//   copy <which> <sparse_x> <es> <n_cu> <n> <d> <nnz> <seed_a> <seed_b>  indptr[n + 1]  indices[nnz]
// For each, build_sp_copy (the specification) and spbuild_copy_plain -- count, padded scan, claim, sort by position -- with the
// claims arriving in two different shuffled orders and in ascending order; every array of the three must equal the
// specification's, element for element.  Prints the dimensions, the segment lengths' digest and the work items, so that the
// caller can hold them against its own restatement; and, first, the verdicts and texts of the argument check.
#include <cstdio>
#include <iostream>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "rri_spbuild.hpp"

using namespace rri;

static bool same(const SpCopyHost& a, const SpCopyHost& b, const char** what) {
    *what = "";
    if (a.segptr != b.segptr) return *what = "segptr", false;
    if (a.idx != b.idx) return *what = "idx", false;
    if (a.perm != b.perm) return *what = "perm", false;
    if (a.count != b.count) return *what = "count", false;
    if (a.lps != b.lps) return *what = "lps", false;
    if (a.longest_row != b.longest_row) return *what = "longest_row", false;
    if (a.work.size() != b.work.size()) return *what = "nwork", false;
    for (size_t i = 0; i < a.work.size(); ++i)
        if (a.work[i].blk != b.work[i].blk || a.work[i].s0 != b.work[i].s0 || a.work[i].s1 != b.work[i].s1 || a.work[i].pad != b.work[i].pad)
            return *what = "work", false;
    return true;
}

static void check(const char* name, bool alive, long long cr, long long cc, long long nnz, int cdev, long long n, long long d, int dev) {
    char why[200] = "";
    const int code = spbuild_check_corpus(alive, cr, cc, nnz, cdev, n, d, dev, why, sizeof why);
    std::printf("check %s : %d : %s\n", name, code, why);
}

int main() {
    check("fine", true, 5, 7, 9, 0, 5, 7, 0);
    check("dead", false, 5, 7, 9, 0, 5, 7, 0);
    check("device", true, 5, 7, 9, 2, 5, 7, 1);
    check("rows", true, 4, 7, 9, 0, 5, 7, 0);
    check("cols", true, 5, 8, 9, 0, 5, 7, 0);
    check("most_entries", true, 5, 7, 2147483646LL, 0, 5, 7, 0);
    check("too_many_entries", true, 5, 7, 2147483647LL, 0, 5, 7, 0);
    check("dead_wins", false, 4, 8, 2147483647LL, 3, 5, 7, 0);
    std::printf("key : %llu %d %d\n", spbuild_key(2147483646LL, 15295), spbuild_key_pos(spbuild_key(2147483646LL, 15295)),
                (int)spbuild_key_off(spbuild_key(2147483646LL, 15295)));
    std::printf("wave : %d %d %d\n", (int)spbuild_wave_sorted(0), (int)spbuild_wave_sorted(64), (int)spbuild_wave_sorted(65));

    std::string what;
    int cases = 0;
    while (std::cin >> what) {
        if (what != "copy") {
            std::printf("unknown request %s\n", what.c_str());
            return 1;
        }
        int which, sparse_x, n_cu;
        long long es, n, d, nnz;
        unsigned seed_a, seed_b;
        std::cin >> which >> sparse_x >> es >> n_cu >> n >> d >> nnz >> seed_a >> seed_b;
        std::vector<int64_t> indptr((size_t)n + 1);
        std::vector<int32_t> indices((size_t)nnz);
        for (auto& v : indptr) std::cin >> v;
        for (auto& v : indices) std::cin >> v;
        if (!std::cin) {
            std::printf("short input\n");
            return 1;
        }
        const SpDims dims = sp_dims(n, d, which, sparse_x != 0, (size_t)es);
        const int target = sp_target_items(n_cu, sparse_x != 0);
        const SpCopyHost ref = build_sp_copy(indptr.data(), indices.data(), n, nnz, which, dims, target);
        std::vector<int64_t> order((size_t)nnz);
        int equal = 1;
        const char* first = "";
        for (int trial = 0; trial < 3; ++trial) {
            std::iota(order.begin(), order.end(), (int64_t)0);
            if (trial < 2) {
                std::mt19937 gen(trial == 0 ? seed_a : seed_b);
                std::shuffle(order.begin(), order.end(), gen);
            }
            const SpCopyHost got = spbuild_copy_plain(indptr.data(), indices.data(), n, nnz, which, dims, target, trial < 2 ? order.data() : nullptr);
            const char* w = "";
            if (!same(ref, got, &w) && equal) {
                equal = 0;
                first = w;
            }
        }
        // the two shuffles differ from each other and from the ascending order wherever there is something to shuffle
        int shuffled = nnz < 8;
        if (!shuffled) {
            std::vector<int64_t> a((size_t)nnz), b((size_t)nnz);
            std::iota(a.begin(), a.end(), (int64_t)0);
            b = a;
            std::mt19937 ga(seed_a), gb(seed_b);
            std::shuffle(a.begin(), a.end(), ga);
            std::shuffle(b.begin(), b.end(), gb);
            shuffled = a != b && !std::is_sorted(a.begin(), a.end()) && !std::is_sorted(b.begin(), b.end());
        }
        long long pads = 0;
        for (size_t q = 0; q < ref.perm.size(); ++q) pads += ref.perm[q] < 0;
        std::printf("copy %d which=%d equal=%d differs=%s shuffled=%d nblk=%d bw=%d nseg=%lld gdim=%lld lps=%d nwork=%d count=%lld longest_row=%lld "
                    "pads=%lld slots=%lld\n", cases, which, equal, first[0] ? first : "-", shuffled, dims.nblk, dims.bw, dims.nseg, dims.gdim, ref.lps,
                    (int)ref.work.size(), ref.count, ref.longest_row, pads, (long long)ref.perm.size());
        std::printf("work %d :", cases);
        for (const SpWork& w : ref.work) std::printf(" %d %d %d %d", w.blk, w.s0, w.s1, w.pad);
        std::printf("\nseglen %d :", cases);
        for (int b = 0; b < dims.nblk; ++b)
            for (long long s = 0; s < dims.nseg; ++s) {
                // the stored (unpadded) length of segment (b, s): its slots that are not pads
                long long len = 0;
                for (long long q = ref.segptr[(size_t)(b * (dims.nseg + 1) + s)]; q < ref.segptr[(size_t)(b * (dims.nseg + 1) + s + 1)]; ++q)
                    len += ref.perm[(size_t)q] >= 0;
                std::printf(" %lld", len);
            }
        std::printf("\n");
        ++cases;
    }
    std::printf("ok %d cases\n", cases);
    return 0;
}
