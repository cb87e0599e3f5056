// Stand-alone program over rri_nmf_amd/csrc/rri_early_deal.hpp, the host-and-device header that says where the workgroups of the
// early-sums job sit in the grid of the fused pass, and over the stride dense_plan (rri_layout.hpp) hands to it.  It reads requests
// on stdin, one per line:
//     grid P first nblocks s        every position 0 .. P + nblocks - 1 through early_slot: the program checks the map itself (each
//                                   job index once, each own index once and ascending, nothing out of range, the job's workgroups at
//                                   first + i (s + 1)) and prints it -- 'kind' (1: the job's) and 'index' per position
//     stride P first nblocks        early_deal_stride
//     plan n d k dtype flavour n_cu pk_rows pk_il deal      the early-sums part of the plan under RRI_PASS_PK_GEOM = pk_rows, pk_il
//                                   and RRI_EARLY_DEAL = deal
// tests/test_early_deal_cpu.py compares every line with a Python restatement.  Built with the host compiler, also under
// AddressSanitizer and UndefinedBehaviorSanitizer.
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "rri_early_deal.hpp"
#include "rri_hip.h"
#include "rri_layout.hpp"

using namespace rri;

static int fail(const char* what, int pos) {
    std::printf("FAILED %s at position %d\n", what, pos);
    return 1;
}

static int walk(int P, int first, int nblocks, int s) {
    const int total = P + nblocks;
    std::vector<int> kind((size_t)total), index((size_t)total), job_seen((size_t)nblocks, 0), own_seen((size_t)P, 0);
    int next_own = 0;
    for (int pos = 0; pos < total; ++pos) {
        const EarlySlot e = early_slot(pos, first, nblocks, s);
        kind[(size_t)pos] = e.job ? 1 : 0;
        index[(size_t)pos] = e.index;
        if (e.job) {
            if (e.index < 0 || e.index >= nblocks) return fail("job index out of range", pos);
            if (pos != first + e.index * (s + 1)) return fail("job workgroup i is not at first + i (s + 1)", pos);
            job_seen[(size_t)e.index] += 1;
        } else {
            if (e.index < 0 || e.index >= P) return fail("own index out of range", pos);
            if (e.index != next_own) return fail("own indices are not 0, 1, 2, ... in the order of the positions", pos);
            own_seen[(size_t)e.index] += 1;
            next_own += 1;
        }
    }
    for (int i = 0; i < nblocks; ++i)
        if (job_seen[(size_t)i] != 1) return fail("a job index does not occur exactly once: index", i);
    for (int i = 0; i < P; ++i)
        if (own_seen[(size_t)i] != 1) return fail("an own index does not occur exactly once: index", i);
    std::printf("grid P=%d first=%d nblocks=%d s=%d positions=%d\n", P, first, nblocks, s, total);
    std::printf("kind");
    for (int v : kind) std::printf(" %d", v);
    std::printf("\nindex");
    for (int v : index) std::printf(" %d", v);
    std::printf("\n");
    return 0;
}

int main() {
    std::string what;
    while (std::cin >> what) {
        if (what == "grid") {
            int P, first, nblocks, s;
            std::cin >> P >> first >> nblocks >> s;
            if (walk(P, first, nblocks, s)) return 1;
        } else if (what == "stride") {
            int P, first, nblocks;
            std::cin >> P >> first >> nblocks;
            std::printf("stride %d\n", early_deal_stride(P, first, nblocks));
        } else if (what == "plan") {
            long long n, d;
            int k, dtype, flavour, n_cu, deal;
            rri_switches sw;
            std::cin >> n >> d >> k >> dtype >> flavour >> n_cu >> sw.pk_rows >> sw.pk_il >> deal;
            sw.early_deal = deal != 0;
            const DensePlan p = dense_plan(n, d, k, dtype, flavour, sw, n_cu);
            const int P = p.npanels * p.nrb;
            std::printf("plan P=%d first=%d e_blocks=%d e_tpb=%d e_stride=%d\n", P, early_job_first(P, n_cu), p.e_blocks, p.e_tpb, p.e_stride);
        } else {
            std::printf("unknown request %s\n", what.c_str());
            return 2;
        }
    }
    std::printf("ok\n");
    return 0;
}
