// Stand-alone program over rri_nmf_amd/csrc/rri_layout.hpp, the host-only header that decides the geometry of a handle: the
// dense plan of rri_create, pass_keep, the persistent sweep's geometry, the blocked copies of a CSR pattern, the CSR argument
// checks and the small grids.  It reads requests on stdin (one per line, the arrays of a request on the same line) and prints
// one line per answer, the arrays of a blocked copy on lines of their own; tests/test_layout_cpu.py compares every line with the
// Python restatements of the suites and with values worked out by hand, and tests/test_layout_plan_gpu.py with what a handle
// reports.  Built with the host compiler, on the CPU under AddressSanitizer and UndefinedBehaviorSanitizer.
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "rri_hip.h"
#include "rri_layout.hpp"

using namespace rri;

template <typename T>
static std::vector<T> read_array(long long len) {
    std::vector<T> v((size_t)(len > 0 ? len : 0));
    for (auto& x : v) {
        long long t = 0;
        std::cin >> t;
        x = (T)t;
    }
    return v;
}

template <typename V>
static void print_array(const char* name, const V& v) {
    std::printf("%s", name);
    for (const auto& x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}

static DensePlan read_plan(int* k_out, int* dtype_out, rri_switches* sw_out) {
    long long n, d;
    int k, dtype, flavour, n_cu;
    rri_switches sw;
    std::cin >> n >> d >> k >> dtype >> flavour >> n_cu >> sw.pk_rows >> sw.pk_il >> sw.x_pack >> sw.pass_cache_mb;
    *k_out = k;
    *dtype_out = dtype;
    *sw_out = sw;
    return dense_plan(n, d, k, dtype, flavour, sw, n_cu);
}

int main() {
    std::string what;
    while (std::cin >> what) {
        if (what == "plan") {
            int k, dtype;
            rri_switches sw;
            const DensePlan p = read_plan(&k, &dtype, &sw);
            std::printf("plan LD=%lld VN=%d PW=%d kp=%d npanels=%d rpb=%d nrb=%d nwb=%d nwb256=%d ntb=%d ntb32=%d nsplit=%d red_elems=%lld "
                        "ro_il=%d cpart_rows=%d gpart_rows=%lld ttpart_rows=%lld tpart_rows=%lld xy_stride=%d interleaved=%d wtrow_small=%d "
                        "load_bytes=%d dtype_size=%d sparse=%d sp0_nblk=%d sp0_bw=%d sp1_nblk=%d sp1_bw=%d\n",
                        p.LD, p.VN, p.PW, p.kp, p.npanels, p.rpb, p.nrb, p.nwb, p.nwb256, p.ntb, p.ntb32, p.nsplit, p.red_elems, p.ro_il,
                        p.cpart_rows, p.gpart_rows, p.ttpart_rows, p.tpart_rows, p.xy_stride,
                        (int)ro_pass_interleaved(p.ro_il, p.npanels, p.nrb), (int)wtrow_small(false, p.nrb), load_bytes(dtype),
                        (int)dtype_size(dtype), (int)p.sparse, p.sp[0].nblk, p.sp[0].bw, p.sp[1].nblk, p.sp[1].bw);
        } else if (what == "early") {
            // the early-sums schedule of the plan: where the job sits among the pass's P own workgroups, how many of its workgroups
            // walk no tile, the grids of k_trow_early and k_wfin, and the job's LDS against the pass's own (LK::early_ok)
            int k, dtype;
            rri_switches sw;
            const DensePlan p = read_plan(&k, &dtype, &sw);
            int n_cu;
            std::cin >> n_cu;
            const int P = p.npanels * p.nrb;
            const long long tiles = (p.n + 63) / 64;
            const long long busy = (tiles + p.e_tpb - 1) / p.e_tpb;
            std::printf("early npanels=%d rpb=%d nrb=%d P=%d first=%d e_blocks=%d e_tpb=%d idle=%lld tiles=%lld nte=%d nwfin=%d nsplit=%d ntb=%d "
                        "job_lds=%lld pass_lds=%lld interleaved=%d\n",
                        p.npanels, p.rpb, p.nrb, P, early_job_first(P, n_cu), p.e_blocks, p.e_tpb, (long long)p.e_blocks - busy, tiles, p.nte,
                        p.nwfin, p.nsplit, p.ntb, (long long)early_job_lds_doubles(k), 5LL * p.rpb + 4 * 8 * 72,
                        (int)ro_pass_interleaved(p.ro_il, p.npanels, p.nrb));
        } else if (what == "keep") {
            int k, dtype, xp_valid;
            rri_switches sw;
            const DensePlan p = read_plan(&k, &dtype, &sw);
            long long ldw;
            std::cin >> ldw >> xp_valid;
            const double cache_mb = sw.pass_cache_mb;
            const PassKeepTerms t = pass_keep_terms(p, k, ldw, dtype_size(dtype), xp_valid != 0, cache_mb);
            std::printf("keep q=%d nrb=%d chain=%.17g budget=%.17g block=%.17g x_bytes=%.17g\n",
                        pass_keep(p, k, ldw, dtype_size(dtype), xp_valid != 0, cache_mb), p.nrb, t.chain, t.budget, t.block, t.x_bytes);
        } else if (what == "onchip") {
            long long n, LD;
            int k, f32, proj, n_cu;
            std::cin >> n >> LD >> k >> f32 >> proj >> n_cu;
            OnchipGeom g{};
            const bool geom = onchip_geometry(n, LD, k, f32 != 0, proj != 0, n_cu, &g);
            OnchipGeom g2{};
            const bool ok = onchip_shape_ok(n, LD, k, f32 != 0, proj != 0, n_cu, &g2);
            const int kt = onchip_kt(k);
            const bool few = g.rpw <= onchip_rpw(f32 != 0, proj != 0, kt, true);
            std::printf("onchip ok=%d geom=%d CG=%d RG=%d rows_wg=%d rpw=%d NA=%d kS=%d G=%d shmem=%lld KT=%d few=%d RPW=%d cap=%d\n", (int)ok,
                        (int)geom, g.CG, g.RG, g.rows_wg, g.rpw, g.NA, g.kS, g.G, (long long)g.shmem, kt, (int)few,
                        onchip_rpw(f32 != 0, proj != 0, kt, few), onchip_rpw(f32 != 0, proj != 0, kt, false));
        } else if (what == "copy") {
            int which, sparse_x, es, n_cu;
            long long n, d, nnz;
            std::cin >> which >> sparse_x >> es >> n_cu >> n >> d >> nnz;
            const std::vector<int64_t> indptr = read_array<int64_t>(n + 1);
            const std::vector<int32_t> indices = read_array<int32_t>(nnz);
            const SpDims dims = sp_dims(n, d, which, sparse_x != 0, (size_t)es);
            const SpCopyHost h = build_sp_copy(indptr.data(), indices.data(), n, nnz, which, dims, sp_target_items(n_cu, sparse_x != 0));
            std::printf("copy nblk=%d bw=%d nseg=%lld gdim=%lld lps=%d nwork=%d count=%lld longest_row=%lld\n", dims.nblk, dims.bw, dims.nseg,
                        dims.gdim, h.lps, (int)h.work.size(), h.count, h.longest_row);
            std::vector<int> flat;
            for (const SpWork& w : h.work) { flat.push_back(w.blk); flat.push_back(w.s0); flat.push_back(w.s1); flat.push_back(w.pad); }
            print_array("work", flat);
            print_array("segptr", h.segptr);
            print_array("idx", h.idx);
            print_array("perm", h.perm);
        } else if (what == "csr") {
            int rules, dtype, has_data;
            long long n, d, nnz, len_indptr, len_indices;
            std::cin >> rules >> n >> d >> nnz >> dtype >> has_data >> len_indptr;
            const std::vector<int64_t> indptr = read_array<int64_t>(len_indptr);
            std::cin >> len_indices;
            const std::vector<int32_t> indices = read_array<int32_t>(len_indices);
            const double dummy = 0.0;
            // (a vector of length 0 still stands for an array that is there: a pointer that is never read)
            static const int64_t no_indptr[1] = {0};
            static const int32_t no_indices[1] = {0};
            const std::string bad = csr_check(len_indptr < 0 ? nullptr : indptr.empty() ? no_indptr : indptr.data(),
                                              len_indices < 0 ? nullptr : indices.empty() ? no_indices : indices.data(),
                                              has_data ? (const void*)&dummy : nullptr, nnz, dtype, n, d, (CsrRules)rules);
            std::printf("csr %s\n", bad.empty() ? "ok" : bad.c_str());
        } else if (what == "sort") {
            int ds;
            long long n, nnz;
            std::cin >> ds >> n >> nnz;
            const std::vector<int64_t> indptr = read_array<int64_t>(n + 1);
            const std::vector<int32_t> indices = read_array<int32_t>(nnz);
            const std::vector<long long> vals = read_array<long long>(nnz);
            std::vector<float> v4(vals.begin(), vals.end());
            std::vector<double> v8(vals.begin(), vals.end());
            const void* data = ds == 4 ? (const void*)v4.data() : (const void*)v8.data();
            std::vector<int32_t> sidx;
            std::vector<unsigned char> sval;
            const bool copied = csr_sort_rows(indptr.data(), indices.data(), data, n, nnz, (size_t)ds, sidx, sval);
            const int32_t* ix = copied ? sidx.data() : indices.data();
            const std::string dup = csr_duplicates(indptr.data(), ix, n);
            std::printf("sort copied=%d copies=%lld/%lld dup=%s\n", (int)copied, (long long)sidx.size(), (long long)sval.size(),
                        dup.empty() ? "ok" : dup.c_str());
            std::vector<long long> out_i, out_v;
            for (long long p = 0; p < nnz; ++p) {
                out_i.push_back(ix[p]);
                const void* src = copied ? (const void*)sval.data() : data;
                out_v.push_back(ds == 4 ? (long long)((const float*)src)[p] : (long long)((const double*)src)[p]);
            }
            print_array("sorted_indices", out_i);
            print_array("sorted_values", out_v);
        } else if (what == "wmcorr_cols") {
            long long n, LD;
            int n_cu;
            std::cin >> n >> LD >> n_cu;
            const WmcorrGrid g = wmcorr_cols_grid(n, LD, n_cu);
            std::printf("wmcorr_cols npg=%d nrb=%lld rpb=%lld wcorr_nrb=%d\n", g.npg, g.nrb, g.rpb, g.wcorr_nrb);
        } else if (what == "wmcorr") {
            long long n, ldb;
            int bits, npanels, n_cu, cpart_rows;
            std::cin >> n >> bits >> ldb >> npanels >> n_cu >> cpart_rows;
            const WmcorrGrid g = wmcorr_grid(n, bits != 0, ldb, npanels, n_cu, cpart_rows);
            std::printf("wmcorr npg=%d nrb=%lld rpb=%lld wcorr_nrb=%d\n", g.npg, g.nrb, g.rpb, g.wcorr_nrb);
        } else if (what == "resid") {
            long long n, d;
            int k, n_cu, sums;
            std::cin >> n >> d >> k >> n_cu >> sums;
            const ResidGrid g = resid_grid(n, d, n_cu, sums != 0);
            std::printf("resid ks=%d nb=%u ny=%u nsplit=%d dchunk=%d\n", resid_ks(k), g.nb, g.ny, g.nsplit, g.dchunk);
        } else if (what == "small") {
            int gpart_rows, k, ntb32, comm, nrb;
            std::cin >> gpart_rows >> k >> ntb32 >> comm >> nrb;
            std::printf("small trow_small=%d wtrow_small=%d\n", (int)trow_small(gpart_rows, k, ntb32), (int)wtrow_small(comm != 0, nrb));
        } else if (what == "tall") {
            long long rows;
            std::cin >> rows;
            std::printf("tall parts=%d\n", tall_gram_parts(rows));
        } else if (what == "spxlps") {
            long long nnz, n;
            std::cin >> nnz >> n;
            std::printf("spxlps lps=%d\n", spx_scale_lps(nnz, n));
        } else if (what == "xpack") {
            long long n, flagged;
            int npanels, tile_rows;
            std::cin >> n >> npanels >> tile_rows >> flagged;
            const long long tiles = xpack_tiles(n, npanels, tile_rows);
            std::printf("xpack tiles=%lld too_many=%d\n", tiles, (int)xpack_too_many_flagged(flagged, tiles));
        } else {
            std::printf("unknown request %s\n", what.c_str());
            return 2;
        }
    }
    std::printf("ok\n");
    return 0;
}
