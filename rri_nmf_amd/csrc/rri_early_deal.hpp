// rri_early_deal.hpp -- where the workgroups of the early-sums job sit in the grid of the fused pass, written once.
//
// The pass has P workgroups of its own and the job `nblocks`; the grid (behind TgramJob's blocks) has P + nblocks positions.  Up to
// position `first` (early_job_first in rri_layout.hpp: the first round of the pass) all are the pass's own.  From there the job's
// workgroups are DEALT through what is left: job workgroup i sits at first + i (s + 1), s = (P - first) / nblocks own workgroups
// follow each of them, and the own workgroups left over come behind the last.  s = 0 is the contiguous run [first, first + nblocks)
// of RRI_EARLY_DEAL=0, and of every shape whose pass has fewer than nblocks workgroups behind `first`.  The own workgroups keep
// their order: position -> own index is a plain renumbering, which rot's groups of 8 and the kept row blocks of k_pass rely on.
//
// Plain inline functions, host and device: k_pass maps its block index with early_slot, LK::early_job (rri_hip.hip) takes the
// stride from the plan (dense_plan in rri_layout.hpp), and the stand-alone CPU test (tests/c/early_deal_main.cpp) compiles this
// header with the host compiler and walks every position of a grid.  The inverse map is used by nothing and is not written.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RRI_DEAL_FN __host__ __device__ inline
#else
#define RRI_DEAL_FN inline
#endif

namespace rri {

// own workgroups of the pass between two workgroups of the job
RRI_DEAL_FN int early_deal_stride(int P, int first, int nblocks) { return nblocks > 0 && P > first ? (P - first) / nblocks : 0; }

struct EarlySlot { int job, index; };   // job != 0: workgroup `index` of the job; else own workgroup `index` of the pass

RRI_DEAL_FN EarlySlot early_slot(int pos, int first, int nblocks, int s) {
    if (pos < first) return EarlySlot{0, pos};
    const unsigned r = (unsigned)(pos - first), g = (unsigned)s + 1u;
    if (r >= (unsigned)nblocks * g) return EarlySlot{0, pos - nblocks};      // the own workgroups behind the last of the job
    const unsigned q = r / g;                                                // job workgroups in front of this position, but for ...
    if (r == q * g) return EarlySlot{1, (int)q};                             // ... the one AT it
    return EarlySlot{0, pos - (int)q - 1};
}

}  // namespace rri
