// sparse_plan.h -- host-side decisions of the sparse (chain-major) ZL operator: which backward kernel, which fused
// block kernel, the chunk height of the per-chain sums.  hmc.hip launches by these functions and the test hook
// glmmr_mcml_dbg_sparse_plan (ctx_hooks.hip) reports them, so the two cannot drift apart.
#pragma once
#include <cstdlib>
#include <cstring>
#include "ctx.h"

namespace mcml {

constexpr int CM_ROWS = 64;       // rows per workgroup in the elementwise / partial-sum kernels (16 per wave)

// rows of the random-effect-sized arrays per workgroup of the per-chain kernels: small chunks when Q is small, so
// that config 4's 320 effects still spread over the chip
__host__ __device__ inline int cm_qrows(int Q) { return Q <= 4096 ? 16 : CM_ROWS; }

// chain blocks of 64 (one wave's lanes)
inline int cm_chain_blocks(int C) { return (C + 63) / 64; }

// the backward product takes k_cm_backward_long (a workgroup per random effect and chain block) when the rows of the
// operand it gathers through -- Z' in the factored form, ZL' otherwise -- hold 24 entries or more on average
inline bool cm_long_rows(const Ctx& c) { return (c.sp.factored ? c.sp.nnz_z : c.sp.nnz) >= 24L * c.Q; }

// the factored operator's k_cm_Lcol of a leapfrog step and k_cm_Lrow of the next as one launch: DMAX of k_cm_Lcol_Lrow
// (8 or 16), or 0 for the separate kernels (blocks above 16, blocks not contiguous, or GLMMR_MCML_CM_LFUSE=0: the A/B
// switch, read per call because a test compares the two in one process)
inline int cm_fuse_width(const Ctx& c)
{
    const char* e = getenv("GLMMR_MCML_CM_LFUSE");
    const bool v = !(e && !strcmp(e, "0"));
    if (!(v && c.sp.factored && c.sp.nblk > 0 && c.sp.max_blk <= 16)) return 0;
    return c.sp.max_blk <= 8 ? 8 : 16;
}

}  // namespace mcml
