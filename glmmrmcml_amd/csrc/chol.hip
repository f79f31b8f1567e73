// chol.hip -- the dense Cholesky stack (chol.h): right-looking blocked factorisation whose panel and trailing updates are
// FP64-MFMA GEMMs (dgemm_dl.h, dgemm_mfma.h), 128-wide leaves factorised and inverted in LDS, the eager fork-join
// schedule and the captured two-chain one with its calibration, the two triangular solves against the factor's inverted
// diagonal blocks and the one-vector solve.  State: Ctx::chol.
#include "ctx.h"
#include "dgemm_mfma.h"
#include "dgemm_dl.h"
#include "reduce.h"
#include "vecops.h"

namespace mcml {

CholState::~CholState()
{
    for (hipEvent_t e : ev_ring) if (e) (void)hipEventDestroy(e);
    if (ev_col) (void)hipEventDestroy(ev_col);
    if (ev_leaf) (void)hipEventDestroy(ev_leaf);
    if (aux) (void)hipStreamDestroy(aux);
    if (aux_lo) (void)hipStreamDestroy(aux_lo);
}

// broadcast lane `src` (compile-time constant) of a double: two v_readlane_b32, no LDS round trip
template <int SRC>
__device__ __forceinline__ double bcast_lane(double v)
{
    union { double d; int i[2]; } u;
    u.d = v;
    u.i[0] = __builtin_amdgcn_readlane(u.i[0], SRC);
    u.i[1] = __builtin_amdgcn_readlane(u.i[1], SRC);
    return u.d;
}

template <int C, int J>
__device__ __forceinline__ void potrf16_upd(double (&a)[16], double l, int r)
{
    // rows r < J hold (never read) upper-triangle entries: updating them too saves the select
    const double lj = bcast_lane<J>(l);
    a[J] = __builtin_fma(-l, lj, a[J]);
    if constexpr (J < 15) potrf16_upd<C, J + 1>(a, l, r);
}

// 1 / sqrt(x) to double precision without the division: v_rsq_f64 seed (~2^-26) + two Newton
// steps, all fused multiply-adds (about 8 dependent instructions instead of ~35 for sqrt + div:
// the 16 x 16 diagonal tile is a serial chain, one of these per column)
__device__ __forceinline__ double rsqrt_nr(double x)
{
    double y = __builtin_amdgcn_rsq(x);
    const double h = 0.5 * x;
    double e = __builtin_fma(-(h * y), y, 0.5);
    y = __builtin_fma(y, e, y);
    e = __builtin_fma(-(h * y), y, 0.5);
    y = __builtin_fma(y, e, y);
    return y;
}

// One column of the 16 x 16 diagonal tile, branch-free (the 16 columns are one serial dependency
// chain on a single wave: every exec-mask branch in it costs a pipeline bubble).  Lane `ln` holds one
// ROW of the 16 columns being eliminated: lanes 0-15 are the tile's own rows (lane C is the pivot row of
// column C), lanes >= 16 are rows that ride along (x L11' = a for any row a costs no extra instruction on
// a 64-lane wave).  `bad` accumulates failed pivots, `yv` collects lane C's reciprocal pivot 1 / L_CC.
template <int C>
__device__ __forceinline__ void potrf16_col(double (&a)[16], int ln, int& bad, double& yv)
{
    double diag = bcast_lane<C>(a[C]);
    const bool ok = diag > 0.0;
    bad |= ok ? 0 : 1;
    diag = ok ? diag : 1.0;
    const double y = rsqrt_nr(diag);
    // every row, the pivot row included, is scaled by the reciprocal pivot: L_CC = diag * rsqrt(diag) is sqrt(diag) to
    // ~1.5 ulp (no separate square root, no lane-dependent branch on the serial chain)
    const double l = a[C] * y;
    yv = (ln == C) ? y : yv;
    a[C] = l;
    if constexpr (C < 15) {
        // a[j] -= l * l_j for j > C, l_j = lane j's l
        potrf16_upd<C, C + 1>(a, l, ln);
    }
}

// Leaf of the blocked factorisation: n <= 128.  One workgroup keeps the block in LDS (row stride 129:
// conflict-free column walks) and factorises it in 16-wide steps; the unused upper triangle receives the
// inverse X = inv(L) (X[i][j], i > j, at S[j][i]; its diagonal = the reciprocal pivots, in xd).  Writes L over
// the lower triangle of A and inv(L) to Linv (128 x 128, ld 128; the caller has zeroed it: entries above the
// diagonal and beyond n are never written).
//
// Step kt (columns kb = 16 kt ...) is software-pipelined so that the serial part is as short as possible:
//   P1  wave 0: the 16 x 16 diagonal tile in registers, one row per lane, readlane broadcasts.  Lanes 16-31
//       carry the 16 rows of the identity (their solution is X_II, the diagonal tile of the inverse) and lanes
//       32-63 the first 32 rows of the panel below -- on a 64-lane wave those rows cost nothing.
//       waves 1-7 meanwhile: the trailing-update tiles of step kt-1 that wave 0 did not need, then block row
//       kt-1 of the inverse (MFMA), stored straight to Linv.
//   P2  all waves: the rest of the panel, rows x X_II' on the matrix cores (4 MFMAs per 16 rows).
//   P3  wave 0: the three trailing tiles the next step's P1 reads (next diagonal tile + its 32 ride-along
//       rows), then straight into P1 of step kt+1 with no workgroup barrier in between.
constexpr int LEAF_NT = 512, LEAF_NW = LEAF_NT / 64;
// LDS layout of the leaf, offsets in doubles: the 128 * 129 block first, then
constexpr int LEAF_LS = CHOL_NB + 1;                 // row stride of the block
constexpr int LEAF_XD = CHOL_NB * LEAF_LS;           // 128 reciprocal pivots = the diagonal of the inverse
constexpr int LEAF_TT = LEAF_XD + CHOL_NB;           // 7 scratch tiles of 16 x 16 (one per wave 1..7)
constexpr int LEAF_DUMMY = LEAF_TT + (LEAF_NW - 1) * 256;   // 64 doubles nobody reads (address-select stores)
constexpr size_t POTRF_LDS = sizeof(double) * (LEAF_DUMMY + 64);
// phase clocks (shader clock) of the profiling instance, see potrf_leaf_profile; the production instance has none
template <bool PROF> struct LeafProf {};
template <> struct LeafProf<true> {
    unsigned long long* out = nullptr;               // ten slots, read by scripts/leaf_profile.py
    unsigned long long ta = 0, tb = 0, tc = 0, q0 = 0, q1 = 0, q2 = 0, q3 = 0, t = 0, u = 0;
    // the clock is a scalar read with no data dependence on the phase it closes: keep the compiler from moving it
    __device__ static unsigned long long now() {
        __builtin_amdgcn_sched_barrier(0);
        const unsigned long long t = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
        return t;
    }
    __device__ void stamp(int i) const { if (threadIdx.x == 0) out[i] = now(); }
};
template <bool PROF>
__global__ __launch_bounds__(LEAF_NT) void k_potrf_leaf(double* A, int lda, int n, double* Linv, int* errflag,
                                                    size_t bsA, size_t bsL, LeafProf<PROF> prof)
{
#pragma clang fp contract(fast)      // the factorisation is not part of the bit-exact RNG / leapfrog contract
    // blockIdx.x: one of several matrices factorised side by side (mvn_loglik_batch), each with its own flag
    A += (size_t)blockIdx.x * bsA; Linv += (size_t)blockIdx.x * bsL; errflag += blockIdx.x;
    if constexpr (PROF) prof.stamp(0);
    extern __shared__ __attribute__((aligned(16))) double S[];
    constexpr int LS = LEAF_LS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lk = lane >> 4;
    {   // load the lower triangle: thread = (row, column parity); 16 loads in flight per thread
        constexpr int JG = LEAF_NT / 128;
        const int i = tid & 127, j0 = tid >> 7;
        for (int jb = 0; jb < 128; jb += 16 * JG) {
            double v[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int j = jb + j0 + JG * q;
                v[q] = (i < n && j < n && i >= j) ? A[i + (size_t)j * lda] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) S[i * LS + jb + j0 + JG * q] = v[q];
        }
    }
    __syncthreads();
    const int ntile = (n + 15) >> 4;
    double* xd = S + LEAF_XD;
    double* Tt = S + LEAF_TT;
    double* dummy = S + LEAF_DUMMY;

    // block row I of the inverse (waves 1..7: wave w owns column tile J = w - 1)
    auto inverse_row = [&](int I) {
        const int J = wave - 1;
        if (J >= I) return;
        // T_J = sum_{K=J}^{I-1} L_IK X_KJ on the matrix cores
        d4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int K = J; K < I; ++K) {
#pragma unroll
            for (int kc = 0; kc < 4; ++kc) {
                const int t = kc * 4 + lk;
                // A operand: L_IK[row l15][t];  B operand: X_KJ[t][col l15]
                const double pa = S[(I * 16 + l15) * LS + K * 16 + t];
                double pb;
                if (K == J) pb = (t == l15) ? xd[J * 16 + l15] : (t > l15 ? S[(J * 16 + l15) * LS + J * 16 + t] : 0.0);
                else pb = S[(J * 16 + l15) * LS + K * 16 + t];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa, pb, acc, 0, 0, 0);
            }
        }
        // T_J[row][col]: row = lk + 4 r, col = l15 -> this wave's scratch tile
#pragma unroll
        for (int r = 0; r < 4; ++r) Tt[J * 256 + (lk + 4 * r) * 16 + l15] = acc[r];
        // X_IJ = -X_II T_J
        d4 acc2 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) {
            const int t = kc * 4 + lk;
            // A operand: X_II[row l15][t] (lower triangular);  B operand: T_J[t][col l15]
            const double pa = (t == l15) ? xd[I * 16 + l15]
                                         : (t < l15 ? S[(I * 16 + t) * LS + I * 16 + l15] : 0.0);
            const double pb = Tt[J * 256 + t * 16 + l15];
            acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(pa, pb, acc2, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gi = I * 16 + lk + 4 * r, gj = J * 16 + l15;
            if (gi < n) {
                S[gj * LS + gi] = -acc2[r];
                Linv[gi + gj * 128] = -acc2[r];
            }
        }
    };
    // trailing tile (ti, tj) -= P_ti P_tj' with the panel of step kb (K = 16), on the matrix cores
    auto upd_tile = [&](int ti, int tj, int kb) {
        const int ri = ti * 16, rj = tj * 16;
        d4 acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = S[(ri + lk + 4 * r) * LS + rj + l15];
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) {
            const double pa = -S[(ri + l15) * LS + kb + kc * 4 + lk];
            const double pb = S[(rj + l15) * LS + kb + kc * 4 + lk];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa, pb, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) S[(ri + lk + 4 * r) * LS + rj + l15] = acc[r];
    };
    // the tiles of step kt's trailing update that wave 0 does NOT do itself, shared out over waves 1..7
    auto rest_update = [&](int kt) {
        int cnt = 0;
        for (int tj = kt + 1; tj < ntile; ++tj)
            for (int ti = tj; ti < ntile; ++ti) {
                if (tj == kt + 1 && ti <= kt + 3) continue;            // wave 0's (P3)
                if (cnt % (LEAF_NW - 1) == wave - 1) upd_tile(ti, tj, kt * 16);
                ++cnt;
            }
    };

    for (int kt = 0; kt < ntile; ++kt) {
        const int kb = kt * 16;
        if constexpr (PROF) prof.t = prof.u = prof.now();
        if (wave == 0) {
            // P1: lane < 16 tile row kb + lane; 16..31 identity row lane - 16; 32..63 panel row kb + 16 + (lane - 32)
            const int prow = kb + 16 + (lane - 32);
            const bool pvalid = lane >= 32 && prow < ntile * 16;
            int bad = 0; double yv = 1.0;
            double a[16];
            if constexpr (PROF) prof.u = prof.now();
            // branch-free: one load per column from a clamped, always valid row; selects supply the identity
            // (padding rows of the tile, lanes 16-31) and zeros (padding rows of the panel)
            const int lrow = lane < 32 ? kb + l15 : (pvalid ? prow : 0);
            const bool ld_row = lane < 16 ? (kb + lane < n) : pvalid;
            const double* srow = S + lrow * LS + kb;
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                const double v = srow[c];
                const bool use = ld_row && (lane >= 32 || kb + c < n);
                a[c] = use ? v : ((lane < 32 && l15 == c) ? 1.0 : 0.0);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if constexpr (PROF) { prof.q0 += prof.now() - prof.u; prof.u = prof.now(); }
            potrf16_col<0>(a, lane, bad, yv);  potrf16_col<1>(a, lane, bad, yv);
            potrf16_col<2>(a, lane, bad, yv);  potrf16_col<3>(a, lane, bad, yv);
            potrf16_col<4>(a, lane, bad, yv);  potrf16_col<5>(a, lane, bad, yv);
            potrf16_col<6>(a, lane, bad, yv);  potrf16_col<7>(a, lane, bad, yv);
            potrf16_col<8>(a, lane, bad, yv);  potrf16_col<9>(a, lane, bad, yv);
            potrf16_col<10>(a, lane, bad, yv); potrf16_col<11>(a, lane, bad, yv);
            potrf16_col<12>(a, lane, bad, yv); potrf16_col<13>(a, lane, bad, yv);
            potrf16_col<14>(a, lane, bad, yv); potrf16_col<15>(a, lane, bad, yv);
            if constexpr (PROF) { prof.q1 += prof.now() - prof.u; prof.u = prof.now(); }
            // lanes 0-15 write row kb + l15 up to the diagonal (L), lanes 16-31 the SAME row above it (x[c] =
            // X_II[c][jj], c > jj: kept in the tile's upper part for the MFMA phases), lanes 32-63 their panel row.
            // Full leaves (n = 128) store through ADDRESS selects (a lane with nothing to store hits a dummy slot):
            // per-column exec masks cost this wave ~100 SGPRs, which spill, and the serial chain pays the reloads.
            double* drow = S + lrow * LS + kb;
            if (n == 128) {
                double* dmy = dummy + lane;
                double* w1 = (lane < 16 || pvalid) ? drow : nullptr;
#pragma unroll
                for (int c = 0; c < 16; ++c) *(w1 ? w1 + c : dmy) = a[c];          // rows, all 16 columns
                // then (LDS keeps a wave's accesses in order) the identity lanes overwrite the part above the diagonal
#pragma unroll
                for (int c = 0; c < 16; ++c) *((lk == 1 && c > l15) ? drow + c : dmy) = a[c];
                if (lane < 16) xd[kb + lane] = yv;         // reciprocal diagonal = the inverse's diagonal
                if (lk == 1) {
                    // the diagonal tile of the inverse is final: x[c] = X_II[c][jj] for c >= jj, exact zeros above
                    double* g = Linv + (kb + l15) * 128 + kb;
#pragma unroll
                    for (int c = 0; c < 16; ++c) g[c] = a[c];
                }
            } else {
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const bool st = lane < 16 ? (l15 >= c && kb + l15 < n && kb + c < n) : (lane < 32 ? c > l15 : pvalid);
                    if (st) drow[c] = a[c];
                }
                if (lane < 16) xd[kb + lane] = yv;
                if (lk == 1) {
                    double* g = Linv + (kb + l15) * 128 + kb;
#pragma unroll
                    for (int c = 0; c < 16; ++c)
                        if (c >= l15 && kb + c < n && kb + l15 < n) g[c] = a[c];
                }
            }
            if (bad && lane == 0) atomicExch(errflag, 1);
            if constexpr (PROF) { prof.q2 += prof.now() - prof.u; prof.u = prof.now(); }
        } else if (kt >= 1) {
            rest_update(kt - 1);
            inverse_row(kt - 1);
        }
        lds_barrier();
        if constexpr (PROF) {
            prof.q3 += prof.now() - prof.u;      // wave 0's wait at the barrier
            prof.ta += prof.now() - prof.t; prof.t = prof.now();
        }
        // P2: panel rows beyond the 32 that rode along: x = a inv(L11)' = a X_II' on the matrix cores
        for (int t = kt + 3 + wave; t < ntile; t += LEAF_NW) {
            const int r0 = t * 16;
            d4 acc = {0.0, 0.0, 0.0, 0.0};
            double pa[4], pb[4];
#pragma unroll
            for (int kc = 0; kc < 4; ++kc) {
                const int k = kc * 4 + lk;
                pa[kc] = S[(r0 + l15) * LS + kb + k];                      // a[i = l15][k]
                // B[k][j = l15] = X_II[j][k]
                pb[kc] = (l15 == k) ? xd[kb + k] : (l15 > k ? S[(kb + k) * LS + kb + l15] : 0.0);
            }
#pragma unroll
            for (int kc = 0; kc < 4; ++kc) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[kc], pb[kc], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) S[(r0 + lk + 4 * r) * LS + kb + l15] = acc[r];
        }
        lds_barrier();
        if constexpr (PROF) { prof.tb += prof.now() - prof.t; prof.t = prof.now(); }
        // P3: wave 0 updates what its next P1 reads and goes on without a barrier; the other waves pick up the
        // rest of this step's trailing update at the top of the next iteration
        if (wave == 0) {
            for (int ti = kt + 1; ti < ntile && ti <= kt + 3; ++ti) upd_tile(ti, kt + 1, kb);
            // the next P1 reads, one row per lane, what other lanes of this wave have just written: LDS executes a
            // wave's accesses in order; this keeps the compiler from moving them
            asm volatile("" ::: "memory");
        }
        if constexpr (PROF) prof.tc += prof.now() - prof.t;
    }
    lds_barrier();
    if constexpr (PROF) prof.stamp(5);
    {   // write L
        const int i = tid & 127, j0 = tid >> 7;
        if (i < n)
            for (int j = j0; j <= i && j < n; j += LEAF_NT / 128) A[i + (size_t)j * lda] = S[i * LS + j];
    }
    // the last block row of the inverse (the earlier ones were done under the later steps' P1)
    if (wave >= 1) inverse_row(ntile - 1);
    if constexpr (PROF) {
        prof.stamp(9);
        if (threadIdx.x == 0) {
            prof.out[1] = prof.q3; prof.out[2] = prof.ta; prof.out[3] = prof.tb; prof.out[4] = prof.tc;
            prof.out[6] = prof.q0; prof.out[7] = prof.q1; prof.out[8] = prof.q2;
        }
    }
}

// The K = 128 products of the blocked factorisation and of the blocked solve: deep-ring direct-to-LDS kernel
// (dgemm_dl.h) when its contract holds, the register-staged kernel otherwise (one matrix, no shifted lower-only
// update).
//   inplace: 0 none, 1 = C aliases A (N <= 128), 2 = C aliases B (M <= 128)
template <bool BNMAJOR>
static int chol_gemm(hipStream_t s, int M, int N, int K, const double* A, int lda, const double* B, int ldb,
                     const EpiAxpby& epi, bool lower_only, int tile, int inplace, int shift = 0, int nbatch = 1,
                     size_t bsA = 0, size_t bsB = 0)
{
    if (dl_applicable(M, N, K, A, lda, B, ldb, BNMAJOR))
        return launch_gemm_dl<BNMAJOR>(s, M, N, K, A, lda, B, ldb, epi, lower_only, tile, inplace, shift, nbatch, bsA, bsB);
    MCML_REQUIRE(nbatch == 1, "potrf: a batch of factorisations needs the LDS-DMA kernel for every panel product");
    MCML_REQUIRE(shift == 0 || !lower_only, "potrf: shifted lower-only update needs the LDS-DMA kernel");
    return launch_gemm<BNMAJOR>(s, M, N, K, A, lda, B, ldb, epi, lower_only, inplace ? inplace : -1);
}

// what every run of leaves needs first: room for the inverted diagonal blocks of `nbatch` n x n matrices, zeroed (the
// leaves write the lower triangles of their inverses only, k_potrf_leaf), and the leaf's LDS
int leaf_prepare(Ctx& c, int n, int nbatch)
{
    const size_t bytes = sizeof(double) * linv_size(n) * nbatch;
    MCML_TRY(c.chol.linv.ensure(bytes));
    MCML_HIP(hipMemsetAsync(c.chol.linv.p, 0, bytes, c.stream));
    return ensure_dynamic_lds(reinterpret_cast<const void*>(&k_potrf_leaf<false>), (int)POTRF_LDS);
}

// the launches and the step geometry both schedules of the factorisation (potrf_blocked, potrf_la2_capture) are made of
struct PotrfLaunch {
    Ctx& c; double* A; int lda; Bat bt; int* errflag;
    PotrfLaunch(Ctx& c_, double* A_, int lda_, const Bat& b)
        : c(c_), A(A_), lda(lda_), bt(b), errflag(b.err ? b.err : c_.errflag()) {}
    double* linv(int k) const { return c.chol.linv.d() + (size_t)(k / CHOL_NB) * CHOL_NB * CHOL_NB; }
    // factorise + invert the nb x nb diagonal block at (k, k)
    int leaf(hipStream_t s, int k, int nb) const {
        hipLaunchKernelGGL(k_potrf_leaf<false>, dim3(bt.n), dim3(LEAF_NT), POTRF_LDS, s, A + k + (size_t)k * lda, lda, nb,
                           linv(k), errflag, bt.sA, bt.sL, LeafProf<false>());
        MCML_HIP(hipGetLastError());
        return MCML_OK;
    }
    // C (M x N) = alpha A B' + beta C with B N-major, preferring the LDS-DMA kernel with a given tile
    int gemm_nt(hipStream_t s, int M, int N, int K, const double* Ap, const double* Bp, int ldb, double* Cp,
                double alpha, double beta, bool lower, int tile, int inplace, int shift) const {
        EpiAxpby epi{Cp, lda, alpha, beta, bt.sA};
        const size_t sB = (ldb == CHOL_NB) ? bt.sL : bt.sA;            // B is an inverted diagonal block, or part of the matrix
        return chol_gemm<true>(s, M, N, K, Ap, lda, Bp, ldb, epi, lower, tile, inplace, shift, bt.n, bt.sA, sB);
    }
    // Step t of an n x n factorisation with `extra` rows carried below: the panel's first column k and width nb, the
    // rem columns right of it, the R rows below its diagonal block A11 (R <= 0: nothing left to do), the R x nb panel
    // A21 there, the nb2 rows of the next diagonal block (0 at the end), and the inverse leaf(k) left of A11.
    struct Step { int k, nb, rem, R, nb2; double *A11, *A21; const double* Linv; };
    Step step(int t, int n, int extra) const {
        const int k = t * CHOL_NB, nb = (n - k < CHOL_NB) ? n - k : CHOL_NB, rem = n - k - nb;
        double* A11 = A + k + (size_t)k * lda;
        return Step{k, nb, rem, rem + extra, rem < CHOL_NB ? rem : CHOL_NB, A11, A11 + nb, linv(k)};
    }
};

// side streams + events of the look-ahead (potrf_blocked) and of the captured schedule (potrf_la2_capture)
static int lookahead_setup(Ctx& c)
{
    if (c.chol.aux) return MCML_OK;
    int lo = 0, hi = 0;
    MCML_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
    MCML_HIP(hipStreamCreateWithPriority(&c.chol.aux, hipStreamNonBlocking, hi));
    MCML_HIP(hipStreamCreateWithPriority(&c.chol.aux_lo, hipStreamNonBlocking, lo));
    MCML_HIP(hipEventCreateWithFlags(&c.chol.ev_col, hipEventDisableTiming));
    MCML_HIP(hipEventCreateWithFlags(&c.chol.ev_leaf, hipEventDisableTiming));
    return MCML_OK;
}

// Right-looking blocked Cholesky of the n x n lower triangle of A, 128-wide panels -- leaf (factor + invert the
// diagonal block in LDS), panel TRSM as a GEMM against the inverted block, SYRK of the trailing matrix -- with `extra`
// more ROWS carried below the matrix (rows n .. n+extra of the same column-major array): they receive every panel
// operation the rows of the matrix receive, i.e. X <- X inv(L)'.  With X = U' (the sample columns, one per
// extra row) that is the forward substitution inv(L) U of mvn_ll, done inside the factorisation's own GEMMs
// -- no separate TRSM pass, and the late panels, whose trailing matrices are tiny, still fill the chip.
//
// Look-ahead (the leaf is a single-workgroup, latency-bound kernel and the late panels' GEMMs are small: back to back
// they leave the chip idle most of the time).  Step t, on the main stream: the ONE 128 x 128 panel block that becomes the next diagonal block's multiplier
// and that block's own update (two single-block products spread over 8 / 16 CUs); then, forked to a
// high-priority side stream, leaf(t+1) -- while the main stream runs the bulk: the rest of panel t and the
// whole trailing update except that block, one launch, lower tiles only, balanced over the XCDs.  The leaf
// (ONE workgroup that needs a whole CU's LDS) becomes ready together with the bulk and is dispatched first, so
// it never waits for a CU to drain.  The main stream joins the leaf before step t+1.  Period: two small GEMMs
// + max(bulk, leaf).  (A freer two-queue schedule measured ~10 % faster live but
// hung intermittently; it exists as a captured graph only -- see "the hang" above potrf_la2_capture.)
int potrf_blocked(Ctx& c, double* A, int lda, int n, int extra, Bat bt)
{
    const PotrfLaunch L(c, A, lda, bt);
    const bool two = n > 2 * CHOL_NB;
    hipStream_t sM = c.stream, sL = c.stream;
    if (two) { MCML_TRY(lookahead_setup(c)); sL = c.chol.aux; }
    const int nsteps = (n + CHOL_NB - 1) / CHOL_NB;
    constexpr int SPW = CHOL_NB * 8;                              // super-panel width: 8 panels
    // decided by the ROUND the matrices come from, not by how many of its candidates are factorised: a round whose
    // candidates share a factorisation (theta_scale.h) keeps the regrouped sums of the full round, so a candidate's
    // value does not depend on which of its neighbours happened to need a matrix of their own
    const bool twolevel = (bt.round ? bt.round : bt.n) > 1 && n > SPW + CHOL_NB;
    MCML_TRY(L.leaf(sM, 0, n < CHOL_NB ? n : CHOL_NB));
    bool forked = false;
    for (int t = 0; t < nsteps; ++t) {
        const PotrfLaunch::Step s = L.step(t, n, extra);
        const int k = s.k, nb = s.nb, rem = s.rem, R = s.R, nb2 = s.nb2;
        if (R <= 0) break;
        if (forked) { MCML_HIP(hipStreamWaitEvent(sM, c.chol.ev_leaf, 0)); forked = false; }   // leaf(t) done
        // Two levels of blocking for a BATCH (a round of more than one candidate), whose rounds are bound by the trailing updates, not by the chain:
        // inside a super-panel of 8 panels the K = 128 updates touch the super-panel's own columns only; the columns to
        // its right receive all eight panels in ONE pass with K = 1024 when the super-panel is done (the same LDS-DMA
        // kernel: 48 against 35 TF on the trailing update of a 4000 x 4000 block, scripts/dl_k_sweep.py) -- five
        // read-modify-write passes over the trailing matrix at Q = 5000 instead of forty.  The sums are regrouped, so a
        // batched value equals the single evaluation to rounding (1e-13), not to the bit.
        const int sp0 = twolevel ? (k / SPW) * SPW : 0, sp1 = twolevel ? (sp0 + SPW < n ? sp0 + SPW : n) : n;
        const int inner = sp1 - (k + nb);                         // trailing columns this step's K = 128 update covers
        if (twolevel && inner == 0 && rem > 0) {
            // last panel of a super-panel: the whole panel, then everything to the right in one pass, then the next leaf
            MCML_TRY(L.gemm_nt(sM, R, nb, nb, s.A21, s.Linv, CHOL_NB, s.A21, 1.0, 0.0, false, 0, 1, 0));
            const double* Asp = A + sp1 + (size_t)sp0 * lda;      // rows below the super-panel, its columns
            double* Csp = A + sp1 + (size_t)sp1 * lda;
            MCML_TRY(L.gemm_nt(sM, R, rem, sp1 - sp0, Asp, Asp, lda, Csp, -1.0, 1.0, true, 0, 0, 0));
            MCML_TRY(L.leaf(sM, k + nb, nb2));
            continue;
        }
        if (nb2 > 0) {
            // the next diagonal block: its multiplier, its update, its factorisation
            MCML_TRY(L.gemm_nt(sM, nb2, nb, nb, s.A21, s.Linv, CHOL_NB, s.A21, 1.0, 0.0, false, 7, 1, 0));
            double* T = s.A11 + nb + (size_t)nb * lda;
            MCML_TRY(L.gemm_nt(sM, nb2, nb2, nb, s.A21, s.A21, lda, T, -1.0, 1.0, false, 8, 0, 0));
            if (two) {
                MCML_HIP(hipEventRecord(c.chol.ev_col, sM));
                MCML_HIP(hipStreamWaitEvent(sL, c.chol.ev_col, 0));
            }
            MCML_TRY(L.leaf(sL, k + nb, nb2));
            if (two) { MCML_HIP(hipEventRecord(c.chol.ev_leaf, sL)); forked = true; }
        }
        // the bulk: the rest of the panel, then the whole trailing update except the block above
        if (R - nb2 > 0)
            MCML_TRY(L.gemm_nt(sM, R - nb2, nb, nb, s.A21 + nb2, s.Linv, CHOL_NB, s.A21 + nb2, 1.0, 0.0, false, 0, 1, 0));
        if (rem > 0 && R - nb2 > 0) {
            double* C2 = s.A11 + nb + nb2 + (size_t)nb * lda;     // rows nb2.. of the trailing matrix, all its columns
            MCML_TRY(L.gemm_nt(sM, R - nb2, twolevel ? inner : rem, nb, s.A21 + nb2, s.A21, lda, C2, -1.0, 1.0, true, 0, 0, nb2));
        }
    }
    if (forked) MCML_HIP(hipStreamWaitEvent(sM, c.chol.ev_leaf, 0));
    return MCML_OK;
}

// The dependency structure the GRAPH is captured with (never launched eagerly, see "the hang" below).
// Two chains that only meet through events:
//   critical (capture stream):  P_small(t)  the 128 x 128 panel block under the diagonal block, X <- X inv(L_t)'
//                               U_small(t)  D_{t+1} -= X X'
//                               leaf(t+1)
//   bulk (side stream):         a(t)  the rest of panel t                       (needs leaf(t))
//                               b(t)  column blocks t+1 AND t+2, rows below block t+1, -= panel t   (needs P_small(t))
//                               c(t)  column blocks t+3.., lower tiles only, -= panel t
// P_small(t+1) / U_small(t+1) touch block (t+2, t+1) and D_{t+2}: both were brought up to date by b(t), so the
// critical chain waits for b(t) and never for the big update c(t) OF THE SAME STEP.  It is not independent of the big
// updates: b(t) sits behind c(t-1) on the bulk queue (and must: column block t+2 was last written by c(t-1)), so the
// critical chain has one step of slack against the bulk chain, which is what the early, throughput-bound steps use up;
// in the late steps the bulk chain runs ahead and the three critical kernels sit back to back on one queue.
// Every tile still receives its updates in panel order from kernels that accumulate k = 0..127 in order, launched by
// the same PotrfLaunch from the same step geometry: the factor is bit-identical to potrf_blocked's.
//
// The hang (round 2: this structure as two LIVE streams, cross waits both ways, hung the process -- not the GPU -- on
// three of ~20 boxes; no log of it was kept).  What the code says: the dependency structure is acyclic if every
// hipStreamWaitEvent binds to the event's record AT THE TIME OF THE CALL, which is what HIP documents (CUDA's
// semantics) and what a capture does by construction -- the same structure has replayed > 27 000 times as a graph.
// The live version re-recorded the SAME four events every step while the other stream could still hold a pending
// wait on the previous record.  If the runtime ever resolves such a wait against the event's LATEST record instead,
// the bulk stream's wait for leaf(t+1) can land on leaf(t+2), which waits (through P_small(t+2)) for b(t+1) on the
// bulk stream behind that very wait: a cycle, and a host thread blocked in the next enqueue on a full queue -- the
// observed symptom.  That reading cannot be proved without the runtime's source; what is done instead is to remove
// the question: every dependency edge below has ITS OWN event (a ring, never re-recorded within a capture), so no wait
// can be bound to anything but the one record it was written for, and live launches keep the fork-join of
// potrf_blocked, whose waits always follow the record they mean on the same host thread with no later record pending.
// If the two-chain schedule is ever wanted live again, it must use the same ring.
static hipEvent_t ring_event(Ctx& c, size_t idx)
{
    while (c.chol.ev_ring.size() <= idx) {
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
        c.chol.ev_ring.push_back(e);
    }
    return c.chol.ev_ring[idx];
}
static int potrf_la2_capture(Ctx& c, double* A, int lda, int n, int extra, Bat bt = Bat())
{
    const PotrfLaunch L(c, A, lda, bt);
    hipStream_t sC = c.stream, sB = c.chol.aux_lo;
    const int nsteps = (n + CHOL_NB - 1) / CHOL_NB;
    // one event per dependency edge: 3 per step (leaf, P_small, b) + the first leaf + the join
    auto EV = [&](int step, int kind) -> hipEvent_t { return ring_event(c, (size_t)3 * (step + 1) + kind); };
    MCML_REQUIRE(ring_event(c, (size_t)3 * (nsteps + 2)) != nullptr, "potrf: could not create the capture's events");
    MCML_TRY(L.leaf(sC, 0, n < CHOL_NB ? n : CHOL_NB));
    MCML_HIP(hipEventRecord(EV(-1, 0), sC));
    MCML_HIP(hipStreamWaitEvent(sB, EV(-1, 0), 0));                  // the side stream joins the capture; a(0) needs leaf(0)
    hipEvent_t last_b = nullptr;
    for (int t = 0; t < nsteps; ++t) {
        const PotrfLaunch::Step s = L.step(t, n, extra);
        const int k = s.k, nb = s.nb, rem = s.rem, R = s.R, nb2 = s.nb2;
        if (R <= 0) break;
        const int nb3 = (rem - nb2 < CHOL_NB) ? rem - nb2 : CHOL_NB;
        const int w = nb2 + nb3;                                      // columns b(t) covers
        // ---- critical chain
        if (nb2 > 0) {
            if (last_b) MCML_HIP(hipStreamWaitEvent(sC, last_b, 0));  // b(t-1)
            MCML_TRY(L.gemm_nt(sC, nb2, nb, nb, s.A21, s.Linv, CHOL_NB, s.A21, 1.0, 0.0, false, 7, 1, 0));
            double* T = s.A11 + nb + (size_t)nb * lda;
            MCML_TRY(L.gemm_nt(sC, nb2, nb2, nb, s.A21, s.A21, lda, T, -1.0, 1.0, false, 8, 0, 0));
            MCML_HIP(hipEventRecord(EV(t, 1), sC));
            MCML_TRY(L.leaf(sC, k + nb, nb2));
            MCML_HIP(hipEventRecord(EV(t, 0), sC));
        }
        // ---- bulk chain
        const int Rb = R - nb2;
        if (Rb > 0) {
            MCML_TRY(L.gemm_nt(sB, Rb, nb, nb, s.A21 + nb2, s.Linv, CHOL_NB, s.A21 + nb2, 1.0, 0.0, false, 0, 1, 0));
            if (nb2 > 0) {
                MCML_HIP(hipStreamWaitEvent(sB, EV(t, 1), 0));
                double* Cb = s.A11 + nb + nb2 + (size_t)nb * lda;     // rows below block t+1, columns of blocks t+1, t+2
                MCML_TRY(L.gemm_nt(sB, Rb, w, nb, s.A21 + nb2, s.A21, lda, Cb, -1.0, 1.0, false, 0, 0, 0));
                MCML_HIP(hipEventRecord(EV(t, 2), sB));
                last_b = EV(t, 2);
                if (rem - w > 0) {
                    double* Cc = s.A11 + nb + w + (size_t)(nb + w) * lda;
                    MCML_TRY(L.gemm_nt(sB, R - w, rem - w, nb, s.A21 + w, s.A21 + w, lda, Cc, -1.0, 1.0, true, 0, 0, 0));
                }
            }
        } else if (nb2 > 0) {
            MCML_HIP(hipStreamWaitEvent(sB, EV(t, 1), 0));            // keep the side stream a descendant of every node
            MCML_HIP(hipEventRecord(EV(t, 2), sB));
            last_b = EV(t, 2);
        }
        if (nb2 > 0) MCML_HIP(hipStreamWaitEvent(sB, EV(t, 0), 0));   // a(t+1) needs leaf(t+1)
    }
    MCML_HIP(hipEventRecord(EV(nsteps, 0), sB));                      // join
    MCML_HIP(hipStreamWaitEvent(sC, EV(nsteps, 0), 0));
    return MCML_OK;
}

// The same factorisation replayed as a hipGraph.  A theta-step evaluates one (matrix, shape) 40 times per MCML
// iteration and every evaluation is ~200 launches, ~80 event operations and the host calls behind them: the first
// call with a given key runs eagerly (function attributes, allocations), the second is captured (fork / join of the
// look-ahead included: the side stream joins the capture through its event waits), later ones are one hipGraphLaunch.
// The capture records potrf_la2_capture; GLMMR_MCML_CHOL_GRAPH=0 keeps the eager launches of potrf_blocked.
// Single evaluations only (bt.n == 1): a batch runs potrf_blocked eagerly, see mvn_large_blocks.
static bool chol_graph_on()
{
    static const bool on = !(getenv("GLMMR_MCML_CHOL_GRAPH") && !strcmp(getenv("GLMMR_MCML_CHOL_GRAPH"), "0"));
    return on;
}
static bool graph_timer_begin(Ctx& c, CholGraph& g)
{
    if (!g.t0 && (hipEventCreate(&g.t0) != hipSuccess || hipEventCreate(&g.t1) != hipSuccess)) { (void)hipGetLastError(); return false; }
    return hipEventRecord(g.t0, c.stream) == hipSuccess;
}
// Calibration of a fresh executable (see CholGraph): the previous replay's time is known by now -- every caller
// synchronises for its result -- and an executable slower than the eager launches is instantiated again.
static void calibrate(CholGraph& g)
{
    float ms = 0.f;
    g.timed = false;
    bool done = true;
    const hipError_t ee = hipEventElapsedTime(&ms, g.t0, g.t1);
    static const bool cal_trace = getenv("GLMMR_MCML_GRAPH_TRACE") != nullptr;
    if (cal_trace) fprintf(stderr, "graph calibration: n=%d extra=%d trial %d: %.3f ms (eager %.3f, best %.3f) rc=%d\n", g.n, g.extra, g.tries, ms, g.eager_ms, g.best_ms, (int)ee);
    if (ee == hipSuccess && g.eager_ms > 0.f && g.tmpl) {
        // keep the fastest executable seen; try another instantiation unless this one clearly beats the eager
        // launches or four have been tried
        if (!g.best || ms < g.best_ms) {
            if (g.best && g.best != g.exec) (void)hipGraphExecDestroy(g.best);
            g.best = g.exec; g.best_ms = ms;
        } else if (g.exec != g.best) (void)hipGraphExecDestroy(g.exec);
        g.exec = g.best;
        if (!(g.best_ms <= 0.93f * g.eager_ms) && g.tries < 3) {
            hipGraphExec_t ex2 = nullptr;
            if (hipGraphInstantiate(&ex2, g.tmpl, nullptr, nullptr, 0) == hipSuccess) { g.exec = ex2; ++g.tries; g.trial_launches = 0; done = false; }
            else (void)hipGetLastError();
        }
    } else (void)hipGetLastError();
    if (done) {
        g.settled = true; g.best = nullptr;
        if (g.tmpl) { (void)hipGraphDestroy(g.tmpl); g.tmpl = nullptr; }
    }
}
// Records potrf_la2_capture and instantiates it into g.exec, ready for calibration.  Whatever goes wrong while
// recording (nothing has run; e.g. the legacy default stream cannot be captured) leaves g.exec null.
static int capture_and_instantiate(Ctx& c, CholGraph& g, double* A, int lda, int n, int extra, const Bat& bt)
{
    MCML_TRY(lookahead_setup(c));
    if (hipStreamBeginCapture(c.stream, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); return MCML_OK; }
    const int rc = potrf_la2_capture(c, A, lda, n, extra, bt);
    hipGraph_t graph = nullptr;
    const hipError_t e = hipStreamEndCapture(c.stream, &graph);
    if (rc != MCML_OK || e != hipSuccess || !graph || hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0) != hipSuccess) {
        if (graph) (void)hipGraphDestroy(graph);
        (void)hipGetLastError();
        g.exec = nullptr;
        return MCML_OK;
    }
    g.tmpl = graph; g.tries = 0; g.settled = !(g.eager_ms > 0.f); g.timed = false; g.best = nullptr; g.best_ms = 0.f;
    if (g.settled) { (void)hipGraphDestroy(g.tmpl); g.tmpl = nullptr; }
    return MCML_OK;
}
// no graph for this key: the capture is never tried again
static void eager_for_good(CholGraph& g) { g.seen = -(1 << 30); }

int potrf_graphed(Ctx& c, double* A, int lda, int n, int extra, Bat bt)
{
    if (!chol_graph_on() || n <= 2 * CHOL_NB) return potrf_blocked(c, A, lda, n, extra, bt);
    CholGraph& g = c.chol.graphs.find(A, c.chol.linv.d(), lda, n, extra);
    if (g.exec) {
        if (!g.settled && g.timed) calibrate(g);
        const bool tm = !g.settled && g.trial_launches >= 1 && graph_timer_begin(c, g);
        MCML_HIP(hipGraphLaunch(g.exec, c.stream));
        if (tm) g.timed = hipEventRecord(g.t1, c.stream) == hipSuccess;
        ++g.trial_launches;
        return MCML_OK;
    }
    if (g.seen++ <= 1) {   // eager twice first (attributes, allocations): the second run's time is the calibration's yardstick
        const bool tm = graph_timer_begin(c, g);
        MCML_TRY(potrf_blocked(c, A, lda, n, extra, bt));
        if (tm && hipEventRecord(g.t1, c.stream) == hipSuccess && hipEventSynchronize(g.t1) == hipSuccess)
            (void)hipEventElapsedTime(&g.eager_ms, g.t0, g.t1);
        (void)hipGetLastError();
        return MCML_OK;
    }
    MCML_TRY(capture_and_instantiate(c, g, A, lda, n, extra, bt));
    if (!g.exec) {         // eager launches from now on, the error if that fails too
        eager_for_good(g);
        return potrf_blocked(c, A, lda, n, extra, bt);
    }
    g.trial_launches = 1;                     // this first launch is not timed (it carries the executable's upload)
    MCML_HIP(hipGraphLaunch(g.exec, c.stream));
    return MCML_OK;
}

// In-place factorisation of the lower triangle of A.  The strict upper triangle is never read, by this or by the solves
// below (the leaf loads i >= j only, every operand panel lies below a diagonal block, a diagonal tile's update rewrites its own
// upper half from itself): it may hold anything, NaN included, and comes back changed (tests/test_gpu_chol_solve.py).
int potrf_lower(Ctx& c, double* A, int n, int lda)
{
    MCML_REQUIRE(n > 0 && lda >= n && (lda & 1) == 0, "potrf: bad shape n=%d lda=%d", n, lda);
    MCML_TRY(leaf_prepare(c, n, 1));
    return potrf_blocked(c, A, lda, n, 0);
}

// debug: phase timestamps (shader clock) of one 128 x 128 leaf on a random SPD block, from the kernel's profiling instance
int potrf_leaf_profile(Ctx& c, unsigned long long* host10)
{
    DevMat A; DevBuf prof;
    MCML_TRY(A.alloc(128, 128));
    MCML_TRY(prof.ensure(80));
    std::vector<double> h((size_t)A.ld * 128, 0.0);
    for (int j = 0; j < 128; ++j) for (int i = 0; i < 128; ++i) h[i + (size_t)j * A.ld] = (i == j ? 130.0 : 1.0 / (1 + abs(i - j)));
    MCML_TRY(leaf_prepare(c, 128, 1));
    MCML_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(&k_potrf_leaf<true>), (int)POTRF_LDS));
    LeafProf<true> lp;
    lp.out = prof.as<unsigned long long>();
    for (int rep = 0; rep < 3; ++rep) {
        MCML_TRY(copy_h2d(A.d(), h.data(), sizeof(double) * h.size(), 0)); MCML_HIP(hipDeviceSynchronize());
        hipLaunchKernelGGL(k_potrf_leaf<true>, dim3(1), dim3(LEAF_NT), POTRF_LDS, c.stream, A.d(), A.ld, 128, c.chol.linv.d(),
                           c.errflag(), (size_t)0, (size_t)0, lp);
        MCML_HIP(hipStreamSynchronize(c.stream));
    }
    MCML_HIP(hipMemcpy(host10, prof.p, 80, hipMemcpyDeviceToHost));
    return MCML_OK;
}

// U (n x m) <- inv(L) U, L lower n x n; needs the leaf inverses potrf_lower left in c.chol.linv.  Panel by panel: the
// diagonal block against its inverse, then the rows below -= L21 U_k with K = 128 (a recursive variant with long-K
// updates measured 3-15 % slower at Q = 5000, m = 1024, and was removed)
int trsm_left_lower(Ctx& c, const double* L, int ldl, int n, double* U, int ldu, int m)
{
    for (int k = 0; k < n; k += CHOL_NB) {
        const int nb = (n - k < CHOL_NB) ? n - k : CHOL_NB;
        const double* Linv = c.chol.linv.d() + (size_t)(k / CHOL_NB) * CHOL_NB * CHOL_NB;
        double* Uk = U + k;
        {
            EpiAxpby epi{Uk, ldu, 1.0, 0.0};
            MCML_TRY(chol_gemm<false>(c.stream, nb, m, nb, Linv, CHOL_NB, Uk, ldu, epi, false, 0, 2));
        }
        const int rem = n - k - nb;
        if (rem <= 0) break;
        const double* L21 = L + (k + nb) + (size_t)k * ldl;
        EpiAxpby epi{Uk + nb, ldu, -1.0, 1.0};
        MCML_TRY(chol_gemm<false>(c.stream, rem, m, nb, L21, ldl, Uk, ldu, epi, false, 0, 0));
    }
    return MCML_OK;
}

// T (n x m) <- inv(R)' T, R lower n x n; needs the leaf inverses potrf_lower left in c.chol.linv.  Panels from the last to the
// first: the diagonal block against its inverse transposed, then the rows above -= R21' T_k with K = nb <= 128.  Both
// products read their A operand transposed in place (dgemm_mfma.h ATRANS: A(i, p) = R[k + p, i] is K-contiguous), so no
// transposed copy of the factor is made.  A column of R and of T is read up to row round_up(n, 2) - 1.
int trsm_left_lower_trans(Ctx& c, const double* R, int ldr, int n, double* T, int ldt, int m)
{
    MCML_REQUIRE(R && T && n > 0 && m > 0, "trsm_left_lower_trans: empty operand");
    MCML_REQUIRE(ldr >= n + (n & 1) && ldt >= n + (n & 1) && (ldr & 1) == 0 && (ldt & 1) == 0,
                 "trsm_left_lower_trans: bad leading dimensions %d, %d for n = %d", ldr, ldt, n);
    MCML_REQUIRE(c.chol.linv.bytes >= sizeof(double) * linv_size(n), "trsm_left_lower_trans: no factorisation of this size before it");
    for (int k = (n - 1) / CHOL_NB * CHOL_NB; k >= 0; k -= CHOL_NB) {
        const int nb = (n - k < CHOL_NB) ? n - k : CHOL_NB;
        const double* Linv = c.chol.linv.d() + (size_t)(k / CHOL_NB) * CHOL_NB * CHOL_NB;
        double* Tk = T + k;
        {
            EpiAxpby epi{Tk, ldt, 1.0, 0.0};               // in place: one 128-row tile holds all of T_k's rows (tile 2)
            MCML_TRY(launch_gemm_at(c.stream, nb, m, nb, Linv, CHOL_NB, Tk, ldt, epi, 2));
        }
        if (k == 0) break;
        EpiAxpby epi{T, ldt, -1.0, 1.0};
        MCML_TRY(launch_gemm_at(c.stream, k, m, nb, R + k, ldr, Tk, ldt, epi));
    }
    return MCML_OK;
}

int check_errflag(Ctx& c, const char* message)
{
    int flag = 0;
    MCML_TRY(copy_d2h(&flag, c.errflag(), sizeof(int), c.stream));
    MCML_HIP(hipStreamSynchronize(c.stream));
    if (flag) {
        MCML_HIP(hipMemsetAsync(c.errflag(), 0, sizeof(int), c.stream));
        set_error("%s", message);
        return MCML_ENOTPD;
    }
    return MCML_OK;
}

int potrf_lower_checked(Ctx& c, double* A, int n, int lda)
{
    MCML_TRY(potrf_lower(c, A, n, lda));
    return check_errflag(c, "potrf: covariance block is not positive definite");
}

// x <- L'^-1 (L^-1 x): forward solve through the blocked TRSM (one right-hand side), backward
// solve block by block with the inverted diagonal blocks potrf_lower left in c.chol.linv
int potrs_lower_vec(Ctx& c, const double* L, int ldl, int n, double* x, double* tmp)
{
    MCML_TRY(trsm_left_lower(c, L, ldl, n, x, pad_ld(n), 1));
    const int nblk = (n + CHOL_NB - 1) / CHOL_NB;
    for (int kb = nblk - 1; kb >= 0; --kb) {
        const int k0 = kb * CHOL_NB, nb = (n - k0 < CHOL_NB) ? n - k0 : CHOL_NB;
        const double* Linv = c.chol.linv.d() + (size_t)kb * CHOL_NB * CHOL_NB;
        MCML_TRY(dev_gemv_t(c, Linv, CHOL_NB, nb, nb, x + k0, tmp, 1.0, 0.0));
        MCML_TRY(dev_copy(c, x + k0, tmp, nb));
        if (k0 > 0) MCML_TRY(dev_gemv_t(c, L + k0, ldl, nb, k0, x + k0, x, -1.0, 1.0));
    }
    return MCML_OK;
}

}  // namespace mcml
