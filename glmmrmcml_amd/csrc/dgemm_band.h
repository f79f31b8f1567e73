// dgemm_band.h -- the HMC products with structural-zero skipping, any number of chains.
//
// For the geospatial designs Z = I, so ZL = L is lower triangular (and ZL' upper): half of
// the K tiles a dense GEMM multiplies are exactly zero.  More generally, whenever the rows of
// ZL (or ZL') touch only a range of columns, the products outside that range contribute
// nothing.  When L is refreshed, k_band_ranges records for every 80-row band of the A operand
// the first and last K tile that holds a nonzero; the kernel runs each band's K loop over that
// range only.  Skipping exact zeros does not change any sum (0*x adds nothing for finite x).
// Inside that range the operand is still ragged at the granularity of an MFMA (a triangle's diagonal crosses the last
// 2.5 - 3 K tiles of a band, the last band may have fewer than 80 rows, K is padded to a multiple of 32): the same scan
// records per 16-row tile of a band the K substeps (4 columns = one v_mfma_f64_16x16x4) between its first and last nonzero
// (the row-tile extents, band_plan.h).  K tiles that every row tile's extent covers whole are INTERIOR and run the plain
// tile body; the others are EDGE tiles: same LDS reads, waits and barrier, but the MFMA of row tile i in substep s is
// issued only inside the extent -- a scalar branch per row tile and substep in the MFMA waves.  An item's K loop is three
// loops in a row, edge / interior / edge; fill, DMA, barriers, ring and epilogues do not know about it.
// GLMMR_MCML_BAND_ROWTILES=0: no extents, every tile interior.
//
// Work decomposition (BandPlan, built on the host per number of column tiles):
//   * whole bands (BandPlanDev::paired): a workgroup owns a group of whole bands of one column
//     tile, back to back.  The launch is one wave of workgroups, as long as its costliest group,
//     so the bands are dealt costliest first into the least loaded of 256 / (column tiles) groups:
//     63 bands x 8 column tiles -> 32 x 8 = 256 workgroups (one per CU) for the 5000 x 1024
//     products, the longest of them 158 K steps forward and 157 backward, the mean rounded up
//     (band p with its mirror nbands-1-p, the earlier rule: 161 and 160, because the 80-row
//     bands' K ranges round up to whole 32-wide tiles and the last band has 40 rows).  A group
//     holds one, two, three or more bands.  No partial sums, every band one ordered K loop.
//   * streamed (few column tiles: a rank of the chain-sharded job holds 1024/8 = 128 chains = ONE
//     column tile, which whole bands would run on 32 of the 256 CUs): the (band, K tile) iteration
//     space of a column tile is flattened and cut into equal runs of K tiles, one run per
//     workgroup, ~256 workgroups in all.  A run may end one band and start the next.  A band
//     covered by one run is finished by that workgroup; a band cut into several pieces has each
//     piece stored as a raw accumulator tile (in register order: 512-byte coalesced stores) and
//     k_band_reduce sums the pieces IN K ORDER and applies the same epilogue functor -- a
//     fixed-order two-stage reduction, bit-reproducible for a given (operand, chain count).
//     (Measured dead end, round 3: folding the second stage into the piece that ARRIVES LAST -- write-through
//     (sc1) tile stores, one relaxed agent-scope counter per band, sc1 loads by the last arriver -- is correct
//     (parity suite green) but no faster: 80.4 / 82.7 us against 76.7 / 82.4 us per forward / backward product at
//     n = 5000 with 128 chains, 44.5 / 47.9 against 39.2 / 41.7 us at n = 2000 with 256 -- one workgroup per band
//     reads up to eight 80 KB pieces back from memory in dependent batches, where this kernel spreads a band
//     over four workgroups and finds the pieces in L2.  With agent-scope release / acquire fences instead of
//     write-through stores every wave issues a buffer_wbl2, a walk over the XCD's whole L2: 160 us per product.)
//
// One pipeline (band_walk), the direct-to-LDS machinery of dgemm_dlds.h: 80 x 128 tile, 512 threads, K step 32,
// 3-stage LDS ring (156 KB), counted vmcnt + raw barriers.  The A image [k][80 doubles] has 640-byte rows = 32 banks
// mod 64, so the two 16-lane halves of a ds_read_b64 (rows k, k+1) are conflict-free without a swizzle.  A wave of
// the pipeline has up to two jobs: it FILLS the ring -- a BandFill issues every STRIDE-th of the 52 one-KiB LDS-DMA
// pieces of a stage and keeps the counted vmcnt -- and it MULTIPLIES, NS 80 x 16 strips of the tile (5 x NS
// v_mfma_f64_16x16x4 tiles per K substep, operands read from LDS by hand-scheduled ds_reads, the reads of substep
// s + 1 issued between the MFMAs of substep s and the next tile's first reads between those of the last substep,
// behind the barrier: profiles/band_kloop_codegen.txt has the compiled loops).  All waves walk the
// same item list and pass the same barriers.  Two kernels instantiate it:
//   * dgemm_band_kernel, the 8-wave form: every wave does both, pieces wave, wave + 8, ... (7 per tile) and strip
//     `wave` (NS = 1).  Its waves issue their pieces back to back at the top of a K tile, and a wave inside that
//     block issues no MFMA (waves issue in order); the two waves of a SIMD are there together.
//   * dgemm_band_feed_kernel, the feeder form (what the sampler runs where its instantiation needs no scratch):
//     waves 4-7 only fill, 13 pieces each per tile, and run no epilogue, so the next item's first ring stages are in
//     flight while the MFMA waves are still in theirs; waves 0-3 (their SIMD partners) only multiply, strips 2 wave
//     and 2 wave + 1 (NS = 2), with NO vector-memory instruction and no vmcnt wait inside a K loop -- their
//     epilogue's stores drain under the next item's K loop.
// Every output element is accumulated by one wave, over K in the same order, by the same instruction with the same
// operand roles, and the epilogue functor is called once per 16-column strip in both: same bits from both.
// Selected per epilogue type (BandFeed<Epi>::ok: instantiations that compile without scratch);
// GLMMR_MCML_BAND_FEED=0 keeps the 8-wave form everywhere.
#pragma once
#include "dgemm_dlds.h"
#include "band_plan.h"

namespace mcml {

struct BandP {
    GemmP g;
    const BandItem* items;
    const int* wg_ptr;     // items of workgroup w (of any column tile): [wg_ptr[w], wg_ptr[w+1])
    const int* ext;        // row-tile extents, BD_EXT ints per band; null: every K tile is multiplied whole
    int nwg;               // workgroups per column tile
    double* part;          // partial tiles: [(slot * gn + column tile) * BD_TILE_ELEMS]
    int mode;              // DBG kernels only -- bit 16: per-workgroup phase stamps into clocks[8 ..]
    unsigned long long* clocks;   // DBG kernels only (nullable): workgroup 0 adds its shader-clock and 100 MHz real-time ticks
};

// first / last nonzero K tile of every 80-row band of A (M x K, column-major) -> krange, 2 ints per band, and of the
// same scan the first / one-past-last nonzero K substep (4 columns) of each of the band's five 16-row tiles -> ext,
// BD_EXT ints per band (band_plan.h; a row tile without a nonzero, or past M: s0 = s1 = 0)
static __global__ __launch_bounds__(256) void k_band_ranges(const double* A, int lda, int M, int K, int* krange, int* ext)
{
    __shared__ int smin[BD_RT][256], smax[BD_RT][256];
    const int band = blockIdx.x, r0 = band * BD_BM;
    const int rows = (M - r0 < BD_BM) ? (M - r0) : BD_BM;
    int kmin[BD_RT], kmax[BD_RT];
#pragma unroll
    for (int i = 0; i < BD_RT; ++i) { kmin[i] = 1 << 30; kmax[i] = -1; }
    for (int k = threadIdx.x; k < K; k += 256) {
        const double* col = A + r0 + (size_t)k * lda;
#pragma unroll
        for (int i = 0; i < BD_RT; ++i) {
            bool nz = false;
            for (int r = 16 * i; r < 16 * i + 16 && r < rows; ++r) nz |= (col[r] != 0.0);
            if (nz) { kmin[i] = min(kmin[i], k); kmax[i] = max(kmax[i], k); }
        }
    }
#pragma unroll
    for (int i = 0; i < BD_RT; ++i) { smin[i][threadIdx.x] = kmin[i]; smax[i][threadIdx.x] = kmax[i]; }
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int i = 0; i < BD_RT; ++i) {
                smin[i][threadIdx.x] = min(smin[i][threadIdx.x], smin[i][threadIdx.x + o]);
                smax[i][threadIdx.x] = max(smax[i][threadIdx.x], smax[i][threadIdx.x + o]);
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int lo = 1 << 30, hi = -1;
        for (int i = 0; i < BD_RT; ++i) {
            const int a = smin[i][0], b = smax[i][0];
            ext[BD_EXT * band + 2 * i] = b < 0 ? 0 : a / 4;
            ext[BD_EXT * band + 2 * i + 1] = b < 0 ? 0 : b / 4 + 1;
            lo = min(lo, a); hi = max(hi, b);
        }
        if (hi < 0) { krange[2 * band] = 0; krange[2 * band + 1] = 0; }
        else { krange[2 * band] = lo / BD_BK; krange[2 * band + 1] = hi / BD_BK + 1; }
    }
}

// ---- hand-scheduled operand reads -------------------------------------------------------
// The compiler's waitcnt insertion puts `s_waitcnt lgkmcnt(0)` in front of every MFMA group,
// which also waits for the reads just issued for the NEXT group: measured (with a compiler-scheduled
// copy of the K loop, since removed) the matrix pipe then idles ~14% of the K loop on LDS latency.
// The reads are therefore issued through inline asm the compiler does not track, and the
// waits are placed by hand.  A substep's reads are not a block in front of its MFMAs (a wave
// issues in order: inside the block it issues no MFMA, and the MFMA waves of a workgroup reach
// the CU's one LDS pipe with their blocks together) but go one or two at a time BEHIND
// individual MFMAs of the substep before (bd_step), the last of them early enough that the
// MFMAs behind it cover its latency; the next substep opens with lgkmcnt(0), nothing else being
// in flight.  The waits carry the operand registers as in/out operands and pin the order
// behind them, so the MFMAs that consume them cannot be scheduled above the wait; the
// compiler knows of no read in flight, so none may be in flight where it may copy an operand
// register -- where a loop closes or begins (BD_TILE).
#if defined(__HIP_DEVICE_COMPILE__)
#define BD_RD(dst, addr, off) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(off))
#else
#define BD_RD(dst, addr, off) (dst = 0.0)
#endif
// Read R (0 .. 4 + NS) of the operands of K substep KS (4 k's) of the stage whose per-lane byte addresses are aaddr /
// baddr, for NS adjacent 16-column strips, in the order the MFMAs of a substep want them: b0, a0 .. a4, b1 (the second
// strip's B is the first one's + 256 bytes)
template <int KS, int NS, int R>
__device__ __forceinline__ void bd_read1(double (&a)[5], double (&b)[NS], unsigned aaddr, unsigned baddr)
{
    static_assert(NS == 1 || NS == 2, "one or two strips per wave");
    static_assert(R >= 0 && R < 5 + NS, "one substep's reads");
    if constexpr (R == 0) BD_RD(b[0], baddr, KS * 2 * BD_BN * 16);
    else if constexpr (R <= 5) BD_RD(a[R - 1], aaddr, KS * 4 * BD_BM * 8 + (R - 1) * 128);
    else BD_RD(b[1], baddr, KS * 2 * BD_BN * 16 + 256);
}
// reads [R0, R1) of a substep, clipped to the reads there are
template <int KS, int NS, int R0, int R1>
__device__ __forceinline__ void bd_reads(double (&a)[5], double (&b)[NS], unsigned aaddr, unsigned baddr)
{
    if constexpr (R0 < R1 && R0 < 5 + NS) {
        bd_read1<KS, NS, R0>(a, b, aaddr, baddr);
        bd_reads<KS, NS, R0 + 1, R1>(a, b, aaddr, baddr);
    }
}
// all of them as a block: the first reads of an item, which nothing is there to cover
template <int KS, int NS>
__device__ __forceinline__ void bd_read(double (&a)[5], double (&b)[NS], unsigned aaddr, unsigned baddr)
{
    bd_reads<KS, NS, 0, 5 + NS>(a, b, aaddr, baddr);
}
// every read issued so far has landed (rule: an MFMA must not be scheduled above the wait that its operands need --
// the operands are in / out operands of the wait, and the order is pinned behind it)
template <int NS>
__device__ __forceinline__ void bd_wait(double (&a)[5], double (&b)[NS])
{
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (NS == 1)
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(b[0]));
    else
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(b[0]), "+v"(b[1]));
    __builtin_amdgcn_sched_barrier(0);
#endif
}

// The MFMAs of one K substep on the operands (a, b), which have landed, with the reads of the NEXT substep -- substep
// KSN of the stage at aaddr / baddr, into (na, nb) -- slotted one or two at a time behind individual MFMAs: a wave
// issues in order, so a block of reads in front of the MFMAs is time in which it issues none, and the four MFMA waves
// of a workgroup, which leave every barrier together, put their blocks on the CU's one LDS pipe at the same moment.
//   interior tile (EDGE = false), MFMAs in the order (b0, a0 .. a4), (b1, a0 .. a4):
//     NS = 2: one read behind each of the first 7 of the 10 MFMAs; three MFMAs (192 cycles) follow the last read;
//     NS = 1: two reads behind each of the first 3 of the 5 MFMAs; two MFMAs of this wave, and those of the SIMD's
//             other wave, follow the last read.
//   edge tile (band_plan.h): row tile i's NS MFMAs only where its extent reaches substep KS, m[i] bit KS -- a
//     wave-uniform condition, a scalar branch around them; two reads behind each row tile, taken or not.
// Every accumulator sees one MFMA per substep, in K order, whatever the order inside a substep: same bits.
template <int KS, int KSN, int NS, bool EDGE>
__device__ __forceinline__ void bd_step(d4 (&acc)[NS][5][1], const double (&a)[5], const double (&b)[NS],
                                        double (&na)[5], double (&nb)[NS], unsigned aaddr, unsigned baddr,
                                        const unsigned (&m)[5])
{
    if constexpr (EDGE) {
#define BD_ROW(I)                                                                                                         \
        if (m[I] & (1u << KS)) {                                                                                          \
            asm volatile("" ::: "memory");      /* a branch, not both arms and a select */                                \
            _Pragma("unroll")                                                                                             \
            for (int j = 0; j < NS; ++j) acc[j][I][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(b[j], a[I], acc[j][I][0], 0, 0, 0); \
        }                                                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                                \
        bd_reads<KSN, NS, 2 * I, 2 * I + 2>(na, nb, aaddr, baddr);                                                        \
        __builtin_amdgcn_sched_barrier(0);
        BD_ROW(0) BD_ROW(1) BD_ROW(2) BD_ROW(3) BD_ROW(4)
#undef BD_ROW
    } else {
        constexpr int PER = NS == 2 ? 1 : 2;    // reads behind one MFMA
#define BD_ONE(J, I)                                                                                                      \
        acc[J][I][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(b[J], a[I], acc[J][I][0], 0, 0, 0);                           \
        __builtin_amdgcn_sched_barrier(0);                                                                                \
        bd_reads<KSN, NS, PER * (5 * J + I), PER * (5 * J + I + 1)>(na, nb, aaddr, baddr);                                \
        __builtin_amdgcn_sched_barrier(0);
        BD_ONE(0, 0) BD_ONE(0, 1) BD_ONE(0, 2) BD_ONE(0, 3) BD_ONE(0, 4)
        if constexpr (NS == 2) { BD_ONE(1, 0) BD_ONE(1, 1) BD_ONE(1, 2) BD_ONE(1, 3) BD_ONE(1, 4) }
#undef BD_ONE
    }
}

// The item list is read with a SCALAR load (hand-written: the compiler will not scalarise a load it
// cannot prove unclobbered by the epilogue's stores).  A vector load here sits behind the previous item's
// epilogue stores -- vector memory completes in order, its `s_waitcnt vmcnt(0)` drains every store before
// the next item's first LDS-DMA can even be issued: measured 471 vs 428 us per launch at 1024 chains.
__device__ __forceinline__ BandItem band_item(const BandItem* ip)
{
    BandItem item{0, 0, 0, -1};
#if defined(__HIP_DEVICE_COMPILE__)
    typedef int i4s __attribute__((ext_vector_type(4)));
    i4s raw;
    asm volatile("s_load_dwordx4 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(raw) : "s"(ip) : "memory");
    item.band = raw.x; item.kt0 = raw.y; item.kt1 = raw.z; item.slot = raw.w;
#else
    item = *ip;
#endif
    return item;
}

// a band's row-tile extents, read like the item
__device__ __forceinline__ void band_ext_load(const int* ep, int (&e)[BD_EXT])
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef int i8s __attribute__((ext_vector_type(8)));
    typedef int i2s __attribute__((ext_vector_type(2)));
    i8s lo; i2s hi;
    asm volatile("s_load_dwordx8 %0, %2, 0x0\n\ts_load_dwordx2 %1, %2, 0x20\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(lo), "=&s"(hi) : "s"(ep) : "memory");
#pragma unroll
    for (int i = 0; i < 8; ++i) e[i] = lo[i];
    e[8] = hi.x; e[9] = hi.y;
#else
    for (int i = 0; i < BD_EXT; ++i) e[i] = ep[i];
#endif
}

// ---- the fill role ------------------------------------------------------------------------
// One wave's share of the ring fill: pieces f, f + STRIDE, ... of the 20 A and the 32 B one-KiB pieces of a stage,
// NA + NB LDS-DMAs per K tile (lane l's 16 bytes of a piece land at its LDS address + 16 l).
// Operand addressing: a UNIFORM base (SGPR pair, advanced per K tile by scalar adds) plus a per-lane 32-bit
// byte offset that never changes inside a K loop (lds_dma16, dgemm_dlds.h, says why).
template <int STRIDE, int NA, int NB>
struct BandFill {
    static constexpr int PER_TILE = NA + NB, A_CHUNKS = BD_A_BYTES / 1024;
    static_assert(STRIDE * NA >= A_CHUNKS && STRIDE * NB * 1024 == BD_B_BYTES, "the role's waves cover a stage");
    const GemmP& p;
    const BandItem* items;
    const int f, lane;
    const unsigned lds0;
    const size_t stepA;                                      // bytes per K tile
    unsigned voa[NA], vob[NB];
    const char* sA = nullptr; const char* sB = nullptr;      // uniform
    BandItem item{0, 0, 0, -1};                              // the item being worked on; load_item() replaces it

    // A piece s of this wave is chunk f + a_rel(s).  Where STRIDE waves x NA pieces exceed the 20 chunks (8-wave
    // form: waves 4-7), the wave repeats its second chunk, so that every wave issues PER_TILE loads: uniform vmcnt
    __device__ __forceinline__ int a_rel(int s) const
    {
        return (STRIDE * NA > A_CHUNKS && f + STRIDE * s >= A_CHUNKS) ? STRIDE : STRIDE * s;
    }
    __device__ __forceinline__ BandFill(const BandP& bp, int f_, int lane_, int n0, unsigned lds0_)
        : p(bp.g), items(bp.items), f(f_), lane(lane_), lds0(lds0_), stepA((size_t)BD_BK * bp.g.lda * 8)
    {
        // B pieces do not depend on the band: chunk c -> (kp = c >> 1, half = c & 1)
#pragma unroll
        for (int s = 0; s < NB; ++s) {
            const int c = f + STRIDE * s;
            const int kp = c >> 1, n = ((c & 1) << 6) + lane;
            int gn = n0 + n;
            if (gn >= p.N) gn = 0;
            vob[s] = (unsigned)((2 * kp + (size_t)gn * p.ldb) * 8);
        }
    }
    __device__ __forceinline__ void load_item(int it)
    {
        item = band_item(items + it);
        const int m0 = item.band * BD_BM;
#pragma unroll
        for (int s = 0; s < NA; ++s) {
            const int o = (f + a_rel(s)) * 1024 + lane * 16;
            const int k = o / (BD_BM * 8), m = (o - k * BD_BM * 8) >> 3;
            int gm = m0 + m;
            if (gm >= p.M) gm = 0;
            voa[s] = (unsigned)((gm + (size_t)k * p.lda) * 8);
        }
        sA = reinterpret_cast<const char*>(p.A) + (size_t)item.kt0 * stepA;
        sB = reinterpret_cast<const char*>(p.B) + (size_t)item.kt0 * (BD_BK * 8);
    }
    // the item's next K tile into ring stage `stage`
    __device__ __forceinline__ void issue(int stage)
    {
        const unsigned lbase = lds0 + stage * BD_STAGE_BYTES + f * 1024;
#pragma unroll
        for (int s = 0; s < NA; ++s) lds_dma16(lbase + a_rel(s) * 1024, voa[s], sA);
#pragma unroll
        for (int s = 0; s < NB; ++s) lds_dma16(lbase + BD_A_BYTES + STRIDE * s * 1024, vob[s], sB);
        sA += stepA;
        sB += BD_BK * 8;
    }
    // wait until at most `tiles` of this wave's tiles are in flight
    __device__ __forceinline__ void wait_leave(int tiles) const
    {
        if (tiles >= 2) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * PER_TILE) : "memory");
        else if (tiles == 1) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(PER_TILE) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
};
// a wave that leaves the fill to others (the feeder form's MFMA waves): the item alone, nothing to issue or wait for
struct BandNoFill {
    const BandItem* items;
    BandItem item{0, 0, 0, -1};
    __device__ __forceinline__ BandNoFill(const BandP& bp, int, int, int, unsigned) : items(bp.items) {}
    __device__ __forceinline__ void load_item(int it) { item = band_item(items + it); }
    __device__ __forceinline__ void issue(int) {}
    __device__ __forceinline__ void wait_leave(int) const {}
};
constexpr int BF_NA = 5, BF_NB = 8;      // LDS-DMA pieces per feeder wave per tile (BD_NA, BD_NB: per wave of the 8-wave form)

// raw accumulator tile of one 16-column strip (0..7) in register order: element (strip, i, r, lane) -- each store
// instruction writes 512 contiguous bytes; k_band_reduce reads it back with the same thread mapping
__device__ __forceinline__ void band_store_partial(double* tile, int strip, int lane, const d4 (&acc)[5][1])
{
    double* P = tile + (size_t)strip * (20 * 64) + lane;
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) P[(i * 4 + r) * 64] = acc[i][0][r];
}

// what the waves of a workgroup start from: the wave's number, the thread's lane, the column tile, the items
struct BandWg {
    int wave, lane, bj, it0, it1;
    __device__ __forceinline__ explicit BandWg(const BandP& bp)
    {
        const int tid = threadIdx.x;
        lane = tid & 63;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        // XCD-aware map over (workgroup of the plan, column tile): the column tiles of one run of K tiles
        // share an XCD (they read the same pieces of A)
        const int nid = xcd_block_map(blockIdx.x, bp.nwg * bp.g.gn);
        const int pw = nid / bp.g.gn;
        bj = nid - pw * bp.g.gn;
        it0 = bp.wg_ptr[pw]; it1 = bp.wg_ptr[pw + 1];
    }
};

// ---- the item walk ------------------------------------------------------------------------
// What one wave does with its workgroup's items.  Fill: its share of the ring fill (BandFill), or BandNoFill.
// NS: the number of 16-column strips it multiplies, strip0, strip0 + 1, ...; 0 for a wave that only fills.
// Whatever its jobs, a wave passes the barriers of this one function: per item with K tiles one before the K loop
// and one per tile, and one behind an item whose successor's ring fill is not already in flight (`pre`).
// DBG = true only for the timing hooks of debug_hooks.hip (bp.mode / bp.clocks); the other instantiations carry no
// stamp and read no clock.
template <int NS, class Fill, bool DBG, class Epi>
__device__ __forceinline__ void band_walk(const BandP& bp, const Epi& epi, const BandWg& wg, int piece0, int strip0)
{
    constexpr int NJ = NS > 0 ? NS : 1;     // a wave that only fills declares the operand registers and never touches them
    const GemmP& p = bp.g;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const unsigned lds0 = (unsigned)(size_t)(lds_ptr_t) reinterpret_cast<char*>(smem);
    const int lane = wg.lane, l15 = lane & 15, lk = lane >> 4;
    const int bj = wg.bj, n0 = bj * BD_BN, it0 = wg.it0, it1 = wg.it1;

    // DBG, mode bit 16: every workgroup leaves 100 MHz real-time stamps of its phases at clocks[8 + 8 * bid ..]:
    // [start, first ring stages landed, K loop of the first item done, its epilogue / partial store issued, end]
    auto stamp = [&](int i) {
        if constexpr (DBG)
            if ((bp.mode & 16) && bp.clocks && threadIdx.x == 0)
                bp.clocks[8 + 8 * (size_t)blockIdx.x + i] = __builtin_amdgcn_s_memrealtime();
    };
    stamp(0);
    bool first_item = true;
    Fill fill(bp, piece0, lane, n0, lds0);
    // `pre`: the first ring stages of the item about to start are already in flight -- they were issued BEFORE the
    // previous item's epilogue (the ring is free once every wave has passed the last barrier of a K loop), so the
    // fill's memory latency runs under the epilogue's loads and stores instead of after them
    bool pre = false;
    int issued = 0;
    // MFMA waves: the item's band's row-tile extents (without them: every row tile reaches everywhere, every K tile is
    // interior -- GLMMR_MCML_BAND_ROWTILES=0)
    int ext[BD_EXT];
    auto load_ext = [&]() {
        if constexpr (NS > 0) {
            if (bp.ext) band_ext_load(bp.ext + BD_EXT * fill.item.band, ext);
            else {
#pragma unroll
                for (int i = 0; i < BD_RT; ++i) { ext[2 * i] = 0; ext[2 * i + 1] = 1 << 30; }
            }
        }
    };
    if (it0 < it1) { fill.load_item(it0); load_ext(); }
    for (int it = it0; it < it1;) {
        const int band = fill.item.band, slot = fill.item.slot;
        const int kt0 = fill.item.kt0, nk = fill.item.kt1 - kt0;
        // tiles [il, ih) of this item are interior: two uniform bounds
        int il = 0, ih = 0;
        if constexpr (NS > 0) { band_ext_interior(ext, il, ih); il -= kt0; ih -= kt0; }

        d4 acc[NJ][5][1];
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int i = 0; i < 5; ++i) acc[j][i][0] = d4{0.0, 0.0, 0.0, 0.0};

        if (nk > 0) {
            // per-lane LDS byte addresses of the operand reads inside stage 0
            const unsigned aoff = lds0 + lk * (BD_BM * 8) + l15 * 8;
            const unsigned boff = lds0 + BD_A_BYTES + (((lk >> 1) * BD_BN + strip0 * 16 + l15) << 4) + ((lk & 1) << 3);
            if (!pre) { issued = 0; for (; issued < BD_STAGES - 1 && issued < nk; ++issued) fill.issue(issued); }
            fill.wait_leave(issued - 1);
            __builtin_amdgcn_s_barrier();
            if (first_item) stamp(1);
            int st = 0;
            double ra[2][5], rb[2][NJ];
            if constexpr (NS > 0) { bd_read<0>(ra[0], rb[0], aoff, boff); bd_wait(ra[0], rb[0]); }
            // The K loop: LAST tiles of it with the tile body BODY.  The stage of tile kt - 1 is free to fill: every wave
            // finished its reads before that tile's barrier.
#define BD_KLOOP(LAST, BODY)                                                                         \
            for (; kt < (LAST); ++kt) {                                                              \
                if (issued < nk) {                                                                   \
                    int sn = st + BD_STAGES - 1; if (sn >= BD_STAGES) sn -= BD_STAGES;               \
                    fill.issue(sn);                                                                  \
                    ++issued;                                                                        \
                }                                                                                    \
                const unsigned aaddr = aoff + st * BD_STAGE_BYTES, baddr = boff + st * BD_STAGE_BYTES; \
                int stn = st + 1; if (stn >= BD_STAGES) stn = 0;                                     \
                BODY                                                                                 \
                st = stn;                                                                            \
            }
            // The tile body of an MFMA wave, EDGE: all of a substep's MFMAs or those inside the extents (bd_step).  A
            // substep waits for its operands -- the only reads in flight -- and issues its MFMAs with the next substep's
            // reads between them.  Last substep: synchronise first (this wave's pieces of tile kt + 1 landed, its own reads
            // of tile kt complete); its operands are in registers, so the first instruction behind the barrier is an MFMA,
            // and the next tile's first reads go between its MFMAs like any substep's.  Behind the item's last tile there
            // is no next stage: the same reads go to the stage just finished, straight-line code instead of a second copy
            // of the MFMAs; what they return is never an operand, and the wait that ends the tile retires them.
            // The wait for substep 0's operands stands at the END of the tile before (and behind the item's first reads):
            // the same place in the instruction stream, but no read is in flight where a loop closes or the next loop
            // begins -- there the compiler may copy a loop-carried operand register, and it does not know of the reads.
#define BD_STEP(KS, CUR, NXT, EDGE)                                                                                       \
                    bd_step<KS, KS + 1, NS, EDGE>(acc, ra[CUR], rb[CUR], ra[NXT], rb[NXT], aaddr, baddr, em);             \
                    bd_wait(ra[NXT], rb[NXT]);
#define BD_TILE(EDGE)                                                                                                     \
                    BD_STEP(0, 0, 1, EDGE) BD_STEP(1, 1, 0, EDGE) BD_STEP(2, 0, 1, EDGE) BD_STEP(3, 1, 0, EDGE)           \
                    BD_STEP(4, 0, 1, EDGE) BD_STEP(5, 1, 0, EDGE)                                                         \
                    bd_step<6, 7, NS, EDGE>(acc, ra[0], rb[0], ra[1], rb[1], aaddr, baddr, em);                           \
                    const int sr = kt + 1 < nk ? stn : st;                                                                \
                    fill.wait_leave(issued - kt - 2);                                                                     \
                    bd_wait(ra[1], rb[1]);                                                                                \
                    __builtin_amdgcn_s_barrier();                                                                         \
                    __builtin_amdgcn_sched_barrier(0);                                                                    \
                    bd_step<7, 0, NS, EDGE>(acc, ra[1], rb[1], ra[0], rb[0], aoff + sr * BD_STAGE_BYTES,                  \
                                            boff + sr * BD_STAGE_BYTES, em);                                              \
                    bd_wait(ra[0], rb[0]);
            // an interior tile: no mask is looked at
#define BD_TILE_ALL                                                                                                       \
                    const unsigned em[BD_RT] = {~0u, ~0u, ~0u, ~0u, ~0u};                                                 \
                    BD_TILE(false)
            // an edge tile: the same reads, waits and barrier; per row tile the substeps inside its extent
#define BD_TILE_EDGE                                                                                                      \
                    unsigned em[BD_RT];                                                                                   \
                    _Pragma("unroll")                                                                                     \
                    for (int i = 0; i < BD_RT; ++i) em[i] = band_ext_mask(ext[2 * i], ext[2 * i + 1], kt0 + kt);          \
                    BD_TILE(true)
            int kt = 0;
            if constexpr (NS > 0) {
                // edge tiles [0, e0), interior tiles [e0, e1), edge tiles [e1, nk): three loops in a row, so that the
                // accumulators stay in their registers from one to the next (as two arms of one loop's body they were
                // copied, all 80 registers, where the arms meet) and the interior loop is the loop it was
                const int e0 = il < 0 ? 0 : (il < nk ? il : nk);
                const int e1 = ih < e0 ? e0 : (ih < nk ? ih : nk);
                BD_KLOOP(e0, BD_TILE_EDGE)
                BD_KLOOP(e1, BD_TILE_ALL)
                BD_KLOOP(nk, BD_TILE_EDGE)
            } else {
                BD_KLOOP(nk, fill.wait_leave(issued - kt - 2); __builtin_amdgcn_s_barrier();)
            }
#undef BD_TILE_EDGE
#undef BD_TILE_ALL
#undef BD_TILE
#undef BD_STEP
#undef BD_KLOOP
        }
        if (first_item) stamp(2);
        ++it;
        pre = false;
        if (it < it1) {
            fill.load_item(it);
            load_ext();
            const int nkn = fill.item.kt1 - fill.item.kt0;
            if (nk > 0 && nkn > 0) {
                issued = 0;
                for (; issued < BD_STAGES - 1 && issued < nkn; ++issued) fill.issue(issued);
                pre = true;
            }
        }
        if constexpr (NS > 0) {
            if (slot < 0) {
                // Register budget with two strips (80 accumulator registers stay live into the first call): one call
                // at a time, and the lane number made opaque per item, or the epilogue's per-lane addresses of BOTH
                // strips are hoisted out of the item loop and held across the K loop -- EpiBackward then spills
                int elane = lane;
                if constexpr (NS > 1) asm volatile("" : "+v"(elane));
                epi(acc[0], band * BD_BM, n0 + strip0 * 16, elane, p.M, p.N, band);
                if constexpr (NS > 1) {
                    __builtin_amdgcn_sched_barrier(0);
                    epi(acc[1], band * BD_BM, n0 + strip0 * 16 + 16, elane, p.M, p.N, band);
                }
            } else {
                double* tile = bp.part + ((size_t)slot * p.gn + bj) * BD_TILE_ELEMS;
#pragma unroll
                for (int j = 0; j < NS; ++j) band_store_partial(tile, strip0 + j, lane, acc[j]);
            }
        }
        if (first_item) { stamp(3); first_item = false; }
        // without a prefetch the next item's first LDS-DMA may overwrite a stage another wave is still reading
        if (!pre) __builtin_amdgcn_s_barrier();
    }
    if constexpr (DBG)
        if ((bp.mode & 16) && bp.clocks) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); stamp(4); }
}

// the 8-wave form: every wave fills (pieces wave, wave + 8, ...) and multiplies strip `wave`
template <class Epi, bool DBG>
__global__ __launch_bounds__(512) void dgemm_band_kernel(BandP bp, Epi epi)
{
    const BandWg wg(bp);
    unsigned long long t0c = 0, t0r = 0;
    if constexpr (DBG)
        if (bp.clocks && blockIdx.x == 0 && threadIdx.x == 0) { t0c = __builtin_amdgcn_s_memtime(); t0r = __builtin_amdgcn_s_memrealtime(); }
    band_walk<1, BandFill<8, BD_NA, BD_NB>, DBG>(bp, epi, wg, wg.wave, wg.wave);
    if constexpr (DBG)
        if (bp.clocks && blockIdx.x == 0 && threadIdx.x == 0) {
            atomicAdd(bp.clocks, __builtin_amdgcn_s_memtime() - t0c);
            atomicAdd(bp.clocks + 1, __builtin_amdgcn_s_memrealtime() - t0r);
        }
}

// which epilogues run the feeder form (specialised where the epilogue is defined)
template <class Epi> struct BandFeed { static constexpr bool ok = false; };
template <> struct BandFeed<EpiAxpby> { static constexpr bool ok = true; };

static inline bool band_feed_enabled()         // read per call: the parity tests run both forms in one process
{
    const char* e = getenv("GLMMR_MCML_BAND_FEED");
    return !(e && !strcmp(e, "0"));
}

// the feeder form: waves 4-7 fill (pieces wave - 4, wave, ...), waves 0-3 multiply strips 2 wave and 2 wave + 1
// (one static s_setprio 1 in the feeders measured no different: 839.4 / 844.9 against 842.9 / 842.9 ms per bench step)
template <class Epi>
__global__ __launch_bounds__(512) void dgemm_band_feed_kernel(BandP bp, Epi epi)
{
    const BandWg wg(bp);
    if (wg.wave >= 4) band_walk<0, BandFill<4, BF_NA, BF_NB>, false>(bp, epi, wg, wg.wave - 4, 0);
    else band_walk<2, BandNoFill, false>(bp, epi, wg, 0, 2 * wg.wave);
}

// second stage of the streamed decomposition: one workgroup of 2 waves per (split band, column tile,
// wave pair) sums the band's pieces in K order and applies the epilogue with the GEMM kernel's own
// register mapping
template <class Epi>
__global__ __launch_bounds__(128) void k_band_reduce(const BandRed* red, const double* part, int gn, int M, int N, Epi epi)
{
    const BandRed rd = red[blockIdx.x];
    const int bj = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = blockIdx.z * 2 + (threadIdx.x >> 6);
    d4 acc[5][1];
#pragma unroll
    for (int i = 0; i < 5; ++i) acc[i][0] = d4{0.0, 0.0, 0.0, 0.0};
    // four pieces' loads in flight at a time (the kernel is latency-bound: a handful of pieces per band); the adds
    // stay in K order
    const size_t pstride = (size_t)gn * BD_TILE_ELEMS;
    const double* P0 = part + ((size_t)rd.s0 * gn + bj) * BD_TILE_ELEMS + (size_t)wave * (20 * 64) + lane;
    for (int s = rd.s0; s < rd.s1; s += 4) {
        double v[4][20];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double* P = P0 + (size_t)(s - rd.s0 + (s + u < rd.s1 ? u : 0)) * pstride;
#pragma unroll
            for (int t = 0; t < 20; ++t) v[u][t] = P[t * 64];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (s + u < rd.s1) {
#pragma unroll
                for (int i = 0; i < 5; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[i][0][r] += v[u][i * 4 + r];
            }
    }
    epi(acc, rd.band * BD_BM, bj * BD_BN + wave * 16, lane, M, N, rd.band);
}

// form: BAND_FORM_AUTO, or one of the two kernels whatever the plan (debug hooks: the parity tests compare them);
// whole_band (nullable): whether the plan is the whole-band one
enum { BAND_FORM_AUTO = -1, BAND_FORM_8WAVE = 0, BAND_FORM_FEED = 1 };
template <class Epi, bool DBG = false>
static inline int launch_gemm_band(hipStream_t s, BandPlan& plan, int N, const double* A, int lda,
                                   const double* B, int ldb, const Epi& epi,
                                   unsigned long long* clocks = nullptr, int mode = 0, int form = BAND_FORM_AUTO,
                                   int* whole_band = nullptr)
{
    const int gn = (N + BD_BN - 1) / BD_BN;
    BandPlanDev* d = nullptr;
    MCML_TRY(plan.device_plan(gn, s, &d));
    BandP bp;
    bp.clocks = clocks;
    bp.mode = mode;
    bp.g = GemmP{plan.M, N, plan.K, A, lda, B, ldb, 0, gn, 0};
    bp.items = d->items.as<BandItem>();
    bp.wg_ptr = d->wg_ptr.as<int>();
    bp.nwg = d->nwg;
    bp.ext = band_rowtiles_enabled() ? d->ext.as<int>() : nullptr;
    bp.part = d->part.d();
    if (whole_band) *whole_band = d->paired;
    bool feed = false;
    if constexpr (BandFeed<Epi>::ok && !DBG) {
        // whole-band and streamed plans alike: at 128 chains the feeder form measured 181.0 against 187.5 ms per step
        feed = form == BAND_FORM_AUTO ? band_feed_enabled() : form == BAND_FORM_FEED;
        if (feed) {
            MCML_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(&dgemm_band_feed_kernel<Epi>), (int)BD_LDS_BYTES));
            hipLaunchKernelGGL((dgemm_band_feed_kernel<Epi>), dim3(d->nwg * gn), dim3(512), BD_LDS_BYTES, s, bp, epi);
        }
    }
    MCML_REQUIRE(feed || form != BAND_FORM_FEED, "launch_gemm_band: no feeder form of this instantiation");
    if (!feed) {
        MCML_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(&dgemm_band_kernel<Epi, DBG>), (int)BD_LDS_BYTES));
        hipLaunchKernelGGL((dgemm_band_kernel<Epi, DBG>), dim3(d->nwg * gn), dim3(512), BD_LDS_BYTES, s, bp, epi);
    }
    if (d->nred > 0)
        hipLaunchKernelGGL((k_band_reduce<Epi>), dim3(d->nred, gn, 4), dim3(128), 0, s, d->red.as<BandRed>(),
                           d->part.d(), gn, plan.M, N, epi);
    MCML_HIP(hipGetLastError());
    return MCML_OK;
}


}  // namespace mcml
