// band_plan.h -- host side of dgemm_band.h: tile constants and the work decomposition of the banded
// HMC products (whole bands dealt into balanced groups, or the flattened (band, K tile) space cut into
// equal runs with a fixed-order second stage).  Kept apart from the kernels so that ctx.h stays light.
#pragma once
#include "common.h"
#include <algorithm>
#include <map>
#include <memory>

namespace mcml {

constexpr int BD_BM = 80, BD_BN = 128, BD_BK = 32, BD_STAGES = 3;
constexpr int BD_A_BYTES = BD_BK * BD_BM * 8;      // 20480: 20 chunks of 1 KiB
constexpr int BD_B_BYTES = BD_BK * BD_BN * 8;      // 32768: 32 chunks
constexpr int BD_STAGE_BYTES = BD_A_BYTES + BD_B_BYTES;
constexpr size_t BD_LDS_BYTES = (size_t)BD_STAGES * BD_STAGE_BYTES;   // 159744
constexpr int BD_NA = 3, BD_NB = 4, BD_PER_TILE = BD_NA + BD_NB;      // LDS-DMA pieces per wave per tile
constexpr int BD_TILE_ELEMS = BD_BM * BD_BN;                          // one raw accumulator tile (doubles)
constexpr int BD_RT = BD_BM / 16;         // 16-row tiles of a band: one v_mfma_f64_16x16x4 accumulator each per strip
constexpr int BD_SUB = BD_BK / 4;         // K substeps (4 columns: one MFMA per row tile and strip) of a K tile
constexpr int BD_EXT = 2 * BD_RT;         // ints of a band's row-tile extents

// one run of K tiles of one band.  slot < 0: the band's only run, the epilogue is applied here;
// slot >= 0: the raw accumulator tile goes to partial slot `slot` of this column tile
struct BandItem { int band, kt0, kt1, slot; };
// a band whose pieces k_band_reduce sums: slots [s0, s1) in K order
struct BandRed { int band, s0, s1, pad; };

// ---- row-tile extents ---------------------------------------------------------------------
// Beside its K-tile range a band has, for each of its five 16-row tiles i, the K substeps [s0_i, s1_i) -- absolute,
// 4 columns each -- outside which the row tile holds exact zeros (s0_i = s1_i: no nonzero, or past M): e[2 i], e[2 i + 1].
// A K tile kt is INTERIOR when every row tile's extent covers all of it, [8 kt, 8 kt + 8): the kernel runs its plain tile
// body there.  In an EDGE tile it issues the MFMA of row tile i in substep s only where band_ext_mask says so.  The same
// three functions serve the kernel (dgemm_band.h), the flop accounting and the host test driver.
#if defined(__HIPCC__)
#define BD_HD __host__ __device__
#else
#define BD_HD
#endif
// the interior K tiles [lo, hi) of a band (absolute; lo >= hi: none)
BD_HD inline void band_ext_interior(const int* e, int& lo, int& hi)
{
    int s0 = e[0], s1 = e[1];
    for (int i = 1; i < BD_RT; ++i) { if (e[2 * i] > s0) s0 = e[2 * i]; if (e[2 * i + 1] < s1) s1 = e[2 * i + 1]; }
    lo = (s0 + BD_SUB - 1) / BD_SUB; hi = s1 / BD_SUB;
}
// bit s (0..7) set: K substep 8 kt + s lies inside [s0, s1)
BD_HD inline unsigned band_ext_mask(int s0, int s1, int kt)
{
    int a = s0 - BD_SUB * kt, b = s1 - BD_SUB * kt;
    a = a < 0 ? 0 : a;
    b = b > BD_SUB ? BD_SUB : b;
    return b > a ? ((1u << b) - 1u) & ~((1u << a) - 1u) : 0u;      // 0 <= a < b <= 8 where it shifts
}
// MFMAs per 16-column strip that the K tiles [kt0, kt1) of a band issue
inline long band_ext_issued(const int* e, int kt0, int kt1)
{
    long n = 0;
    for (int i = 0; i < BD_RT; ++i) {
        const int a = std::max(e[2 * i], BD_SUB * kt0), b = std::min(e[2 * i + 1], BD_SUB * kt1);
        if (b > a) n += b - a;
    }
    return n;
}

// GLMMR_MCML_BAND_ROWTILES=0: every K tile of a band's range is multiplied whole, no row-tile extents (read per call)
static inline bool band_rowtiles_enabled()
{
    const char* e = getenv("GLMMR_MCML_BAND_ROWTILES");
    return !(e && !strcmp(e, "0"));
}

// ---- host: the decomposition ------------------------------------------------------------
struct BandPlanDev {
    int gn = 0, nwg = 0, nred = 0, nslots = 0;
    int paired = 0;                       // decompose() chose whole bands, no partial sums (else streamed)
    DevBuf items, wg_ptr, red, part;
    DevBuf ext;                           // the row-tile extents, BD_EXT ints per band
};

// the few-column products (dgemm_skinny.h): chunk range of every 256-row block, partial sums
struct SkinnyPlan {
    int nrb = 0, nkc = 0, ldp = 0;
    DevBuf range;                 // int2 per row block: first chunk of 128 K columns, one past the last
    DevBuf part;                  // nkc x 16 x ldp doubles
};

struct BandPlan {
    int M = 0, K = 0, nbands = 0;
    std::vector<int> kr;                  // host copy of the K-tile ranges, 2 per band
    std::vector<int> ext;                 // host copy of the row-tile extents, BD_EXT per band
    long tiles = 0;                       // sum over bands of K tiles multiplied
    long mfmas = 0;                       // sum over bands of the MFMAs per 16-column strip inside the extents
    std::map<int, std::unique_ptr<BandPlanDev>> by_gn;
    std::unique_ptr<SkinnyPlan> skinny;

    void reset(int M_, int K_, const std::vector<int>& kr_, const std::vector<int>& ext_)
    {
        M = M_; K = K_; kr = kr_; ext = ext_; nbands = (M + BD_BM - 1) / BD_BM;
        tiles = 0; mfmas = 0;
        for (int b = 0; b < nbands; ++b) {
            tiles += kr[2 * b + 1] - kr[2 * b];
            mfmas += band_ext_issued(ext.data() + BD_EXT * b, kr[2 * b], kr[2 * b + 1]);
        }
        by_gn.clear();
        skinny.reset();
    }

    // MFMAs per 16-column strip that a launch issues: inside the extents, or every one of the K tiles' (the switch off)
    long issued(bool rowtiles) const { return rowtiles ? mfmas : tiles * (BD_RT * BD_SUB); }

    // target_wg: workgroups the launch should have in all (one per CU).  Returns true for the whole-band form.  The
    // plan is a function of (kr, nbands, gn, target_wg) alone.
    static bool decompose(const std::vector<int>& kr, int nbands, int gn, int target_wg, std::vector<BandItem>& items,
                          std::vector<int>& wg_ptr, std::vector<BandRed>& red, int& nslots)
    {
        items.clear(); wg_ptr.clear(); red.clear(); nslots = 0;
        // Cost of an item in half K tiles, both forms: 2 per K tile + OVH (ring fill, barrier, epilogue or partial
        // store).  Per-workgroup phase stamps (scripts/band_clocks.py 5000 128 1 48) put a second item at about one
        // K tile: with OVH = 5 the two-item workgroups ended 8 us before the single-item ones and only 249 of 256 CUs
        // were used at n = 5000, 128 chains; OVH = 3 fills all 256 and the longest run drops from 21 to 20 K tiles.
        constexpr long OVH = 3;
        const int npairs = (nbands + 1) / 2;
        if ((long)npairs * gn * 5 >= (long)target_wg * 4) {          // mirror pairs would fill >= 80% of the CUs: no partial sums
            // Whole bands, one group of them per workgroup.  The launch is one wave of workgroups, so it lasts as long
            // as its costliest group: deal the bands, costliest first (ties: lowest band), each into the least loaded
            // of G groups (ties: lowest group) -- longest-processing-time greedy.  An empty band costs OVH and still
            // gets its item: its epilogue has to run.  The first G bands open the groups in order, so group g and
            // g + 1 start on adjacent long bands and the groups that share an XCD stay roughly in step on B.
            auto cost = [&](int b) { return 2L * (kr[2 * b + 1] - kr[2 * b]) + OVH; };
            int G = target_wg / gn; if (G > nbands) G = nbands; if (G < 1) G = 1;
            std::vector<int> order(nbands);
            for (int b = 0; b < nbands; ++b) order[b] = b;
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost(a) > cost(b); });
            std::vector<long> load(G, 0);
            std::vector<std::vector<int>> group(G);
            for (int b : order) {
                const int g = (int)(std::min_element(load.begin(), load.end()) - load.begin());
                group[g].push_back(b); load[g] += cost(b);
            }
            // against band p with its mirror nbands-1-p (equal K steps when the ranges are exactly linear in the band):
            // waves of workgroups x costliest group; the mirror pairs stay only where they are strictly better
            long pair_max = 0;
            for (int p = 0; p < npairs; ++p)
                pair_max = std::max(pair_max, cost(p) + (nbands - 1 - p > p ? cost(nbands - 1 - p) : 0));
            auto waves = [&](int groups) { return ((long)groups * gn + target_wg - 1) / target_wg; };
            if (waves(npairs) * pair_max < waves(G) * *std::max_element(load.begin(), load.end())) {
                group.assign(npairs, std::vector<int>());
                for (int p = 0; p < npairs; ++p) {
                    group[p].push_back(p);
                    if (nbands - 1 - p > p) group[p].push_back(nbands - 1 - p);
                }
            }
            for (std::vector<int>& g : group) {
                std::sort(g.begin(), g.end());
                wg_ptr.push_back((int)items.size());
                for (int b : g) items.push_back({b, kr[2 * b], kr[2 * b + 1], -1});
            }
            wg_ptr.push_back((int)items.size());
            return true;
        }
        // Streamed: walk the bands in order and fill one workgroup after another up to a cost cap.  The cap is
        // the smallest one whose greedy fill needs at most nwg workgroups (bisection).
        int nwg = target_wg / gn; if (nwg < 1) nwg = 1;
        auto fill = [&](long cap, bool emit) -> int {
            int used = 1; long room = cap;
            if (emit) wg_ptr.push_back(0);
            for (int b = 0; b < nbands; ++b) {
                int k0 = kr[2 * b]; const int k1 = kr[2 * b + 1];
                const int first = (int)items.size();
                int pieces = 0;
                do {
                    if (room < OVH + 2) { ++used; room = cap; if (emit) wg_ptr.push_back((int)items.size()); }
                    long take = (room - OVH) / 2; if (take > k1 - k0) take = k1 - k0;
                    if (emit) items.push_back({b, k0, k0 + (int)take, -1});
                    k0 += (int)take; room -= OVH + 2 * take; ++pieces;
                } while (k0 < k1);
                if (emit && pieces > 1) {
                    for (int t = 0; t < pieces; ++t) items[first + t].slot = nslots + t;
                    red.push_back({b, nslots, nslots + pieces, 0});
                    nslots += pieces;
                }
            }
            if (emit) wg_ptr.push_back((int)items.size());
            return used;
        };
        long T = 0;
        for (int b = 0; b < nbands; ++b) T += kr[2 * b + 1] - kr[2 * b];
        long lo = OVH + 2, hi = 2 * T + OVH * nbands + OVH + 2;      // hi: everything in one workgroup
        while (lo < hi) {
            const long mid = (lo + hi) / 2;
            if (fill(mid, false) <= nwg) hi = mid; else lo = mid + 1;
        }
        fill(lo, true);
        return false;
    }

    int device_plan(int gn, hipStream_t s, BandPlanDev** out)
    {
        auto it = by_gn.find(gn);
        if (it != by_gn.end()) { *out = it->second.get(); return MCML_OK; }
        std::unique_ptr<BandPlanDev> d(new BandPlanDev());
        std::vector<BandItem> items; std::vector<int> wg_ptr; std::vector<BandRed> red; int nslots = 0;
        d->paired = decompose(kr, nbands, gn, 256, items, wg_ptr, red, nslots) ? 1 : 0;
        d->gn = gn; d->nwg = (int)wg_ptr.size() - 1; d->nred = (int)red.size(); d->nslots = nslots;
        MCML_TRY(d->items.ensure(sizeof(BandItem) * (items.size() + 1)));
        MCML_TRY(d->wg_ptr.ensure(sizeof(int) * wg_ptr.size()));
        MCML_HIP(hipMemcpyAsync(d->items.p, items.data(), sizeof(BandItem) * items.size(), hipMemcpyHostToDevice, s));
        MCML_HIP(hipMemcpyAsync(d->wg_ptr.p, wg_ptr.data(), sizeof(int) * wg_ptr.size(), hipMemcpyHostToDevice, s));
        MCML_TRY(d->ext.ensure(sizeof(int) * (ext.size() + 1)));
        MCML_HIP(hipMemcpyAsync(d->ext.p, ext.data(), sizeof(int) * ext.size(), hipMemcpyHostToDevice, s));
        if (nslots > 0) {
            MCML_TRY(d->red.ensure(sizeof(BandRed) * red.size()));
            MCML_HIP(hipMemcpyAsync(d->red.p, red.data(), sizeof(BandRed) * red.size(), hipMemcpyHostToDevice, s));
            MCML_TRY(d->part.ensure(sizeof(double) * (size_t)nslots * gn * BD_TILE_ELEMS));
        }
        MCML_HIP(hipStreamSynchronize(s));       // the host vectors go out of scope
        *out = d.get();
        by_gn[gn] = std::move(d);
        return MCML_OK;
    }
};

}  // namespace mcml
