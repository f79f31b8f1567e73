// Host arithmetic of the row-tile extents of the banded HMC products (glmmrmcml_amd/csrc/band_plan.h: band_ext_interior,
// band_ext_mask, band_ext_issued, BandPlan::reset / issued) under AddressSanitizer + UBSan, against a brute-force scan of
// small operands: a mask never drops a 16 x 4 block that holds a nonzero, it is exactly the extent's substeps, a K tile
// is interior exactly when all five masks are full, and the issued counts add up -- per band, per plan and per item of
// every decomposition (whole bands and streamed runs cut inside a band).  Built and run by tests/test_band_rowtiles_cpu.py.
#include "band_plan.h"
#include <cstdio>
#include <functional>
using namespace mcml;

typedef std::function<bool(int, int)> Pattern;       // (row, column) -> nonzero

// what k_band_ranges records, restated: K-tile range per band, substep extents per (band, 16-row tile)
static void scan(const Pattern& nz, int M, int K, std::vector<int>& kr, std::vector<int>& ext)
{
    const int nb = (M + BD_BM - 1) / BD_BM;
    kr.assign(2 * nb, 0); ext.assign(BD_EXT * nb, 0);
    for (int b = 0; b < nb; ++b) {
        int lo = 1 << 30, hi = -1;
        for (int i = 0; i < BD_RT; ++i) {
            int a = 1 << 30, z = -1;
            for (int k = 0; k < K; ++k) {
                bool any = false;
                for (int r = b * BD_BM + 16 * i; r < b * BD_BM + 16 * i + 16 && r < M && !any; ++r) any = nz(r, k);
                if (any) { a = std::min(a, k); z = std::max(z, k); }
            }
            if (z >= 0) { ext[BD_EXT * b + 2 * i] = a / 4; ext[BD_EXT * b + 2 * i + 1] = z / 4 + 1; lo = std::min(lo, a); hi = std::max(hi, z); }
        }
        if (hi >= 0) { kr[2 * b] = lo / BD_BK; kr[2 * b + 1] = hi / BD_BK + 1; }
    }
}

static int popcount8(unsigned m) { int n = 0; for (int s = 0; s < 8; ++s) n += (m >> s) & 1; return n; }

// -> failures; *issued_out = MFMAs per 16-column strip by brute force over the masks
static int check(const char* what, const Pattern& nz, int M, int K, long* issued_out = nullptr, bool blocks = true)
{
    int fails = 0;
    std::vector<int> kr, ext;
    scan(nz, M, K, kr, ext);
    BandPlan plan;
    plan.reset(M, K, kr, ext);
    const int nb = plan.nbands;
    long total = 0;
    for (int b = 0; b < nb; ++b) {
        const int* e = ext.data() + BD_EXT * b;
        int lo, hi;
        band_ext_interior(e, lo, hi);
        long band_total = 0;
        for (int kt = kr[2 * b]; kt < kr[2 * b + 1]; ++kt) {
            bool all_full = true;
            for (int i = 0; i < BD_RT; ++i) {
                const unsigned m = band_ext_mask(e[2 * i], e[2 * i + 1], kt);
                if (m > 0xffu) { printf("%s: band %d tile %d row tile %d: mask %x\n", what, b, kt, i, m); ++fails; }
                all_full = all_full && m == 0xffu;
                band_total += popcount8(m);
                for (int s = 0; s < BD_SUB; ++s) {
                    const int sub = BD_SUB * kt + s;
                    const bool bit = (m >> s) & 1, in = e[2 * i] <= sub && sub < e[2 * i + 1];
                    if (bit != in) { printf("%s: band %d substep %d row tile %d: bit %d, extent says %d\n", what, b, sub, i, bit, in); ++fails; }
                    if (!blocks || bit) continue;
                    for (int r = b * BD_BM + 16 * i; r < b * BD_BM + 16 * i + 16 && r < M; ++r)
                        for (int k = 4 * sub; k < 4 * sub + 4 && k < K; ++k)
                            if (nz(r, k)) { printf("%s: nonzero (%d, %d) masked out\n", what, r, k); ++fails; }
                }
            }
            const bool interior = lo <= kt && kt < hi;
            if (interior != all_full) { printf("%s: band %d tile %d: interior %d, masks full %d\n", what, b, kt, interior, all_full); ++fails; }
        }
        // nothing of an extent lies outside the band's K-tile range
        if (band_total != band_ext_issued(e, kr[2 * b], kr[2 * b + 1])) { printf("%s: band %d issued\n", what, b); ++fails; }
        long whole = 0;
        for (int i = 0; i < BD_RT; ++i) whole += e[2 * i + 1] - e[2 * i];
        if (band_total != whole) { printf("%s: band %d: %ld inside its K tiles, extents hold %ld\n", what, b, band_total, whole); ++fails; }
        total += band_total;
    }
    if (total != plan.mfmas || plan.issued(true) != total || plan.issued(false) != plan.tiles * BD_RT * BD_SUB || total > plan.issued(false)) {
        printf("%s: plan issued %ld / %ld, brute force %ld\n", what, plan.issued(true), plan.issued(false), total); ++fails;
    }
    // every decomposition covers the same MFMAs, item by item (a streamed run may end inside an edge region)
    for (int gn = 1; gn <= 9; gn += (gn < 3 ? 1 : 3)) {
        std::vector<BandItem> items; std::vector<int> wg; std::vector<BandRed> red; int nslots = 0;
        BandPlan::decompose(kr, nb, gn, 256, items, wg, red, nslots);
        long sum = 0;
        for (const BandItem& x : items) sum += band_ext_issued(ext.data() + BD_EXT * x.band, x.kt0, x.kt1);
        if (sum != total) { printf("%s: gn %d items issue %ld, not %ld\n", what, gn, sum, total); ++fails; }
    }
    if (issued_out) *issued_out = total;
    return fails;
}

int main()
{
    int fails = 0;
    long got = 0;
    const Pattern lower = [](int r, int c) { return c <= r; }, upper = [](int r, int c) { return c >= r; };

    // triangular, n = 200: bands 0 and 1 need 100 p + 60, the 40-row band 2 needs 44 + 48 + 50
    fails += check("lower 200", lower, 200, 200, &got);
    if (got != 60 + 160 + 142) { printf("lower 200: %ld\n", got); ++fails; }
    // its transpose: row tile t of all (16 t / 4 .. 50), 200 -> 224 K columns of which the last 24 hold nothing
    fails += check("upper 200", upper, 200, 200, &got);
    { long want = 0; for (int t = 0; 16 * t < 200; ++t) want += 50 - 4 * t; if (got != want) { printf("upper 200: %ld, not %ld\n", got, want); ++fails; } }
    // one live row tile in the last band, four empty ones
    fails += check("lower 176", lower, 176, 176, &got);
    fails += check("upper 176", upper, 176, 176, &got);
    // a block operand: row tiles of one band with different extents at both ends, zero rows inside an extent, a zero
    // column range inside an extent, an empty band, a single nonzero
    const Pattern block = [](int r, int c) {
        if (r >= 160 && r < 240) return false;                      // band 2: empty
        if (r == 100) return false;                                 // a zero row inside an extent
        if (r >= 32 && r < 48) return r == 40 && c == 77;           // row tile 2 of band 0: a single entry
        const int t = r / 16;
        return c >= 3 * t + (r % 5) && c < 40 + 7 * t + (r % 3) && !(c >= 50 && c < 58);
    };
    fails += check("block 333 x 250", block, 333, 250, &got);
    const Pattern holes = [](int r, int c) { return ((r * 2654435761u + c * 40503u) >> 7) % 11 == 0 && (r / 16) % 4 != 1 && c > r / 3; };
    fails += check("holes 500 x 420", holes, 500, 420, &got);
    fails += check("dense 81 x 33", [](int, int) { return true; }, 81, 33, &got);
    if (got != (5 * 9 + 1 * 9)) { printf("dense 81 x 33: %ld\n", got); ++fails; }
    fails += check("zero 100 x 100", [](int, int) { return false; }, 100, 100, &got);
    if (got != 0) { printf("zero: %ld\n", got); ++fails; }

    // n = 5000, the flagship operands (no per-block scan: 25 M entries twice is enough).  Forward: bands 0..61 need
    // 100 p + 60 each and the 40-row band 62 needs 1244 + 1248 + 1250 = 3742 -> 196 562 of the whole tiles' 202 200.
    // Backward: row tile t (rows 16 t ..) runs substeps 4 t .. 1250 -> sum over 313 row tiles of (1250 - 4 t) = 195 938.
    fails += check("lower 5000", lower, 5000, 5000, &got, false);
    if (got != 196562) { printf("lower 5000: %ld\n", got); ++fails; }
    {
        std::vector<int> kr, ext; scan(lower, 5000, 5000, kr, ext);
        BandPlan p; p.reset(5000, 5000, kr, ext);
        if (p.issued(false) != 202200 || p.issued(false) - p.issued(true) != 5638) { printf("lower 5000: whole tiles %ld\n", p.issued(false)); ++fails; }
    }
    fails += check("upper 5000", upper, 5000, 5000, &got, false);
    { long want = 0; for (int t = 0; 16 * t < 5000; ++t) want += 1250 - 4 * t; if (want != 195938 || got != want) { printf("upper 5000: %ld, not %ld\n", got, want); ++fails; } }
    printf("fails=%d\n", fails);
    return fails ? 1 : 0;
}
