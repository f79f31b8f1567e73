// component_plan.h -- host side of component.h: the connected components of the coupling graph of ZL, the records its kernels
// read (hmc_traj.h, component.hip, hmc_exact_comp.h) and the work items of the trajectory kernel.  In the whitened variables the
// prior is N(0, I), so two random effects interact only through an observation whose row of ZL touches both: a union-find over
// the ELL rows gives components whose whole leapfrog trajectory needs no data of any other component (configs 1, 4, 5: 10 / 40 /
// 2000 components of at most 6 / 8 / 11 variables).  Plain vectors in, plain vectors out: no device, no HIP header, so
// that tests/host_component_plan_driver.cpp compiles it with g++ under the sanitizers.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace mcml {

// One wave keeps x, r and the gradient accumulator of a component in LDS as [local variable][64 lanes] doubles: 1.5 KB per
// variable (WAVES = 1); the four-wave form shares x and r and gives every wave its own accumulator: 3 KB per variable
// per workgroup.  160 KB of LDS per CU / 4.5 KB = 35 variables would still leave a CU room for one workgroup of either
// form plus one more wave; 32 keeps the four-wave form at 104 KB (one workgroup per CU) and three single waves per CU.
constexpr int CP_LDS_BYTES_PER_CU = 160 * 1024;
constexpr int CP_MAX_VARS = 32;
static_assert(CP_MAX_VARS >= 16 && CP_MAX_VARS < 48, "the fallback tests rely on a sparse design above the cap");
static_assert(CP_MAX_VARS * 3 * 512 * 3 <= CP_LDS_BYTES_PER_CU && CP_MAX_VARS * 6 * 512 + 8192 <= CP_LDS_BYTES_PER_CU, "LDS budget");
// The factor kernels (component.hip) keep only the nv x nv matrix of a component in LDS: the workgroup form takes up to
// CP_WIDE_MAX_VARS variables (about 146 KB at the cap, one workgroup per CU).  The trajectory kernel keeps CP_MAX_VARS.
constexpr int CP_WIDE_MAX_VARS = 128;
static_assert(CP_WIDE_MAX_VARS >= CP_MAX_VARS, "a plan the trajectory kernel takes has records");
constexpr int CP_SLOT = 4;            // entries of ZL per metadata record (one batch of scalar loads)
constexpr int CP_TARGET_ITEMS = 1024; // work items aimed at when components are packed (a guess, not measured)
// the four-wave form (a workgroup per component and chain block, the observations split over its waves) is taken when
// the largest component has this many observations or more.  A guess until measured: config 4 has 400 per component
// and only 40 components, configs 1 and 5 have 50 and 10.
constexpr int CP_WAVES4_ROWS = 128;

// the four-wave form adds 8 KB in which the waves' four per-chain sums meet
inline int cp_lds_bytes(int max_vars, int waves) { return waves == 4 ? max_vars * 512 * 6 + 8192 : max_vars * 512 * 3; }

struct ComponentPlan {
    int n = 0, Q = 0, W = 0;
    int ncomp = 0, max_vars = 0, max_rows = 0, empty_comps = 0;
    bool feasible = false;                        // max_vars <= CP_MAX_VARS: the trajectory kernel's work items are built
    bool records = false;                         // max_vars <= CP_WIDE_MAX_VARS: the record arrays are built
    std::vector<int> comp_of_var, local_of_var;   // Q
    std::vector<int> var_ptr, vars;               // ncomp + 1, Q: the global variables of a component, ascending
    std::vector<int> row_ptr, rows;               // ncomp + 1, n: its observations, ascending
    std::vector<int> comp_of_row;                 // n
    // metadata records of CP_SLOT entries, in component order, observations ascending inside a component; an
    // observation of w entries takes ceil(w / CP_SLOT) consecutive records (at least one)
    int nslots = 0;
    std::vector<int> slot_ptr;                    // ncomp + 1
    std::vector<int> slot_quarter;                // 5 per component: where the four waves of the four-wave form start (whole observations)
    std::vector<int> slot_i;                      // 8 per record: local columns [4], entries in the record, 1 if the observation ends here, observation, 0
    std::vector<int> slot_src;                    // 4 per record: index into ell_val (i + k * n), -1 for padding
    std::vector<int> item_ptr;                    // nitems + 1: components [item_ptr[t], item_ptr[t + 1]) in turn
    int nitems() const { return (int)item_ptr.size() - 1; }
};

// waves per component (or work item) of a kernel with two forms: k_cm_traj<FL, 1 | 4> on a feasible plan, k_lac_factor /
// k_lac_factor_wg under "component_wide".  One wave below CP_WAVES4_ROWS observations in the largest component (config 5: 10), a
// guess for both: config 4 (400) is the one measured point above it (profiles/la_component_wide_timing.json).  forced: 1 or 4
// for that form, else the rule; above CP_MAX_VARS variables only the workgroup form exists: forcing one wave is ignored
inline int cp_waves(const ComponentPlan& p, int forced = -1)
{
    if (p.max_vars > CP_MAX_VARS) return 4;
    if (forced == 1 || forced == 4) return forced;
    return p.max_rows >= CP_WAVES4_ROWS ? 4 : 1;
}
// the A/B switch of the two forms, = 1 | 4, read per call (a test runs both in one process)
constexpr const char* CP_TRAJ_WAVES_ENV = "GLMMR_MCML_TRAJ_WAVES";   // the trajectory kernel's
constexpr const char* CP_LA_WAVES_ENV = "GLMMR_MCML_LA_WAVES";       // the factor kernels'
inline int cp_forced_waves(const char* env)
{
    const char* e = getenv(env);
    if (e && !strcmp(e, "1")) return 1;
    if (e && !strcmp(e, "4")) return 4;
    return -1;
}
// where the nv x nv factor of each component starts in the exact draws' scratch: ncomp + 1 offsets in doubles
inline std::vector<int> comp_factor_offsets(const ComponentPlan& p)
{
    std::vector<int> off(p.ncomp + 1, 0);
    for (int k = 0; k < p.ncomp; ++k) { const int nv = p.var_ptr[k + 1] - p.var_ptr[k]; off[k + 1] = off[k] + nv * nv; }
    return off;
}

// col, width: the ELL rows of ZL (col[i + k * n], k < width[i]), as sparse_zl_setup builds them
inline void component_plan_build(int n, int Q, int W, const std::vector<int>& col, const std::vector<int>& width, ComponentPlan& p)
{
    p = ComponentPlan();
    p.n = n; p.Q = Q; p.W = W;
    std::vector<int> parent(Q);
    for (int q = 0; q < Q; ++q) parent[q] = q;
    auto find = [&](int q) { while (parent[q] != q) { parent[q] = parent[parent[q]]; q = parent[q]; } return q; };
    for (int i = 0; i < n; ++i)
        for (int k = 1; k < width[i]; ++k) {
            const int a = find(col[i]), b = find(col[i + (size_t)k * n]);
            if (a != b) parent[a > b ? a : b] = a > b ? b : a;     // the root is the smallest variable: components in order of it
        }
    p.comp_of_var.assign(Q, -1); p.local_of_var.assign(Q, 0);
    std::vector<int> cnt;
    for (int q = 0; q < Q; ++q) {
        const int r = find(q);
        if (p.comp_of_var[r] < 0) { p.comp_of_var[r] = p.ncomp++; cnt.push_back(0); }     // r <= q: seen first
        p.comp_of_var[q] = p.comp_of_var[r];
        p.local_of_var[q] = cnt[p.comp_of_var[q]]++;
    }
    p.var_ptr.assign(p.ncomp + 1, 0);
    for (int c = 0; c < p.ncomp; ++c) p.var_ptr[c + 1] = p.var_ptr[c] + cnt[c];
    p.vars.assign(Q, 0);
    for (int q = 0; q < Q; ++q) p.vars[p.var_ptr[p.comp_of_var[q]] + p.local_of_var[q]] = q;
    p.comp_of_row.assign(n, 0);
    std::vector<int> rcnt(p.ncomp, 0);
    for (int i = 0; i < n; ++i) {
        // an observation without entries couples nothing; it still adds its log f to the density: component 0 takes it
        const int c = width[i] > 0 ? p.comp_of_var[col[i]] : 0;
        p.comp_of_row[i] = c; ++rcnt[c];
    }
    p.row_ptr.assign(p.ncomp + 1, 0);
    for (int c = 0; c < p.ncomp; ++c) p.row_ptr[c + 1] = p.row_ptr[c] + rcnt[c];
    p.rows.assign(n, 0);
    {
        std::vector<int> fill(p.row_ptr.begin(), p.row_ptr.end() - 1);
        for (int i = 0; i < n; ++i) p.rows[fill[p.comp_of_row[i]]++] = i;
    }
    for (int c = 0; c < p.ncomp; ++c) {
        p.max_vars = std::max(p.max_vars, cnt[c]);
        p.max_rows = std::max(p.max_rows, rcnt[c]);
        p.empty_comps += rcnt[c] == 0;
    }
    p.feasible = p.ncomp > 0 && p.max_vars <= CP_MAX_VARS;
    p.records = p.ncomp > 0 && p.max_vars <= CP_WIDE_MAX_VARS;
    if (!p.records) return;
    // records: read by the trajectory kernel and by the Laplace kernels
    p.slot_ptr.assign(p.ncomp + 1, 0);
    p.slot_quarter.assign(5 * (size_t)p.ncomp, 0);
    for (int c = 0; c < p.ncomp; ++c) {
        const int r0 = p.row_ptr[c], r1 = p.row_ptr[c + 1], nr = r1 - r0, per = (nr + 3) / 4;
        p.slot_ptr[c] = (int)(p.slot_i.size() / 8);
        std::vector<int> first(nr + 1);
        for (int t = r0; t < r1; ++t) {
            first[t - r0] = (int)(p.slot_i.size() / 8);
            const int i = p.rows[t], wi = width[i], nrec = std::max(1, (wi + CP_SLOT - 1) / CP_SLOT);
            for (int s = 0; s < nrec; ++s) {
                const int k0 = s * CP_SLOT, ne = std::max(0, std::min(CP_SLOT, wi - k0));
                int rec[8] = {0, 0, 0, 0, ne, s + 1 == nrec ? 1 : 0, i, 0}, src[4] = {-1, -1, -1, -1};
                for (int u = 0; u < ne; ++u) { rec[u] = p.local_of_var[col[i + (size_t)(k0 + u) * n]]; src[u] = i + (k0 + u) * n; }
                p.slot_i.insert(p.slot_i.end(), rec, rec + 8);
                p.slot_src.insert(p.slot_src.end(), src, src + 4);
            }
        }
        first[nr] = (int)(p.slot_i.size() / 8);
        for (int w = 0; w <= 4; ++w) p.slot_quarter[5 * (size_t)c + w] = first[std::min(w * per, nr)];   // contiguous quarters of the observations
    }
    p.nslots = (int)(p.slot_i.size() / 8);
    p.slot_ptr[p.ncomp] = p.nslots;
    if (!p.feasible) return;
    // work items: consecutive components, packed until an item costs what the costliest component does or the total spread
    // over CP_TARGET_ITEMS items, whichever is more -- so that a one-variable component rides with its neighbours
    auto cost = [&](int c) { return (long)(p.slot_ptr[c + 1] - p.slot_ptr[c]) + 2L * (p.var_ptr[c + 1] - p.var_ptr[c]); };
    long total = 0, big = 0;
    for (int c = 0; c < p.ncomp; ++c) { total += cost(c); big = std::max(big, cost(c)); }
    const long target = std::max(big, (total + CP_TARGET_ITEMS - 1) / CP_TARGET_ITEMS);
    long run = 0;
    p.item_ptr.push_back(0);
    for (int c = 0; c < p.ncomp; ++c) {
        if (run > 0 && run + cost(c) > target) { p.item_ptr.push_back(c); run = 0; }
        run += cost(c);
    }
    p.item_ptr.push_back(p.ncomp);
}

}  // namespace mcml
