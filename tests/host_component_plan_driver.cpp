// Host-side component plan of the trajectory kernel (glmmrmcml_amd/csrc/component_plan.h) under AddressSanitizer +
// UBSan.  Reads the ELL rows of ZL from the file named on the command line ("n Q W", n widths, n * W columns in
// column-major order), builds the plan, checks its invariants -- the components partition 0 .. Q-1, every observation
// lies in exactly one component together with all its columns, the local indices are a bijection, the records hold
// every entry once and in order, the quarters cut at whole observations, the work items cover every component exactly
// once -- and prints the counts.  Built and run by tests/test_component_plan_cpu.py.
#include "component_plan.h"
#include <cstdio>
using namespace mcml;

#define CHECK(cond, ...) do { if (!(cond)) { printf(__VA_ARGS__); printf("\n"); ++fails; } } while (0)

int main(int argc, char** argv)
{
    if (argc < 2) { printf("usage: driver FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    int n = 0, Q = 0, W = 0;
    if (fscanf(f, "%d %d %d", &n, &Q, &W) != 3 || n <= 0 || Q <= 0 || W <= 0) { printf("bad header\n"); return 2; }
    std::vector<int> width(n), col((size_t)n * W);
    for (int& v : width) if (fscanf(f, "%d", &v) != 1) { printf("bad widths\n"); return 2; }
    for (int& v : col) if (fscanf(f, "%d", &v) != 1) { printf("bad columns\n"); return 2; }
    fclose(f);
    ComponentPlan p;
    component_plan_build(n, Q, W, col, width, p);
    int fails = 0;
    // partition of the variables, bijective local indices
    CHECK((int)p.var_ptr.size() == p.ncomp + 1 && p.var_ptr[0] == 0 && p.var_ptr[p.ncomp] == Q, "var_ptr does not cover Q");
    std::vector<int> seen(Q, 0);
    int max_vars = 0;
    for (int c = 0; c < p.ncomp; ++c) {
        const int nv = p.var_ptr[c + 1] - p.var_ptr[c];
        CHECK(nv >= 1, "component %d has no variable", c);
        max_vars = std::max(max_vars, nv);
        for (int j = 0; j < nv; ++j) {
            const int q = p.vars[p.var_ptr[c] + j];
            CHECK(q >= 0 && q < Q, "variable out of range");
            if (q < 0 || q >= Q) continue;
            ++seen[q];
            CHECK(p.comp_of_var[q] == c && p.local_of_var[q] == j, "variable %d: component / local index", q);
            CHECK(j == 0 || q > p.vars[p.var_ptr[c] + j - 1], "component %d: variables not ascending", c);
        }
    }
    for (int q = 0; q < Q; ++q) CHECK(seen[q] == 1, "variable %d in %d components", q, seen[q]);
    CHECK(max_vars == p.max_vars, "max_vars");
    // observations
    CHECK(p.row_ptr[0] == 0 && p.row_ptr[p.ncomp] == n, "row_ptr does not cover n");
    std::vector<int> rseen(n, 0);
    int max_rows = 0, empty = 0;
    for (int c = 0; c < p.ncomp; ++c) {
        const int nr = p.row_ptr[c + 1] - p.row_ptr[c];
        max_rows = std::max(max_rows, nr); empty += nr == 0;
        for (int t = p.row_ptr[c]; t < p.row_ptr[c + 1]; ++t) {
            const int i = p.rows[t];
            CHECK(i >= 0 && i < n, "observation out of range");
            if (i < 0 || i >= n) continue;
            ++rseen[i];
            CHECK(t == p.row_ptr[c] || i > p.rows[t - 1], "component %d: observations not ascending", c);
            for (int k = 0; k < width[i]; ++k) CHECK(p.comp_of_var[col[i + (size_t)k * n]] == c, "observation %d leaves its component", i);
        }
    }
    for (int i = 0; i < n; ++i) CHECK(rseen[i] == 1, "observation %d in %d components", i, rseen[i]);
    CHECK(max_rows == p.max_rows && empty == p.empty_comps, "max_rows / empty_comps");
    CHECK(p.feasible == (p.max_vars <= CP_MAX_VARS), "feasible");
    // two variables of different components share no observation is implied above; the components are also maximal:
    // variables of one component are linked through observations (checked by counting: a finer partition would pass the
    // tests above, so compare with a second union-find)
    {
        std::vector<int> par(Q);
        for (int q = 0; q < Q; ++q) par[q] = q;
        auto find = [&](int q) { while (par[q] != q) q = par[q] = par[par[q]]; return q; };
        for (int i = 0; i < n; ++i) for (int k = 1; k < width[i]; ++k) par[find(col[i + (size_t)k * n])] = find(col[i]);
        int roots = 0;
        for (int q = 0; q < Q; ++q) roots += find(q) == q;
        CHECK(roots == p.ncomp, "%d components, a second union-find finds %d", p.ncomp, roots);
    }
    if (p.feasible) {
        CHECK((int)p.slot_i.size() == 8 * p.nslots && (int)p.slot_src.size() == 4 * p.nslots, "record arrays");
        CHECK(p.slot_ptr[0] == 0 && p.slot_ptr[p.ncomp] == p.nslots, "slot_ptr");
        for (int c = 0; c < p.ncomp; ++c) {
            int s = p.slot_ptr[c];
            const int nv = p.var_ptr[c + 1] - p.var_ptr[c];
            std::vector<int> starts;
            for (int t = p.row_ptr[c]; t < p.row_ptr[c + 1]; ++t) {
                const int i = p.rows[t];
                starts.push_back(s);
                int k = 0;
                for (;; ++s) {
                    CHECK(s < p.slot_ptr[c + 1], "component %d: records run out", c);
                    if (s >= p.slot_ptr[c + 1]) break;
                    const int* r = &p.slot_i[8 * (size_t)s];
                    CHECK(r[6] == i && r[4] >= 0 && r[4] <= CP_SLOT, "record %d: observation / count", s);
                    for (int u = 0; u < r[4] && u < CP_SLOT; ++u, ++k) {
                        CHECK(k < width[i] && r[u] >= 0 && r[u] < nv && p.vars[p.var_ptr[c] + r[u]] == col[i + (size_t)k * n], "record %d entry %d: column", s, u);
                        CHECK(p.slot_src[4 * (size_t)s + u] == i + k * n, "record %d entry %d: source", s, u);
                    }
                    for (int u = r[4]; u < CP_SLOT; ++u) CHECK(p.slot_src[4 * (size_t)s + u] == -1, "record %d: padding", s);
                    if (r[5]) { ++s; break; }
                }
                CHECK(k == width[i], "observation %d: %d of %d entries", i, k, width[i]);
            }
            CHECK(s == p.slot_ptr[c + 1], "component %d: records left over", c);
            starts.push_back(p.slot_ptr[c + 1]);
            const int* qv = &p.slot_quarter[5 * (size_t)c];
            CHECK(qv[0] == p.slot_ptr[c] && qv[4] == p.slot_ptr[c + 1], "component %d: quarters do not span it", c);
            for (int w = 0; w < 4; ++w) {
                CHECK(qv[w] <= qv[w + 1], "component %d: quarters not monotone", c);
                CHECK(std::find(starts.begin(), starts.end(), qv[w]) != starts.end(), "component %d: a quarter cuts an observation", c);
            }
        }
        CHECK(p.nitems() >= 1 && p.item_ptr[0] == 0 && p.item_ptr.back() == p.ncomp, "items do not cover the components");
        for (int t = 0; t < p.nitems(); ++t) CHECK(p.item_ptr[t] < p.item_ptr[t + 1], "item %d is empty", t);
    }
    printf("ncomp=%d max_vars=%d max_rows=%d empty_comps=%d feasible=%d nitems=%d waves=%d cap=%d\n", p.ncomp, p.max_vars, p.max_rows,
           p.empty_comps, p.feasible ? 1 : 0, p.feasible ? p.nitems() : 0, p.feasible ? cp_waves(p) : 0, CP_MAX_VARS);
    printf("fails=%d\n", fails);
    return fails ? 1 : 0;
}
