// Host-side component plan (glmmrmcml_amd/csrc/component_plan.h) above the trajectory kernel's cap, under
// AddressSanitizer + UBSan: the record arrays that the Laplace kernels read are built up to CP_WIDE_MAX_VARS variables
// per component, the trajectory's work items only up to CP_MAX_VARS.  Reads the ELL rows of ZL as
// host_component_plan_driver.cpp does ("n Q W", n widths, n * W columns in column-major order), checks the flags and,
// where the plan has records, the invariants of the records -- their sizes, the bounds of slot_ptr, every local column
// below the component's variable count, every entry once and in order, the flag of an observation's last record, the
// quarters -- and prints the counts and an FNV-1a hash of every record array.  Built and run by
// tests/test_component_plan_wide_cpu.py.
#include "component_plan.h"
#include <cstdint>
#include <cstdio>
using namespace mcml;

#define CHECK(cond, ...) do { if (!(cond)) { printf(__VA_ARGS__); printf("\n"); ++fails; } } while (0)

static unsigned long long fnv(const std::vector<int>& v)
{
    unsigned long long h = 1469598103934665603ull;
    for (int x : v)
        for (int b = 0; b < 4; ++b) { h ^= ((uint32_t)x >> (8 * b)) & 0xffu; h *= 1099511628211ull; }
    return h;
}

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
    CHECK(p.feasible == (p.ncomp > 0 && p.max_vars <= CP_MAX_VARS), "feasible");
    CHECK(p.records == (p.ncomp > 0 && p.max_vars <= CP_WIDE_MAX_VARS), "records");
    CHECK(!p.feasible || p.records, "a feasible plan has records");
    if (!p.records) CHECK(p.nslots == 0 && p.slot_ptr.empty() && p.slot_i.empty() && p.slot_src.empty() && p.slot_quarter.empty(), "no records, yet record arrays");
    if (!p.feasible) CHECK(p.item_ptr.empty(), "not feasible, yet work items");
    if (p.records) {
        CHECK((int)p.slot_i.size() == 8 * p.nslots && (int)p.slot_src.size() == 4 * p.nslots, "record arrays");
        CHECK((int)p.slot_ptr.size() == p.ncomp + 1 && (int)p.slot_quarter.size() == 5 * p.ncomp, "slot_ptr / slot_quarter sizes");
        CHECK(p.slot_ptr[0] == 0 && p.slot_ptr[p.ncomp] == p.nslots, "slot_ptr");
        for (int c = 0; c < p.ncomp; ++c) {
            CHECK(p.slot_ptr[c] <= p.slot_ptr[c + 1], "slot_ptr not monotone at %d", c);
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
                    CHECK(r[6] == i && r[4] >= 0 && r[4] <= CP_SLOT && r[7] == 0, "record %d: observation / count", s);
                    CHECK(r[5] == 0 || r[5] == 1, "record %d: flag", s);
                    for (int u = 0; u < r[4] && u < CP_SLOT; ++u, ++k) {
                        CHECK(k < width[i] && r[u] >= 0 && r[u] < nv && p.vars[p.var_ptr[c] + r[u]] == col[i + (size_t)k * n], "record %d entry %d: column", s, u);
                        CHECK(p.slot_src[4 * (size_t)s + u] == i + k * n, "record %d entry %d: source", s, u);
                    }
                    for (int u = r[4]; u < CP_SLOT; ++u) CHECK(r[u] == 0 && p.slot_src[4 * (size_t)s + u] == -1, "record %d: padding", s);
                    // the flag is set on the record that holds the observation's last entry, and on no earlier one
                    CHECK((r[5] == 1) == (k >= width[i]), "record %d: last-record flag", s);
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
    }
    if (p.feasible) {
        CHECK(p.nitems() >= 1 && p.item_ptr[0] == 0 && p.item_ptr.back() == p.ncomp, "items do not cover the components");
        for (int t = 0; t < p.nitems(); ++t) CHECK(p.item_ptr[t] < p.item_ptr[t + 1], "item %d is empty", t);
    }
    // the fields of host_component_plan_driver.cpp's line, then the flags and hashes
    printf("ncomp=%d max_vars=%d max_rows=%d empty_comps=%d feasible=%d nitems=%d waves=%d cap=%d\n", p.ncomp, p.max_vars, p.max_rows,
           p.empty_comps, p.feasible ? 1 : 0, p.feasible ? p.nitems() : 0, p.feasible ? cp_waves(p) : 0, CP_MAX_VARS);
    printf("wide records=%d wide_cap=%d nslots=%d h_slot_ptr=%llu h_slot_i=%llu h_slot_src=%llu h_slot_quarter=%llu h_item_ptr=%llu\n",
           p.records ? 1 : 0, CP_WIDE_MAX_VARS, p.nslots, fnv(p.slot_ptr), fnv(p.slot_i), fnv(p.slot_src), fnv(p.slot_quarter), fnv(p.item_ptr));
    printf("fails=%d\n", fails);
    return fails ? 1 : 0;
}
