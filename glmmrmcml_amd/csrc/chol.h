// chol.h -- the dense Cholesky stack (chol.hip): blocked factorisation with its captured two-chain schedule, the two
// triangular solves against the factor and the one-vector solve.  The MVN likelihood (mvn.hip), the Laplace fits
// (laplace.hip), the exact conditional draws (hmc_exact.h) and glmmr_mcml_dbg_chol all factorise through it; its state
// lives in Ctx::chol.
#pragma once
#include "common.h"

namespace mcml {

struct Ctx;

constexpr int CHOL_NB = 128;     // panel / leaf size of the blocked Cholesky / TRSM
constexpr int SMALL_BLOCK = 32;  // blocks up to this size are factorised one wave each

// the factorisation's launch sequence as a hipGraph (chol.hip potrf_graphed): the theta-step evaluates the same
// (matrix, shape) dozens of times per MCML iteration; key = what the captured kernels' arguments depend on
struct CholGraph {
    hipGraphExec_t exec = nullptr;
    const double* A = nullptr; const double* linv = nullptr; int lda = 0, n = 0, extra = 0, seen = 0;
    long long used = 0;                 // launch counter value at the last use (the least recently used entry is replaced)
    // Calibration (chol.hip potrf_graphed).  On this stack every other hipGraphInstantiate in a process yields an
    // executable whose two chains run 1.5-2x slower than the same graph instantiated before or after it (measured: the
    // 3rd and 5th instantiation; the parallel branch lands on a hardware queue that does not overlap with the launch
    // stream's).  The first replays are therefore timed against the eager launch sequence and a slow executable is
    // instantiated again from the kept template.
    hipGraph_t tmpl = nullptr;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    float eager_ms = 0.f, best_ms = 0.f;
    hipGraphExec_t best = nullptr;      // fastest executable seen so far while `exec` is the one on trial
    int tries = 0, trial_launches = 0;  // an executable's first launch carries its upload: the second one is timed
    bool timed = false, settled = false;
    void release() {
        if (best && best != exec) (void)hipGraphExecDestroy(best);
        best = nullptr;
        if (exec) { (void)hipGraphExecDestroy(exec); exec = nullptr; }
        if (tmpl) { (void)hipGraphDestroy(tmpl); tmpl = nullptr; }
        if (t0) { (void)hipEventDestroy(t0); t0 = nullptr; }
        if (t1) { (void)hipEventDestroy(t1); t1 = nullptr; }
    }
};
// a few graphs side by side: a model with two or more large covariance blocks of different size evaluates them in turn,
// and a one-entry cache would re-capture (i.e. run eagerly) every time.  Every graph is a two-chain one (a single
// evaluation): at most two of those are kept alive (of three or more alive in a process every new instantiation measured
// slow, whatever the number of tries)
struct CholGraphCache {
    static constexpr int CAP = 2;
    std::vector<CholGraph> g;
    long long tick = 0;
    void clear() { for (CholGraph& e : g) e.release(); g.clear(); }
    ~CholGraphCache() { clear(); }
    CholGraphCache() = default;
    CholGraphCache(const CholGraphCache&) = delete;
    CholGraphCache& operator=(const CholGraphCache&) = delete;
    CholGraphCache(CholGraphCache&& o) noexcept : g(std::move(o.g)), tick(o.tick) { o.g.clear(); }
    CholGraphCache& operator=(CholGraphCache&& o) noexcept { if (this != &o) { clear(); g = std::move(o.g); tick = o.tick; o.g.clear(); } return *this; }
    CholGraph& find(const double* A, const double* linv, int lda, int n, int extra) {
        ++tick;
        for (CholGraph& e : g)
            if (e.A == A && e.linv == linv && e.lda == lda && e.n == n && e.extra == extra) { e.used = tick; return e; }
        size_t old = 0;
        for (size_t i = 1; i < g.size(); ++i)
            if (g[i].used < g[old].used) old = i;
        if ((int)g.size() >= CAP) {
            g[old].release();
            g[old] = CholGraph();
            std::swap(g[old], g.back());
        } else g.push_back(CholGraph());
        CholGraph& e = g.back();
        e.A = A; e.linv = linv; e.lda = lda; e.n = n; e.extra = extra; e.seen = 0; e.used = tick;
        return e;
    }
};

// what the stack keeps between calls (Ctx::chol)
struct CholState {
    DevBuf linv;                    // the inverted diagonal blocks of the last factorisation: (n/128 + 1) x 128 x 128 per matrix
    // side streams + events for the look-ahead (potrf_blocked)
    hipStream_t aux = nullptr;      // high priority: the leaf of the eager fork-join
    hipStream_t aux_lo = nullptr;   // lowest priority: the bulk chain of the captured schedule
    hipEvent_t ev_col = nullptr, ev_leaf = nullptr;
    CholGraphCache graphs;
    std::vector<hipEvent_t> ev_ring;    // one event per dependency edge of the captured schedule (potrf_la2_capture)
    ~CholState();
};

// Several matrices of the same shape factorised side by side (the candidate thetas of one theta-step round): every
// launch of the schedule covers all of them (leaf: one workgroup per matrix; products: blockIdx.y), so the latency
// chain of the late steps -- leaf, two single-block products, their gaps -- is paid once per round, not once per
// candidate.  sA / sL: element strides from one matrix / one set of inverted diagonal blocks to the next.
// round: candidates of the optimiser's round the n matrices stand for (0: n itself) -- what the schedule is chosen by
struct Bat { int n = 1; size_t sA = 0, sL = 0; int* err = nullptr; int round = 0; };   // err: one flag per matrix (null: the context's own)

// size of c.chol.linv for an n x n factorisation, in doubles: one inverted 128 x 128 diagonal block per panel
inline size_t linv_size(int n) { return (size_t)(n / CHOL_NB + 1) * CHOL_NB * CHOL_NB; }

// what every run of leaves needs first: room for the inverted diagonal blocks of `nbatch` n x n matrices, zeroed, and the
// leaf's LDS
int leaf_prepare(Ctx& c, int n, int nbatch);
// the n x n lower triangle of A factorised in place with `extra` more rows carried below it (they leave as X inv(L)'),
// for every matrix of bt: the eager launches, or (one matrix, n > 256) the captured two-chain schedule replayed.
// After leaf_prepare
int potrf_blocked(Ctx& c, double* A, int lda, int n, int extra, Bat bt = Bat());
int potrf_graphed(Ctx& c, double* A, int lda, int n, int extra, Bat bt = Bat());
int potrf_lower(Ctx& c, double* A, int n, int lda);                          // in place
int potrf_leaf_profile(Ctx& c, unsigned long long* host10);                 // debug: phase clocks of one leaf
int potrf_lower_checked(Ctx& c, double* A, int n, int lda);                  // + MCML_ENOTPD if a pivot failed
// a kernel raised c.errflag() (a non-positive pivot): the flag is cleared, `message` becomes the error, MCML_ENOTPD.
// Synchronises the stream
int check_errflag(Ctx& c, const char* message);
// x <- (L L')^-1 x for one vector, L from the LAST potrf_lower (its diagonal-block inverses are in c.chol.linv)
int potrs_lower_vec(Ctx& c, const double* L, int ldl, int n, double* x, double* tmp);
int trsm_left_lower(Ctx& c, const double* L, int ldl, int n, double* U, int ldu, int m);
// T <- R^-T T (the transposed solve of the same factor, all m columns at once)
int trsm_left_lower_trans(Ctx& c, const double* R, int ldr, int n, double* T, int ldt, int m);

}  // namespace mcml
