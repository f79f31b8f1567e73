"""Sequences of calls on ONE resident context against fresh twins (test_gpu_context_sequences.py), and the inputs they
run on with the properties those inputs are named for (test_context_sequences_cpu.py).  Importable without a GPU.

The contract (DESIGN.md "What a context holds between calls"): what a call returns depends on its arguments and on the
context's LOGICAL state -- the model, the last successful update_L / set_L, the samples, the mode setters in force --
never on the calls that came before.  A Twin keeps that logical state beside its long-lived context, and every step
that returns something is run again on a context created for it and given only that state: the two results must be
equal bit for bit (plans are functions of the K-tile ranges and the column-tile count alone, every reduction has a
fixed order, graph replay is pinned to the eager bits: test_gpu_band_bits.py, test_gpu_sampler_bits.py,
test_gpu_dense_la_bits.py)."""
import numpy as np

from glmmrmcml_amd import api, synth

import test_gpu_dense_products as dp
from test_gpu_dense_products import ADAPT, IT, LAM, MS, SEED, TA, WARM

THETA = dp.THETA
THETA2 = (0.08, 0.15)
BM, BK = 80, 32                        # band_plan.h BD_BM, BD_BK
NUTS = dict(warmup=14, max_treedepth=6)


# ------------------------------------------------------------------------------------------ S1: the four structures
def s1_design(Q=333):
    return dp.design("binomial", "logit", Q)


def s1_factors(LA):
    """LA the factor itself; LB its entries more than 96 below the diagonal dropped (every band starts at a later K
    tile); LC a strictly upper part added (nothing to skip: no banded kernel); LD = LB without rows and columns 160..239
    (one empty band of ZL and one of ZL')"""
    Q = LA.shape[0]
    i, j = np.indices((Q, Q))
    LB = np.where(i - j > 96, 0.0, LA)
    LC = LA + 0.01 * np.triu(np.random.default_rng(17).normal(size=(Q, Q)), 1)
    LD = LB.copy()
    LD[160:240, :] = 0.0
    LD[:, 160:240] = 0.0
    return dict(LA=np.asfortranarray(LA), LB=np.asfortranarray(LB), LC=np.asfortranarray(LC), LD=np.asfortranarray(LD))


def band_ranges(A):
    """k_band_ranges (dgemm_band.h) restated: per 80-row band of A the first and one past the last 32-wide K tile that
    holds a nonzero, (0, 0) for an empty band"""
    out = []
    for r0 in range(0, A.shape[0], BM):
        cols = np.flatnonzero((A[r0:r0 + BM] != 0.0).any(axis=0))
        out.append((0, 0) if cols.size == 0 else (int(cols[0]) // BK, int(cols[-1]) // BK + 1))
    return out


def band_rule(A):
    """model_update_L's rule: the banded kernel is used when it skips at least a fifth of the K tiles"""
    kr = band_ranges(A)
    tiles = sum(k1 - k0 for k0, k1 in kr)
    dense = len(kr) * -(-A.shape[1] // BK)
    return tiles * 5 <= dense * 4


# ------------------------------------------------------------------------------------------ S2: the sparse designs
def s2_designs():
    """name -> (design, second theta, the sparse operator is the factored one)"""
    out = {"product": (synth.cluster_rct(ncl=6, nt=4, nind=5, family="poisson"), (0.3, 0.15), False),
           "factored": (synth.stepped_wedge(ncl=6, nt=4, nind=30), (0.3, 0.7), True),
           "gaussian": (gaussian_rct(), (0.3, 0.15), False)}
    for d, _, _ in out.values():
        d["zkind"] = "general"                     # dense_products._oracle_model: ZL = Z L
    return out


def gaussian_rct():
    """cluster_rct's design with a gaussian / identity response (the exact draws apply)"""
    d = synth.cluster_rct(ncl=6, nt=4, nind=5)
    rng = np.random.default_rng(91)
    Lb = np.r_[np.full(6, d["theta"][0]), np.full(24, d["theta"][1])]
    d.update(family="gaussian", link="identity", y=d["X"] @ d["beta"] + d["Z"] @ (Lb * rng.normal(size=d["Q"]))
             + 0.7 * rng.normal(size=d["n"]))
    return d


def cov_blocks(cov):
    """(first row, dimension) of every covariance block of a cov table"""
    cov = np.asarray(cov)
    first = np.r_[True, cov[1:, 0] != cov[:-1, 0]]
    dims = cov[first, 1]
    return list(zip(np.r_[0, np.cumsum(dims)[:-1]].tolist(), dims.tolist()))


def sparse_form(d):
    """(nnz(ZL), nnz(Z), nnz(L), factored) by sparse_zl_setup's rule 4 (nz + nl + 2 Q) < 3 nnz (model.hip)"""
    start = np.zeros(d["Q"], dtype=int)
    nl = 0
    for m0, dim in cov_blocks(d["cov"]):
        start[m0:m0 + dim] = m0
        nl += dim * (dim + 1) // 2
    _, cols = np.nonzero(d["Z"])
    nnz = int((cols - start[cols] + 1).sum())
    nz = int(cols.size)
    return nnz, nz, nl, 4 * (nz + nl + 2 * d["Q"]) < 3 * nnz


# ------------------------------------------------------------------------------------------ S5: theta without a value
def bad_thetas():
    """(design, a theta whose D the oracle factorises, one it refuses)"""
    sw = synth.stepped_wedge(ncl=6, nt=4, nind=30)
    return {"fexp": (s1_design(), np.array(THETA), np.array([-0.05, 0.1])),
            "ar1": (sw, sw["theta"], np.array([0.25, 1.156]))}


# ------------------------------------------------------------------------------------------ steps
def vp_of(d):
    return next(c[2] for c in dp.CASES if c[:2] == (d["family"], d["link"]))


def new_context(d):
    return api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"])


def hmc(d, C, nsamp=None, seed=SEED):
    """the sampler settings of test_gpu_dense_products.py: C chains, one draw each unless nsamp says otherwise"""
    def step(ctx):
        diag, flags, probs = ctx.hmc_sample(d["beta"], vp_of(d), WARM, nsamp or C, LAM, MS, TA, seed, chains=C, iter_idx=IT,
                                            adapt=ADAPT, want_trace=True)
        return dict(u=ctx.get_u(), flags=flags.copy(), probs=probs.copy(), diag=diag, kernels=ctx.last_kernels())
    return step


def nuts(d, C):
    def step(ctx):
        diag, tr = ctx.nuts_sample(d["beta"], vp_of(d), NUTS["warmup"], C, SEED, chains=C, iter_idx=IT,
                                   max_treedepth=NUTS["max_treedepth"], want_trace=True)
        return dict(u=ctx.get_u(), diag=diag, kernels=ctx.last_kernels(), **tr)
    return step


def lpg_input(d, ncols, seed=3):
    return np.asfortranarray(np.random.default_rng(seed).normal(size=(d["Q"], ncols)) * 0.3)


def log_prob_grad(d, V):
    def step(ctx):
        lp, G = ctx.log_prob_grad(d["beta"], vp_of(d), V)
        return dict(lp=lp, G=G, kernels=ctx.last_kernels())
    return step


def plans(C):
    """every *_plan() getter for C chains; the dictionaries are part of what must not depend on history"""
    def band(ctx, which):
        p = ctx.band_plan(C, which)
        del p["built"]                 # whether the device copy exists yet: a cache, it changes no other entry
        return p

    def step(ctx):
        return dict(band_fwd=band(ctx, "fwd"), band_bwd=band(ctx, "bwd"), sparse=ctx.sparse_plan(C),
                    component=ctx.component_plan(C), draws=ctx.draws_plan(), exact_component=ctx.exact_component_plan())
    return step


def same(a, b):
    """bit equality of two step results (NaN equals NaN: a refused candidate is a value too)"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    if isinstance(a, float):
        return np.float64(a).tobytes() == np.float64(b).tobytes()
    return a == b


def diff(a, b, path=""):
    """where two step results differ, for the assertion message"""
    if isinstance(a, dict):
        return [x for k in a for x in diff(a[k], b.get(k) if isinstance(b, dict) else None, path + "/" + str(k))]
    return [] if same(a, b) else [path]


class Twin:
    """one long-lived context and its logical state; step() runs on it and on a fresh context given only that state"""

    def __init__(self, d, make=new_context):
        self.d, self.make = d, make
        self.ctx = make(d)
        self.L = None                  # ("theta", theta) | ("given", L): the last successful update_L / set_L
        self.u = None                  # (u, niter): the samples as the last set_u or sampler call left them
        self.modes = {}                # setter name -> argument, in the order first set
        self.log = []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ctx.close()

    # -- state changes (on a failure the logical state follows the contract: see lose_L)
    def update_L(self, theta):
        self.ctx.update_L(theta)
        self.L = ("theta", np.array(theta, dtype=float))

    def set_L(self, L):
        self.ctx.set_L(L)
        self.L = ("given", L)

    def lose_L(self):
        """after a failed update_L / set_L there is no L"""
        self.L = None

    def set_u(self, u, niter=None):
        self.ctx.set_u(u, niter)
        self.u = (np.array(u, order="F"), niter)

    def mode(self, setter, arg):
        getattr(self.ctx, setter)(arg)
        self.modes[setter] = arg

    # -- twins
    def fresh(self, with_u=True):
        ctx = self.make(self.d)
        try:
            for setter, arg in self.modes.items():
                getattr(ctx, setter)(arg)
            if self.L is not None:
                (ctx.update_L if self.L[0] == "theta" else ctx.set_L)(self.L[1])
            if with_u and self.u is not None:
                ctx.set_u(*self.u)
        except Exception:
            ctx.close()
            raise
        return ctx

    def step(self, name, fn, samples=False):
        """fn(ctx) -> result, on the long-lived context and on a fresh one; samples: the call leaves new samples (its
        result's "u", every column read by the beta-step as well)"""
        got = fn(self.ctx)
        with self.fresh() as ctx:
            want = fn(ctx)
        self.log.append(name)
        assert same(got, want), "step %d (%s) differs from a fresh context in %s; steps so far: %s" % (
            len(self.log), name, diff(got, want), self.log)
        if samples:
            self.u = (got["u"], None)
        return got

    def sample(self, name, fn):
        return self.step(name, fn, samples=True)


# ------------------------------------------------------------------------------------------ S3: one context, every user
THETA3 = (0.06, 0.12)


def s3_design():
    """gaussian / identity, Q = 300: above 256, the smallest size at which the factorisations are captured as graphs"""
    return dp.design("gaussian", "identity", 300)


def mvn_ll(theta):
    def step(ctx):
        return dict(ll=ctx.mvn_ll(theta))
    return step


def s3_sequence(d):
    """HMC, NUTS, the exact draws and mvn_ll in turn on one context (each step against its fresh twin) -> [(name, result)].
    update_L, the exact draws' M and mvn_ll's workspace are three matrices of one shape factorised in turn: three graph
    keys for two cache slots"""
    rng = np.random.default_rng(29)
    U64 = np.asfortranarray(rng.normal(size=(d["Q"], 64)) * 0.2)
    U300 = np.asfortranarray(rng.normal(size=(d["Q"], 300)) * 0.2)
    V = lpg_input(d, 40)
    out = []

    def keep(name, r, exact=None):
        if exact is not None:
            assert (r["kernels"] == ("exact", "exact")) == exact, (name, r["kernels"])
        out.append((name, r))
        return r
    with Twin(d) as t:
        t.update_L(THETA)
        h1 = keep("hmc 40", t.sample("hmc 40", hmc(d, 40)), exact=False)
        keep("nuts 4", t.sample("nuts 4", nuts(d, 4)))
        keep("nuts 40", t.sample("nuts 40", nuts(d, 40)))
        h2 = t.sample("hmc 40 again", hmc(d, 40))
        assert same(h1, h2), "the same HMC call after NUTS: %s" % diff(h1, h2)
        keep("log_prob_grad", t.step("log_prob_grad", log_prob_grad(d, V)))
        t.mode("set_draws", "exact")
        keep("exact 40", t.sample("exact 40", hmc(d, 40)), exact=True)
        t.set_u(U64)
        keep("mvn_ll 64", t.step("mvn_ll 64", mvn_ll(THETA)))
        for k, th in enumerate((THETA2, THETA3, THETA, THETA2)):
            t.update_L(th)
            keep("exact round %d" % k, t.sample("exact round %d" % k, hmc(d, 40)), exact=True)
            keep("mvn_ll round %d" % k, t.step("mvn_ll round %d" % k, mvn_ll(th)))
        t.mode("set_draws", "hmc")
        keep("hmc 40, draws back", t.sample("hmc 40, draws back", hmc(d, 40)), exact=False)
        keep("nuts 40, draws back", t.sample("nuts 40, draws back", nuts(d, 40)))
        for k, U in enumerate((U64, U300, U64)):          # mvn_ll's workspace holds the sample rows below the matrix: it moves
            t.set_u(U)
            keep("mvn_ll m %d" % k, t.step("mvn_ll m %d (%d columns)" % (k, U.shape[1]), mvn_ll(THETA3)))
    return out


def flatten(results):
    """[(name, result)] -> {key: array}, for numpy.savez: every number of every result (the kernel names are left out)"""
    flat = {}
    for i, (name, r) in enumerate(results):
        for k, v in r.items():
            if k == "kernels":
                continue
            if isinstance(v, dict):
                v = np.array([float(v[kk]) for kk in sorted(v)])
            flat["%02d %s %s" % (i, name, k)] = np.asarray(v)
    return flat
