"""Host-side mirror of glmmrMCML's Rcpp export surface (R/RcppExports.R:35-303)
over the C ABI of libglmmr_mcml_hip.so.  R is not in the image, so this module
stands where ``R6ModelExtMCML.R`` does: same export names, same argument order
and meaning, numpy arrays instead of R vectors.  Everything is converted to
column-major float64 / int32 and handed over as plain pointers; no torch types
cross the boundary.
"""
import ctypes as C
from contextlib import contextmanager as _contextmanager

import numpy as np

from . import _lib

c_dp = C.POINTER(C.c_double)
c_ip = C.POINTER(C.c_int32)

REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int)


class Problem(C.Structure):
    _fields_ = [("cov", c_ip), ("cov_rows", C.c_int), ("data", c_dp), ("data_len", C.c_int),
                ("eff_range", c_dp), ("eff_len", C.c_int), ("Z", c_dp), ("X", c_dp), ("y", c_dp),
                ("n", C.c_int), ("Q", C.c_int), ("P", C.c_int), ("family", C.c_char_p),
                ("link", C.c_char_p)]


class DevOpts(C.Structure):
    _fields_ = [("device", C.c_int), ("stream", C.c_void_p), ("rank", C.c_int), ("world", C.c_int),
                ("reduce", REDUCE_FN), ("reduce_user", C.c_void_p)]


class HmcOpts(C.Structure):
    _fields_ = [("warmup", C.c_int), ("nsamp", C.c_int), ("adapt", C.c_int), ("lambda_", C.c_double),
                ("max_steps", C.c_int), ("target_accept", C.c_double), ("chains", C.c_int),
                ("chain_offset", C.c_int)]


class Ext(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("chains", C.c_int), ("maxfun", C.c_int), ("device", C.c_int),
                ("theta_batch", C.c_int)]


class HmcDiag(C.Structure):
    _fields_ = [("accept_rate", C.c_double), ("mean_e", C.c_double), ("min_e", C.c_double),
                ("max_e", C.c_double), ("max_steps_used", C.c_int), ("leapfrog_total", C.c_longlong)]


class NutsOpts(C.Structure):
    _fields_ = [("warmup", C.c_int), ("nsamp", C.c_int), ("max_treedepth", C.c_int), ("adapt_delta", C.c_double),
                ("stepsize", C.c_double), ("chains", C.c_int), ("chain_offset", C.c_int), ("metric", C.c_int)]


class NutsDiag(C.Structure):
    _fields_ = [("mean_e", C.c_double), ("min_e", C.c_double), ("max_e", C.c_double), ("divergent", C.c_longlong),
                ("treedepth_hits", C.c_longlong), ("batched_leapfrogs", C.c_longlong),
                ("stepsize_search_leapfrogs", C.c_longlong), ("packs", C.c_longlong)]


def phase_ms(enable=True, reset=False):
    """host wall-clock per phase of the MCML iterations of this process since the last reset (csrc/trace.h)"""
    out = np.zeros(8)
    _lib.check(_lib.lib().glmmr_mcml_dbg_phase_ms(int(enable), int(reset), _p(out)))
    return {k: float(out[i]) for i, k in enumerate(("sample", "beta_step", "theta_step", "refresh"))}


class _Mode:
    """One of the three opt-in modes of a context (include/glmmr_mcml_c.h): its names in the order of their codes, the
    process default new contexts start with and the setter of one context.  An unknown name is a KeyError."""

    def __init__(self, entry, *names):
        self.entry = entry                                  # glmmr_mcml_{set_default_, get_default_, ctx_set_}<entry>
        self.code = {k: i for i, k in enumerate(names)}
        self.name = dict(enumerate(names))

    def set_default(self, mode):
        _lib.check(getattr(_lib.lib(), "glmmr_mcml_set_default_" + self.entry)(self.code[mode]))

    def get_default(self):
        return self.name[getattr(_lib.lib(), "glmmr_mcml_get_default_" + self.entry)()]

    def set(self, ctx, mode):
        _lib.check(getattr(_lib.lib(), "glmmr_mcml_ctx_set_" + self.entry)(ctx._h, self.code[mode]))

    @_contextmanager
    def default(self, mode):
        """mode=None leaves the process default alone; otherwise it is set for the duration of a call and restored"""
        prev = None if mode is None else self.get_default()
        if mode is not None:
            self.set_default(mode)
        try:
            yield
        finally:
            if mode is not None:
                self.set_default(prev)


_TRAJ = _Mode("trajectory", "step", "component")
_DRAWS = _Mode("draws", "hmc", "exact", "exact_component")
_LA_OP = _Mode("la_operator", "dense", "component", "component_wide")
_INFO_OP = {None: 0, "dense": 1, "component": 2}            # glmmr_mcml_ctx_information's op; an unknown name is a KeyError


def set_default_trajectory(mode):
    """the trajectory mode new contexts start with ("step" or "component"), the contexts the one-shot exports create
    included (include/glmmr_mcml_c.h glmmr_mcml_set_default_trajectory)"""
    _TRAJ.set_default(mode)


def get_default_trajectory():
    return _TRAJ.get_default()


def set_default_draws(mode):
    """what hmc_sample draws on new contexts ("hmc", "exact" or "exact_component"), the contexts the one-shot exports create included
    (include/glmmr_mcml_c.h glmmr_mcml_set_default_draws)"""
    _DRAWS.set_default(mode)


def get_default_draws():
    return _DRAWS.get_default()


def set_default_la_operator(mode):
    """the operator of the Laplace fits new contexts start with ("dense", "component" or "component_wide"), the contexts mcml_la /
    mcml_la_nr create included (include/glmmr_mcml_c.h glmmr_mcml_set_default_la_operator)"""
    _LA_OP.set_default(mode)


def get_default_la_operator():
    return _LA_OP.get_default()


def la_component_launches():
    """k_lac_factor launches of this process so far, over all contexts (test hook, glmmr_mcml_dbg_la_component_launches)"""
    return int(_lib.lib().glmmr_mcml_dbg_la_component_launches())


def traj_launches():
    """k_cm_traj launches of this process so far, over all contexts (test hook, glmmr_mcml_dbg_traj_launches)"""
    return int(_lib.lib().glmmr_mcml_dbg_traj_launches())


def dbg_dgemm_at(A, B, C0, K, alpha=1.0, beta=0.0, tile=-1):
    """alpha A[:K]' B[:K] + beta C0 through the transposed-A operand form of the GEMM (test hook, include/glmmr_mcml_c.h
    glmmr_mcml_dbg_dgemm_at).  A (K2 x M) and B (K2 x N) hold K2 = round_up(K, 2) rows and go to the device as they are: row
    K of an odd K is the pad row the kernel must ignore.  C0 = None: in place, the product overwrites the first M = K rows
    of B, which are returned."""
    A = np.array(A, dtype=np.float64, order="F"); B = np.array(B, dtype=np.float64, order="F")
    K2 = K + (K & 1)
    assert A.shape[0] == K2 and B.shape[0] == K2, "operands hold round_up(K, 2) rows"
    M, N = A.shape[1], B.shape[1]
    out = B if C0 is None else np.array(C0, dtype=np.float64, order="F")
    assert C0 is None or out.shape == (M, N)
    _lib.check(_lib.lib().glmmr_mcml_dbg_dgemm_at(M, N, int(K), _p(A), K2, _p(B), K2, alpha, beta,
                                                  _p(out), out.shape[0], int(tile)))
    return out[:M]


def rccl_unique_id():
    """128 opaque bytes from ncclGetUniqueId: made on rank 0, handed to every rank's Context.comm_init_rccl"""
    buf = (C.c_ubyte * 128)()
    _lib.check(_lib.lib().glmmr_mcml_rccl_unique_id(buf))
    return bytes(buf)


def _f(a):
    return np.asfortranarray(np.asarray(a, dtype=np.float64))


def _i(a):
    return np.asfortranarray(np.asarray(a, dtype=np.int32))


def _p(a):
    """the address of an array's data, whatever its dtype: the prototypes (_lib.py) take every pointer as void*"""
    return None if a is None else a.ctypes.data_as(c_dp)


def _weights(weights, m):
    """the sample weights of mvn_ll_grad as the C ABI takes them (None stays None); a wrong count is refused here, the
    library does not know the caller's"""
    if weights is None:
        return None
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).ravel())
    if m > 0 and w.size != m:
        raise _lib.McmlError(-1, "mvn_ll_grad: %d weights for %d sample columns" % (w.size, m))
    return w


def _newdata(newdata, cov):
    """(nnew, flat, K) of the prediction calls: newdata is a list with one k_b x ncol_b array per covariance block (None or an
    empty array: no new points there; a vector is one column for a block of one variable, else one point), ncol_b read off
    the block's rows of cov"""
    cov = np.asarray(cov)
    first = np.r_[True, cov[1:, 0] != cov[:-1, 0]]
    ncol = np.add.reduceat(cov[:, 3], np.flatnonzero(first))
    if len(newdata) != ncol.size:
        raise ValueError("newdata must list %d blocks (None for a block without new points)" % ncol.size)
    nnew, flat = np.zeros(ncol.size, dtype=np.int32), []
    for b, x in enumerate(newdata):
        if x is None or np.size(x) == 0:
            continue
        x = np.asarray(x, dtype=np.float64)
        if x.ndim == 1:
            x = x.reshape(-1, 1) if ncol[b] == 1 else x.reshape(1, -1)
        if x.ndim != 2 or x.shape[1] != ncol[b]:
            raise ValueError("newdata[%d] must have %d columns, the block's variables" % (b, ncol[b]))
        nnew[b] = x.shape[0]
        flat.append(x.ravel(order="F"))
    flat = np.concatenate(flat) if flat else np.zeros(0)
    return nnew, np.ascontiguousarray(flat), int(nnew.sum())


def _prediction(summary, mm):
    out = dict(mean=summary[:, 0].copy(), cond_var=summary[:, 1].copy(), sample_var=summary[:, 2].copy())
    if mm is not None:
        out["means"] = mm
    return out


def _cols(u):
    """samples as a column-major matrix; a vector is one column"""
    u = _f(u)
    return u.reshape(-1, 1, order="F") if u.ndim == 1 else u


def _diag(d):
    """a diagnostics struct (HmcDiag, NutsDiag) as the dict of its fields"""
    return {k: getattr(d, k) for k, _ in d._fields_}


def _plan(fn, ctype, keys, *args, bools=(), named=()):
    """a plan hook's integers as a dict: fn(*args, out) fills len(keys) values of `ctype`; the keys in `bools` become bool,
    named = (a _Mode, its keys) become that mode's names"""
    out = (ctype * len(keys))()
    _lib.check(fn(*args, out))
    d = dict(zip(keys, (int(v) for v in out)))
    d.update((k, bool(d[k])) for k in bools)
    d.update((k, named[0].name[d[k]]) for k in named[1:])
    return d


class Context:
    """A device-resident MCML problem (glmmr_mcml_ctx).  Inputs are uploaded once;
    afterwards only parameter vectors go down and scalars come back."""

    def __init__(self, cov, data, eff_range, Z=None, X=None, y=None, family=None, link=None,
                 device=0, stream=None, rank=0, world=1, reduce=None):
        L = _lib.lib()
        p, self._keep = _problem(cov, data, eff_range, Z, X, y, family, link)
        cv = self._keep["cov"]
        assert cv.ndim == 2 and cv.shape[1] == 5, "cov must be rows x 5"
        self.n, self.P = p.n, p.P
        if Z is not None:
            self.Q = p.Q
            assert self._keep["X"].shape[0] == self.n and self._keep["y"].size == self.n
        o = DevOpts()
        o.device = device; o.stream = stream; o.rank = rank; o.world = world
        self._reduce_cb = REDUCE_FN(reduce) if reduce is not None else REDUCE_FN()
        o.reduce = self._reduce_cb
        self._h = C.c_void_p()
        self._world = int(world)
        _lib.check(L.glmmr_mcml_ctx_create(C.byref(p), C.byref(o), C.byref(self._h)))
        self.family, self.link = family, link
        if Z is None:
            self.Q = int(sum(cv[np.r_[True, cv[1:, 0] != cv[:-1, 0]], 1]))
        self.mcols = 0

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().glmmr_mcml_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- native multi-GPU exchange (comm.hip): RCCL all-reduce on the context's stream
    def comm_init_rccl(self, unique_id, rank, world):
        buf = (C.c_ubyte * 128).from_buffer_copy(bytes(unique_id))
        _lib.check(_lib.lib().glmmr_mcml_ctx_comm_init_rccl(self._h, buf, int(rank), int(world)))
        self._world = int(world)

    def comm_allreduce(self, vals):
        """sum over the ranks through the path the statistics take (self-test of the exchange)"""
        v = np.ascontiguousarray(vals, dtype=np.float64).copy()
        _lib.check(_lib.lib().glmmr_mcml_ctx_comm_allreduce(self._h, _p(v), v.size))
        return v

    def comm_stats(self):
        calls = C.c_longlong(); dbl = C.c_longlong(); nat = C.c_int()
        _lib.check(_lib.lib().glmmr_mcml_ctx_comm_stats(self._h, C.byref(calls), C.byref(dbl), C.byref(nat)))
        return dict(calls=calls.value, doubles=dbl.value, native=bool(nat.value))

    # -- samples
    def set_u(self, u, niter=None):
        u = _cols(u)
        _lib.check(_lib.lib().glmmr_mcml_set_u(self._h, _p(u), u.shape[0], u.shape[1],
                                               u.shape[1] if niter is None else niter))
        self.mcols = u.shape[1]                 # after the check: a refused call leaves get_u() as it was

    def get_u(self):
        u = np.zeros((self.Q, self.mcols), order="F")
        _lib.check(_lib.lib().glmmr_mcml_get_u(self._h, _p(u), self.Q))
        return u

    def get_u_all(self, world=None):
        """every rank's samples, rank r's columns at r * mcols: the u mcml_full returns (mcml_full.cpp:144-145).
        Collective unless called right after mcml_full / mcml_optim (the theta-step has gathered them)."""
        w = int(world) if world else max(1, int(getattr(self, "_world", 1)))
        u = np.zeros((self.Q, self.mcols * w), order="F")
        nc = C.c_int()
        _lib.check(_lib.lib().glmmr_mcml_get_u_all(self._h, _p(u), self.Q, C.byref(nc)))
        assert nc.value == u.shape[1], (nc.value, u.shape)
        return u

    def shard_stats(self):
        out = (C.c_longlong * 6)()
        _lib.check(_lib.lib().glmmr_mcml_ctx_shard_stats(self._h, out))
        return dict(gathers=out[0], gather_doubles=out[1], theta_rounds=out[2], theta_evals_own=out[3],
                    theta_evals_all=out[4], theta_factorised=out[5])

    def emulate_world(self, world, mode):
        """bench.py --as-rank-of N (include/glmmr_mcml_c.h glmmr_mcml_dbg_emulate_world): 1 record, 2 replay"""
        _lib.check(_lib.lib().glmmr_mcml_dbg_emulate_world(self._h, int(world), int(mode)))
        self._world = int(world) if world and world > 1 else 1

    # -- A8
    def mvn_ll(self, theta):
        theta = _f(theta).ravel()
        out = C.c_double()
        _lib.check(_lib.lib().glmmr_mcml_ctx_mvn_ll(self._h, _p(theta), C.byref(out)))
        return out.value

    def mvn_ll_batch(self, thetas):
        """mvn_ll at several thetas (rows of `thetas`) evaluated side by side on the device"""
        th = np.ascontiguousarray(np.atleast_2d(np.asarray(thetas, dtype=np.float64)))     # row j = candidate j = column-major R x k
        out = np.zeros(th.shape[0])
        _lib.check(_lib.lib().glmmr_mcml_ctx_mvn_ll_batch(self._h, _p(th), th.shape[0], _p(out)))
        return out

    def mvn_ll_grad(self, theta, weights=None):
        """(value, grad): value = sum_j w_j sum_b log N(u_bj; 0, D_b(theta)) over the context's own sample columns and its
        gradient in theta, analytically (csrc/mvn_grad.h).  weights = None: 1 / mcols each, value is mvn_ll(theta) to the
        bit.  A query: the context is left as mvn_ll(theta) leaves it.  McmlError -1 for weights of the wrong length,
        negative or not finite; -3 where D(theta) is not positive definite"""
        theta = _f(theta).ravel()
        w = _weights(weights, self.mcols)
        out = C.c_double()
        grad = np.zeros(theta.size)
        _lib.check(_lib.lib().glmmr_mcml_ctx_mvn_ll_grad(self._h, _p(theta), _p(w), C.byref(out), _p(grad)))
        return out.value, grad

    def mvn_workspace(self, cand=-1):
        """(L, X, dims): what the last mvn_ll call (cand = -1) or candidate `cand` of the last mvn_ll_batch call left in its
        workspace for the last large block -- the d x d array holding the factor, the m x d solved sample rows below it,
        dims = (d, round_up(d, 16), m, leading dimension) (test hook, include/glmmr_mcml_c.h glmmr_mcml_dbg_mvn_workspace)"""
        f = _lib.lib().glmmr_mcml_dbg_mvn_workspace
        dims = (C.c_int * 4)()
        _lib.check(f(self._h, int(cand), None, 0, None, 0, dims))
        d, m = dims[0], dims[2]
        L = np.zeros((d, d), order="F"); X = np.zeros((m, d), order="F")
        _lib.check(f(self._h, int(cand), _p(L), d, _p(X), m, dims))
        return L, X, tuple(dims)

    def dbg_chol(self, A, B=None, linv=True):
        """The dense Cholesky stack on the caller's matrix (test hook, include/glmmr_mcml_c.h glmmr_mcml_dbg_chol): A (n x n) is
        uploaded as given, upper triangle included.  -> dict(A = the whole array as the device left it, fwd / trans / potrs =
        inv(L) B, inv(L)' B, inv(L L') B, each solved on its own copy of B (absent without B), linv = the ceil(n / 128)
        inverted diagonal blocks, nblk x 128 x 128 with [k, i, j] = entry (i, j) of block k).  Raises McmlError (code -3) if A
        is not positive definite."""
        A = np.array(A, dtype=np.float64, order="F")
        n = A.shape[0]
        assert A.shape == (n, n)
        out = dict(A=A)
        m = 0
        if B is not None:
            B = _f(B).reshape(n, -1, order="F")
            m = B.shape[1]
            for k in ("fwd", "trans", "potrs"):
                out[k] = np.zeros((n, m), order="F")
        nblk = (n + 127) // 128
        li = np.zeros((nblk, 128, 128)) if linv else None
        _lib.check(_lib.lib().glmmr_mcml_dbg_chol(self._h, n, _p(A), n, m, _p(B), n, _p(out.get("fwd")), _p(out.get("trans")),
                                                  _p(out.get("potrs")), _p(li)))
        if linv:
            out["linv"] = li.transpose(0, 2, 1)         # the blocks are column-major on the device
        return out

    def gen_D(self, theta, chol=False):
        theta = _f(theta).ravel()
        D = np.zeros((self.Q, self.Q), order="F")
        _lib.check(_lib.lib().glmmr_mcml_ctx_gen_D(self._h, _p(theta), int(chol), _p(D), self.Q))
        return D

    # -- A6 / A7
    def loglik(self, beta, var_par):
        beta = _f(beta).ravel()
        out = C.c_double()
        _lib.check(_lib.lib().glmmr_mcml_ctx_loglik(self._h, _p(beta), var_par, C.byref(out)))
        return out.value

    def mcnr(self, beta, var_par):
        beta = _f(beta).ravel()
        bout = np.zeros(self.P); sig = C.c_double()
        stats = np.zeros(self.P * self.P + self.P + 1)
        _lib.check(_lib.lib().glmmr_mcml_ctx_mcnr(self._h, _p(beta), var_par, _p(bout),
                                                  C.byref(sig), _p(stats)))
        P = self.P
        return dict(beta=bout, sigma=sig.value, XtWX=stats[:P * P].reshape(P, P, order="F"),
                    XtWr=stats[P * P:P * P + P], sigma_sum=stats[-1])

    # -- model state / sampler
    def update_L(self, theta):
        theta = _f(theta).ravel()
        _lib.check(_lib.lib().glmmr_mcml_ctx_update_L(self._h, _p(theta)))

    def set_L(self, Lmat):
        Lmat = _f(Lmat)
        _lib.check(_lib.lib().glmmr_mcml_ctx_set_L(self._h, _p(Lmat), Lmat.shape[0]))

    def log_prob_grad(self, beta, var_par, V):
        """log_prob / log_grad of every column of V (test hook for A4/A5)"""
        beta = _f(beta).ravel(); V = _f(V)
        lp = np.zeros(V.shape[1]); G = np.zeros_like(V, order="F")
        _lib.check(_lib.lib().glmmr_mcml_dbg_log_prob_grad(self._h, _p(beta), var_par, _p(V),
                                                           V.shape[1], _p(lp), _p(G)))
        return lp, G

    def hmc_sample(self, beta, var_par, warmup, nsamp, lambda_, max_steps, target_accept, seed,
                   chains=1, chain_offset=0, iter_idx=0, adapt=100, inj_init=None, inj_mom=None,
                   want_trace=False):
        beta = _f(beta).ravel()
        o = HmcOpts(warmup, nsamp, adapt, lambda_, max_steps, target_accept, chains, chain_offset)
        d = HmcDiag()
        ii = None if inj_init is None else _f(inj_init)
        im = None if inj_mom is None else _f(inj_mom)
        total = warmup + (nsamp if chains == 1 else -(-nsamp // chains))   # proposals per chain
        flags = np.zeros((chains, total), dtype=np.uint8, order="F") if want_trace else None
        probs = np.zeros((chains, total), order="F") if want_trace else None
        ncols = C.c_int()
        _lib.check(_lib.lib().glmmr_mcml_ctx_hmc_sample(
            self._h, _p(beta), var_par, C.byref(o), seed, iter_idx, _p(ii), _p(im), _p(flags), _p(probs), C.byref(d),
            C.byref(ncols)))
        self.mcols = ncols.value
        return (_diag(d), flags, probs) if want_trace else _diag(d)

    def nuts_sample(self, beta, var_par, warmup, nsamp, seed, chains=1, chain_offset=0, iter_idx=0, max_treedepth=10,
                    adapt_delta=0.8, stepsize=1.0, want_trace=False, metric="diag_e"):
        """the sampler that stands where the reference calls Stan (gen_u_samples.R, inst/stan): csrc/nuts.h"""
        beta = _f(beta).ravel()
        o = NutsOpts(warmup, nsamp, max_treedepth, adapt_delta, stepsize, chains, chain_offset,
                     {"diag_e": 0, "unit_e": 1}[metric])
        d = NutsDiag()
        total = warmup + -(-nsamp // chains)
        tr = None
        if want_trace:
            tr = dict(depth=np.zeros((chains, total), dtype=np.int32, order="F"),
                      nleap=np.zeros((chains, total), dtype=np.int32, order="F"),
                      eps=np.zeros((chains, total), order="F"), accept=np.zeros((chains, total), order="F"))
        ncols = C.c_int()
        _lib.check(_lib.lib().glmmr_mcml_ctx_nuts_sample(
            self._h, _p(beta), var_par, C.byref(o), seed, iter_idx,
            *(_p(tr[k]) if tr else None for k in ("depth", "nleap", "eps", "accept")), C.byref(d), C.byref(ncols)))
        self.mcols = ncols.value
        return (_diag(d), tr) if want_trace else _diag(d)

    # -- drivers on the resident context
    def _ext(self, seed, chains, maxfun, theta_batch=0):
        return Ext(int(seed or 0), int(chains or 1), int(maxfun or 0), 0, int(theta_batch or 0))

    def npar(self):
        return _lib.lib().glmmr_mcml_ctx_npar(self._h)

    def theta_log(self, enable=None, last=None):
        """test hook: the theta-step's objective evaluations, rows (theta..., log-likelihood); enable True clears + starts"""
        w = self.npar() + 1
        n = C.c_int()
        _lib.check(_lib.lib().glmmr_mcml_dbg_theta_log(self._h, -1, None, 0, C.byref(n)))
        rows = n.value if last is None else min(int(last), n.value)
        out = np.zeros((rows, w))
        _lib.check(_lib.lib().glmmr_mcml_dbg_theta_log(self._h, -1 if enable is None else int(bool(enable)),
                                                       _p(out) if rows else None, rows, C.byref(n)))
        return out

    def last_kernels(self):
        """kernel family of the sampler's last (forward, backward) product"""
        names = {-1: None, 0: "skinny", 1: "band", 2: "dlds", 3: "reg", 4: "sparse", 5: "component", 6: "exact",
                 7: "exact_component"}
        f = C.c_int(); b = C.c_int()
        _lib.check(_lib.lib().glmmr_mcml_ctx_last_kernels(self._h, C.byref(f), C.byref(b)))
        return names[f.value], names[b.value]

    def band_plan(self, chains, which="fwd"):
        """the banded kernel's decomposition of the forward / backward product for `chains` columns (test hook,
        include/glmmr_mcml_c.h glmmr_mcml_dbg_band_plan)"""
        keys = ("used", "nbands", "tiles", "gn", "nwg", "nred", "nslots", "paired", "nempty", "built")
        return _plan(_lib.lib().glmmr_mcml_dbg_band_plan, C.c_int, keys, self._h, {"fwd": 0, "bwd": 1}[which], int(chains),
                     bools=("used", "paired", "built"))

    def band_extents(self, which="fwd"):
        """the row-tile extents of the forward / backward operand of the banded kernel: (ext, issued, whole) -- an int
        array (bands, 5, 2) of first / one-past-last nonzero K substep per 16-row tile, the MFMAs per 16-column strip
        inside them, and those of the whole K tiles (test hook, include/glmmr_mcml_band.h glmmr_mcml_dbg_band_extents)"""
        w = {"fwd": 0, "bwd": 1}[which]
        out3 = (C.c_longlong * 3)()
        _lib.check(_lib.lib().glmmr_mcml_dbg_band_extents(self._h, w, None, 0, out3))
        ext = np.zeros((int(out3[0]), 5, 2), dtype=np.int32)
        _lib.check(_lib.lib().glmmr_mcml_dbg_band_extents(self._h, w, ext.ctypes.data_as(C.POINTER(C.c_int)),
                                                          int(ext.size), out3))
        return ext, int(out3[1]), int(out3[2])

    def sparse_plan(self, chains):
        """the sparse chain-major operator as hmc_sample / log_prob_grad would run it with `chains` chains, valid after update_L (test hook,
        include/glmmr_mcml_c.h glmmr_mcml_dbg_sparse_plan)"""
        keys = ("active", "factored", "W", "nnz", "nnz_z", "nnz_l", "nblk", "max_blk", "long_rows", "fused", "qrows", "ncb")
        return _plan(_lib.lib().glmmr_mcml_dbg_sparse_plan, C.c_longlong, keys, self._h, int(chains),
                     bools=("active", "factored", "long_rows"))

    def set_trajectory(self, mode):
        """how hmc_sample runs a trajectory on the sparse operator: "step" (a forward and a backward launch per leapfrog
        step) or "component" (csrc/hmc_traj.h: one launch per proposal, where the component plan is feasible)"""
        _TRAJ.set(self, mode)

    def component_plan(self, chains):
        """the component-local trajectory path as the next hmc_sample with `chains` chains would take it, valid after
        update_L (test hook, include/glmmr_mcml_c.h glmmr_mcml_dbg_component_plan)"""
        keys = ("requested", "feasible", "used", "ncomp", "max_vars", "max_rows", "empty_comps", "nitems", "waves_per_item",
                "cap_vars", "lds_bytes_per_workgroup")
        return _plan(_lib.lib().glmmr_mcml_dbg_component_plan, C.c_longlong, keys, self._h, int(chains),
                     bools=("requested", "feasible", "used"))

    def set_draws(self, mode):
        """what hmc_sample draws: "hmc" (trajectories) or "exact" (csrc/hmc_exact.h: the conditional distribution of the
        whitened effects directly, where it is Gaussian -- gaussian / identity on the dense ZL operator; elsewhere the
        request changes nothing) or "exact_component" ("exact", and on the sparse operator of a block-structured design the
        same draw one connected component at a time, csrc/hmc_exact_comp.h, where no component has more than 128 variables)"""
        _DRAWS.set(self, mode)

    def draws_plan(self):
        """the exact path as the next hmc_sample would (not) take it (test hook, include/glmmr_mcml_c.h
        glmmr_mcml_dbg_draws_plan)"""
        return _plan(_lib.lib().glmmr_mcml_dbg_draws_plan, C.c_int, ("requested", "applicable", "Q", "m_bytes"), self._h,
                     bools=("applicable",), named=(_DRAWS, "requested"))

    def exact_sample(self, beta, var_par, nsamp, seed, chains=1, chain_offset=0, iter_idx=0, inj_z=None, operator="dense"):
        """exact conditional draws whatever set_draws says (McmlError where the path does not apply); the samples have
        hmc_sample's shape.  inj_z (Q x columns) replaces the generated standard normals.  operator: "dense"
        (csrc/hmc_exact.h) or "component" (csrc/hmc_exact_comp.h, on the sparse operator)"""
        entry = {"dense": "glmmr_mcml_ctx_exact_sample", "component": "glmmr_mcml_ctx_exact_component_sample"}[operator]
        beta = _f(beta).ravel()
        o = HmcOpts(0, nsamp, 0, 1.0, 1, 0.9, chains, chain_offset)
        d = HmcDiag()
        iz = None if inj_z is None else _f(inj_z)
        want = nsamp + 1 if chains == 1 else chains * -(-nsamp // chains)
        if iz is not None and iz.shape != (self.Q, want):
            raise ValueError("inj_z must be Q x %d" % want)
        ncols = C.c_int()
        _lib.check(getattr(_lib.lib(), entry)(
            self._h, _p(beta), var_par, C.byref(o), seed, iter_idx, _p(iz), C.byref(d), C.byref(ncols)))
        self.mcols = ncols.value
        return _diag(d)

    def exact_component_plan(self):
        """the component-wise exact path as the next hmc_sample would (not) take it, valid after update_L (test hook,
        include/glmmr_mcml_c.h glmmr_mcml_dbg_exact_component_plan)"""
        keys = ("requested", "applicable", "ncomp", "max_vars", "max_rows", "factor_waves", "draw_lds_bytes", "factor_bytes")
        return _plan(_lib.lib().glmmr_mcml_dbg_exact_component_plan, C.c_longlong, keys, self._h, bools=("applicable",),
                     named=(_DRAWS, "requested"))

    def exact_component_phases(self, enable=True):
        """HIP-event ms of the phases of the last component-wise exact call recorded; enable: record the following calls"""
        out = np.zeros(4)
        _lib.check(_lib.lib().glmmr_mcml_dbg_exact_component_phases(self._h, int(enable), _p(out)))
        return dict(zip(("factor_mean", "draw", "transpose", "lv"), (float(v) for v in out)))

    def exact_phases(self, enable=True):
        """HIP-event ms of the phases of the last exact call recorded; enable: record the following calls"""
        out = np.zeros(5)
        _lib.check(_lib.lib().glmmr_mcml_dbg_exact_phases(self._h, int(enable), _p(out)))
        return dict(zip(("m_build", "factorisation", "rhs_fill", "transposed_solve", "lv"), (float(v) for v in out)))

    def set_la_operator(self, mode):
        """how mcml_la / la_probe run on this context: "dense" (the dense ZL and M = ZL' W ZL + I), "component"
        (csrc/component.hip: M one connected component at a time on the sparse operator, a wave each, where no component has
        more than 32 variables) or "component_wide" (the same up to 128 variables per component: a wave each, or a workgroup
        each where a component has more than 32 variables or 128 observations and more; GLMMR_MCML_LA_WAVES=1|4 forces a
        form).  Where the asked-for operator cannot run, the dense one does"""
        _LA_OP.set(self, mode)

    def la_plan(self):
        """what was asked for and what the last Laplace call on this context ran (test hook, include/glmmr_mcml_c.h
        glmmr_mcml_dbg_la_plan); waves: per component in that call, 0 (dense), 1 or 4"""
        keys = ("requested", "operator", "ncomp", "max_vars", "max_rows", "launches", "dense_bytes", "waves")
        return _plan(_lib.lib().glmmr_mcml_dbg_la_plan, C.c_longlong, keys, self._h, named=(_LA_OP, "requested", "operator"))

    def information_matrix(self, beta, var_par, theta=None, operator=None):
        """The GLS information of the fixed effects, X' (W^-1 + Z D Z')^-1 X (P x P), on the device (csrc/info.hip,
        include/glmmr_mcml_info.h glmmr_mcml_ctx_information): the weights are dhdmu(X beta) times the family's scale in
        var_par, with no random-effect term; y is not read.  theta = None: the resident L of the last update_L / set_L, the
        context is left untouched; given: the context is left as update_L(theta) leaves it.  operator: None (the component
        operator where the context runs the sparse one and no component has more than 128 variables, else the dense one),
        "dense" or "component" (McmlError -2 where it does not apply).  McmlError -1 for a weight that is not finite, -3
        for a failed pivot"""
        beta = _f(beta).ravel()
        if beta.size != self.P:
            raise ValueError("beta must hold %d values" % self.P)
        th = None if theta is None else _f(theta).ravel()
        out = np.zeros((self.P, self.P), order="F")
        _lib.check(_lib.lib().glmmr_mcml_ctx_information(self._h, _p(beta), float(var_par), _p(th), _INFO_OP[operator], _p(out),
                                                         self.P))
        return out

    def information_plan(self):
        """what the last information_matrix on this context was asked for and ran (test hook, include/glmmr_mcml_info.h
        glmmr_mcml_dbg_information_plan): op 0 dense, 1 component (several components per wave), 2 component-wide; waves: per
        component of the factor kernel, 0 (dense), 1 or 4"""
        keys = ("requested", "op", "ncomp", "max_vars", "waves", "launches", "dense_bytes", "P")
        return _plan(_lib.lib().glmmr_mcml_dbg_information_plan, C.c_longlong, keys, self._h)

    def theta_information(self, beta, var_par, theta, operator=None):
        """The GLS (expected) information of the covariance parameters, 1/2 tr(Sigma^-1 d_r Sigma Sigma^-1 d_s Sigma) with
        Sigma = W^-1 + Z D(theta) Z', on the device (csrc/theta_info.hip, include/glmmr_mcml_theta_info.h
        glmmr_mcml_ctx_theta_information) -> dict(information, names).  The weights are information_matrix's; neither y nor the
        samples are read.  names: "theta0", "theta1", ... and, for gaussian / identity, "sigma" last -- there the matrix is the
        (R + 1) x (R + 1) information of (theta, sigma), sigma = var_par.  theta is required (McmlError -1 for None) and the
        context is left as update_L(theta) leaves it.  operator: None (the component operator where the context runs the sparse
        one, no component has more than 64 variables and every covariance block lies inside one component, else the dense
        one), "dense" or "component" (McmlError -2 where it does not apply).  McmlError -1 for a weight that is not finite, -3
        for a failed pivot or a D(theta) that is not positive definite"""
        beta = _f(beta).ravel()
        if beta.size != self.P:
            raise ValueError("beta must hold %d values" % self.P)
        R = self.npar()
        th = None if theta is None else _f(theta).ravel()
        if th is not None and th.size < R:
            raise ValueError("theta must hold %d values" % R)
        out = np.zeros((R + 1, R + 1), order="F")
        got = C.c_int()
        _lib.check(_lib.lib().glmmr_mcml_ctx_theta_information(self._h, _p(beta), float(var_par), _p(th), _INFO_OP[operator],
                                                               _p(out), R + 1, C.byref(got)))
        return _theta_info_result(out, R, got.value)

    def theta_information_plan(self):
        """what the last theta_information on this context was asked for and ran (test hook, include/glmmr_mcml_theta_info.h
        glmmr_mcml_dbg_theta_information_plan): op 0 dense, 1 component; launches: of csrc/theta_info.hip's own kernels;
        dense_bytes: of the Q x Q / Q x n matrices the call built (0 on the component operator)"""
        keys = ("requested", "op", "ncomp", "max_vars", "launches", "dense_bytes", "R", "rows")
        return _plan(_lib.lib().glmmr_mcml_dbg_theta_information_plan, C.c_longlong, keys, self._h)

    def small_sample(self, beta, var_par, theta, operator=None):
        """The ingredients of the Kenward-Roger / Satterthwaite small-sample corrections of the fixed effects on the device
        (csrc/small_sample.hip, include/glmmr_mcml_small_sample.h glmmr_mcml_ctx_small_sample) ->
        dict(information, theta_information, P, Q, R, names): information = X' Sigma^-1 X (information_matrix's bits on the
        operator run), theta_information = theta_information's bits, and with d_r Sigma = Z (d_r D) Z' (2 sigma I for "sigma")
        P[r] = -X' Sigma^-1 d_r Sigma Sigma^-1 X, Q[r, s] = X' Sigma^-1 d_r Sigma Sigma^-1 d_s Sigma Sigma^-1 X,
        R[r, s] = X' Sigma^-1 d2_rs Sigma Sigma^-1 X, arrays of shape (no, P, P) and (no, no, P, P); names as
        theta_information.  theta, operator and the errors: as theta_information"""
        beta = _f(beta).ravel()
        if beta.size != self.P:
            raise ValueError("beta must hold %d values" % self.P)
        R = self.npar()
        th = None if theta is None else _f(theta).ravel()
        if th is not None and th.size < R:
            raise ValueError("theta must hold %d values" % R)
        buf = _small_sample_buffers(self.P, R)
        got = C.c_int()
        _lib.check(_lib.lib().glmmr_mcml_ctx_small_sample(self._h, _p(beta), float(var_par), _p(th), _INFO_OP[operator],
                                                          _p(buf[0]), self.P, _p(buf[1]), R + 1, _p(buf[2]), _p(buf[3]),
                                                          _p(buf[4]), C.byref(got)))
        return _small_sample_result(buf, self.P, R, got.value)

    def small_sample_plan(self):
        """what the last small_sample on this context was asked for and ran (test hook, include/glmmr_mcml_small_sample.h
        glmmr_mcml_dbg_small_sample_plan): op 0 dense, 1 component; launches: of csrc/small_sample.hip's own kernels; bytes: of
        the matrices the new part allocated, Q x P, Q x (R + the pairs a block reads together) P and n x P ones -- none of them Q x Q"""
        keys = ("requested", "op", "ncomp", "max_vars", "launches", "bytes", "R", "rows")
        return _plan(_lib.lib().glmmr_mcml_dbg_small_sample_plan, C.c_longlong, keys, self._h)

    def sandwich(self, beta, var_par, theta=None, cluster=None, operator=None, scores=False):
        """The cluster-robust (sandwich) covariance of the fixed effects on the device (csrc/sandwich.hip,
        include/glmmr_mcml_sandwich.h glmmr_mcml_ctx_sandwich) -> dict(information, meat, vcov, ncluster[, scores]):
        information = X' Sigma^-1 X (information_matrix's bits), meat = G' G with the cluster scores
        G[c] = sum_{i in c} x_i (Sigma^-1 e)_i of the working residuals e = (y - h(X beta)) d eta / d mu, and
        vcov = information^-1 meat information^-1, solved here.  cluster: n integer ids 0 .. ncl - 1, or None for the connected
        components of ZL's coupling graph (McmlError -1 where the context does not run the sparse operator or an observation
        has no entry of ZL).  theta and operator: as information_matrix.  McmlError -1 for an id out of range or a residual /
        weight that is not finite, -2 for "component" where it does not apply, -3 for a failed pivot"""
        beta = _f(beta).ravel()
        if beta.size != self.P:
            raise ValueError("beta must hold %d values" % self.P)
        th = None if theta is None else _f(theta).ravel()
        cl, ncl = _cluster_ids(cluster, self.n)
        r = _sandwich_call(lambda *a: _lib.lib().glmmr_mcml_ctx_sandwich(self._h, _p(beta), float(var_par), _p(th),
                                                                         _INFO_OP[operator], *a), self.n, self.P, cl, ncl, scores)
        return r

    def sandwich_plan(self):
        """what the last sandwich on this context was asked for and ran (test hook, include/glmmr_mcml_sandwich.h
        glmmr_mcml_dbg_sandwich_plan): op as information_plan's, the clusters and the rows of the largest, whether they were
        the default ones, the launches of csrc/sandwich.hip's kernels"""
        keys = ("requested", "op", "ncluster", "max_rows", "default_clusters", "launches", "dense_bytes", "P")
        return _plan(_lib.lib().glmmr_mcml_dbg_sandwich_plan, C.c_longlong, keys, self._h, bools=("default_clusters",))

    def predict_re(self, theta, newdata, means=False):
        """Conditional (kriging) prediction of the random effects at new locations given the context's sample columns
        (csrc/predict.hip, include/glmmr_mcml_predict.h glmmr_mcml_ctx_predict_re).  newdata: one k_b x ncol_b array per
        covariance block with the columns of the block's data matrix, None for no new points.  -> dict(mean, cond_var,
        sample_var[, means]) over the K = sum k_b new points in block order: the mean over the sample columns of the
        conditional mean C D^-1 u_j, the conditional variance max(p - C D^-1 C', 0), the variance of the conditional mean
        across the sample columns (divisor m - 1, NaN for one column) and, on request, the K x m conditional means.  A
        query: the context is left as it was.  McmlError -1 without samples, for a wrong shape or K = 0, -3 where D(theta)
        is not positive definite"""
        theta = _f(theta).ravel()
        nnew, flat, K = _newdata(newdata, self._keep["cov"])
        summary = np.zeros((max(K, 1), 3), order="F")
        mm = np.zeros((max(K, 1), self.mcols), order="F") if means else None
        _lib.check(_lib.lib().glmmr_mcml_ctx_predict_re(self._h, _p(theta), _p(nnew), _p(flat), flat.size, _p(summary),
                                                        summary.shape[0], _p(mm), summary.shape[0]))
        return _prediction(summary, mm)

    def predict_plan(self):
        """what the last predict_re on this context did (test hook, include/glmmr_mcml_predict.h glmmr_mcml_dbg_predict_plan):
        blocks served by each path, new points, chunks and factorisations run, workspace bytes, sample columns"""
        keys = ("diag", "small", "large", "K", "chunks", "factorisations", "workspace_bytes", "m")
        return _plan(_lib.lib().glmmr_mcml_dbg_predict_plan, C.c_longlong, keys, self._h)

    def mcml_optim(self, start, trace=0, mcnr=False, maxfun=0, theta_batch=0):
        start = _f(start).ravel(); R = self.npar()
        b = np.zeros(self.P); t = np.zeros(R); sg = C.c_double()
        e = self._ext(0, 1, maxfun, theta_batch)
        _lib.check(_lib.lib().glmmr_mcml_ctx_optim(self._h, _p(start), start.size, int(trace), int(mcnr),
                                                   C.byref(e), _p(b), _p(t), C.byref(sg)))
        return dict(beta=b, theta=t, sigma=sg.value)

    def mcml_simlik(self, start, trace=0, maxfun=0, theta_batch=0):
        start = _f(start).ravel(); R = self.npar()
        b = np.zeros(self.P); t = np.zeros(R); sg = C.c_double()
        e = self._ext(0, 1, maxfun, theta_batch)
        _lib.check(_lib.lib().glmmr_mcml_ctx_simlik(self._h, _p(start), start.size, int(trace), C.byref(e),
                                                    _p(b), _p(t), C.byref(sg)))
        return dict(beta=b, theta=t, sigma=sg.value)

    def mcml_hess(self, start, tol=1e-5, trace=0):
        start = _f(start).ravel(); nv = self.P + self.npar()
        H = np.zeros((nv, nv), order="F")
        _lib.check(_lib.lib().glmmr_mcml_ctx_hess(self._h, _p(start), start.size, tol, int(trace), _p(H)))
        return H

    def aic_mcml(self, beta_par, cov_par):
        bp = _f(beta_par).ravel(); cp = _f(cov_par).ravel()
        out = C.c_double()
        _lib.check(_lib.lib().glmmr_mcml_ctx_aic(self._h, _p(bp), bp.size, _p(cp), cp.size, C.byref(out)))
        return out.value

    def mcml_full(self, start, mcnr=False, m=500, maxiter=30, warmup=500, tol=1e-3, verbose=False,
                  lambda_=0.05, trace=0, refresh=500, maxsteps=100, target_accept=0.9, seed=0, chains=1,
                  maxfun=0, theta_batch=0):
        start = _f(start).ravel(); R = self.npar()
        b = np.zeros(self.P); t = np.zeros(R); sg = C.c_double(); conv = C.c_int(); it = C.c_int()
        d = HmcDiag()
        e = self._ext(seed, chains, maxfun, theta_batch)
        _lib.check(_lib.lib().glmmr_mcml_ctx_full(
            self._h, _p(start), start.size, int(mcnr), int(m), int(maxiter), int(warmup), tol,
            int(verbose), lambda_, int(trace), int(refresh), int(maxsteps), target_accept,
            C.byref(e), _p(b), _p(t), C.byref(sg), C.byref(conv), C.byref(it), C.byref(d)))
        self.mcols = _lib.lib().glmmr_mcml_ctx_ncols(self._h)
        return dict(beta=b, theta=t, sigma=sg.value, converged=bool(conv.value), iters=it.value,
                    accept_rate=d.accept_rate, mean_e=d.mean_e, leapfrog_total=d.leapfrog_total)

    def mcml_la(self, start, usehess=False, tol=1e-3, verbose=False, trace=0, maxiter=10, nr=False, maxfun=0,
                operator=None):
        """mcml_la / mcml_la_nr on the resident model (src/mcml_la.cpp:28-290); operator ("dense" / "component" /
        "component_wide", None = the context's setting): set_la_operator for this call only"""
        if operator is not None:
            prev = self.la_plan()["requested"]
            self.set_la_operator(operator)
            try:
                return self.mcml_la(start, usehess, tol, verbose, trace, maxiter, nr, maxfun)
            finally:
                self.set_la_operator(prev)
        start = _f(start).ravel(); R = self.npar()
        b = np.zeros(self.P); t = np.zeros(R); sg = C.c_double(); conv = C.c_int(); it = C.c_int()
        se = np.zeros(start.size); u = np.zeros(self.Q)
        e = self._ext(0, 1, maxfun)
        _lib.check(_lib.lib().glmmr_mcml_ctx_la(
            self._h, _p(start), start.size, int(nr), int(usehess), tol, int(verbose), int(trace),
            int(maxiter), C.byref(e), _p(b), _p(t), C.byref(sg), _p(se), _p(u), C.byref(conv), C.byref(it)))
        return dict(beta=b, theta=t, sigma=sg.value, se=se, u=u, converged=bool(conv.value), iters=it.value)

    def la_probe(self, start, kind, v=None, var_par=1.0, par=None):
        """test hook: LA functor values (kind 0, 1, 2) or one mcnr_b step (kind 3)"""
        start = _f(start).ravel()
        vv = None if v is None else _f(v).ravel()
        if kind == 3:
            vo = np.zeros(self.Q); bo = np.zeros(self.P); so = C.c_double()
            _lib.check(_lib.lib().glmmr_mcml_dbg_la_probe(self._h, _p(start), start.size, 3, _p(vv),
                                                          var_par, None, 0, None, _p(vo), _p(bo),
                                                          C.byref(so)))
            return dict(v=vo, beta=bo, sigma=so.value)
        pr = _f(par).ravel(); out = C.c_double()
        _lib.check(_lib.lib().glmmr_mcml_dbg_la_probe(self._h, _p(start), start.size, int(kind), _p(vv),
                                                      var_par, _p(pr), pr.size, C.byref(out), None, None,
                                                      None))
        return out.value

    def profile(self, enable=True, reset=False):
        out = np.zeros(8)
        fa = C.c_longlong(); ba = C.c_longlong()
        _lib.check(_lib.lib().glmmr_mcml_ctx_profile_launches(self._h, C.byref(fa), C.byref(ba)))
        _lib.check(_lib.lib().glmmr_mcml_ctx_profile(self._h, int(enable), int(reset), _p(out)))
        # fwd_n / bwd_n: launches that were TIMED (the sampler times one proposal in four); *_all: every launch
        return dict(fwd_ms=out[0], fwd_n=int(out[1]), bwd_ms=out[2], bwd_n=int(out[3]), fwd_flops=out[4],
                    bwd_flops=out[5], dense_flops=out[6], operator=("dense", "banded", "sparse")[int(out[7])],
                    fwd_n_all=fa.value, bwd_n_all=ba.value)


def _problem(cov, data, eff_range, Z=None, X=None, y=None, family=None, link=None):
    """(Problem, the arrays it points into: to be kept as long as it is in use).  Z = None: the covariance alone, no model"""
    keep = dict(cov=_i(cov), data=_f(data).ravel(), eff=_f(eff_range).ravel())
    p = Problem()
    p.cov = keep["cov"].ctypes.data_as(c_ip); p.cov_rows = keep["cov"].shape[0]
    p.data = _p(keep["data"]); p.data_len = keep["data"].size
    p.eff_range = _p(keep["eff"]); p.eff_len = keep["eff"].size
    if Z is not None:
        keep.update(Z=_f(Z), X=_f(X), y=_f(y).ravel())
        p.Z = _p(keep["Z"]); p.X = _p(keep["X"]); p.y = _p(keep["y"])
        p.n, p.Q = keep["Z"].shape; p.P = keep["X"].shape[1]
        p.family = family.encode(); p.link = link.encode()
    return p, keep


# ---------------------------------------------------------------------------
# Mirrors of the Rcpp exports
# ---------------------------------------------------------------------------
def mcml_full(cov, data, eff_range, Z, X, y, family, link, start, mcnr=False, m=500, maxiter=30,
              warmup=500, tol=1e-3, verbose=True, lambda_=0.05, trace=0, refresh=500, maxsteps=100,
              target_accept=0.9, seed=0, chains=1, maxfun=0):
    """mcml_full(...) -> dict(beta, theta, sigma, converged, u)   (src/mcml_full.cpp:41-148).
    seed / chains / maxfun are the build's additions (reference: random_device, 1 chain, 10000)."""
    p, keep = _problem(cov, data, eff_range, Z, X, y, family, link)
    start = _f(start).ravel()
    L = _lib.lib()
    ncol = L.glmmr_mcml_sample_cols(int(m), int(chains))
    R = int(start.size - p.P - 1)
    b = np.zeros(p.P); t = np.zeros(R); sg = C.c_double(); conv = C.c_int(); uc = C.c_int()
    u = np.zeros((p.Q, ncol), order="F")
    e = Ext(int(seed), int(chains), int(maxfun), 0, 0)
    _lib.check(L.glmmr_mcml_full(C.byref(p), _p(start), start.size, int(mcnr), int(m), int(maxiter), int(warmup),
                                 tol, int(verbose), lambda_, int(trace), int(refresh),
                                 int(maxsteps), target_accept, C.byref(e), _p(b), _p(t), C.byref(sg),
                                 C.byref(conv), _p(u), p.Q, C.byref(uc)))
    return dict(beta=b, theta=t, sigma=sg.value, converged=bool(conv.value), u=u[:, :uc.value])


def _la_call(fn, cov, data, eff_range, Z, X, y, family, link, start, usehess, tol, verbose, trace, maxiter, maxfun):
    p, keep = _problem(cov, data, eff_range, Z, X, y, family, link)
    start = _f(start).ravel()
    R = int(start.size - p.P - 1)
    b = np.zeros(p.P); t = np.zeros(R); sg = C.c_double(); se = np.zeros(start.size); u = np.zeros(p.Q)
    e = Ext(0, 1, int(maxfun), 0, 0)
    _lib.check(fn(C.byref(p), _p(start), start.size, int(usehess), tol, int(verbose), int(trace),
                  int(maxiter), C.byref(e), _p(b), _p(t), C.byref(sg), _p(se), _p(u)))
    return dict(beta=b, theta=t, sigma=sg.value, se=se, u=u.reshape(-1, 1))


def mcml_la(cov, data, eff_range, Z, X, y, family, link, start, usehess=False, tol=1e-3, verbose=True, trace=0,
            maxiter=10, maxfun=0, operator=None):
    """mcml_la(...) -> dict(beta, theta, sigma, se, u)   (src/mcml_la.cpp:28-155).  operator ("dense" / "component" /
    "component_wide", None = the process default): the default operator of the Laplace fits for the duration of the call"""
    with _LA_OP.default(operator):
        return _la_call(_lib.lib().glmmr_mcml_la, cov, data, eff_range, Z, X, y, family, link, start, usehess, tol,
                        verbose, trace, maxiter, maxfun)


def mcml_la_nr(cov, data, eff_range, Z, X, y, family, link, start, usehess=False, tol=1e-3, verbose=True, trace=0,
               maxiter=10, maxfun=0, operator=None):
    """mcml_la_nr(...) -> dict(beta, theta, sigma, se, u)   (src/mcml_la.cpp:174-290); operator ("dense" / "component" /
    "component_wide") as mcml_la"""
    with _LA_OP.default(operator):
        return _la_call(_lib.lib().glmmr_mcml_la_nr, cov, data, eff_range, Z, X, y, family, link, start, usehess, tol,
                        verbose, trace, maxiter, maxfun)


def information_matrix(cov, data, eff_range, Z, X, family, link, beta, theta, var_par=1.0, operator=None):
    """Context.information_matrix on a context made for the call (glmmr_mcml_information): the P x P GLS information
    X' (W^-1 + Z D(theta) Z')^-1 X at beta / var_par; beyond the reference's exports.  y is not read: zeros stand in for it"""
    Z = _f(Z)
    p, keep = _problem(cov, data, eff_range, Z, X, np.zeros(Z.shape[0]), family, link)
    beta = _f(beta).ravel(); theta = _f(theta).ravel()
    if beta.size != p.P:
        raise ValueError("beta must hold %d values" % p.P)
    out = np.zeros((p.P, p.P), order="F")
    _lib.check(_lib.lib().glmmr_mcml_information(C.byref(p), _p(beta), _p(theta), theta.size, float(var_par),
                                                 _INFO_OP[operator], _p(out), p.P))
    return out


def _theta_info_result(out, R, rows):
    """dict(information, names) from the (R + 1) x (R + 1) buffer a theta_information call filled with `rows` rows"""
    names = ["theta%d" % r for r in range(R)] + (["sigma"] if rows > R else [])
    return dict(information=np.ascontiguousarray(out[:rows, :rows]), names=names)


def theta_information(cov, data, eff_range, Z, X, family, link, beta, theta, var_par=1.0, operator=None):
    """Context.theta_information on a context made for the call (glmmr_mcml_theta_information): the GLS information of the
    covariance parameters (and of sigma for gaussian / identity) at beta / theta / var_par -> dict(information, names); beyond
    the reference's exports.  y is not read: zeros stand in for it"""
    Z = _f(Z)
    p, keep = _problem(cov, data, eff_range, Z, X, np.zeros(Z.shape[0]), family, link)
    beta = _f(beta).ravel(); theta = _f(theta).ravel()
    if beta.size != p.P:
        raise ValueError("beta must hold %d values" % p.P)
    R = _npar_of(cov)
    out = np.zeros((R + 1, R + 1), order="F")
    got = C.c_int()
    _lib.check(_lib.lib().glmmr_mcml_theta_information(C.byref(p), _p(beta), _p(theta), theta.size, float(var_par),
                                                       _INFO_OP[operator], _p(out), R + 1, C.byref(got)))
    return _theta_info_result(out, R, got.value)


def _small_sample_buffers(P, R):
    """the five outputs of a small_sample call, sized for the sigma row"""
    no = R + 1
    return (np.zeros((P, P), order="F"), np.zeros((no, no), order="F"), np.zeros(no * P * P), np.zeros(no * no * P * P),
            np.zeros(no * no * P * P))


def _small_sample_result(buf, P, R, rows):
    """dict(information, theta_information, P, Q, R, names) from the buffers a small_sample call filled with `rows` rows: the
    stacks hold column-major P x P matrices at r and r + rows s"""
    ti = _theta_info_result(buf[1], R, rows)
    Pm = buf[2][:rows * P * P].reshape(rows, P, P).transpose(0, 2, 1)
    Qm, Rm = (b[:rows * rows * P * P].reshape(rows, rows, P, P).transpose(1, 0, 3, 2) for b in buf[3:])
    return dict(information=buf[0], theta_information=ti["information"], P=np.ascontiguousarray(Pm), Q=np.ascontiguousarray(Qm),
                R=np.ascontiguousarray(Rm), names=ti["names"])


def small_sample(cov, data, eff_range, Z, X, family, link, beta, theta, var_par=1.0, operator=None):
    """Context.small_sample on a context made for the call (glmmr_mcml_small_sample): the ingredients of the Kenward-Roger /
    Satterthwaite corrections at beta / theta / var_par -> dict(information, theta_information, P, Q, R, names); beyond the
    reference's exports.  y is not read: zeros stand in for it"""
    Z = _f(Z)
    p, keep = _problem(cov, data, eff_range, Z, X, np.zeros(Z.shape[0]), family, link)
    beta = _f(beta).ravel(); theta = _f(theta).ravel()
    if beta.size != p.P:
        raise ValueError("beta must hold %d values" % p.P)
    R = _npar_of(cov)
    buf = _small_sample_buffers(p.P, R)
    got = C.c_int()
    _lib.check(_lib.lib().glmmr_mcml_small_sample(C.byref(p), _p(beta), _p(theta), theta.size, float(var_par), _INFO_OP[operator],
                                                  _p(buf[0]), p.P, _p(buf[1]), R + 1, _p(buf[2]), _p(buf[3]), _p(buf[4]),
                                                  C.byref(got)))
    return _small_sample_result(buf, p.P, R, got.value)


def _cluster_ids(cluster, n):
    """(the ids as the C ABI takes them, their count) -- (None, 0) for the default clusters; a wrong length is refused here"""
    if cluster is None:
        return None, 0
    cl = np.ascontiguousarray(np.asarray(cluster).ravel(), dtype=np.int32)
    if cl.size != n:
        raise ValueError("cluster must hold %d ids" % n)
    return cl, int(cl.max()) + 1 if cl.size else 0


def _sandwich_call(fn, n, P, cl, ncl, scores):
    """fn(cluster, ncluster, info, ldi, meat, ldm, scores, lds, ncluster_out) -> the dict of Context.sandwich"""
    info = np.zeros((P, P), order="F"); meat = np.zeros((P, P), order="F")
    rows = max(ncl if cl is not None else n, 1)                     # the default clusters are at most n
    G = np.zeros((rows, P), order="F") if scores else None
    got = C.c_int()
    _lib.check(fn(_p(cl), ncl, _p(info), P, _p(meat), P, _p(G), rows, C.byref(got)))
    out = dict(information=info, meat=meat, vcov=np.linalg.solve(info, np.linalg.solve(info, meat).T), ncluster=got.value)
    if scores:
        out["scores"] = np.ascontiguousarray(G[:got.value])
    return out


def sandwich(cov, data, eff_range, Z, X, y, family, link, beta, theta, var_par=1.0, cluster=None, operator=None, scores=False):
    """Context.sandwich on a context made for the call (glmmr_mcml_sandwich): the bread, the meat and the cluster-robust
    covariance of the fixed effects at beta / theta / var_par; beyond the reference's exports.  y IS read"""
    p, keep = _problem(cov, data, eff_range, Z, X, y, family, link)
    beta = _f(beta).ravel(); theta = _f(theta).ravel()
    if beta.size != p.P:
        raise ValueError("beta must hold %d values" % p.P)
    cl, ncl = _cluster_ids(cluster, p.n)
    return _sandwich_call(lambda *a: _lib.lib().glmmr_mcml_sandwich(C.byref(p), _p(beta), _p(theta), theta.size, float(var_par),
                                                                    _INFO_OP[operator], *a), p.n, p.P, cl, ncl, scores)


def _sampler_args(Z, L, X, y, beta, family, link):
    """the model with the caller's L as mcmc_sample / gen_u_samples pass it: (leading arguments, Q, the arrays to keep)"""
    Z = _f(Z); L = _f(L); X = _f(X); y = _f(y).ravel(); beta = _f(beta).ravel()
    n, Q = Z.shape
    return (_p(Z), _p(L), _p(X), _p(y), n, Q, X.shape[1], _p(beta), family.encode(), link.encode()), Q, (Z, L, X, y, beta)


def mcmc_sample(Z, L, X, y, beta, family, link, warmup, nsamp, lambda_, var_par=1, trace=0, refresh=500,
                maxsteps=100, target_accept=0.9, seed=0, chains=1):
    """mcmc_sample(...) -> Q x (nsamp+1) matrix of u = L v   (src/mcml_full.cpp:314-338)"""
    model, Q, keep = _sampler_args(Z, L, X, y, beta, family, link)
    lib = _lib.lib()
    ncol = lib.glmmr_mcml_sample_cols(int(nsamp), int(chains))
    out = np.zeros((Q, ncol), order="F"); nc = C.c_int()
    e = Ext(int(seed), int(chains), 0, 0, 0)
    _lib.check(lib.glmmr_mcml_mcmc_sample(*model, int(warmup), int(nsamp), lambda_, var_par, int(trace), int(refresh),
                                          int(maxsteps), target_accept, C.byref(e), _p(out), Q, C.byref(nc)))
    return out[:, :nc.value]


def gen_u_samples(y, X, Z, L, beta, family, link, sigma=1.0, warmup_iter=100, m=100, seed=0, chains=1,
                  max_treedepth=10, adapt_delta=0.8):
    """gen_u_samples(y, X, Z, L, beta, family, sigma, warmup_iter, m) -> Q x m matrix of u = L gamma
    (R/gen_u_samples.R:38-69; the NUTS sampler of csrc/nuts.h stands where cmdstanr is called)"""
    model, Q, keep = _sampler_args(Z, L, X, y, beta, family, link)
    ncol = chains * -(-int(m) // chains)
    out = np.zeros((Q, ncol), order="F"); nc = C.c_int()
    e = Ext(int(seed), int(chains), 0, 0, 0)
    o = NutsOpts(int(warmup_iter), int(m), int(max_treedepth), float(adapt_delta), 0.0, int(chains), 0, 0)
    _lib.check(_lib.lib().glmmr_mcml_gen_u_samples(*model, sigma, int(warmup_iter), int(m), C.byref(o), C.byref(e), _p(out), Q,
                                                   C.byref(nc)))
    return out[:, :nc.value]


def _call(fn, p, u, head, tail, sparse=None, maxfun=0):
    """the calling sequence the mirrors that take samples share: fn(problem[, Ap, Ai, nnz], u, ucols, *head, ext, *tail)"""
    u = _f(u)
    e = Ext(0, 1, int(maxfun), 0, 0)
    pattern = []
    if sparse is not None:
        Ap, Ai = _i(sparse[0]).ravel(), _i(sparse[1]).ravel()
        pattern = [_p(Ap), _p(Ai), Ai.size]
    _lib.check(fn(C.byref(p), *pattern, _p(u), u.shape[1], *head, C.byref(e), *tail))


def _fit_call(fn, prob_args, u, start, extra, sparse=None, maxfun=0):
    p, keep = _problem(*prob_args)
    start = _f(start).ravel()
    R = int(start.size - p.P - 1) if start.size > p.P + 1 else 0
    b = np.zeros(p.P); t = np.zeros(max(R, 64)); sg = C.c_double()
    _call(fn, p, u, [_p(start), start.size] + extra, [_p(b), _p(t), C.byref(sg)], sparse, maxfun)
    return b, t, sg.value


def _npar_of(cov):
    fnpar = [0, 1, 1, 1, 2, 2, 1, 2, 2, 2, 2, 2, 2, 2, 1]
    cov = _i(cov)
    return int(max(cov[r, 4] + fnpar[cov[r, 2]] for r in range(cov.shape[0])))


def mcml_optim(cov, data, eff_range, Z, X, y, u, family, link, start, trace=0, mcnr=False, maxfun=0):
    """mcml_optim(...) -> dict(beta, theta, sigma)   (src/mcml_optim.cpp:35-68)"""
    b, t, s = _fit_call(_lib.lib().glmmr_mcml_optim, (cov, data, eff_range, Z, X, y, family, link), u, start,
                        [int(trace), int(mcnr)], maxfun=maxfun)
    return dict(beta=b, theta=t[:_npar_of(cov)], sigma=s)


def mcml_simlik(cov, data, eff_range, Z, X, y, u, family, link, start, trace=0, maxfun=0):
    """mcml_simlik(...)   (src/mcml_optim.cpp:90-117)"""
    b, t, s = _fit_call(_lib.lib().glmmr_mcml_simlik, (cov, data, eff_range, Z, X, y, family, link), u, start,
                        [int(trace)], maxfun=maxfun)
    return dict(beta=b, theta=t[:_npar_of(cov)], sigma=s)


def mcml_optim_sparse(cov, data, eff_range, Ap, Ai, Z, X, y, u, family, link, start, trace=0, mcnr=False,
                      maxfun=0):
    """mcml_optim_sparse(...) -> dict(beta, theta, sigma, Ap, Ai, Ax, D)   (src/mcml_optim.cpp:147-184):
    Ap/Ai/Ax = the unit lower LDL' factor of D(theta) without its diagonal, D its pivots."""
    p, keep = _problem(cov, data, eff_range, Z, X, y, family, link)
    start = _f(start).ravel()
    lib = _lib.lib()
    cap = lib.glmmr_mcml_sparse_factor_nnz(p.cov, p.cov_rows, p.data, p.data_len)
    b = np.zeros(p.P); t = np.zeros(_npar_of(cov)); sg = C.c_double()
    Lp = np.zeros(p.Q + 1, dtype=np.int32); Li = np.zeros(max(cap, 1), dtype=np.int32)
    Lx = np.zeros(max(cap, 1)); D = np.zeros(p.Q)
    _call(lib.glmmr_mcml_optim_sparse, p, u, [_p(start), start.size, int(trace), int(mcnr)],
          [_p(b), _p(t), C.byref(sg), _p(Lp), _p(Li), _p(Lx), _p(D), cap], (Ap, Ai), maxfun)
    return dict(beta=b, theta=t, sigma=sg.value, Ap=Lp, Ai=Li[:cap], Ax=Lx[:cap], D=D)


def mcml_simlik_sparse(cov, data, eff_range, Ap, Ai, Z, X, y, u, family, link, start, trace=0, maxfun=0):
    """mcml_simlik_sparse(...)   (src/mcml_optim.cpp:210-239)"""
    b, t, s = _fit_call(_lib.lib().glmmr_mcml_simlik_sparse, (cov, data, eff_range, Z, X, y, family, link), u,
                        start, [int(trace)], sparse=(Ap, Ai), maxfun=maxfun)
    return dict(beta=b, theta=t[:_npar_of(cov)], sigma=s)


def mcml_hess(cov, data, eff_range, Z, X, y, u, family, link, start, tol=1e-5, trace=0, sparse=None):
    """mcml_hess(...) -> (P+R) x (P+R)   (src/mcml_optim.cpp:263-285; _sparse :313-337)"""
    p, keep = _problem(cov, data, eff_range, Z, X, y, family, link)
    start = _f(start).ravel()
    nv = p.P + _npar_of(cov)
    H = np.zeros((nv, nv), order="F")
    lib = _lib.lib()
    _call(lib.glmmr_mcml_hess if sparse is None else lib.glmmr_mcml_hess_sparse, p, u,
          [_p(start), start.size, tol, int(trace)], [_p(H)], sparse)
    return H


def mcml_hess_sparse(cov, data, eff_range, Ap, Ai, Z, X, y, u, family, link, start, tol=1e-5, trace=0):
    return mcml_hess(cov, data, eff_range, Z, X, y, u, family, link, start, tol, trace, sparse=(Ap, Ai))


def aic_mcml(cov, data, eff_range, Z, X, y, u, family, link, beta_par, cov_par):
    """aic_mcml(...) -> double   (src/mcml_optim.cpp:356-392)"""
    p, keep = _problem(cov, data, eff_range, Z, X, y, family, link)
    bp = _f(beta_par).ravel(); cp = _f(cov_par).ravel()
    out = C.c_double()
    _call(_lib.lib().glmmr_mcml_aic, p, u, [_p(bp), bp.size, _p(cp), cp.size], [C.byref(out)])
    return out.value


def _mvn_args(cov, data, eff_range, gamma, u):
    """what mvn_ll / mvn_ll_grad pass ahead of their outputs: (arguments, gamma, the sample matrix, the arrays to keep)"""
    p, keep = _problem(cov, data, eff_range)
    gamma = _f(gamma).ravel(); u = _cols(u)
    return (p.cov, p.cov_rows, p.data, p.data_len, p.eff_range, p.eff_len, _p(gamma), gamma.size, _p(u), u.shape[0],
            u.shape[1]), gamma, u, keep


def mvn_ll(cov, data, eff_range, gamma, u):
    """mvn_ll(cov, data, eff_range, gamma, u)  -- src/mcml_optim.cpp:406-414"""
    args, gamma, u, keep = _mvn_args(cov, data, eff_range, gamma, u)
    out = C.c_double()
    _lib.check(_lib.lib().glmmr_mcml_mvn_ll(*args, C.byref(out)))
    return out.value


def predict_re(cov, data, eff_range, gamma, u, newdata, means=False):
    """Context.predict_re on a context made for the call (glmmr_mcml_predict_re): the conditional prediction of the random
    effects at the new points of newdata given the Q x m sample columns u; beyond the reference's exports"""
    args, gamma, u, keep = _mvn_args(cov, data, eff_range, gamma, u)
    nnew, flat, K = _newdata(newdata, keep["cov"])
    summary = np.zeros((max(K, 1), 3), order="F")
    mm = np.zeros((max(K, 1), u.shape[1]), order="F") if means else None
    _lib.check(_lib.lib().glmmr_mcml_predict_re(*args, _p(nnew), _p(flat), flat.size, _p(summary), summary.shape[0], _p(mm),
                                                summary.shape[0]))
    return _prediction(summary, mm)


def mvn_ll_grad(cov, data, eff_range, gamma, u, weights=None):
    """(value, grad) of Context.mvn_ll_grad on a context made for the call (glmmr_mcml_mvn_ll_grad): the analytic score of
    mvn_ll in gamma; beyond the reference's exports"""
    args, gamma, u, keep = _mvn_args(cov, data, eff_range, gamma, u)
    w = _weights(weights, u.shape[1])
    out = C.c_double()
    grad = np.zeros(gamma.size)
    _lib.check(_lib.lib().glmmr_mcml_mvn_ll_grad(*args, _p(w), C.byref(out), _p(grad)))
    return out.value, grad
