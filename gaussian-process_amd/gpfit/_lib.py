"""ctypes binding of libgpfit.so (the C-ABI in include/gpfit.h).

There is deliberately no CPU fallback: if the HIP library is missing or no
device is visible, every entry point raises. The checker (oracle/) is a
separate, test-only tree.
"""
from __future__ import annotations

import ctypes
import hashlib
import os
from pathlib import Path

import numpy as np

from .kernels import KINDS, kernel_kind

PKG_DIR = Path(__file__).resolve().parent.parent
LIB_PATH = Path(os.environ.get("GPFIT_LIB", PKG_DIR / "libgpfit.so"))

GPF_OK, GPF_NOT_PD, GPF_HIP_ERROR, GPF_BAD_ARG = 0, 1, 2, 3
GPF_COMM_RCCL, GPF_COMM_HOST = 1, 2
GPF_OP_SUM, GPF_OP_MAX = 0, 1
ABI_VERSION = 2
MEAN_MAX = 32  # rows of a mean function's basis at most (gpf_set_basis)

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)
_vp = ctypes.c_void_p

# name -> (restype, argtypes); mirrors include/gpfit.h
SIGNATURES = {
    "gpf_version": (ctypes.c_int, []),
    "gpf_tile": (ctypes.c_int, []),
    "gpf_open": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_vp)]),
    "gpf_close": (None, [_vp]),
    "gpf_last_error": (ctypes.c_char_p, [_vp]),
    "gpf_set_data": (ctypes.c_int, [_vp, _dp, _dp, _dp, ctypes.c_int64, ctypes.c_int]),
    "gpf_set_grid": (ctypes.c_int, [_vp, _dp, _dp, ctypes.c_int, _dp, _dp]),
    "gpf_set_kernel": (ctypes.c_int, [_vp, ctypes.c_int]),
    "gpf_get_kernel": (ctypes.c_int, [_vp, _ip]),
    "gpf_eval_batch": (ctypes.c_int, [_vp, _dp, ctypes.c_int, _dp, _dp, _dp, _ip]),
    "gpf_predict": (ctypes.c_int, [_vp, _dp, _dp, ctypes.c_int64, ctypes.c_int64, _dp, _dp]),
    "gpf_predict_cov": (ctypes.c_int, [_vp, _dp, _dp, ctypes.c_int64, _dp, _dp]),
    "gpf_predict_linear": (ctypes.c_int, [_vp, _dp, _dp, ctypes.c_int64, _dp, ctypes.c_int, ctypes.c_int64, _dp, _dp, _dp]),
    "gpf_predict_conditioned": (ctypes.c_int, [_vp, _dp, _dp, ctypes.c_int64, _dp, ctypes.c_int, _dp, _dp, ctypes.c_int64,
                                               _dp, _dp, _dp, _dp, _dp]),
    "gpf_chol_dense": (ctypes.c_int, [_vp, _dp, ctypes.c_int64, _dp, ctypes.c_int, _dp, _dp, _ip]),
    "gpf_posterior_draws": (ctypes.c_int, [_vp, _dp, _dp, ctypes.c_int64, _dp, ctypes.c_int64, _dp, ctypes.c_int,
                                           _dp, _dp, _dp, _dp, _ip]),
    "gpf_kernel": (ctypes.c_int, [_vp, _dp, ctypes.c_int64, _dp, ctypes.c_int64, ctypes.c_int, _dp, _dp]),
    "gpf_log_marginal_likelihood": (ctypes.c_int, [_vp, _dp, _dp]),
    "gpf_lml_batch": (ctypes.c_int, [_vp, _dp, ctypes.c_int, _dp, _dp, _ip, _ip]),
    "gpf_loo_batch": (ctypes.c_int, [_vp, _dp, ctypes.c_int, _dp, _dp, _dp, _dp, _ip, _ip]),
    "gpf_lml_hyper_batch": (ctypes.c_int, [_vp, _dp, ctypes.c_int, _dp, _dp, _dp, _ip, _ip]),
    "gpf_set_basis": (ctypes.c_int, [_vp, _dp, ctypes.c_int]),
    "gpf_lml_mean_batch": (ctypes.c_int, [_vp, _dp, ctypes.c_int, _dp, _dp, _dp, _dp, _ip, _ip]),
    "gpf_predict_mean": (ctypes.c_int, [_vp, _dp, _dp, _dp, ctypes.c_int64, ctypes.c_int64, _dp, _dp, _dp, _dp]),
    "gpf_predict_batch": (ctypes.c_int, [_vp, _dp, ctypes.c_int, _dp, _dp, ctypes.c_int64, ctypes.c_int64,
                                         _dp, _dp, _dp, _dp, _ip]),
    "gpf_predict_batch_plan": (ctypes.c_int, [ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                              ctypes.c_double, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_double,
                                              ctypes.c_double, _ip, ctypes.POINTER(ctypes.c_int64), _ip]),
    "gpf_set_profiling": (ctypes.c_int, [_vp, ctypes.c_int]),
    "gpf_get_profile": (ctypes.c_int, [_vp, _dp, ctypes.c_int]),
    "gpf_reset_profile": (ctypes.c_int, [_vp]),
    "gpf_selftest_mfma": (ctypes.c_int, [_vp, _dp, _dp, _dp]),
    "gpf_debug_factor": (ctypes.c_int, [_vp, _dp, _dp, _dp, _dp, _dp]),
    "gpf_debug_factor128": (ctypes.c_int, [_vp, _dp, _dp, ctypes.c_int, _dp, _dp, _dp, _dp, _dp, _ip, _dp]),
    "gpf_mfma_peak": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _dp]),
    "gpf_prob_surface": (ctypes.c_int, [_vp, _dp, ctypes.c_int64, ctypes.c_int, _dp, _dp,
                                        ctypes.POINTER(ctypes.c_int)]),
    "gpf_hull_fill": (ctypes.c_int, [_vp, _dp, ctypes.c_int64, ctypes.c_int, _dp, ctypes.POINTER(ctypes.c_int),
                                     ctypes.POINTER(ctypes.c_int64)]),
    "gpf_hull_fetch": (ctypes.c_int, [_vp, _dp]),
    "gpf_gemm_bench": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_int, _dp]),
    "gpf_build_info": (ctypes.c_char_p, []),
    "gpf_sync": (ctypes.c_int, [_vp]),
    "gpf_comm_open": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
                                     ctypes.POINTER(_vp)]),
    "gpf_comm_close": (None, [_vp]),
    "gpf_comm_rank": (ctypes.c_int, [_vp]),
    "gpf_comm_size": (ctypes.c_int, [_vp]),
    "gpf_comm_last_error": (ctypes.c_char_p, [_vp]),
    "gpf_comm_stats": (ctypes.c_int, [_vp, _dp, ctypes.POINTER(ctypes.c_longlong)]),
    "gpf_comm_allreduce": (ctypes.c_int, [_vp, _dp, ctypes.c_int64, ctypes.c_int]),
    "gpf_comm_exchange_scores": (ctypes.c_int, [_vp, ctypes.c_int, _dp, ctypes.c_int, ctypes.c_int, _dp, _ip]),
    "gpf_eval_batch_sharded": (ctypes.c_int, [_vp, _vp, _dp, ctypes.c_int, _dp, _ip]),
    "gpf_plan_check": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong),
                                      ctypes.c_char_p, ctypes.c_int]),
    "gpf_bench_clock": (ctypes.c_int, [_vp, _dp]),
    "gpf_kmeans_set": (ctypes.c_int, [_vp, _dp, ctypes.c_int64, ctypes.c_int]),
    "gpf_kmeans_step": (ctypes.c_int, [_vp, _dp, ctypes.c_int, ctypes.c_int, _ip, _dp, _dp, _dp]),
}

_LIB = None


class GPFitError(RuntimeError):
    """HIP runtime failure inside libgpfit."""


def load_library():
    """Load libgpfit.so (raises OSError with a build hint if it is missing)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not LIB_PATH.exists():
        raise OSError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = ctypes.CDLL(str(LIB_PATH))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.gpf_version() != ABI_VERSION:
        raise OSError(f"libgpfit ABI {lib.gpf_version()} != expected {ABI_VERSION}")
    _LIB = lib
    return lib


def build_info():
    """Provenance string baked into the loaded library (gpf_build_info)."""
    return load_library().gpf_build_info().decode()


def plan_check(particles, nt):
    """Host-side check of the k_step dispatch plan (gpf_plan_check); raises AssertionError
    naming the first violation, else returns the stats dict. Reads the GPF_* environment."""
    lib = load_library()
    stats = (ctypes.c_longlong * 11)()
    msg = ctypes.create_string_buffer(256)
    rc = lib.gpf_plan_check(int(particles), int(nt), stats, msg, 256)
    if rc != GPF_OK:
        raise AssertionError(f"plan_check(pc={particles}, nt={nt}): {msg.value.decode()}")
    keys = ("launches", "workgroups", "whole_tiles", "split_tiles", "S", "Smax", "groups", "diag_workgroups",
            "syrk_workgroups", "persistent", "lead_launches")
    return dict(zip(keys, list(stats)))


def predict_batch_plan(free_b, held_b, cap_slots, per_particle_b, per_col_b, fixed_b, particles, m_pad, chunk=0,
                       keep_b=2048 * 1048576.0, mem_fraction=0.85):
    """gpf_predict_batch's memory plan for given byte counts (gpf_predict_batch_plan; host only):
    {"pc", "cq", "regrow"}, or ValueError if one particle at chunk 128 does not fit."""
    lib = load_library()
    pc, cq, regrow = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int(0)
    rc = lib.gpf_predict_batch_plan(float(free_b), float(held_b), int(cap_slots), float(per_particle_b), float(per_col_b),
                                    float(fixed_b), int(particles), int(m_pad), int(chunk), float(keep_b), float(mem_fraction),
                                    ctypes.byref(pc), ctypes.byref(cq), ctypes.byref(regrow))
    if rc != GPF_OK:
        raise ValueError("predict_batch_plan: does not fit, or bad arguments")
    return {"pc": pc.value, "cq": cq.value, "regrow": bool(regrow.value)}


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    return a.ctypes.data_as(_dp)


JITTERS = (1e-12, 1e-10, 1e-8, 1e-6)   # gpfit.posterior's ladder: GP_func.py:39's variance floor, x 100 per failure


def check_jitters(jitters):
    """The jitter ladder as a (nj,) float64 array; ValueError if it is empty, not one-dimensional,
    not finite, negative or not strictly ascending (checked before the library is touched)."""
    j = np.array(jitters, dtype=np.float64, ndmin=1)
    if j.ndim != 1 or j.size < 1:
        raise ValueError("jitters must be a non-empty sequence")
    if not np.all(np.isfinite(j)) or np.any(j < 0.0):
        raise ValueError("jitters must be finite and >= 0")
    if np.any(np.diff(j) <= 0.0):
        raise ValueError("jitters must be strictly ascending")
    return np.ascontiguousarray(j)


def check_draw_args(d, lengths, x_fit, z, jitters):
    """Shapes and ladder of a posterior_draws call against the data's dimensionality d, before the
    library is touched: (ls (d,), xf (d, M), z (S, M), jitters (nj,)) as contiguous float64 arrays;
    ValueError otherwise."""
    j = check_jitters(jitters)
    ls, xf, z = _f64(lengths).reshape(-1), _f64(x_fit), _f64(z)
    if xf.ndim != 2 or xf.shape[0] != d or ls.shape[0] != d:
        raise ValueError(f"x_fit must be ({d}, M) and lengths ({d},)")
    if z.ndim != 2 or z.shape[1] != xf.shape[1]:
        raise ValueError(f"z must be (S, {xf.shape[1]})")
    return ls, xf, z, j


def _digest(*arrays):
    """sha256 over the arrays' shapes and bytes: the key that decides whether an upload can be
    skipped (a Python hash() collision would silently score stale data)."""
    h = hashlib.sha256()
    for a in arrays:
        h.update(repr(a.shape).encode())
        h.update(a.tobytes())
    return h.digest()


def default_device():
    """One process per GPU: torch.distributed launchers export LOCAL_RANK."""
    return int(os.environ.get("GPFIT_DEVICE", os.environ.get("LOCAL_RANK", "0")))


def use_kernel(ctx, kernel):
    """Set ``kernel`` on the context a call is about to use: every entry point with a kernel= keyword
    does this on every call, so a call without the keyword is "se" whatever ran before on a shared
    context. A stand-in context without set_kernel (the host tests') can only be "se"."""
    kind = kernel_kind(kernel)
    setter = getattr(ctx, "set_kernel", None)
    if setter is not None:
        setter(kernel)
    elif kind != 0:
        raise ValueError(f"kernel={kernel!r}: this context has no set_kernel")


class Context:
    """One HIP device, one stream, device-resident training data (gpf_ctx)."""

    def __init__(self, device=None):
        self.lib = load_library()
        self.device = default_device() if device is None else int(device)
        h = _vp()
        rc = self.lib.gpf_open(self.device, ctypes.byref(h))
        if rc != GPF_OK or not h.value:
            raise GPFitError(f"gpf_open(device={self.device}) failed (rc={rc}); is a GPU visible?")
        self._h = h
        self.N = 0
        self.d = 0
        self.m = 0  # rows of the mean function's basis (set_basis), 0: none
        self._data_key = None
        self._grid_key = None

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.gpf_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- error mapping: same exception types as the reference's numpy path --
    def _check(self, rc, what, bad=None):
        if rc == GPF_OK:
            return
        msg = self.lib.gpf_last_error(self._h).decode(errors="replace")
        if rc == GPF_NOT_PD:
            err = np.linalg.LinAlgError("Matrix is not positive definite")
            # the batch row of the first failing particle (gpf_eval_batch's bad_idx), or None
            err.particle = None if bad is None or bad.value < 0 else int(bad.value)
            raise err
        if rc == GPF_BAD_ARG:
            raise ValueError(f"{what}: {msg}")
        raise GPFitError(f"{what}: {msg}")

    def set_data(self, x_dN, y, e):
        x = _f64(x_dN)
        if x.ndim != 2:
            raise ValueError("x must be (d, N)")
        y, e = _f64(y), _f64(e)
        d, n = x.shape
        key = _digest(x, y, e)
        if key == self._data_key:
            return
        self._check(self.lib.gpf_set_data(self._h, _ptr(x), _ptr(y), _ptr(e), n, d), "gpf_set_data")
        self.N, self.d = n, d
        self._data_key = key
        self._grid_key = None
        self.m = 0  # gpf_set_data discards the mean function's basis

    def set_kernel(self, kernel):
        """The covariance kernel of every later call on this context: "se" (the default, the
        reference's kernel_func), "matern32" or "matern52" (gpf_set_kernel; gpfit.kernels has the
        formulas). Needs no data and persists across set_data. An unknown name is a ValueError before
        the library is called. On the process-wide default_context() the kind does not outlive the next
        drop-in call: GP(), kernel_func(), evaluate_loss() and every entry point with a kernel= keyword set
        their own (the keyword's, "se" without it) on the context they use."""
        kind = kernel_kind(kernel)
        self._check(self.lib.gpf_set_kernel(self._h, kind), "gpf_set_kernel")

    @property
    def kernel_name(self):
        """The context's covariance kernel (gpf_get_kernel): "se", "matern32" or "matern52"."""
        kind = ctypes.c_int(-1)
        self._check(self.lib.gpf_get_kernel(self._h, ctypes.byref(kind)), "gpf_get_kernel")
        return KINDS[kind.value]

    def set_grid(self, sigma_vals, expected, lo, hi):
        s, ex = _f64(sigma_vals), _f64(expected)
        lo, hi = _f64(lo).reshape(-1), _f64(hi).reshape(-1)
        # gpf_set_grid reads K doubles of each grid array and d of each bound: check the lengths here
        if s.ndim != 1:
            raise ValueError(f"set_grid: sigma_vals must be one-dimensional, got shape {s.shape}")
        if ex.shape != s.shape:
            raise ValueError(f"set_grid: expected has shape {ex.shape}, sigma_vals {s.shape}")
        if not lo.shape == hi.shape == (self.d,):
            raise ValueError(f"set_grid: lo {lo.shape} and hi {hi.shape} must both be ({self.d},), the data's d "
                             "(call set_data first)")
        key = _digest(s, ex, lo, hi)
        if key == self._grid_key:
            return
        self._check(self.lib.gpf_set_grid(self._h, _ptr(s), _ptr(ex), s.shape[0], _ptr(lo), _ptr(hi)),
                    "gpf_set_grid")
        self._grid_key = key

    # gpf_eval_batch, gpf_predict, gpf_log_marginal_likelihood and gpf_debug_factor read d doubles per
    # length-scale row (and d rows of x_fit) whatever the caller's arrays hold: the shapes are checked here
    def _check_positions(self, P):
        if P.ndim != 2 or (self.d and P.shape[1] != self.d):
            raise ValueError(f"positions must be (P, {self.d})")

    def _check_lengths(self, ls):
        if self.d and ls.shape[0] != self.d:
            raise ValueError(f"lengths must be ({self.d},)")

    def _lengths_and_queries(self, lengths, x_fit):
        """(ls (d,), xf (d, M)) of a posterior call as contiguous float64 arrays; ValueError otherwise."""
        ls, xf = _f64(lengths).reshape(-1), _f64(x_fit)
        if xf.ndim != 2:
            raise ValueError("x_fit must be (d, M)")
        if self.d and (xf.shape[0] != self.d or ls.shape[0] != self.d):
            raise ValueError(f"x_fit must be ({self.d}, M) and lengths ({self.d},)")
        return ls, xf

    def eval_batch(self, positions, want_mu_sd=False):
        P = _f64(positions)
        if P.ndim == 1:
            P = P.reshape(1, -1)
        self._check_positions(P)
        n = P.shape[0]
        loss = np.empty(n)
        mu = np.empty((n, self.N)) if want_mu_sd else None
        sd = np.empty((n, self.N)) if want_mu_sd else None
        bad = ctypes.c_int(-1)
        rc = self.lib.gpf_eval_batch(self._h, _ptr(P), n, _ptr(loss),
                                     _ptr(mu) if want_mu_sd else None,
                                     _ptr(sd) if want_mu_sd else None, ctypes.byref(bad))
        self._check(rc, "gpf_eval_batch", bad)
        return (loss, mu, sd) if want_mu_sd else loss

    def eval_batch_sharded(self, comm, positions):
        """This rank's rows of the (P, d) batch on this GPU, then the swarm exchange
        (gpf_eval_batch_sharded): every rank returns the same (P,) scores, or raises the same
        error (LinAlgError for a non-PD particle on any rank)."""
        P = _f64(positions)
        if P.ndim == 1:
            P = P.reshape(1, -1)
        self._check_positions(P)
        loss = np.empty(P.shape[0])
        bad = ctypes.c_int(-1)
        rc = self.lib.gpf_eval_batch_sharded(self._h, comm.handle, _ptr(P), P.shape[0], _ptr(loss), ctypes.byref(bad))
        self._check(rc, "gpf_eval_batch_sharded", bad)
        return loss

    def synchronize(self):
        """Device-wide fence (gpf_sync): all queued work on this context's GPU has finished."""
        self._check(self.lib.gpf_sync(self._h), "gpf_sync")

    def predict(self, lengths, x_fit, batch_size=10000):
        ls, xf = self._lengths_and_queries(lengths, x_fit)
        m = xf.shape[1]
        mu, sd = np.empty(m), np.empty(m)
        self._check(self.lib.gpf_predict(self._h, _ptr(ls), _ptr(xf), m, int(batch_size), _ptr(mu), _ptr(sd)),
                    "gpf_predict")
        return mu, sd

    def predict_cov(self, lengths, x_fit):
        """Joint latent posterior of the query points x_fit (d, M) (gpf_predict_cov):
        (mu (M,), cov (M, M)), cov = K_ss - K_s^T Kn^-1 K_s exactly symmetric with an unclipped
        diagonal; mu is bitwise predict()'s. LinAlgError if the covariance of the training points
        is not positive definite, ValueError for bad arguments or an M whose dense cov does not
        fit the device (the message names the largest M that does)."""
        ls, xf = self._lengths_and_queries(lengths, x_fit)
        m = xf.shape[1]
        mu, cov = np.empty(m), np.empty((m, m))
        self._check(self.lib.gpf_predict_cov(self._h, _ptr(ls), _ptr(xf), m, _ptr(mu), _ptr(cov)), "gpf_predict_cov")
        return mu, cov

    def predict_linear(self, lengths, x_fit, weights, chunk=0, want_prior=False):
        """Linear functionals of the latent posterior at x_fit (d, M) with the weights (R, M), one row
        per functional (gpf_predict_linear): (mean (R,), cov (R, R)) = (A mu, A Sigma A^T) with
        predict_cov's Sigma, without the M x M matrix: the query axis is folded away ``chunk`` points
        per pass (rounded up to 128; 0: the library's default). With want_prior also the prior
        covariance A K_ss A^T (R, R). cov and prior are exactly symmetric and not clipped. The same
        chunk gives the same bits on every call; another chunk may differ in the last bits.
        LinAlgError if the covariance of the training points is not positive definite, ValueError for
        bad arguments or an M that does not fit the device at this R (the message names the largest)."""
        ls, xf = self._lengths_and_queries(lengths, x_fit)
        w = _f64(weights)
        m = xf.shape[1]
        if w.ndim != 2 or w.shape[1] != m:
            raise ValueError(f"weights must be (R, {m})")
        r = w.shape[0]
        mean, cov = np.empty(r), np.empty((r, r))
        prior = np.empty((r, r)) if want_prior else None
        rc = self.lib.gpf_predict_linear(self._h, _ptr(ls), _ptr(xf), m, _ptr(w), r, int(chunk), _ptr(mean), _ptr(cov),
                                         _ptr(prior) if want_prior else None)
        self._check(rc, "gpf_predict_linear")
        return (mean, cov, prior) if want_prior else (mean, cov)

    def predict_conditioned(self, lengths, x_fit, weights, values, noise, chunk=0, want_functionals=False):
        """The latent posterior at x_fit (d, M) conditioned on R measured linear functionals
        (gpf_predict_conditioned): values[r] = sum_q weights[r, q] f(x_q) + N(0, noise[r]^2), the
        errors independent, noise[r] >= 0. Returns (mu' (M,), sd' (M,), info) with info["chi2"] =
        (b - A mu)^T H^-1 (b - A mu), H = A Sigma A^T + diag(noise^2): the agreement of the
        measurements with the fit before conditioning (about R is expected). With want_functionals
        also info["fmean"] (R,) and info["fcov"] (R, R): A mu and A Sigma A^T before conditioning,
        bitwise predict_linear()'s at the same chunk. ``chunk`` as predict_linear. With R = 0 the
        plain prediction. LinAlgError if the covariance of the training points or H is not positive
        definite (redundant functionals with zero noise), ValueError for bad arguments."""
        ls, xf = self._lengths_and_queries(lengths, x_fit)
        w, b, s = _f64(weights), _f64(values).reshape(-1), _f64(noise).reshape(-1)
        m = xf.shape[1]
        if w.ndim != 2 or w.shape[1] != m:
            raise ValueError(f"weights must be (R, {m})")
        r = w.shape[0]
        if b.shape != (r,) or s.shape != (r,):
            raise ValueError(f"values and noise must be ({r},)")
        if r == 0:
            mu, sd = self.predict(ls, xf) if m else (np.empty(0), np.empty(0))
            info = {"chi2": 0.0}
            if want_functionals:
                info.update(fmean=np.empty(0), fcov=np.empty((0, 0)))
            return mu, sd, info
        mu, sd = np.empty(m), np.empty(m)
        fmean = np.empty(r) if want_functionals else None
        fcov = np.empty((r, r)) if want_functionals else None
        chi2 = ctypes.c_double(0.0)
        rc = self.lib.gpf_predict_conditioned(self._h, _ptr(ls), _ptr(xf), m, _ptr(w), r, _ptr(b), _ptr(s), int(chunk),
                                              _ptr(mu), _ptr(sd), _ptr(fmean) if want_functionals else None,
                                              _ptr(fcov) if want_functionals else None, ctypes.byref(chi2))
        self._check(rc, "gpf_predict_conditioned")
        info = {"chi2": float(chi2.value)}
        if want_functionals:
            info.update(fmean=fmean, fcov=fcov)
        return mu, sd, info

    def chol_dense(self, a, jitters=JITTERS):
        """Cholesky factor of the dense symmetric matrix a (n, n) on the device (gpf_chol_dense):
        (L (n, n) with zeros above the diagonal, info), L L^T = a + jitter I for the first jitter of
        the ladder that factorises; info: "jitter" and "tries". Only a's lower triangle is read.
        LinAlgError (with .tries) if every jitter fails, ValueError for a bad shape or ladder."""
        j = check_jitters(jitters)
        a = _f64(a)
        if a.ndim != 2 or a.shape[0] != a.shape[1]:
            raise ValueError("a must be a square matrix")
        n = a.shape[0]
        L = np.empty((n, n))
        jit, tries = ctypes.c_double(0.0), ctypes.c_int(0)
        rc = self.lib.gpf_chol_dense(self._h, _ptr(a), n, _ptr(j), int(j.size), _ptr(L), ctypes.byref(jit),
                                     ctypes.byref(tries))
        self._check_ladder(rc, "gpf_chol_dense", tries)
        if n == 0:
            return L, {"jitter": float(j[0]), "tries": 0}
        return L, {"jitter": float(jit.value), "tries": int(tries.value)}

    def _check_ladder(self, rc, what, tries):
        try:
            self._check(rc, what)
        except np.linalg.LinAlgError as err:
            err.tries = int(tries.value)
            raise

    def posterior_draws(self, lengths, x_fit, z, jitters=JITTERS, want_chol=False, out=None):
        """Joint draws of the latent posterior at x_fit (d, M) from the normals z (S, M), Sigma and
        its factor staying on the device (gpf_posterior_draws): (mu (M,), draws (S, M), info).
        mu is bitwise predict_cov()'s; draws = mu + z L^T, L L^T = Sigma + jitter I. info: "jitter",
        "tries" and, with want_chol, "chol" (M, M). ``out`` = (mu, draws) float64 arrays to write into.
        LinAlgError if the training covariance is not positive definite or every jitter fails (the
        outputs are then untouched), ValueError for bad shapes, a bad ladder or an M that does not
        fit the device."""
        if not self.d:
            raise ValueError("posterior_draws: call set_data first")
        ls, xf, z, j = check_draw_args(self.d, lengths, x_fit, z, jitters)
        m, s = xf.shape[1], z.shape[0]
        if out is None:
            mu, draws = np.empty(m), np.empty((s, m))
        else:
            mu, draws = out
            if (mu.shape != (m,) or draws.shape != (s, m) or mu.dtype != np.float64 or draws.dtype != np.float64
                    or not mu.flags.c_contiguous or not draws.flags.c_contiguous):
                raise ValueError(f"out must be C-contiguous float64 arrays ({m},) and ({s}, {m})")
        chol = np.empty((m, m)) if want_chol else None
        jit, tries = ctypes.c_double(0.0), ctypes.c_int(0)
        rc = self.lib.gpf_posterior_draws(self._h, _ptr(ls), _ptr(xf), m, _ptr(z), s, _ptr(j), int(j.size), _ptr(mu),
                                          _ptr(draws), _ptr(chol) if want_chol else None, ctypes.byref(jit),
                                          ctypes.byref(tries))
        self._check_ladder(rc, "gpf_posterior_draws", tries)
        info = {"jitter": float(jit.value), "tries": int(tries.value)}
        if want_chol:
            info["chol"] = chol
        return mu, draws, info

    def kernel(self, x1, x2, l):
        a, b = _f64(x1), _f64(x2)
        ls = _f64(l).reshape(-1)
        # gpf_kernel reads d rows of both point sets and d length scales, d = x1's
        if a.ndim != 2 or b.ndim != 2 or b.shape[0] != a.shape[0]:
            raise ValueError("x1 must be (d, N1) and x2 (d, N2)")
        if ls.shape[0] != a.shape[0]:
            raise ValueError(f"l must be ({a.shape[0]},)")
        out = np.empty((a.shape[1], b.shape[1]))
        self._check(self.lib.gpf_kernel(self._h, _ptr(a), a.shape[1], _ptr(b), b.shape[1], a.shape[0],
                                        _ptr(ls), _ptr(out)), "gpf_kernel")
        return out

    def log_marginal_likelihood(self, lengths):
        ls = _f64(lengths).reshape(-1)
        self._check_lengths(ls)
        out = ctypes.c_double(0.0)
        self._check(self.lib.gpf_log_marginal_likelihood(self._h, _ptr(ls), ctypes.byref(out)),
                    "gpf_log_marginal_likelihood")
        return out.value

    def lml_batch(self, positions, grad=True, strict=True):
        """Log marginal likelihood of every row of positions (P, d) and, with grad, its gradient
        in the length scales (gpf_lml_batch): (lml (P,), grad (P, d) or None). Needs set_data
        only. A particle whose covariance is not positive definite raises LinAlgError with
        .particle set to its row (strict), or gets lml = -inf and a NaN gradient row while the
        other rows are computed (strict=False)."""
        P = _f64(positions)
        if P.ndim == 1:
            P = P.reshape(1, -1)
        n = P.shape[0]
        if self.d and P.shape[1] != self.d:
            raise ValueError(f"positions must be (P, {self.d})")
        lml = np.empty(n)
        g = np.empty((n, P.shape[1])) if grad else None
        status = np.zeros(n, dtype=np.int32)
        bad = ctypes.c_int(-1)
        rc = self.lib.gpf_lml_batch(self._h, _ptr(P), n, _ptr(lml), _ptr(g) if grad else None,
                                    status.ctypes.data_as(_ip), ctypes.byref(bad))
        if rc != GPF_NOT_PD or strict:
            self._check(rc, "gpf_lml_batch", bad)
        return lml, g

    def lml_hyper_batch(self, theta, grad=True, strict=True, want_q=False):
        """Log marginal likelihood of every row (l_1 .. l_d, a, s) of theta (P, d + 2) under
        Kn = a^2 K(l) + s^2 diag(e^2) (a: the prior sd, s: a factor on the quoted errors) and, with
        grad, its gradient in all d + 2 (gpf_lml_hyper_batch): (lml (P,), grad (P, d + 2) or None),
        and with want_q also Q = y^T Kt^-1 y of the unit-amplitude Kt = K + (s/a)^2 diag(e^2): for
        fixed l and s/a the best amplitude is sqrt(Q / N). Needs set_data only. A particle whose
        covariance is not positive definite raises LinAlgError with .particle set to its row
        (strict), or gets lml = -inf and NaN in its gradient row and Q while the other rows are
        computed (strict=False)."""
        th = _f64(theta)
        if th.ndim == 1:
            th = th.reshape(1, -1)
        n = th.shape[0]
        if th.ndim != 2 or th.shape[1] < 3 or (self.d and th.shape[1] != self.d + 2):
            raise ValueError(f"theta must be (P, {self.d + 2}): the length scales, then a and s" if self.d
                             else "theta must be (P, d + 2): the length scales, then a and s")
        lml = np.empty(n)
        g = np.empty(th.shape) if grad else None
        q = np.empty(n) if want_q else None
        status = np.zeros(n, dtype=np.int32)
        bad = ctypes.c_int(-1)
        rc = self.lib.gpf_lml_hyper_batch(self._h, _ptr(th), n, _ptr(lml), _ptr(g) if grad else None,
                                          _ptr(q) if want_q else None, status.ctypes.data_as(_ip), ctypes.byref(bad))
        if rc != GPF_NOT_PD or strict:
            self._check(rc, "gpf_lml_hyper_batch", bad)
        return (lml, g, q) if want_q else (lml, g)

    def set_basis(self, H):
        """The mean function's basis at the training points, H (m, N), 1 <= m <= 32, m < N, finite, full
        row rank (gpf_set_basis; gpfit.meanfn.basis builds the polynomial ones). Every set_data with
        new data discards it."""
        H = _f64(H)
        if H.ndim == 1:
            H = H.reshape(1, -1)
        if not self.N:
            raise ValueError("set_basis: call set_data first")
        if H.ndim != 2 or H.shape[1] != self.N:
            raise ValueError(f"set_basis: H must be (m, {self.N}), the basis at the training points")
        m = H.shape[0]
        if not 1 <= m <= MEAN_MAX:
            raise ValueError(f"set_basis: the basis needs 1 to {MEAN_MAX} rows, got {m}")
        if m >= self.N:
            raise ValueError(f"set_basis: the basis needs fewer rows than there are points ({m} >= {self.N})")
        if not np.all(np.isfinite(H)):
            raise ValueError("set_basis: the basis must be finite")
        if np.linalg.matrix_rank(H) < m:
            raise ValueError("set_basis: H is rank-deficient (its rows must be linearly independent)")
        self._check(self.lib.gpf_set_basis(self._h, _ptr(H), m), "gpf_set_basis")
        self.m = m

    def lml_mean_batch(self, theta, grad=True, strict=True, want_q=False, want_beta=False):
        """lml_hyper_batch with the polynomial mean of set_basis integrated out under a flat prior: the
        restricted log marginal likelihood of every row (l_1 .. l_d, a, s) of theta (P, d + 2) and,
        with grad, its gradient in all d + 2 (gpf_lml_mean_batch): (lml (P,), grad (P, d + 2) or None),
        then with want_q the residual's Q' (P,) (for fixed l and s / a the best amplitude is
        sqrt(Q' / (N - m))) and with want_beta the coefficients beta (P, m). A particle whose
        covariance, or whose H Kt^-1 H^T, is not positive definite raises LinAlgError with .particle
        set (strict), or gets -inf and NaN rows while the others are computed (strict=False)."""
        th = _f64(theta)
        if th.ndim == 1:
            th = th.reshape(1, -1)
        n = th.shape[0]
        if th.ndim != 2 or th.shape[1] < 3 or (self.d and th.shape[1] != self.d + 2):
            raise ValueError(f"theta must be (P, {self.d + 2}): the length scales, then a and s" if self.d
                             else "theta must be (P, d + 2): the length scales, then a and s")
        if self.N and not self.m:
            raise ValueError("lml_mean_batch: no basis for this data: call set_basis after set_data")
        lml = np.empty(n)
        g = np.empty(th.shape) if grad else None
        q = np.empty(n) if want_q else None
        beta = np.empty((n, self.m)) if want_beta else None
        status = np.zeros(n, dtype=np.int32)
        bad = ctypes.c_int(-1)
        rc = self.lib.gpf_lml_mean_batch(self._h, _ptr(th), n, _ptr(lml), _ptr(g) if grad else None,
                                         _ptr(beta) if want_beta else None, _ptr(q) if want_q else None,
                                         status.ctypes.data_as(_ip), ctypes.byref(bad))
        if rc != GPF_NOT_PD or strict:
            self._check(rc, "gpf_lml_mean_batch", bad)
        out = (lml, g)
        if want_q:
            out += (q,)
        if want_beta:
            out += (beta,)
        return out

    def predict_mean(self, lengths, x_fit, h_fit, batch_size=10000, want_beta=False):
        """predict with the mean function of set_basis (gpf_predict_mean, the unit model a = s = 1):
        (mu (M,), sd (M,)) at x_fit (d, M) with h_fit (m, M) the basis there; sd includes the share of
        not knowing the coefficients. With want_beta also (beta (m,), cov(beta) (m, m))."""
        ls, xf = self._lengths_and_queries(lengths, x_fit)
        hf = _f64(h_fit)
        if self.N and not self.m:
            raise ValueError("predict_mean: no basis for this data: call set_basis after set_data")
        if hf.ndim == 1:
            hf = hf.reshape(1, -1)
        mq = xf.shape[1]
        if hf.ndim != 2 or hf.shape != (self.m, mq):
            raise ValueError(f"h_fit must be ({self.m}, {mq}): the basis at the query points")
        if not np.all(np.isfinite(hf)):
            raise ValueError("predict_mean: h_fit must be finite")
        mu, sd = np.empty(mq), np.empty(mq)
        beta = np.empty(self.m) if want_beta else None
        bcov = np.empty((self.m, self.m)) if want_beta else None
        self._check(self.lib.gpf_predict_mean(self._h, _ptr(ls), _ptr(xf), _ptr(hf), mq, int(batch_size), _ptr(mu),
                                              _ptr(sd), _ptr(beta) if want_beta else None,
                                              _ptr(bcov) if want_beta else None), "gpf_predict_mean")
        return (mu, sd, beta, bcov) if want_beta else (mu, sd)

    def loo_batch(self, positions, grad=True, points=False, strict=True):
        """Leave-one-out log predictive density of every row of positions (P, d) and, with grad, its
        gradient in the length scales (gpf_loo_batch): (lpd (P,), grad (P, d) or None), and with
        points also (mu (P, N), sd (P, N)), every training point's prediction from the other N - 1
        (the sd of the measured value: e_i^2 included). Needs set_data only. A particle whose
        covariance is not positive definite raises LinAlgError with .particle set to its row
        (strict), or gets lpd = -inf and NaN gradient, mu and sd rows while the other rows are
        computed (strict=False)."""
        P = _f64(positions)
        if P.ndim == 1:
            P = P.reshape(1, -1)
        n = P.shape[0]
        if self.d and P.shape[1] != self.d:
            raise ValueError(f"positions must be (P, {self.d})")
        lpd = np.empty(n)
        g = np.empty((n, P.shape[1])) if grad else None
        mu = np.empty((n, self.N)) if points else None
        sd = np.empty((n, self.N)) if points else None
        status = np.zeros(n, dtype=np.int32)
        bad = ctypes.c_int(-1)
        rc = self.lib.gpf_loo_batch(self._h, _ptr(P), n, _ptr(lpd), _ptr(g) if grad else None,
                                    _ptr(mu) if points else None, _ptr(sd) if points else None,
                                    status.ctypes.data_as(_ip), ctypes.byref(bad))
        if rc != GPF_NOT_PD or strict:
            self._check(rc, "gpf_loo_batch", bad)
        return (lpd, g, mu, sd) if points else (lpd, g)

    def predict_batch(self, positions, x_fit, weights=None, chunk=0, want_each=False):
        """predict() at every row of positions (P, d) in one batched call, and the mixture of the P
        predictions with the weights (P,) (None: equal; normalised to sum 1) by the law of total
        variance (gpf_predict_batch): (mix_mu (M,), mix_sd (M,), info). With want_each, info["mu"] and
        info["sd"] are the particles' own (P, M) predictions. ``chunk``: query points per pass (rounded
        up to 128; 0: the library's default); it does not change the bits. P = 1 is bitwise predict().
        LinAlgError with .particle set to the first row whose covariance is not positive definite,
        ValueError for bad arguments, P = 0 among them (the C call writes nothing then)."""
        P, xf = _f64(positions), _f64(x_fit)
        if P.ndim == 1:
            P = P.reshape(1, -1)
        if P.ndim != 2 or xf.ndim != 2:
            raise ValueError("positions must be (P, d) and x_fit (d, M)")
        if P.shape[1] != xf.shape[0] or (self.d and xf.shape[0] != self.d):
            raise ValueError(f"positions must be (P, {self.d or xf.shape[0]}) and x_fit ({self.d or xf.shape[0]}, M)")
        n, m = P.shape[0], xf.shape[1]
        if n == 0:
            raise ValueError("positions is empty: a mixture needs at least one particle")
        w = None
        if weights is not None:
            w = _f64(weights).reshape(-1)
            if w.shape != (n,):
                raise ValueError(f"weights must be ({n},)")
        if int(chunk) < 0:
            raise ValueError("chunk must be >= 0")
        mix_mu, mix_sd = np.empty(m), np.empty(m)
        mu = np.empty((n, m)) if want_each else None
        sd = np.empty((n, m)) if want_each else None
        bad = ctypes.c_int(-1)
        rc = self.lib.gpf_predict_batch(self._h, _ptr(P), n, _ptr(w) if w is not None else None, _ptr(xf), m, int(chunk),
                                        _ptr(mix_mu), _ptr(mix_sd), _ptr(mu) if want_each else None,
                                        _ptr(sd) if want_each else None, ctypes.byref(bad))
        self._check(rc, "gpf_predict_batch", bad)
        info = {"particles": n}
        if want_each:
            info.update(mu=mu, sd=sd)
        return mix_mu, mix_sd, info

    # -- measurement hooks --
    def set_profiling(self, on=True):
        self._check(self.lib.gpf_set_profiling(self._h, int(bool(on))), "gpf_set_profiling")

    def reset_profile(self):
        self._check(self.lib.gpf_reset_profile(self._h), "gpf_reset_profile")

    def profile(self):
        buf = np.zeros(27)
        self.lib.gpf_get_profile(self._h, _ptr(buf), 27)
        keys = ["panel_ms", "panel_launches", "panel_flops", "diag_ms", "diag_launches", "diag_flops",
                "build_ms", "build_launches", "build_bytes", "loss_ms", "loss_launches", "evals",
                "factor_wall_ms", "factor_calls", "factor_flops", "predict_ms", "predict_launches",
                "predict_flops", "predict_cov_ms", "predict_cov_launches", "predict_cov_bytes",
                "psurf_ms", "psurf_launches", "psurf_bytes", "factor_sclk_mhz", "cus", "fp64_ceiling_at_sclk_tflops"]
        return dict(zip(keys, buf.tolist()))

    def debug_factor(self, lengths):
        """(L, U, z, alpha) of one particle: Npad x Npad factor and inverse (diagnostic)."""
        ls = _f64(lengths).reshape(-1)
        self._check_lengths(ls)
        t = self.lib.gpf_tile()
        npad = -(-self.N // t) * t
        L, U = np.empty((npad, npad)), np.empty((npad, npad))
        z, al = np.empty(npad), np.empty(self.N)
        rc = self.lib.gpf_debug_factor(self._h, _ptr(ls), _ptr(L), _ptr(U), _ptr(z), _ptr(al))
        if rc not in (GPF_OK, GPF_NOT_PD):
            self._check(rc, "gpf_debug_factor")
        return L, U, z, al

    def debug_factor128(self, a, y):
        """factor128 on n 128x128 blocks a[n,128,128] with right-hand sides y[n,128] (diagnostic):
        dict of L, U, z, s2, sz, bad, cycles (shader cycles per block)."""
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 128, 128)
        n = a.shape[0]
        y = np.ascontiguousarray(y, dtype=np.float64).reshape(n, 128)
        L, U = np.empty_like(a), np.empty_like(a)
        z, s2, sz, cyc = np.empty((n, 128)), np.empty((n, 128)), np.empty((n, 128)), np.empty(n)
        bad = np.zeros(n, dtype=np.int32)
        self._check(self.lib.gpf_debug_factor128(self._h, _ptr(a), _ptr(y), n, _ptr(L), _ptr(U), _ptr(z), _ptr(s2),
                                                 _ptr(sz), bad.ctypes.data_as(_ip), _ptr(cyc)), "gpf_debug_factor128")
        return {"L": L, "U": U, "z": z, "s2": s2, "sz": sz, "bad": bad, "cycles": cyc}

    def mfma_peak(self, blocks=1024, iters=4096):
        out = ctypes.c_double(0.0)
        self._check(self.lib.gpf_mfma_peak(self._h, int(blocks), int(iters), ctypes.byref(out)), "gpf_mfma_peak")
        return out.value

    def bench_clock(self):
        """Shader clock (MHz) the last mfma_peak / gemm_bench held (gpf_bench_clock)."""
        out = ctypes.c_double(0.0)
        self._check(self.lib.gpf_bench_clock(self._h, ctypes.byref(out)), "gpf_bench_clock")
        return out.value

    def kmeans_set(self, X):
        """Keep the (n, d) centred points on the device for kmeans_step (gpf_kmeans_set)."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise ValueError("X must be (n, d)")
        self._check(self.lib.gpf_kmeans_set(self._h, _ptr(X), X.shape[0], X.shape[1]), "gpf_kmeans_set")
        self._km_n, self._km_d = X.shape

    def kmeans_step(self, centers, update=True, want_dist=False):
        """One Lloyd E-step (+ M-step sums) against centers (k, d) (gpf_kmeans_step):
        (labels, sums, counts, dist or None)."""
        C = np.ascontiguousarray(centers, dtype=np.float64)
        # gpf_kmeans_step reads k x d doubles with the d of kmeans_set
        if C.ndim != 2 or C.shape[1] != self._km_d:
            raise ValueError(f"centers must be (k, {self._km_d})")
        k, d = C.shape
        labels = np.empty(self._km_n, dtype=np.int32)
        sums = np.empty((k, d)) if update else None
        counts = np.empty(k) if update else None
        dist = np.empty(self._km_n) if want_dist else None
        nul = ctypes.POINTER(ctypes.c_double)()
        self._check(self.lib.gpf_kmeans_step(self._h, _ptr(C), k, int(bool(update)),
                                             labels.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                             _ptr(sums) if update else nul, _ptr(counts) if update else nul,
                                             _ptr(dist) if want_dist else nul), "gpf_kmeans_step")
        return labels, sums, counts, dist

    def prob_surface(self, tails):
        """(y (M,100), p (M,100), ok (M,) bool) for each row of tail entries (gpf_prob_surface)."""
        t = _f64(tails)
        if t.ndim != 2:
            raise ValueError("tails must be (M, E)")
        m, e = t.shape
        y, p = np.empty((m, 100)), np.empty((m, 100))
        ok = np.empty(m, dtype=np.int32)
        self._check(self.lib.gpf_prob_surface(self._h, _ptr(t), m, e, _ptr(y), _ptr(p),
                                              ok.ctypes.data_as(ctypes.POINTER(ctypes.c_int))), "gpf_prob_surface")
        return y, p, ok.astype(bool)

    def hull_fill(self, shell_rows, res, decimals):
        """The d sort + scan-fill passes of fill_convex_hull on the GPU (gpf_hull_fill): rows
        (m, d) sorted lexicographically."""
        rows = _f64(shell_rows)
        n, d = rows.shape
        r = _f64(res).reshape(-1)
        dec = np.ascontiguousarray(decimals, dtype=np.int32).reshape(-1)
        if r.shape[0] != d or dec.shape[0] != d:
            raise ValueError("res and decimals need one entry per dimension")
        m = ctypes.c_int64(0)
        self._check(self.lib.gpf_hull_fill(self._h, _ptr(rows), n, d, _ptr(r),
                                           dec.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ctypes.byref(m)),
                    "gpf_hull_fill")
        out = np.empty((m.value, d))
        self._check(self.lib.gpf_hull_fetch(self._h, _ptr(out)), "gpf_hull_fetch")
        return out

    def gemm_bench(self, mode=0, npad=4096, particles=64, tiles=15, depth=2048, iters=5):
        """TF/s of the block-column GEMM core alone (gpf_gemm_bench)."""
        out = ctypes.c_double(0.0)
        self._check(self.lib.gpf_gemm_bench(self._h, int(mode), int(npad), int(particles), int(tiles), int(depth),
                                            int(iters), ctypes.byref(out)), "gpf_gemm_bench")
        return out.value

    def selftest_mfma(self, a, b):
        a, b = _f64(a), _f64(b)
        c = np.empty((16, 16))
        self._check(self.lib.gpf_selftest_mfma(self._h, _ptr(a), _ptr(b), _ptr(c)), "gpf_selftest_mfma")
        return c


class Comm:
    """Rank `rank` of `nranks` in a swarm-exchange group (gpf_comm, include/gpfit.h).

    transport "rccl": ncclAllReduce on `ctx`'s GPU (one process per GPU); "host": the same
    exchange over the TCP rendezvous sockets (no device; CPU tests and tools).
    """

    def __init__(self, rank, nranks, host="127.0.0.1", port=29600, transport="rccl", ctx=None):
        self.lib = load_library()
        kind = {"rccl": GPF_COMM_RCCL, "host": GPF_COMM_HOST}[transport]
        if kind == GPF_COMM_RCCL and ctx is None:
            raise ValueError("the rccl transport needs the rank's Context")
        h = _vp()
        rc = self.lib.gpf_comm_open(ctx._h if ctx is not None else None, int(rank), int(nranks), host.encode(),
                                    int(port), kind, ctypes.byref(h))
        if rc != GPF_OK or not h.value:
            why = ctx.lib.gpf_last_error(ctx._h).decode(errors="replace") if ctx is not None else ""
            raise GPFitError(f"gpf_comm_open(rank={rank}, nranks={nranks}, {host}:{port}, {transport}) failed "
                             f"(rc={rc}) {why}")
        self.handle = h
        self.rank, self.size, self.transport = int(rank), int(nranks), transport

    @classmethod
    def from_env(cls, ctx=None, transport=None):
        """torchrun-style environment: RANK, WORLD_SIZE, MASTER_ADDR; the rendezvous port is
        GPF_COMM_PORT, else MASTER_PORT + 1 (MASTER_PORT itself is the launcher's store)."""
        rank = int(os.environ.get("RANK", "0"))
        world = int(os.environ.get("WORLD_SIZE", "1"))
        host = os.environ.get("MASTER_ADDR", "127.0.0.1")
        port = int(os.environ.get("GPF_COMM_PORT", int(os.environ.get("MASTER_PORT", "29599")) + 1))
        transport = transport or os.environ.get("GPF_COMM_TRANSPORT", "rccl" if ctx is not None else "host")
        return cls(rank, world, host, port, transport, ctx)

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self.lib.gpf_comm_close(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self):
        return self.lib.gpf_comm_last_error(self.handle).decode(errors="replace")

    def allreduce(self, values, op="sum"):
        buf = np.array(values, dtype=np.float64, copy=True).reshape(-1)
        rc = self.lib.gpf_comm_allreduce(self.handle, _ptr(buf), buf.shape[0],
                                         {"sum": GPF_OP_SUM, "max": GPF_OP_MAX}[op])
        if rc != GPF_OK:
            raise GPFitError(f"gpf_comm_allreduce: {self._err()}")
        return buf

    def barrier(self):
        self.allreduce(np.zeros(1))

    def stats(self):
        """(ms, count): cumulative wall time this rank spent in the score exchange
        (gpf_comm_exchange_scores: the all-reduce, including the wait for the slowest rank)."""
        ms = ctypes.c_double(0.0)
        n = ctypes.c_longlong(0)
        if self.lib.gpf_comm_stats(self.handle, ctypes.byref(ms), ctypes.byref(n)) != GPF_OK:
            raise GPFitError("gpf_comm_stats failed")
        return ms.value, n.value

    def rows(self, P):
        """This rank's contiguous rows [rP/G, (r+1)P/G) of a P-particle swarm."""
        return self.rank * P // self.size, (self.rank + 1) * P // self.size

    def exchange_scores(self, P, local, local_rc=GPF_OK, local_bad=-1):
        """gpf_comm_exchange_scores: this rank's scores of its rows -> the full (P,) vector on
        every rank; a non-PD particle on any rank raises LinAlgError on every rank."""
        loss = np.empty(P)
        loc = _f64(local) if local is not None else np.zeros(0)
        bad = ctypes.c_int(-1)
        rc = self.lib.gpf_comm_exchange_scores(self.handle, int(P), _ptr(loc), int(local_rc), int(local_bad),
                                               _ptr(loss), ctypes.byref(bad))
        if rc == GPF_NOT_PD:
            err = np.linalg.LinAlgError("Matrix is not positive definite")
            err.bad_index = bad.value  # the smallest failing row of the whole swarm
            raise err
        if rc == GPF_BAD_ARG:
            raise ValueError(f"gpf_comm_exchange_scores: {self._err()}")
        if rc != GPF_OK:
            raise GPFitError(f"gpf_comm_exchange_scores: {self._err()}")
        return loss


_DEFAULT = {}
_COMM = {}


def default_comm(ctx=None):
    """The process-wide swarm-exchange group when the launcher started several ranks
    (WORLD_SIZE > 1 in the environment), else None. Created on first use: RCCL on this
    process's GPU context, or the host transport when no context is given."""
    if int(os.environ.get("WORLD_SIZE", "1")) <= 1:
        return None
    key = "ctx" if ctx is not None else "host"
    if key not in _COMM:
        _COMM[key] = Comm.from_env(ctx)
    return _COMM[key]


def default_context():
    """Process-wide context on this process's GPU (created on first use)."""
    dev = default_device()
    ctx = _DEFAULT.get(dev)
    if ctx is None:
        ctx = Context(dev)
        _DEFAULT[dev] = ctx
    return ctx
