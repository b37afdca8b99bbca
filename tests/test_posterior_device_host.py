"""The device posterior-draw path's host side (gpf_chol_dense / gpf_posterior_draws declarations, the
Python-side validation, method= of sample_posterior): no GPU."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from test_posterior_host import _closed_form

ROOT = Path(__file__).resolve().parent.parent
NEW = {"gpf_chol_dense": 8, "gpf_posterior_draws": 13}


def _header_args(name):
    hdr = (ROOT / "include" / "gpfit.h").read_text()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/gpfit.h"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(NEW))
def test_entry_points_declared_with_matching_argument_counts(name):
    import gpfit._lib as L
    assert name in L.SIGNATURES
    res, args = L.SIGNATURES[name]
    hargs = _header_args(name)
    assert len(args) == len(hargs) == NEW[name]
    # pointer / integer kinds agree position by position
    for a, h in zip(args, hargs):
        assert ("*" in h) == (a not in (ctypes.c_int, ctypes.c_int64)), (name, h, a)
    assert L.ABI_VERSION == 2 and "#define GPF_ABI_VERSION 2" in (ROOT / "include" / "gpfit.h").read_text()
    assert hasattr(L.load_library(), name)


def test_null_context_is_bad_arg_without_a_device():
    import gpfit._lib as L
    lib = L.load_library()
    assert lib.gpf_chol_dense(None, None, 0, None, 0, None, None, None) == L.GPF_BAD_ARG
    assert lib.gpf_posterior_draws(None, None, None, 0, None, 0, None, 0, None, None, None, None, None) == L.GPF_BAD_ARG


@pytest.mark.parametrize("bad", [(), (-1e-12, 1e-10), (1e-10, 1e-12), (1e-12, 1e-12), (1e-12, float("nan")),
                                 (1e-12, float("inf"))])
def test_ladder_validation(bad):
    import gpfit._lib as L
    from gpfit.posterior import sample_posterior
    with pytest.raises(ValueError, match="jitters"):
        L.check_jitters(bad)
    x = np.random.default_rng(0).uniform(size=(2, 10))
    with pytest.raises(ValueError, match="jitters"):  # before any context is opened
        sample_posterior(x, np.zeros(10), np.full(10, 0.1), x[:, :4], [0.3, 0.3], 2, method="device", jitters=bad)
    with pytest.raises(ValueError, match="jitters"):
        L.check_draw_args(2, [0.3, 0.3], x[:, :4], np.zeros((2, 4)), bad)


def test_ladder_accepts_the_default_and_zero():
    import gpfit._lib as L
    from gpfit import posterior
    assert posterior.JITTERS == (1e-12, 1e-10, 1e-8, 1e-6) and posterior.JITTERS is L.JITTERS
    np.testing.assert_array_equal(L.check_jitters(L.JITTERS), np.array(L.JITTERS))
    np.testing.assert_array_equal(L.check_jitters((0.0,)), [0.0])
    np.testing.assert_array_equal(L.check_jitters(1e-9), [1e-9])


def test_z_shape_validation():
    import gpfit._lib as L
    q = np.zeros((2, 5))
    for z in (np.zeros((3, 4)), np.zeros(5), np.zeros((3, 5, 1))):
        with pytest.raises(ValueError, match=r"z must be \(S, 5\)"):
            L.check_draw_args(2, [0.3, 0.3], q, z, L.JITTERS)
    with pytest.raises(ValueError, match="x_fit"):
        L.check_draw_args(3, [0.3, 0.3], q, np.zeros((3, 5)), L.JITTERS)
    with pytest.raises(ValueError, match="x_fit"):
        L.check_draw_args(2, [0.3], q, np.zeros((3, 5)), L.JITTERS)
    ls, xf, z, j = L.check_draw_args(2, [0.3, 0.4], q, np.zeros((3, 5), dtype=np.float32), L.JITTERS)
    assert ls.shape == (2,) and xf.shape == (2, 5) and z.shape == (3, 5) and z.dtype == np.float64 and j.shape == (4,)


def test_unknown_method_and_injected_evaluator():
    from gpfit.posterior import sample_posterior
    mu, cov, (x, y, e, q, l) = _closed_form(30, 2, 12)
    with pytest.raises(ValueError, match="method"):
        sample_posterior(x, y, e, q, l, 2, method="gpu")
    with pytest.raises(ValueError, match="mean_and_cov"):
        sample_posterior(x, y, e, q, l, 2, method="device", mean_and_cov=lambda xf, ls: (mu, cov))
    with pytest.raises(ValueError, match="x_fit"):
        sample_posterior(x, y, e, q[:1], l, 2, method="device")


def test_host_method_is_unchanged():
    """method="host" (explicit or by default) with an injected evaluator returns what it returned
    before the device path existed: draws_from on the evaluator's (mu, cov) with default_rng(seed)."""
    from gpfit.posterior import draws_from, sample_posterior
    mu, cov, (x, y, e, q, l) = _closed_form(40, 2, 25, dup=True)
    ev = lambda xf, ls: (mu, cov)
    want, winfo = draws_from(mu, cov, n_draws=3, seed=9)
    for kw in ({}, {"method": "host"}):
        got, info = sample_posterior(None, None, None, q, l, 3, seed=9, mean_and_cov=ev, **kw)
        np.testing.assert_array_equal(got, want)
        assert sorted(info) == ["cov", "jitter", "mu", "tries"]
        assert info["jitter"] == winfo["jitter"] and info["tries"] == winfo["tries"]
        assert info["mu"] is mu and info["cov"] is cov


def test_gp_draws_passes_method_through():
    import inspect
    import GP_func
    sig = inspect.signature(GP_func.GP_draws)
    assert sig.parameters["method"].default == "host"
    x = np.random.default_rng(0).uniform(size=(2, 10))
    with pytest.raises(ValueError, match="method"):
        GP_func.GP_draws(x, np.zeros(10), np.full(10, 0.1), x[:, :4], [0.3, 0.3], 2, method="nowhere")
