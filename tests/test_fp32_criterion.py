"""The entry-wise single-precision criterion of tests/parity_util.py (fp32_errors, assert_fp32_parity) and the norm-scaled one
it is used with, on synthetic arrays: no GPU needed."""
import numpy as np
import pytest

import parity_util as pu


def _case(seed=0, n=3):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n, 44, 44))
    h = -(a @ a.transpose(0, 2, 1)) - 44 * np.eye(44)     # negative definite, like an ELBO Hessian near its optimum
    d = rng.normal(size=(n, 44)) * 10
    v = rng.normal(size=n) * 1e4
    return v, d, h


def _noisy(v, d, h, rel=1e-7, seed=1):
    rng = np.random.default_rng(seed)
    v2 = v * (1 + rel * rng.normal(size=v.shape))
    d2 = d + rel * np.abs(d) * rng.normal(size=d.shape)
    e = rel * rng.normal(size=h.shape) * np.abs(h)
    return v2, d2, h + (e + e.transpose(0, 2, 1)) / 2


def test_a_small_error_passes_and_the_worst_ratios_are_returned():
    v, d, h = _case()
    w = pu.assert_fp32_parity(_noisy(v, d, h), (v, d, h), h, "small")
    assert 0 < w["v"] <= pu.FP32_T_V and 0 < w["d"] <= pu.FP32_T_D and 0 < w["h"] <= pu.FP32_T_H


@pytest.mark.parametrize("where", ["v", "d", "h"])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_entry_fails(where, bad):
    v, d, h = _case()
    v2, d2, h2 = (x.copy() for x in (v, d, h))
    {"v": lambda: v2.__setitem__(1, bad), "d": lambda: d2.__setitem__((0, 5), bad),
     "h": lambda: h2.__setitem__((0, 3, 3), bad)}[where]()
    e = pu.fp32_errors((v2, d2, h2), (v, d, h), h)
    assert np.isinf(e[where]).any() and not np.isnan(e[where]).any()
    with pytest.raises(AssertionError):
        pu.assert_fp32_parity((v2, d2, h2), (v, d, h), h, "non-finite")
    # the norm-scaled criterion does not step over it either
    assert np.isinf(pu.norm_scaled_fp32_errors((v2, d2, h2), (v, d, h))[where])


def test_exact_zero_rule():
    """where the reference and its scale are exactly 0 (the k block without KL: d = 0 and h = 0), only an exact 0 passes"""
    v, d, h = _case()
    d[:, 28:] = 0.0
    h[:, 28:, :] = 0.0
    h[:, :, 28:] = 0.0
    pu.assert_fp32_parity((v, d.copy(), h.copy()), (v, d, h), h, "zeros kept")
    for t, i in ((0, 30), (2, 43)):
        d2 = d.copy()
        d2[t, i] = 1e-300
        with pytest.raises(AssertionError, match=_names()[i]):
            pu.assert_fp32_parity((v, d2, h), (v, d, h), h, "tiny gradient in the k block")
        h2 = h.copy()
        h2[t, i, 3] = h2[t, 3, i] = -1e-300
        with pytest.raises(AssertionError, match="target %d" % t):
            pu.assert_fp32_parity((v, d, h2), (v, d, h), h, "tiny Hessian entry in the k block")


def _names():
    from celeste_jl_amd.params import ids_names
    return ids_names()


def test_the_failure_names_target_and_parameters():
    v, d, h = _case()
    h2 = h.copy()
    h2[1, 4, 12] *= 1.5
    h2[1, 12, 4] *= 1.5
    with pytest.raises(AssertionError) as ex:
        pu.assert_fp32_parity((v, d, h2), (v, d, h), h, "named")
    msg = str(ex.value)
    assert "target 1" in msg and ("gal_angle x color_mean_3_1" in msg or "color_mean_3_1 x gal_angle" in msg), msg


def test_ratios_do_not_change_when_one_parameter_is_rescaled():
    """x_i = c y_i: d_y = D d_x and h_y = D h_x D with D = diag(1, .., c, .., 1) -- for the result, the reference and the
    Hessian the scales come from alike; every ratio stays the same"""
    v, d, h = _case(3)
    g = _noisy(v, d, h, rel=3e-5, seed=4)
    e0 = pu.fp32_errors(g, (v, d, h), h)
    for i, c in ((5, 1e3), (12, 1e-4), (0, -7.0)):
        D = np.ones(44)
        D[i] = c
        tr = lambda dd, hh: (dd * D, hh * D[:, None] * D[None, :])   # noqa: E731
        gd, gh = tr(g[1], g[2])
        rd, rh = tr(d, h)
        e1 = pu.fp32_errors((g[0], gd, gh), (v, rd, rh), rh)
        np.testing.assert_allclose(e1["d"], e0["d"], rtol=1e-9, atol=0)
        np.testing.assert_allclose(e1["h"], e0["h"], rtol=1e-9, atol=0)
    # the norm-scaled criterion is not invariant: that is the point of the entry-wise one
    D = np.ones(44)
    D[5] = 1e3
    n0 = pu.norm_scaled_fp32_errors(g, (v, d, h))
    n1 = pu.norm_scaled_fp32_errors((g[0], g[1] * D, g[2] * D[:, None] * D), (v, d * D, h * D[:, None] * D))
    assert n1["h"] != pytest.approx(n0["h"], rel=1e-3)


def test_gradient_floor_is_a_fraction_of_the_posterior_standard_deviation():
    """|dd_i| <= T_d max(|d_i|, F sqrt|h_ii|): at a stationary point (d_i = 0) an error of T_d F sqrt|h_ii| passes, twice that
    fails"""
    v, d, h = _case(5)
    d[0, 7] = 0.0
    for k, ok in ((0.99, True), (2.0, False)):
        d2 = d.copy()
        d2[0, 7] = k * pu.FP32_T_D * pu.FP32_F * np.sqrt(abs(h[0, 7, 7]))
        if ok:
            pu.assert_fp32_parity((v, d2, h), (v, d, h), h)
        else:
            with pytest.raises(AssertionError, match="flux_loc_2"):
                pu.assert_fp32_parity((v, d2, h), (v, d, h), h)


def test_gradient_only_results_take_their_scales_from_the_hessian_given():
    v, d, h = _case(6)
    d2 = d.copy()
    d2[2, 20] += 10 * pu.FP32_T_D * max(abs(d[2, 20]), pu.FP32_F * np.sqrt(abs(h[2, 20, 20])))
    e = pu.fp32_errors((v, d2, None), (v, d, None), h)
    assert e["h"] is None and e["d"][2, 20] == pytest.approx(10 * pu.FP32_T_D, rel=1e-9)
    with pytest.raises(AssertionError, match="color_var_3_1"):
        pu.assert_fp32_parity((v, d2, None), (v, d, None), h)
