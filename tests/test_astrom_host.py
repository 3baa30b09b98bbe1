"""libceleste_astrom.so without a GPU: its C ABI (header, exports, Python binding), the refusals that come back before any
device is touched, the untouched defaults of infer_box and celeste_to_rows, and the numpy / torch restatement of the astrometry
(tests/astrom_reference.py) held to properties that do not depend on it: its derivatives against central differences, a
noise-free displaced source recovered by its root, the gate's independence of the pixels, the coverage of its estimates over
Poisson draws, and the summaries on hand-made entries."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _protos():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "celeste_astrom.h")).read(), flags=re.S)
    return {n: (0 if a.strip() in ("", "void") else len(a.split(","))) for n, a in
            re.findall(r"\b(celeste_astrom_\w+)\s*\(([^)]*)\)\s*;", hdr)}


def test_the_astrom_library_exports_its_c_abi_and_nothing_else(lib):
    import ctypes as C
    from celeste_jl_amd import astrom
    protos = _protos()
    assert set(protos) == set(astrom.EXPORTED_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", astrom.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip()) == sorted(astrom.EXPORTED_SYMBOLS)
    emap = open(os.path.join(ROOT, "celeste.jl_amd", "csrc", "astrom", "exports.map")).read()
    assert re.search(r"global:\s*celeste_astrom_\*;\s*local:\s*\*;", emap)
    f = astrom.load_library()
    for name, n_args in protos.items():                       # the ctypes signatures
        at = getattr(f, name).argtypes
        assert (0 if at is None else len(at)) == n_args, name
    assert f.celeste_astrom_version() == astrom.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "celeste_astrom.h")).read()
    assert "#define CELESTE_ASTROM_ABI_VERSION %d" % astrom.ABI_VERSION in hdr
    assert "#define CELESTE_ASTROM_NSUMMARY %d" % astrom.NSUMMARY in hdr
    assert "#define CELESTE_ASTROM_MAX_STEP_PX %r" % astrom.MAX_STEP_PX in hdr
    assert "#define CELESTE_ASTROM_LS_MIN_DEC 1e-3" in hdr and astrom.LS_MIN_DEC == 1e-3
    assert "#define CELESTE_ASTROM_MAX_HALVINGS %d" % astrom.MAX_HALVINGS in hdr
    flags, sflags, slots = re.findall(r"enum \{(.*?)\};", hdr, re.S)
    assert [int(v) for v in re.findall(r"=\s*(\d+)", flags)] == list(range(7)) == [
        astrom.OK, astrom.NO_LIGHT, astrom.TOO_FAINT, astrom.OUT_OF_RANGE, astrom.STALLED, astrom.NOT_CONVERGED, astrom.BAD_MODEL]
    assert [n.strip() for n in re.findall(r"CELESTE_ASTROM_(\w+)\s*=", flags)] == list(astrom.FLAG_NAMES)
    assert [int(v) for v in re.findall(r"=\s*(\d+)", sflags)] == [astrom.NO_EPOCHS, astrom.NO_MOTION]
    assert [int(v) for v in re.findall(r"=\s*(\d+)", slots)] == [astrom.MEAN, astrom.MEAN_COV, astrom.CHI2_CONST, astrom.MOTION,
                                                                 astrom.MOTION_COV, astrom.CHI2_LIN, astrom.T_REF]
    assert astrom.T_REF + 1 == astrom.NSUMMARY
    assert C.sizeof(astrom.ParamsT) == 32 and astrom.ParamsT.max_iters.offset == 24
    assert b"no CPU fallback" in f.celeste_astrom_strerror(5)
    import astrom_reference as AR                                 # the restatement's constants are the header's
    assert (AR.MAX_STEP_PX, AR.LS_MIN_DEC, AR.MAX_HALVINGS) == (astrom.MAX_STEP_PX, astrom.LS_MIN_DEC, astrom.MAX_HALVINGS)


def _call_args(params=None, ctx=None, n=1, epochs=None):
    """a full argument list over arrays filled with -7, and those arrays"""
    import ctypes as C
    from celeste_jl_amd import astrom, cabi
    dp, ip, lp = cabi.c_double_p, cabi.c_int32_p, cabi.c_int64_p
    vp = np.zeros((2, 44))
    tg = np.zeros(1, dtype=np.int32)
    i32 = [np.full(8, -7, dtype=np.int32) for _ in range(7)]           # image, n_pix, iters, flag, n_epochs, summary_flag, status
    f64 = [np.full(64, -7.0) for _ in range(7)]                        # delta, alpha, fisher, cov, chi2, loglik, summary
    off = np.full(2, -7, dtype=np.int64)
    p = astrom._ptr
    args = [ctx, p(vp, dp), n, p(tg, ip), None if params is None else C.byref(params), p(epochs, dp), p(off, lp), p(i32[0], ip),
            p(f64[0], dp), p(f64[1], dp), p(f64[2], dp), p(f64[3], dp), p(f64[4], dp), p(f64[5], dp), p(i32[1], ip), p(i32[2], ip),
            p(i32[3], ip), p(i32[4], ip), p(i32[5], ip), p(f64[6], dp), p(i32[6], ip)]
    return args, [vp, tg, off] + i32 + f64


BAD_PARAMS = [(0.0, 0.2, 2.0, 50), (np.nan, 0.2, 2.0, 50), (1e-6, 0.0, 2.0, 50), (1e-6, np.inf, 2.0, 50), (1e-6, 0.2, -1.0, 50),
              (1e-6, 0.2, np.nan, 50), (1e-6, 0.2, 2.0, 0)]


def test_refusals_come_back_before_any_device_is_touched(lib):
    """invalid arguments are INVALID_ARG, not NO_DEVICE or a HIP error, also on a machine without a device: nothing of HIP
    has been called when they return, and nothing has been written"""
    import ctypes as C
    from celeste_jl_amd import astrom, cabi
    f = astrom.load_library()
    keep = []
    cases = [dict(), dict(n=-1), dict(n=0)] + [dict(params=astrom.ParamsT(*p, 0)) for p in BAD_PARAMS]
    for kw in cases:
        args, arrays = _call_args(**kw)                               # no context
        keep.append(arrays)
        assert f.celeste_astrom_offsets(*args) == cabi.ERR_INVALID_ARG, kw
    for arrays in keep:
        assert all((a == -7).all() for a in arrays[2:])
    assert f.celeste_astrom_last_ms(None, (C.c_float * 4)()) == cabi.ERR_INVALID_ARG
    assert f.celeste_astrom_ctx_create(None, 0, None) == cabi.ERR_INVALID_ARG
    h = C.c_void_p(1234)
    assert f.celeste_astrom_ctx_create(None, 0, C.byref(h)) == cabi.ERR_INVALID_ARG and not h.value
    f.celeste_astrom_ctx_destroy(None)


def test_no_device_no_fallback(lib):
    """without a device the context refuses with NO_DEVICE (there is no CPU path); on a GPU machine it is created"""
    import torch
    from celeste_jl_amd import astrom, cabi, synthetic
    f = synthetic.make_sample_dataset("two_body", seed=1)
    pr = cabi.Problem(f.images, f.patches, f.neighbors)
    if torch.cuda.is_available():
        astrom.AstromContext(pr).close()
    else:
        with pytest.raises(RuntimeError, match="no HIP device") as e:
            astrom.AstromContext(pr)
        assert "status %d" % cabi.ERR_NO_DEVICE in str(e.value)


def test_the_defaults_do_not_import_astrom_and_return_what_they_returned():
    """infer_box and celeste_to_rows with their defaults: the module is not loaded, the rows are the rows"""
    code = r"""
import sys, inspect
import numpy as np
import celeste_jl_amd as cel
from celeste_jl_amd import catalog, infer, synthetic
assert inspect.signature(cel.infer_box).parameters["astrometry"].default is False
assert inspect.signature(cel.infer_box).parameters["epochs"].default is None
assert inspect.signature(catalog.celeste_to_rows).parameters["astrometry"].default is False
f = synthetic.make_sample_dataset("two_body", seed=1)
assert cel.infer_box(f.images, cel.BoundingBox(-9.0, -8.0, -9.0, -8.0), f.catalog) == []          # no target in the box
assert cel.infer_box(f.images, cel.BoundingBox(-9.0, -8.0, -9.0, -8.0), f.catalog, astrometry=True) == []
res = [cel.OptimizedSource(1.0, 2.0, f.vp[0].copy(), False), cel.OptimizedSource(3.0, 4.0, f.vp[1].copy(), True)]
assert res[0].astrometry is None
rows = catalog.celeste_to_rows(res)
assert rows == [catalog.variational_parameters_to_row(f.vp[0])]
assert not set(catalog.ASTROMETRY_COLUMNS) & set(rows[0])
assert catalog.ASTROMETRY_COLUMNS == ("n_epochs_astrom", "pm_ra", "pm_dec", "pm_ra_stderr", "pm_dec_stderr", "astrom_chi2_const",
                                      "astrom_chi2_lin")
assert "celeste_jl_amd.astrom" not in sys.modules
d = catalog.celeste_to_rows(res, astrometry=True)
assert len(d) == 1 and all(d[0][k] is None for k in catalog.ASTROMETRY_COLUMNS)
assert {k: v for k, v in d[0].items() if k not in catalog.ASTROMETRY_COLUMNS} == rows[0]
try:
    cel.infer_box(f.images, cel.BoundingBox(0.0, 30.0, 0.0, 30.0), f.catalog, method="mcmc", astrometry=True)
except ValueError as e:
    assert "mcmc" in str(e) and "astrometry" in str(e)
else:
    raise AssertionError("method='mcmc' with astrometry=True must raise")
assert "celeste_jl_amd.astrom" not in sys.modules
print("ok")
"""
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


def test_astrometry_object_and_row_columns():
    """indexing by target, the offsets on the sky with their covariance, the catalog columns"""
    from celeste_jl_amd import astrom, catalog, infer
    E = 3
    J = np.array([[0.0, 2.0], [-4.0, 0.0]])                    # a rotated, anisotropic pixel grid
    cov = np.zeros((E, 6)); cov[:, 0] = 0.04; cov[:, 3] = 0.01; cov[:, 5] = 1.0
    summary = np.full((2, astrom.NSUMMARY), np.nan)
    summary[1, astrom.MOTION:astrom.MOTION + 4] = [0.1, 0.2, 3.0, -4.0]
    summary[1, astrom.MOTION_COV:astrom.MOTION_COV + 10] = [1, 0, 0, 0, 1, 0, 0, 0.25, 0, 0.0625]
    summary[1, astrom.CHI2_CONST], summary[1, astrom.CHI2_LIN] = 50.0, 1.5
    am = astrom.Astrometry(offsets=np.array([0, 1, 3]), image=np.array([0, 0, 1], dtype=np.int32),
                           delta=np.array([[0.2, 0.4], [0.2, 0.4], [-0.2, 0.0]]), alpha=np.ones(E), fisher=np.zeros((E, 6)), cov=cov,
                           chi2=np.zeros(E), loglik=np.zeros(E), n_pix=np.full(E, 81, dtype=np.int32), iters=np.full(E, 4, dtype=np.int32),
                           flag=np.zeros(E, dtype=np.int32), jac=np.stack([J] * E), n_epochs=np.array([1, 2], dtype=np.int32),
                           summary_flag=np.array([astrom.NO_MOTION, 0], dtype=np.int32), summary=summary, status=np.zeros(2, dtype=np.int32))
    assert len(am) == 2 and am.entry_target().tolist() == [0, 1, 1]
    one = am[1]
    assert len(one) == 1 and one.offsets.tolist() == [0, 2] and one.image.tolist() == [0, 1] and one.jac.shape == (2, 2, 2)
    assert am[[1, 0]].image.tolist() == [0, 1, 0] and am[0:1].offsets.tolist() == [0, 1] and len(am[-1]) == 1
    D, C = am.sky_offset()                                      # delta = J Delta: Delta = (-d2 / 4, d1 / 2)
    assert np.allclose(D, [[-0.1, 0.1], [-0.1, 0.1], [0.0, -0.1]], rtol=0, atol=1e-15)
    assert np.allclose(C[0], [[0.01 / 16, 0], [0, 0.04 / 4]], rtol=1e-15, atol=0)
    assert np.allclose(am.pos_stderr_px(), [[0.2, 0.1]] * 3)
    assert one.motion.tolist() == [[3.0, -4.0]] and one.motion_cov[0, 2, 2] == 0.25 and one.motion_cov[0, 3, 3] == 0.0625
    res = infer.OptimizedSource(0.0, 0.0, np.zeros(44), False, astrometry=one)
    assert catalog.astrometry_columns(res.astrometry) == {
        "n_epochs_astrom": 2, "pm_ra": 3.0, "pm_dec": -4.0, "pm_ra_stderr": 0.5, "pm_dec_stderr": 0.25, "astrom_chi2_const": 50.0,
        "astrom_chi2_lin": 1.5}
    first = catalog.astrometry_columns(am[0])
    assert first["n_epochs_astrom"] == 1 and all(first[k] is None for k in catalog.ASTROMETRY_COLUMNS[1:])


# ---- the restatement ---------------------------------------------------------------------------------------------------
_CACHE = {}


def _star_entry(band=2):
    """the r-band entry of the sample star at the catalog's own row: a bright star, 400-odd pixels"""
    if "star" not in _CACHE:
        import astrom_reference as AR
        from celeste_jl_amd import synthetic
        f = synthetic.make_sample_dataset("star", seed=1, perturb=False)
        _CACHE["star"] = (f, AR.entries_of(f.images, f.patches, f.neighbors, f.vp, 0))
    return _CACHE["star"][1][band]


def _galaxy_entry(band=2):
    if "galaxy" not in _CACHE:
        import astrom_reference as AR
        from celeste_jl_amd import synthetic
        f = synthetic.make_sample_dataset("galaxy", seed=1, perturb=False)
        _CACHE["galaxy"] = (f, AR.entries_of(f.images, f.patches, f.neighbors, f.vp, 0))
    return _CACHE["galaxy"][1][band]


@pytest.mark.parametrize("kind", ["star", "galaxy"])
def test_restatement_derivatives_against_central_differences(lib, kind):
    """dm / d delta from autograd against central differences of m itself (h = 1e-5 px: truncation h^2 m''' / 6
    and rounding 1e-16 m / h, both below 1e-9 of the largest gradient on these smooth densities -- bound 1e-7); the score U
    against central differences of the likelihood; the score of the whole likelihood from autograd against U."""
    e = _star_entry() if kind == "star" else _galaxy_entry()
    d0 = np.array([0.3, -0.2])
    m, dm = e.light(d0)
    h = 1e-5
    worst = 0.0
    for k in range(2):
        dh = np.zeros(2); dh[k] = h
        fd = (e.light(d0 + dh)[0] - e.light(d0 - dh)[0]) / (2 * h)
        worst = max(worst, float(np.abs(fd - dm[k]).max() / np.abs(dm[k]).max()))
    th = np.array([0.3, -0.2, 1.1])
    p = e.evaluate(th)
    # l's central difference: rounding 2e-16 sum |term| / (2 h), truncation of the order h^2 F_kk^(3/2); in standard errors
    hs = [1e-4, 1e-4, 1e-4]
    errs = []
    for k in range(3):
        dt = np.zeros(3); dt[k] = hs[k]
        fd = (e.evaluate(th + dt).l - e.evaluate(th - dt).l) / (2 * hs[k])
        floor = 2e-16 * p.abs_l / (2 * hs[k])
        errs.append((abs(fd - float(p.U[k])) - floor) / np.sqrt(float(p.F[[0, 3, 5][k]])))
    g, J = e.score_and_observed(th)
    rev = float(np.abs(g - p.U.astype(np.float64)).max() / np.abs(p.U.astype(np.float64)).max())
    print("%s: dm %.2e of its maximum (bound 1e-7); U against l's differences %s standard errors above the rounding floor "
          "(bound 1e-3); whole-likelihood score %.2e (bound 1e-10)" % (kind, worst, np.round(errs, 6).tolist(), rev))
    assert worst <= 1e-7 and max(errs) <= 1e-3 and rev <= 1e-10
    assert np.allclose(J, J.T, rtol=1e-9, atol=1e-9 * np.abs(J).max())


@pytest.mark.parametrize("kind", ["star", "galaxy"])
def test_restatement_recovers_a_noise_free_displaced_source(lib, kind):
    """the pixels are the model itself at theta = (0.3, -0.4, 1.2), in float64: the iteration ends OK next to it, and the
    independent root (Newton on the observed information) returns delta and alpha to 1e-9"""
    import copy
    import astrom_reference as AR
    e = copy.copy(_star_entry() if kind == "star" else _galaxy_entry())
    truth = np.array([0.3, -0.4, 1.2])
    m, _ = e.light(truth[:2])
    e.x = np.where(e.visited, e.b + truth[2] * e.iota * m, 0.0)
    r = AR.iterate(e)
    assert r.flag == AR.OK and r.iters < 50
    th, size = e.root(r.theta)
    print("%s: iterate %d passes, |theta - truth| %s; root %s" % (kind, r.iters, np.abs(r.theta - truth), np.abs(th - truth)))
    assert np.abs(th - truth).max() <= 1e-9 and size <= 1e-10
    F = AR.full3(np.asarray(r.F, dtype=np.float64))
    d = r.theta - truth
    rr = e.contraction(th)
    assert rr <= 0.9 and np.sqrt(d @ F @ d) <= 2 * (1e-6 + 1e-8) / (1 - rr)


def test_restatement_gate_does_not_depend_on_the_pixels(lib):
    """F at theta_0, inv(F) and with them the gate are unchanged when the pixels are replaced"""
    import copy
    import astrom_reference as AR
    e = _star_entry(0)                                        # the u band: the faintest
    a = e.evaluate([0.0, 0.0, 1.0])
    e2 = copy.copy(e)
    rng = np.random.Generator(np.random.PCG64(8))
    e2.x = np.where(e.visited, rng.poisson(np.where(e.visited, e.x, 0.0) + 50.0).astype(np.float64), 0.0)
    b = e2.evaluate([0.0, 0.0, 1.0])
    assert np.array_equal(a.F, b.F) and not np.array_equal(a.U, b.U) and a.l != b.l
    sa, sb = AR.step_of(a.F, a.U), AR.step_of(b.F, b.U)
    assert np.array_equal(sa.cov, sb.cov)
    sig = float(np.sqrt(max(sa.cov[0], sa.cov[3])))
    for gate in (sig * 0.99, sig * 1.01):
        ra, rb = AR.iterate(e, max_sigma_px=gate, max_iters=1), AR.iterate(e2, max_sigma_px=gate, max_iters=1)
        assert (ra.flag == AR.TOO_FAINT) == (rb.flag == AR.TOO_FAINT) == (gate < sig)
        if gate < sig:
            assert np.isnan(ra.theta).all() and np.array_equal(ra.cov, np.asarray(sa.cov, dtype=np.float64)) and ra.iters == 1


COVERAGE_SEED, COVERAGE_DRAWS = 2025, 240


def test_restatement_coverage_over_poisson_draws(lib):
    """240 Poisson draws (PCG64(2025)) of the sample star's r-band patch from its own model at theta = (0, 0, 1); each is solved
    by Fisher scoring from the truth (dec <= 1e-6, the header's step).  The pulls (theta_hat - theta_true) / sigma, sigma from
    inv(F) at theta_hat, have mean 0 within 5 / sqrt(N) and variance 1 within 5 sqrt(2 / (N - 1)): the estimate is unbiased
    and inv(F) is its covariance."""
    import copy
    import astrom_reference as AR
    e0 = _star_entry()
    truth = np.array([0.0, 0.0, 1.0])
    m, _ = e0.light(truth[:2])
    lam = np.where(e0.visited, e0.b + e0.iota * m, 0.0)
    rng = np.random.Generator(np.random.PCG64(COVERAGE_SEED))
    pulls = []
    for _ in range(COVERAGE_DRAWS):
        e = copy.copy(e0)
        e.x = np.where(e0.visited, rng.poisson(lam).astype(np.float64), 0.0)
        th = truth.copy()
        for _ in range(20):
            p = e.evaluate(th)
            st = AR.step_of(p.F, p.U)
            assert st.ok
            if st.dec <= 1e-6:
                break
            th = th + np.asarray(st.p, dtype=np.float64)
        else:
            raise AssertionError("scoring from the truth did not converge")
        pulls.append((th - truth) / np.sqrt(np.asarray(st.cov, dtype=np.float64)[[0, 3, 5]]))
    pulls = np.array(pulls)
    N = len(pulls)
    mean, var = pulls.mean(axis=0), pulls.var(axis=0, ddof=1)
    print("pulls over %d draws: mean %s (bound %.3f), variance %s (1 +- %.3f)" % (N, np.round(mean, 3), 5 / np.sqrt(N), np.round(var, 3),
                                                                                 5 * np.sqrt(2 / (N - 1))))
    assert N >= 200 and (np.abs(mean) <= 5 / np.sqrt(N)).all() and (np.abs(var - 1) <= 5 * np.sqrt(2 / (N - 1))).all()


def test_restatement_flags(lib):
    """max_iters = 1, a range that the perturbed row's offset leaves, and a patch of zeros under the source"""
    import copy
    import astrom_reference as AR
    e = _star_entry()
    r = AR.iterate(e, max_iters=1)
    assert r.flag == AR.NOT_CONVERGED and r.iters == 1 and r.theta.tolist() == [0.0, 0.0, 1.0] and np.isfinite(r.cov).all()
    moved = copy.copy(e)
    m, _ = e.light([0.9, 0.0])
    moved.x = np.where(e.visited, e.b + e.iota * m, 0.0)
    assert AR.iterate(moved).flag == AR.OK and AR.iterate(moved, max_shift_px=0.25).flag == AR.OUT_OF_RANGE
    zero = copy.copy(e)
    zero.x = np.zeros_like(e.x)
    rz = AR.iterate(zero)
    print("a patch of zeros ends with flag %d after %d passes, %d halvings, alpha %.3g" % (rz.flag, rz.iters, rz.halvings, rz.theta[2]))
    assert rz.flag in (AR.STALLED, AR.NOT_CONVERGED, AR.OUT_OF_RANGE)


def test_restatement_summary_on_hand_made_entries():
    """a rotated and flipped J, uneven epochs, an exact linear motion: recovered to 1e-12, chi2_lin = 0 to rounding, chi2_const
    large; one epoch: a mean and no motion; none: nothing"""
    import astrom_reference as AR
    rng = np.random.Generator(np.random.PCG64(12))
    c, s = np.cos(0.7), np.sin(0.7)
    J = np.array([[c, -s], [s, c]]) @ np.diag([3600.0, -3600.0]) * 2.5       # pixels per degree, rotated and flipped
    epochs = np.array([0.0, 1.0, 2.5, 4.0, 9.0])
    D0, mu = np.array([2e-5, -1e-5]), np.array([3e-5, 4e-5])
    rows = []
    for n in (0, 1, 2, 3):
        A = rng.normal(size=(6, 3)) * np.array([30.0, 30.0, 5.0])
        F = A.T @ A
        Delta = D0 + mu * epochs[n]
        rows.append((n, AR.OK, J @ Delta, AR.pack3(F), J))
    rows.insert(2, (4, AR.STALLED, np.array([9.0, 9.0]), AR.pack3(np.eye(3)), J))      # not OK: left out (image order is the caller's)
    n, fl, out = AR.summarise(rows, epochs)
    tref = epochs[:4].mean()
    assert n == 4 and fl == 0 and out[21] == tref
    want = np.concatenate([D0 + mu * tref, mu])
    print("motion error %.2e relative, chi2_lin %.2e, chi2_const %.3g" % (np.abs(out[6:10] - want).max() / np.abs(want).max(), out[20], out[5]))
    assert np.abs(out[6:10] - want).max() <= 1e-12 * np.abs(want).max() and 0 <= out[20] <= 1e-18 and out[5] > 100
    bc = np.zeros((4, 4))
    q = 10
    for k in range(4):
        for l in range(k, 4):
            bc[k, l] = bc[l, k] = out[q]; q += 1
    assert q == 20 and (np.linalg.eigvalsh(bc) > 0).all()
    # W of one entry: the inverse of the covariance of Delta with alpha marginalised
    D, W = AR.entry_weight(J, rows[0][2], rows[0][3])
    cov = np.linalg.inv(AR.full3(rows[0][3]))[:2, :2]
    Ji = np.linalg.inv(J)
    assert np.allclose(np.linalg.inv(W), Ji @ cov @ Ji.T, rtol=1e-10) and np.allclose(D, D0, rtol=1e-12)
    n, fl, out = AR.summarise(rows[:1], epochs)
    assert n == 1 and fl == AR.NO_MOTION and np.allclose(out[0:2], D0, rtol=1e-12) and np.isnan(out[6:21]).all() and out[5] <= 1e-20
    n, fl, out = AR.summarise([rows[0], (1, AR.OK) + rows[0][2:]], np.zeros(5))       # two entries at one time
    assert n == 2 and fl == AR.NO_MOTION and np.isfinite(out[:6]).all() and np.isnan(out[6:21]).all()
    n, fl, out = AR.summarise(rows[2:3], epochs)
    assert n == 0 and fl == AR.NO_EPOCHS | AR.NO_MOTION and np.isnan(out).all()
    n2, fl2, out2 = AR.summarise(rows, None)                   # NULL epochs: the image index
    assert n2 == 4 and out2[21] == 1.5


def test_moved_scene_in_the_restatement(lib):
    """three exposures of one region, the brightest source rendered (0.4, -0.3) px away in the second: its displaced entries
    are within 4 sigma of the truth, its chi2_const is above the 0.999 quantile of chi-square with 2 (n - 1) degrees of
    freedom and every other source's is below its own.  Seed: astrom_reference.MOVED_SEED."""
    import astrom_reference as AR
    from scipy.stats import chi2
    f, mv = AR.moved_scene()
    assert len(f.images) == 15 and len(f.catalog) == 6 and [im.b for im in f.images] == [1, 2, 3, 4, 5] * 3
    ref = AR.astrom_reference(f.images, f.patches, f.neighbors, f.vp, list(range(6)))
    _CACHE["moved"] = ref
    assert (ref.status == 0).all()
    flags = np.array([e.result.flag for e in ref.flat])
    print("flags of the moved scene:", np.bincount(flags, minlength=7).tolist(), "n_epochs", ref.n_epochs.tolist())
    check_moved(f, mv, [(e.image, e.result.flag, e.result.theta, e.result.cov) for e in ref.entries[mv]], ref.n_epochs,
                ref.summary[:, 5], chi2)


def check_moved(f, mv, entries, n_epochs, chi2_const, chi2):
    """shared with the device test: entries = [(image, flag, theta, cov)] of the moved source"""
    import astrom_reference as AR
    shift = np.array(AR.MOVED_SHIFT)
    n_disp = 0
    for image, flag, theta, cov in entries:
        if flag != AR.OK:
            continue
        truth = shift if 5 <= image < 10 else np.zeros(2)
        z = (np.asarray(theta)[:2] - truth) / np.sqrt(np.asarray(cov)[[0, 3]])
        assert (np.abs(z) <= 4).all(), (image, z)
        n_disp += 5 <= image < 10
    assert n_disp >= 3
    for s in range(len(n_epochs)):
        if n_epochs[s] < 2:
            continue
        q = chi2.ppf(0.999, 2 * (n_epochs[s] - 1))
        assert (chi2_const[s] > q) == (s == mv), (s, chi2_const[s], q)
    assert n_epochs[mv] >= 8
