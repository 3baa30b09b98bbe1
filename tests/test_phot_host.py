"""libceleste_phot.so without a GPU: its C ABI (header, exports, Python binding), the refusals that come back before any
device is touched, the untouched defaults of infer_box and celeste_to_rows, and the numpy / scipy restatement of the
photometry (tests/phot_reference.py) on Poisson pixels it drew itself and on a scene with one variable source."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _protos():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "celeste_phot.h")).read(), flags=re.S)
    return {n: (0 if a.strip() in ("", "void") else len(a.split(","))) for n, a in
            re.findall(r"\b(celeste_phot_\w+)\s*\(([^)]*)\)\s*;", hdr)}


def test_the_phot_library_exports_its_c_abi_and_nothing_else(lib):
    from celeste_jl_amd import phot
    protos = _protos()
    assert set(protos) == set(phot.EXPORTED_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", phot.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip()) == sorted(phot.EXPORTED_SYMBOLS)
    emap = open(os.path.join(ROOT, "celeste.jl_amd", "csrc", "phot", "exports.map")).read()
    assert re.search(r"global:\s*celeste_phot_\*;\s*local:\s*\*;", emap)
    f = phot.load_library()
    for name, n_args in protos.items():                       # the ctypes signatures
        at = getattr(f, name).argtypes
        assert (0 if at is None else len(at)) == n_args, name
    assert f.celeste_phot_version() == phot.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "celeste_phot.h")).read()
    assert "#define CELESTE_PHOT_ABI_VERSION %d" % phot.ABI_VERSION in hdr
    assert "#define CELESTE_PHOT_BANDS %d" % phot.BANDS in hdr and "#define CELESTE_PHOT_NSUMMARY %d" % phot.NSUMMARY in hdr
    assert "#define CELESTE_PHOT_LDS_PIXELS %d" % phot.LDS_PIXELS in hdr
    flags, sums = re.findall(r"enum \{(.*?)\};", hdr, re.S)
    assert [int(v) for v in re.findall(r"=\s*(\d+)", flags)] == [phot.OK, phot.NO_LIGHT, phot.AT_BOUND, phot.NOT_CONVERGED,
                                                                phot.BAD_MODEL]
    assert [int(v) for v in re.findall(r"=\s*(\d+)", sums)] == [phot.WMEAN, phot.WMEAN_SIGMA, phot.CHI2_VAR]
    import ctypes as C
    assert C.sizeof(phot.ParamsT) == 16 and phot.ParamsT.max_iters.offset == 8 and phot.ParamsT.lds_max_pixels.offset == 12
    assert b"no CPU fallback" in f.celeste_phot_strerror(5)


def _call_args(params=None, ctx=None, n=1):
    """a full argument list over arrays filled with -7, and those arrays"""
    import ctypes as C
    from celeste_jl_amd import cabi, phot
    dp, ip, lp = cabi.c_double_p, cabi.c_int32_p, cabi.c_int64_p
    vp = np.zeros((2, 44))
    tg = np.zeros(1, dtype=np.int32)
    i32 = [np.full(8, -7, dtype=np.int32) for _ in range(6)]           # image, n_pix, iters, flag, n_epochs, status
    f64 = [np.full(16, -7.0) for _ in range(4)]                        # alpha, sigma, chi2, summary
    off = np.full(2, -7, dtype=np.int64)
    p = phot._ptr
    args = [ctx, p(vp, dp), n, p(tg, ip), None if params is None else C.byref(params), p(off, lp), p(i32[0], ip), p(f64[0], dp),
            p(f64[1], dp), p(f64[2], dp), p(i32[1], ip), p(i32[2], ip), p(i32[3], ip), p(i32[4], ip), p(f64[3], dp), p(i32[5], ip)]
    return args, [vp, tg, off] + i32 + f64


def test_refusals_come_back_before_any_device_is_touched(lib):
    """invalid arguments are INVALID_ARG, not NO_DEVICE or a HIP error, also on a machine without a device: nothing of HIP
    has been called when they return, and nothing has been written"""
    import ctypes as C
    from celeste_jl_amd import cabi, phot
    f = phot.load_library()
    keep = []
    for kw in (dict(), dict(n=-1), dict(n=0), dict(params=phot.ParamsT(0.0, 50, 0)), dict(params=phot.ParamsT(1e-9, 0, 0))):
        args, arrays = _call_args(**kw)                               # no context
        keep.append(arrays)
        assert f.celeste_phot_light_curves(*args) == cabi.ERR_INVALID_ARG, kw
    for arrays in keep:
        assert all((a == -7).all() for a in arrays[2:])
    assert f.celeste_phot_last_ms(None, (C.c_float * 4)()) == cabi.ERR_INVALID_ARG
    assert f.celeste_phot_ctx_create(None, 0, None) == cabi.ERR_INVALID_ARG
    h = C.c_void_p(1234)
    assert f.celeste_phot_ctx_create(None, 0, C.byref(h)) == cabi.ERR_INVALID_ARG and not h.value
    f.celeste_phot_ctx_destroy(None)


def test_no_device_no_fallback(lib):
    """without a device the context refuses with NO_DEVICE (there is no CPU path); on a GPU machine it is created"""
    import torch
    from celeste_jl_amd import cabi, phot, synthetic
    f = synthetic.make_sample_dataset("two_body", seed=1)
    pr = cabi.Problem(f.images, f.patches, f.neighbors)
    if torch.cuda.is_available():
        phot.PhotContext(pr).close()
    else:
        with pytest.raises(RuntimeError, match="no HIP device") as e:
            phot.PhotContext(pr)
        assert "status %d" % cabi.ERR_NO_DEVICE in str(e.value)
    assert phot.entry_counts(pr).tolist() == [sum(0 not in p.active_pixel_bitmap.shape for p in row) for row in f.patches]


def test_the_defaults_do_not_import_phot_and_return_what_they_returned():
    """infer_box and celeste_to_rows with their defaults: the module is not loaded, the rows are the rows"""
    code = r"""
import sys, inspect
import numpy as np
import celeste_jl_amd as cel
from celeste_jl_amd import catalog, infer, synthetic
assert inspect.signature(cel.infer_box).parameters["light_curves"].default is False
assert inspect.signature(catalog.celeste_to_rows).parameters["light_curves"].default is False
f = synthetic.make_sample_dataset("two_body", seed=1)
assert cel.infer_box(f.images, cel.BoundingBox(-9.0, -8.0, -9.0, -8.0), f.catalog) == []          # no target in the box
res = [cel.OptimizedSource(1.0, 2.0, f.vp[0].copy(), False), cel.OptimizedSource(3.0, 4.0, f.vp[1].copy(), True)]
assert res[0].light_curve is None and res[0].fit is None
rows = catalog.celeste_to_rows(res)
assert rows == [catalog.variational_parameters_to_row(f.vp[0])]
assert not set(catalog.LIGHT_CURVE_COLUMNS) & set(rows[0]) and catalog.LIGHT_CURVE_COLUMNS == ("n_epochs_r", "var_chi2_r")
assert catalog.celeste_to_rows(res, diagnostics=True) == [dict(rows[0], **{k: None for k in catalog.DIAGNOSTIC_COLUMNS})]
assert "celeste_jl_amd.phot" not in sys.modules and "celeste_jl_amd.fit" not in sys.modules
d = catalog.celeste_to_rows(res, light_curves=True)
assert len(d) == 1 and all(d[0][k] is None for k in catalog.LIGHT_CURVE_COLUMNS)
assert {k: v for k, v in d[0].items() if k not in catalog.LIGHT_CURVE_COLUMNS} == rows[0]
try:
    cel.infer_box(f.images, cel.BoundingBox(0.0, 30.0, 0.0, 30.0), f.catalog, method="mcmc", light_curves=True)
except ValueError as e:
    assert "mcmc" in str(e) and "light_curves" in str(e)
else:
    raise AssertionError("method='mcmc' with light_curves=True must raise")
assert "celeste_jl_amd.phot" not in sys.modules
print("ok")
"""
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


def test_light_curves_object_and_row_columns():
    """indexing by target, the flux in nanomaggies, the reduced variability chi-square, the two catalog columns"""
    from celeste_jl_amd import catalog, infer, phot, synthetic
    f = synthetic.make_sample_dataset("two_body", seed=1)
    E = 7                                                     # target 0: images 0..4 (one epoch per band); target 1: r and i only
    lc = phot.LightCurves(
        offsets=np.array([0, 5, 7]), image=np.array([0, 1, 2, 3, 4, 2, 3], dtype=np.int32),
        band=np.array([0, 1, 2, 3, 4, 2, 3], dtype=np.int32), alpha=np.arange(1.0, 1.0 + E), sigma=np.full(E, 0.5),
        chi2=np.zeros(E), n_pix=np.full(E, 81, dtype=np.int32), iters=np.full(E, 4, dtype=np.int32),
        flag=np.zeros(E, dtype=np.int32), n_epochs=np.array([[1, 1, 1, 1, 1], [0, 0, 3, 1, 0]], dtype=np.int32),
        summary=np.zeros((2, 5, 3)), status=np.zeros(2, dtype=np.int32), band_flux=phot.expected_band_flux(f.vp))
    lc.summary[1, 2] = [1.5, 0.25, 8.0]
    assert len(lc) == 2 and lc.entry_target().tolist() == [0] * 5 + [1] * 2
    one = lc[1]
    assert len(one) == 1 and one.offsets.tolist() == [0, 2] and one.image.tolist() == [2, 3] and one.alpha.tolist() == [6.0, 7.0]
    assert lc[[1, 0]].image.tolist() == [2, 3, 0, 1, 2, 3, 4] and lc[0:1].offsets.tolist() == [0, 5] and len(lc[-1]) == 1
    assert np.array_equal(lc.flux_nmgy()[5:], np.array([6.0, 7.0]) * lc.band_flux[1, [2, 3]])
    assert np.array_equal(one.flux_nmgy(), lc.flux_nmgy()[5:]) and np.array_equal(one.flux_nmgy_sigma(), 0.5 * lc.band_flux[1, [2, 3]])
    r = lc.reduced_chi2_var()
    assert r[1, 2] == 4.0 and np.isnan(r[0]).all() and np.isnan(r[1, 3]) and np.isnan(r[1, 0])
    # the expected band flux against the catalog's own reading of a row (its median flux, for a source of one type)
    vs = f.vp[0].copy()
    vs[26:28] = [1.0, 0.0]
    want = catalog.get_median_fluxes(vs, 0) * np.exp(vs[8] / 2 + np.array([vs[18] + vs[19], vs[19], 0, vs[20], vs[20] + vs[21]]) / 2)
    assert np.allclose(phot.expected_band_flux(vs), want, rtol=1e-13, atol=0)
    res = infer.OptimizedSource(0.0, 0.0, np.zeros(44), False, light_curve=one)
    assert catalog.light_curve_columns(res.light_curve) == {"n_epochs_r": 3, "var_chi2_r": 8.0}
    assert catalog.light_curve_columns(lc[0]) == {"n_epochs_r": 1, "var_chi2_r": 0.0}


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_restatement_on_its_own_poisson_pixels(lib):
    """make_field(96, 96, 6, seed=11), every visited pixel replaced by a Poisson draw (PCG64(2024)) from the table's own
    lam(1) = a + b -- catalog_init_source rows are not the truth of make_field's pixels.  Every entry has a root, and
    z = (alpha_hat - 1) sqrt(I) is a standardised score: |z| <= 5.
    Measured: 30 entries, patches 8 x 8 to 51 x 51, largest |z| 2.71, rms 1.17 (the images are drawn
    one after another from one generator, each image's visited pixels in array order)."""
    import copy
    import fit_reference as FR
    import phot_reference as PR
    from celeste_jl_amd import synthetic
    f = synthetic.make_field(96, 96, 6, seed=11)
    targets = list(range(6))
    expected = {s: FR.expected_nmgy(f.images, f.patches, f.neighbors, f.vp, s) for s in targets}
    lam = [np.full(im.pixels.shape, np.nan) for im in f.images]
    for s in targets:
        for e, (n, visited, E, m, B) in zip(PR.patch_entries(f.images, f.patches, f.neighbors, f.vp, s, expected[s]), expected[s]):
            h0, w0 = f.patches[s][n].bitmap_offset
            sub = lam[n][h0:h0 + visited.shape[0], w0:w0 + visited.shape[1]]
            sub[visited] = e.a + e.b
    rng = np.random.Generator(np.random.PCG64(2024))
    images = [copy.copy(im) for im in f.images]
    for n, im in enumerate(images):
        px = im.pixels.copy()
        ok = ~np.isnan(lam[n])
        px[ok] = rng.poisson(lam[n][ok]).astype(np.float32)
        im.pixels = px
    ref = PR.phot_reference(images, f.patches, f.neighbors, f.vp, targets, expected=expected)
    assert (ref.status == 0).all() and len(ref.flat) == 30 and all(e.flag == PR.OK for e in ref.flat)
    z = np.array([(e.alpha - 1) / e.sigma for e in ref.flat])
    sizes = sorted({p.active_pixel_bitmap.shape for row in f.patches for p in row})
    print("entries %d, patches %s to %s, max |z| %.2f, rms %.2f" % (len(z), sizes[0], sizes[-1], np.abs(z).max(), np.sqrt((z * z).mean())))
    assert np.isfinite(z).all() and (np.abs(z) <= 5).all()
    for e in ref.flat:                                       # the root is a root, right of the edge of the domain
        (g, I, _), _ = e.evaluate(e.alpha)
        assert abs(float(g)) / np.sqrt(float(I)) <= 1e-10 and e.alpha > e.alpha_min
    assert (ref.n_epochs == 1).all() and (ref.summary[:, :, 2] <= 1e-20).all()      # one epoch: (w alpha) / w is alpha to an ulp


def test_restatement_flags():
    import phot_reference as PR
    a, b = np.array([2.0, 1.0, 0.0]), np.array([4.0, 3.0, 5.0])
    e = PR.solve(PR.Entry(0, 2, 3, a, b, np.array([0.0, 0.0, 9.0])))
    assert e.flag == PR.AT_BOUND and e.alpha == -2.0 and np.isnan(e.sigma)
    e = PR.solve(PR.Entry(0, 2, 3, np.zeros(3), b, np.array([4.0, 3.0, 7.0])))
    assert e.flag == PR.NO_LIGHT and np.isnan(e.alpha) and abs(e.chi2 - 0.8) < 1e-15
    for bad_a, bad_b in ((np.array([np.nan, 1, 0]), b), (np.array([-1.0, 1, 0]), b), (a, np.array([4.0, 0.0, 5.0])),
                         (a, np.array([4.0, np.inf, 5.0]))):
        assert PR.solve(PR.Entry(0, 2, 3, bad_a, bad_b, np.ones(3))).flag == PR.BAD_MODEL
    e = PR.solve(PR.Entry(0, 2, 3, a, b, np.array([1.0, 0.0, 5.0])))     # a faint source: a negative scale is allowed
    assert e.flag == PR.OK and e.alpha_min < e.alpha < 0 and abs(e.g(e.alpha)) < 1e-12
    ne, sm = PR.band_summaries([PR.Entry(0, 2, 1, a, b, b, PR.OK, 1.0, -2.0, 0.5), PR.Entry(5, 2, 1, a, b, b, PR.OK, 2.0, -2.0, 0.5),
                                PR.Entry(6, 2, 1, a, b, b, PR.NOT_CONVERGED, 9.0, -2.0, 0.5)])
    assert ne.tolist() == [0, 0, 2, 0, 0] and sm[2].tolist() == [1.5, 0.5 / np.sqrt(2), 2.0] and np.isnan(sm[0]).all()


def test_variability_scene_in_the_restatement(lib):
    """three exposures of one region, one source 1.5 times brighter in the second: its var_chi2_r is the largest of the scene
    and above the 0.999 quantile of chi-square with 2 degrees of freedom; every other source stays below it.
    Seed: phot_reference.VARIABILITY_SEED = 3 (seeds 1, 2, 5 and 7 also do; with 4 and 6 a neighbour that overlaps the
    variable source crosses the quantile too)."""
    import phot_reference as PR
    from scipy.stats import chi2
    from celeste_jl_amd import catalog, infer, phot
    f, var = PR.variability_scene()
    assert PR.VARIABILITY_SEED == 3 and len(f.images) == 15 and len(f.catalog) == 6
    assert f.images[0].pixels.shape == (64, 80) and [im.b for im in f.images] == [1, 2, 3, 4, 5] * 3
    ref = PR.phot_reference(f.images, f.patches, f.neighbors, f.vp, list(range(6)))
    assert (ref.status == 0).all() and all(e.flag == PR.OK for e in ref.flat) and (ref.n_epochs == 3).all()
    q = chi2.ppf(0.999, 2)
    v = ref.summary[:, 2, 2]
    print("var_chi2_r %s, variable source %d, quantile %.3f" % (np.round(v, 2).tolist(), var, q))
    assert int(np.argmax(v)) == var and v[var] > q and (np.delete(v, var) < q).all()
    al = np.array([e.alpha for e in ref.entries[var] if e.band == 2])
    assert al[1] > 1.3 * al[0] and al[1] > 1.3 * al[2]            # the second exposure stands out in the light curve itself
    # the same through the catalog's columns
    off = ref.offsets
    lc = phot.LightCurves(off, *[np.array([getattr(e, k) for e in ref.flat]) for k in ("image", "band", "alpha", "sigma", "chi2")],
                          np.array([e.n_pix for e in ref.flat]), np.zeros(len(ref.flat), dtype=np.int32),
                          np.array([e.flag for e in ref.flat]), ref.n_epochs, ref.summary, ref.status, phot.expected_band_flux(f.vp))
    res = [infer.OptimizedSource(0.0, 0.0, f.vp[s], False, light_curve=lc[s]) for s in range(6)]
    rows = catalog.celeste_to_rows(res, light_curves=True)
    assert [r["n_epochs_r"] for r in rows] == [3] * 6 and [r["var_chi2_r"] for r in rows] == v.tolist()
    assert np.allclose(lc.reduced_chi2_var()[:, 2], v / 2, rtol=1e-15)
