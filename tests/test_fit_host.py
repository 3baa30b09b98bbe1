"""libceleste_fit.so without a GPU: its C ABI (header, exports, Python binding), the refusals that come back before any
device is touched, and the numpy restatement of its statistics (tests/fit_reference.py) -- against an independent rendering
of the expected image, and against Poisson pixels it drew itself."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _protos():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "celeste_fit.h")).read(), flags=re.S)
    return {n: (0 if a.strip() in ("", "void") else len(a.split(","))) for n, a in
            re.findall(r"\b(celeste_fit_\w+)\s*\(([^)]*)\)\s*;", hdr)}


def test_the_fit_library_exports_its_c_abi_and_nothing_else(lib):
    from celeste_jl_amd import fit
    protos = _protos()
    assert set(protos) == set(fit.EXPORTED_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", fit.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip()) == sorted(fit.EXPORTED_SYMBOLS)
    emap = open(os.path.join(ROOT, "celeste.jl_amd", "csrc", "fit", "exports.map")).read()
    assert re.search(r"global:\s*celeste_fit_\*;\s*local:\s*\*;", emap)
    f = fit.load_library()
    for name, n_args in protos.items():                       # the ctypes signatures
        at = getattr(f, name).argtypes
        assert (0 if at is None else len(at)) == n_args, name
    assert f.celeste_fit_version() == fit.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "celeste_fit.h")).read()
    assert "#define CELESTE_FIT_ABI_VERSION %d" % fit.ABI_VERSION in hdr
    assert "#define CELESTE_FIT_BANDS %d" % fit.BANDS in hdr and "#define CELESTE_FIT_NSTATS %d" % fit.NSTATS in hdr
    names = re.search(r"enum \{(.*?)\};", hdr, re.S).group(1)
    assert [int(v) for v in re.findall(r"=\s*(\d+)", names)] == [fit.CHI2, fit.RESID, fit.OWN, fit.SELF, fit.WRES, fit.WINFO,
                                                                fit.MAX_Z]
    assert b"no CPU fallback" in f.celeste_fit_strerror(5)


def test_refusals_come_back_before_any_device_is_touched(lib):
    """invalid arguments are INVALID_ARG, not NO_DEVICE or a HIP error, also on a machine without a device: nothing of HIP
    has been called when they return"""
    import ctypes as C
    from celeste_jl_amd import cabi, fit
    f = fit.load_library()
    vp = np.zeros((2, 44))
    tg = np.zeros(1, dtype=np.int32)
    n_pix = np.full((1, 5), -7, dtype=np.int64)
    st = np.full((1, 5, 7), -7.0)
    status = np.full(1, -7, dtype=np.int32)
    buf = np.full(4, -7.0)
    off = np.full(2, -7, dtype=np.int64)
    p = fit._ptr
    dp, ip, lp = cabi.c_double_p, cabi.c_int32_p, cabi.c_int64_p
    for args in ((None, p(vp, dp), 1, p(tg, ip), p(n_pix, lp), p(st, dp), p(status, ip), None, None),        # no context
                 (None, p(vp, dp), -1, p(tg, ip), p(n_pix, lp), p(st, dp), p(status, ip), None, None),
                 (None, None, 0, None, None, None, None, None, None),
                 (None, p(vp, dp), 1, p(tg, ip), p(n_pix, lp), p(st, dp), p(status, ip), None, p(buf, dp)),
                 (None, p(vp, dp), 1, p(tg, ip), p(n_pix, lp), p(st, dp), p(status, ip), p(off, lp), p(buf, dp))):
        assert f.celeste_fit_stats(*args) == cabi.ERR_INVALID_ARG
    assert (n_pix == -7).all() and (st == -7).all() and (status == -7).all() and (buf == -7).all() and (off == -7).all()
    assert f.celeste_fit_last_ms(None, (C.c_float * 3)()) == cabi.ERR_INVALID_ARG
    assert f.celeste_fit_ctx_create(None, 0, None) == cabi.ERR_INVALID_ARG
    h = C.c_void_p(1234)
    assert f.celeste_fit_ctx_create(None, 0, C.byref(h)) == cabi.ERR_INVALID_ARG and not h.value
    f.celeste_fit_ctx_destroy(None)


def test_no_device_no_fallback(lib):
    """without a device the context refuses with NO_DEVICE (there is no CPU path); on a GPU machine it is created"""
    import torch
    from celeste_jl_amd import cabi, fit, synthetic
    f = synthetic.make_sample_dataset("two_body", seed=1)
    pr = cabi.Problem(f.images, f.patches, f.neighbors)
    if torch.cuda.is_available():
        fit.FitContext(pr).close()
    else:
        with pytest.raises(RuntimeError, match="no HIP device") as e:
            fit.FitContext(pr)
        assert "status %d" % cabi.ERR_NO_DEVICE in str(e.value)
    assert fit.patch_shapes(pr) == [[(n, *p.active_pixel_bitmap.shape) for n, p in enumerate(row)] for row in f.patches]


def test_the_defaults_do_not_import_fit_and_return_what_they_returned():
    """infer_box and celeste_to_rows with their defaults: the module is not loaded, the rows are the rows"""
    code = r"""
import sys, inspect
import numpy as np
import celeste_jl_amd as cel
from celeste_jl_amd import catalog, infer, synthetic
assert inspect.signature(cel.infer_box).parameters["diagnostics"].default is False
assert inspect.signature(catalog.celeste_to_rows).parameters["diagnostics"].default is False
f = synthetic.make_sample_dataset("two_body", seed=1)
assert cel.infer_box(f.images, cel.BoundingBox(-9.0, -8.0, -9.0, -8.0), f.catalog) == []          # no target in the box
res = [cel.OptimizedSource(1.0, 2.0, f.vp[0].copy(), False), cel.OptimizedSource(3.0, 4.0, f.vp[1].copy(), True)]
assert res[0].fit is None
rows = catalog.celeste_to_rows(res)
assert rows == [catalog.variational_parameters_to_row(f.vp[0])]
assert not set(catalog.DIAGNOSTIC_COLUMNS) & set(rows[0])
assert "celeste_jl_amd.fit" not in sys.modules
d = catalog.celeste_to_rows(res, diagnostics=True)
assert len(d) == 1 and all(d[0][k] is None for k in catalog.DIAGNOSTIC_COLUMNS)
assert {k: v for k, v in d[0].items() if k not in catalog.DIAGNOSTIC_COLUMNS} == rows[0]
try:
    cel.infer_box(f.images, cel.BoundingBox(0.0, 30.0, 0.0, 30.0), f.catalog, method="mcmc", diagnostics=True)
except ValueError as e:
    assert "mcmc" in str(e)
else:
    raise AssertionError("method='mcmc' with diagnostics=True must raise")
assert "celeste_jl_amd.fit" not in sys.modules
print("ok")
"""
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


def test_rows_carry_the_diagnostic_columns():
    from celeste_jl_amd import catalog, fit, infer
    n_pix = np.array([0, 0, 100, 50, 0], dtype=np.int64)
    st = np.zeros((5, 7))
    st[2] = [120.0, 3.0, 1000.0, 900.0, -20.0, 16.0, 3.5]
    st[3] = [30.0, 1.0, 500.0, 500.0, 4.0, 4.0, 2.5]
    fs = fit.FitStats(n_pix, st, np.int32(0))
    per_band, total = fs.reduced_chi2()
    assert np.isnan(per_band[0]) and per_band[2] == 1.2 and per_band[3] == 0.6 and total == 1.0
    assert fs.flux_z()[2] == -5.0 and fs.flux_correction()[2] == -1.25 and np.isnan(fs.flux_z()[0])
    assert fs.purity()[2] == 0.9 and fs.purity()[3] == 1.0 and np.isnan(fs.purity()[4])
    r = infer.OptimizedSource(0.0, 0.0, np.zeros(44), False, fit=fs)
    assert catalog.fit_columns(r.fit) == {"chi2_reduced": 1.0, "flux_z_r": -5.0, "purity_r": 0.9, "max_z": 3.5, "n_pix": 150}


# ---- the restatement ---------------------------------------------------------------------------------------------------
_SCENE = {}


def _scene():
    """make_field(160, 200, 30, seed=11, nan_fraction=0.004) and the restatement's expected light of every target"""
    if not _SCENE:
        import fit_reference as FR
        from celeste_jl_amd import synthetic
        f = synthetic.make_field(160, 200, 30, seed=11, nan_fraction=0.004)
        targets = list(range(len(f.catalog)))
        _SCENE.update(f=f, targets=targets,
                      expected={s: FR.expected_nmgy(f.images, f.patches, f.neighbors, f.vp, s) for s in targets})
    return _SCENE


def test_restatement_renders_what_the_joint_objective_renders(lib):
    """eps + m + B at the visited pixels of every target = sky + the sum of every source's light on its own patch
    (joint_objective.expected_planes): equal because the neighbour lists are complete, which is asserted"""
    from celeste_jl_amd.model import find_neighbors
    from joint_objective import expected_planes
    sc = _scene()
    f = sc["f"]
    assert f.neighbors == [find_neighbors(f.patches, s) for s in sc["targets"]]
    planes = expected_planes(f.images, f.patches, f.vp)
    n_checked = 0
    for s in sc["targets"]:
        for n, visited, E, m, B in sc["expected"][s]:
            h0, w0 = f.patches[s][n].bitmap_offset
            H2, W2 = visited.shape
            want = f.images[n].sky[h0:h0 + H2, w0:w0 + W2].astype(np.float64) + planes[n][h0:h0 + H2, w0:w0 + W2]
            assert np.abs(E - want)[visited].max() <= 1e-12 * np.abs(planes[n]).max(), (s, n)
            n_checked += int(visited.sum())
            assert (m[:, -1] == 0).all() and (B >= 0).all()
    assert n_checked > 50000 and any((B > 0).any() for s in sc["targets"] for _, _, _, _, B in sc["expected"][s])


def _poisson_scene():
    """the scene with every visited pixel replaced by a Poisson draw of the restatement's own lam (fixed seed)"""
    if "poisson" not in _SCENE:
        import copy
        import fit_reference as FR
        sc = _scene()
        f = sc["f"]
        ref0 = FR.fit_reference(f.images, f.patches, f.neighbors, f.vp, sc["targets"], expected=sc["expected"])
        assert (ref0.status == 0).all()
        lam = [np.full(im.pixels.shape, np.nan) for im in f.images]
        for s, row in zip(sc["targets"], ref0.stamps):
            for n, st in row:
                h0, w0 = f.patches[s][n].bitmap_offset
                sub = lam[n][h0:h0 + st.shape[0], w0:w0 + st.shape[1]]
                sub[~np.isnan(st)] = st[~np.isnan(st)]
        rng = np.random.Generator(np.random.PCG64(20261019))
        images = [copy.copy(im) for im in f.images]
        for n, im in enumerate(images):
            px = im.pixels.copy()
            ok = ~np.isnan(lam[n])
            assert not np.isnan(px[ok]).any()                      # visited pixels only: the NaN masks stay
            px[ok] = rng.poisson(lam[n][ok]).astype(np.float32)
            im.pixels = px
        _SCENE["poisson"] = (images, FR.fit_reference(images, f.patches, f.neighbors, f.vp, sc["targets"], expected=sc["expected"]))
    return _SCENE["poisson"]


def test_restatement_on_its_own_poisson_pixels(lib):
    """Pearson's statistic over pixels drawn from lam has mean n and variance n (2 + 1 / lam) <= n (2 + 1 / min lam); the
    flux misfit of every target is a standardised score"""
    import fit_reference as FR
    images, ref = _poisson_scene()
    assert (ref.status == 0).all()
    n = int(ref.n_pix.sum())
    chi2 = ref.stats[:, :, FR.CHI2].sum()
    bound = 5 * math.sqrt((2 + 1 / ref.min_lam) / n)
    print("chi2 / n - 1 = %.3e (bound %.3e), n = %d, min lam = %.3f" % (chi2 / n - 1, bound, n, ref.min_lam))
    assert abs(chi2 / n - 1) <= bound
    fs = FR.stats_of(ref)
    z = fs.flux_z()
    has = ref.stats[:, :, FR.WINFO] > 0
    assert has.sum() >= 5 * len(ref.status) - 5
    print("max |flux_z| = %.3f" % np.abs(z[has]).max())
    assert (np.abs(z[has]) <= 5).all()
    assert np.array_equal(np.isnan(z), ~has)


def test_a_flux_too_bright_by_half_shows_in_flux_z_and_nowhere_else(lib):
    import fit_reference as FR
    from celeste_jl_amd.params import ids
    sc = _scene()
    f = sc["f"]
    images, ref = _poisson_scene()
    pur = FR.stats_of(ref).purity()[:, 2]
    own = ref.stats[:, 2, FR.OWN]
    t = int(np.argmax(np.where(pur > 0.999, own, -np.inf)))       # bright and (nearly) alone in the r band
    assert pur[t] > 0.999 and own[t] > 1e4
    vp = f.vp.copy()
    vp[t, ids.flux_loc] += math.log(1.5)
    expected = dict(sc["expected"])
    touched = [t] + [s for s in sc["targets"] if t in f.neighbors[s]]
    for s in touched:
        expected[s] = FR.expected_nmgy(images, f.patches, f.neighbors, vp, s)
    ref2 = FR.fit_reference(images, f.patches, f.neighbors, vp, sc["targets"], expected=expected)
    fs2 = FR.stats_of(ref2)
    print("flux_z_r %.2f -> %.2f, flux_correction_r %.3f" % (FR.stats_of(ref).flux_z()[t, 2], fs2.flux_z()[t, 2],
                                                             fs2.flux_correction()[t, 2]))
    assert fs2.flux_z()[t, 2] < -5 and fs2.flux_correction()[t, 2] < 0
    # the others, rendered again from the changed table (not taken from the cache): unchanged bit for bit
    others = [s for s in sc["targets"] if s not in touched]
    assert len(others) >= 20
    again = FR.fit_reference(images, f.patches, f.neighbors, vp, others)
    k = [sc["targets"].index(s) for s in others]
    assert np.array_equal(again.stats, ref.stats[k]) and np.array_equal(again.n_pix, ref.n_pix[k])
    assert np.array_equal(ref2.stats[k], ref.stats[k])


def test_purity_is_one_without_neighbours_and_below_one_with_an_overlapping_one(lib):
    import fit_reference as FR
    from celeste_jl_amd import synthetic
    f = synthetic.make_sample_dataset("star")
    assert f.neighbors == [[]]
    ref = FR.fit_reference(f.images, f.patches, f.neighbors, f.vp, [0])
    assert np.array_equal(FR.stats_of(ref).purity(), np.ones((1, 5)))
    assert np.array_equal(ref.stats[:, :, FR.SELF], ref.stats[:, :, FR.OWN]) and (ref.stats[:, :, FR.OWN] > 0).all()
    f = synthetic.make_sample_dataset("two_body")
    assert f.neighbors == [[1], [0]]
    pur = FR.stats_of(FR.fit_reference(f.images, f.patches, f.neighbors, f.vp, [0, 1])).purity()
    assert (pur < 1).all() and (pur > 0).all()
