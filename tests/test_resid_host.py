"""libceleste_resid.so without a GPU: its C ABI (header, exports, Python binding), the refusals that come back before any device
is touched, the defaults that load nothing, and the numpy restatement of the search (tests/resid_reference.py) against
properties that do not depend on it; resid.missed_sources on a hand-made search."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _protos():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "celeste_resid.h")).read(), flags=re.S)
    return {n: (0 if a.strip() in ("", "void") else len(a.split(","))) for n, a in
            re.findall(r"\b(celeste_resid_\w+)\s*\(([^)]*)\)\s*;", hdr)}


def test_the_resid_library_exports_its_c_abi_and_nothing_else(lib):
    from celeste_jl_amd import resid
    protos = _protos()
    assert set(protos) == set(resid.EXPORTED_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", resid.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip()) == sorted(resid.EXPORTED_SYMBOLS)
    emap = open(os.path.join(ROOT, "celeste.jl_amd", "csrc", "resid", "exports.map")).read()
    assert re.search(r"global:\s*celeste_resid_\*;\s*local:\s*\*;", emap)
    f = resid.load_library()
    for name, n_args in protos.items():                       # the ctypes signatures
        at = getattr(f, name).argtypes
        assert (0 if at is None else len(at)) == n_args, name
    assert f.celeste_resid_version() == resid.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "celeste_resid.h")).read()
    assert "#define CELESTE_RESID_ABI_VERSION %d" % resid.ABI_VERSION in hdr
    assert "#define CELESTE_RESID_MAX_RADIUS %d" % resid.MAX_RADIUS in hdr
    assert "#define CELESTE_RESID_TRUNCATED %d" % resid.TRUNCATED in hdr
    names = re.search(r"enum \{(.*?)\};", hdr, re.S).group(1)
    assert [int(v) for v in re.findall(r"=\s*(\d+)", names)] == [resid.LAM, resid.N, resid.D, resid.Z, resid.COVERAGE]
    assert b"no CPU fallback" in f.celeste_resid_strerror(5) and b"truncated" in f.celeste_resid_strerror(resid.TRUNCATED)
    # the structures: sizes and offsets as the header lays them out (natural alignment)
    assert resid.FRAME_DTYPE.itemsize == 48 and resid.CANDIDATE_DTYPE.itemsize == 64
    assert [resid.CANDIDATE_DTYPE.fields[k][1] for k in ("image", "h", "w", "dh", "dw", "z", "f", "D", "cov")] == \
        [0, 4, 8, 16, 24, 32, 40, 48, 56]
    import ctypes as C
    assert C.sizeof(resid.OptsT) == 32
    o = resid.OptsT()
    f.celeste_resid_opts_default(C.byref(o))
    assert (o.threshold, o.min_coverage, o.radius, o.psf_K, bool(o.psf)) == (5.0, 0.8, 8, 0, False)


def test_refusals_come_back_before_any_device_is_touched(lib):
    """invalid arguments are INVALID_ARG, not NO_DEVICE or a HIP error, also on a machine without a device: nothing of HIP has
    been called when they return, and nothing has been written"""
    import ctypes as C
    from celeste_jl_amd import cabi, resid
    f = resid.load_library()
    dp, ip = cabi.c_double_p, cabi.c_int32_p
    p = resid._ptr
    vp = np.zeros((2, 44))
    psf = np.zeros((5, 2, 6))
    img = np.array([0], dtype=np.int32)
    frames = np.full(2, -7, dtype=np.int64).repeat(6)
    cand = np.full(64, -7.0)
    nf, st = C.c_int64(-7), C.c_int32(-7)
    good = resid.OptsT(5.0, 0.8, 8, 2, p(psf, dp))
    no_psf = resid.OptsT(5.0, 0.8, 8, 2, None)
    wide = resid.OptsT(5.0, 0.8, 13, 2, p(psf, dp))

    def search(ctx, vp_, n, im, o, fr, ca, mx, nf_, st_):
        return f.celeste_resid_search(ctx, vp_, n, im, None if o is None else C.byref(o), fr, ca, mx, nf_, st_)
    F, Cn = frames.ctypes.data, cand.ctypes.data
    for args in ((None, p(vp, dp), 1, p(img, ip), good, F, Cn, 1, C.byref(nf), C.byref(st)),         # no context
                 (None, None, 1, p(img, ip), good, F, Cn, 1, C.byref(nf), C.byref(st)),
                 (None, p(vp, dp), 1, p(img, ip), None, F, Cn, 1, C.byref(nf), C.byref(st)),
                 (None, p(vp, dp), 1, p(img, ip), no_psf, F, Cn, 1, C.byref(nf), C.byref(st)),
                 (None, p(vp, dp), 1, p(img, ip), wide, F, Cn, 1, C.byref(nf), C.byref(st)),         # radius > 12
                 (None, p(vp, dp), 1, p(img, ip), good, F, Cn, -1, C.byref(nf), C.byref(st)),        # max_candidates < 0
                 (None, p(vp, dp), 1, p(img, ip), good, None, Cn, 1, C.byref(nf), C.byref(st)),
                 (None, p(vp, dp), 1, p(img, ip), good, F, None, 1, C.byref(nf), C.byref(st)),
                 (None, p(vp, dp), 1, p(img, ip), good, F, Cn, 1, None, C.byref(st)),
                 (None, p(vp, dp), 1, p(img, ip), good, F, Cn, 1, C.byref(nf), None)):
        assert search(*args) == cabi.ERR_INVALID_ARG
    out = np.full(4, -7.0)
    assert f.celeste_resid_get_map(None, 0, resid.Z, p(out, dp)) == cabi.ERR_INVALID_ARG          # (and before any search)
    assert f.celeste_resid_sample(None, 1, p(img, ip), p(img, ip), p(img, ip), p(out, dp), p(out, dp), p(out, dp)) == cabi.ERR_INVALID_ARG
    assert f.celeste_resid_last_ms(None, (C.c_float * 4)()) == cabi.ERR_INVALID_ARG
    assert f.celeste_resid_ctx_create(None, 0, None) == cabi.ERR_INVALID_ARG
    h = C.c_void_p(1234)
    assert f.celeste_resid_ctx_create(None, 0, C.byref(h)) == cabi.ERR_INVALID_ARG and not h.value
    f.celeste_resid_ctx_destroy(None)
    z = np.zeros(12)
    for args in ((0, 3, 4, None, None, None, Cn, 1, C.byref(nf), C.byref(st)),
                 (0, 0, 4, p(z, dp), None, None, Cn, 1, C.byref(nf), C.byref(st)),
                 (0, 3, 0, p(z, dp), None, None, Cn, 1, C.byref(nf), C.byref(st)),
                 (0, 3, 4, p(z, dp), None, None, Cn, -1, C.byref(nf), C.byref(st)),
                 (0, 3, 4, p(z, dp), None, None, None, 1, C.byref(nf), C.byref(st)),
                 (0, 3, 4, p(z, dp), None, None, Cn, 1, None, C.byref(st)),
                 (0, 3, 4, p(z, dp), None, None, Cn, 1, C.byref(nf), None)):
        assert f.celeste_resid_find_peaks(*args) == cabi.ERR_INVALID_ARG
    assert (frames == -7).all() and (cand == -7).all() and (out == -7).all() and nf.value == -7 and st.value == -7


def test_no_device_no_fallback(lib):
    """without a device the context and the peak search refuse with NO_DEVICE (there is no CPU path); on a GPU machine both run"""
    import torch
    from celeste_jl_amd import cabi, resid, synthetic
    f = synthetic.make_sample_dataset("two_body", seed=1)
    pr = cabi.Problem(f.images, f.patches, f.neighbors)
    z = np.zeros((3, 4))
    z[1, 2] = 7.0
    if torch.cuda.is_available():
        resid.ResidContext(pr).close()
        c, n, st = resid.find_peaks(z)
        assert n == 1 and st == 0 and (c["h"][0], c["w"][0]) == (1, 2)
    else:
        with pytest.raises(RuntimeError, match="no HIP device") as e:
            resid.ResidContext(pr)
        assert "status %d" % cabi.ERR_NO_DEVICE in str(e.value)
        with pytest.raises(RuntimeError, match="no HIP device"):
            resid.find_peaks(z)


def test_the_defaults_do_not_import_resid_and_return_what_they_returned():
    """infer_box and celeste_to_rows with their defaults: the module is not loaded, the rows are the rows"""
    code = r"""
import sys, inspect
import numpy as np
import celeste_jl_amd as cel
from celeste_jl_amd import catalog, infer, synthetic
assert inspect.signature(cel.infer_box).parameters["refine"].default == 0
assert inspect.signature(catalog.celeste_to_rows).parameters["refined"].default is False
f = synthetic.make_sample_dataset("two_body", seed=1)
assert cel.infer_box(f.images, cel.BoundingBox(-9.0, -8.0, -9.0, -8.0), f.catalog) == []          # no target in the box
assert cel.infer_box(f.images, cel.BoundingBox(-9.0, -8.0, -9.0, -8.0), f.catalog, refine=2) == []
res = [cel.OptimizedSource(1.0, 2.0, f.vp[0].copy(), False), cel.OptimizedSource(3.0, 4.0, f.vp[1].copy(), True),
       cel.OptimizedSource(5.0, 6.0, f.vp[1].copy(), False, refined=1)]
assert res[0].refined is None
rows = catalog.celeste_to_rows(res)
assert rows == [catalog.variational_parameters_to_row(f.vp[0]), catalog.variational_parameters_to_row(f.vp[1])]
assert "refine_round" not in rows[0]
d = catalog.celeste_to_rows(res, refined=True)
assert [r["refine_round"] for r in d] == [None, 1]
assert [{k: v for k, v in r.items() if k != "refine_round"} for r in d] == rows
try:
    cel.infer_box(f.images, cel.BoundingBox(0.0, 30.0, 0.0, 30.0), f.catalog, method="mcmc", refine=1)
except ValueError as e:
    assert "mcmc" in str(e)
else:
    raise AssertionError("method='mcmc' with refine=1 must raise")
assert "celeste_jl_amd.resid" not in sys.modules
print("ok")
"""
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


# ---- the restatement against properties that do not depend on it -------------------------------------------------------------
def _psf():
    """a mixture that is neither centred nor symmetric: phi(dh, dw) != phi(dw, dh)"""
    from celeste_jl_amd.model import make_psf
    return make_psf([0.7, 0.3], [(0.3, -0.2), (-0.4, 0.5)],
                    [np.array([[2.2, 0.6], [0.6, 1.1]]), np.array([[5.0, -1.0], [-1.0, 7.5]])])


def _flat_frame(H, W):
    rng = np.random.Generator(np.random.PCG64(3))
    iota = (900.0 + 50.0 * rng.random(H)).astype(np.float32)
    lam = iota.astype(np.float64)[:, None] * (0.15 + 0.02 * rng.random((H, W)))
    return iota, lam


@pytest.mark.parametrize("nan_block", [False, True])
def test_a_noise_free_point_source_comes_back_exactly(nan_block):
    """x = lam + iota f0 phi(. - p0) gives N = f0 D at p0 whatever taps are masked: f(p0) = f0 and z(p0) = f0 sqrt(D(p0)) to 1e-12
    (relative); a NaN block inside the window only changes D and cov"""
    import resid_reference as RR
    R, H, W, f0, p0 = 8, 41, 37, 3.7, (19, 17)
    iota, lam = _flat_frame(H, W)
    phi = RR.phi_taps(_psf(), R)
    assert abs(phi - phi.T).max() > 1e-3 * phi.max()
    x = lam.copy()
    for dh in range(-R, R + 1):
        for dw in range(-R, R + 1):
            x[p0[0] + dh, p0[1] + dw] += float(iota[p0[0] + dh]) * f0 * phi[dh + R, dw + R]
    clean = RR.filter_maps(x, lam, iota, phi)
    if nan_block:
        x[p0[0] + 3:p0[0] + 6, p0[1] - 6:p0[1] - 3] = np.nan
    mp = RR.filter_maps(x, lam, iota, phi)
    f = mp.N[p0] / mp.D[p0]
    print("f / f0 - 1 = %.3e, z / (f0 sqrt D) - 1 = %.3e, cov = %.6f" % (f / f0 - 1, mp.z[p0] / (f0 * math.sqrt(mp.D[p0])) - 1, mp.cov[p0]))
    assert abs(f / f0 - 1) <= 1e-12 and abs(mp.z[p0] / (f0 * math.sqrt(mp.D[p0])) - 1) <= 1e-12
    if nan_block:
        assert 0.8 <= mp.cov[p0] < 1 and mp.D[p0] < clean.D[p0]
    else:
        assert mp.cov[p0] == 1.0
        assert (mp.cov[R:H - R, R:W - R] == 1.0).all() and (mp.cov[:R] < 1).all() and (mp.cov[:, W - R:] < 1).all()
    pk = RR.find_peaks(mp.z, 5.0)
    assert [(h, w) for h, w, _, _ in pk] == [p0]


def test_a_plateau_yields_its_lowest_raster_index():
    import resid_reference as RR
    z = np.zeros((9, 8))
    z[3:6, 2:5] = 7.0                      # a 3 x 3 plateau: raster index h + 9 w is lowest at (3, 2)
    z[7, 6] = 5.0                          # threshold equality counts
    z[0, 7] = 6.0                          # a corner
    z[1, 7] = np.nan
    pk = RR.find_peaks(z, 5.0)
    assert [(h, w) for h, w, _, _ in pk] == [(3, 2), (7, 6), (0, 7)]
    assert pk[0][2:] == (0.0, 0.0) or all(abs(v) <= 0.5 for v in pk[0][2:])
    assert pk[2][2:] == (0.0, 0.0)         # a neighbour is missing on both axes
    # the sub-pixel step: a parabola through (-1, 4), (0, 6), (1, 5) peaks at 0.5 (4 - 5) / (4 - 12 + 5) = 1 / 6
    assert abs(RR.subpixel(4.0, 6.0, 5.0) - 1.0 / 6.0) <= 1e-15 and RR.subpixel(6.0, 6.0, 6.0) == 0.0
    assert RR.subpixel(5.0, 5.0, 1.0) == -0.5 and RR.subpixel(6.0, 5.0, 1.0) == -0.5 and RR.subpixel(1.0, 5.0, 6.0) == 0.5   # (the last two clamped)
    assert RR.subpixel(None, 5.0, 1.0) == 0.0 and RR.subpixel(np.nan, 5.0, 1.0) == 0.0 and RR.subpixel(6.0, 5.0, 6.0) == 0.0


def test_z_is_a_standard_score_on_poisson_pixels_drawn_from_the_model():
    """On x ~ Poisson(lam), Var N = sum phi^2 iota^2 / lam = D exactly, so z has mean 0 and variance 1.  z is correlated over the
    window: with rho(d) = sum_t phi(t) phi(t + d) / sum phi^2 (lam is nearly flat here), the mean of n values has variance
    (1 / n) sum_d rho(d) and their sample variance (2 / n) sum_d rho(d)^2 (Gaussian field; the Poisson excess is of order 1 / lam =
    0.7 %).  Both within 5 such standard errors."""
    import resid_reference as RR
    R, H, W = 8, 200, 200
    iota, lam = _flat_frame(H, W)
    phi = RR.phi_taps(_psf(), R)
    x = np.random.Generator(np.random.PCG64(20261020)).poisson(lam).astype(np.float64)
    mp = RR.filter_maps(x, lam, iota, phi)
    z = mp.z[R:H - R, R:W - R]
    assert np.isfinite(z).all()
    T = 2 * R + 1
    pad = np.zeros((3 * T, 3 * T))
    pad[T:2 * T, T:2 * T] = phi
    rho = np.array([[(pad[T:2 * T, T:2 * T] * pad[T + a:2 * T + a, T + b:2 * T + b]).sum() for b in range(-T + 1, T)]
                    for a in range(-T + 1, T)]) / (phi * phi).sum()
    n = z.size
    se_mean, se_var = math.sqrt(rho.sum() / n), math.sqrt(2 * (rho * rho).sum() / n)
    print("mean z = %.4f (5 se = %.4f), var z - 1 = %.4f (5 se = %.4f), n = %d" % (z.mean(), 5 * se_mean, z.var() - 1, 5 * se_var, n))
    assert abs(z.mean()) <= 5 * se_mean and abs(z.var() - 1) <= 5 * se_var


# ---- missed_sources ------------------------------------------------------------------------------------------------------------
class _StubSearch:
    """what missed_sources asks of a search, over hand-made maps"""

    def __init__(self, images, candidates, maps, min_coverage=0.8):
        self.images, self.candidates, self.maps, self.min_coverage = list(range(len(images))), candidates, maps, min_coverage

    def sample(self, image, h, w):
        return tuple(np.array([self.maps[int(n)][k][hh, ww] for n, hh, ww in zip(image, h, w)]) for k in range(3))


def test_missed_sources_drops_catalog_neighbours_and_joins_bands():
    import resid_reference as RR
    from celeste_jl_amd import resid, synthetic
    images = synthetic.blank_images(40, 50)              # world = 1-based pixel coordinates in every image
    images += synthetic.blank_images(40, 50)[2:3]        # a second r-band image
    rng = np.random.Generator(np.random.PCG64(5))
    maps = [(rng.normal(size=(40, 50)), 1.0 + rng.random((40, 50)), np.ones((40, 50))) for _ in images]
    maps[5][2][20, 25] = 0.5                             # the second r image does not cover the object
    cand = np.zeros(4, dtype=resid.CANDIDATE_DTYPE)
    for k, (n, h, w, dh, dw) in enumerate([(0, 10, 10, 0.0, 0.0), (0, 20, 25, 0.1, -0.2), (1, 20, 25, -0.3, 0.2), (2, 21, 25, -0.4, 0.1)]):
        cand[k] = (n, h, w, 0, dh, dw, 6.0, 1.0, 1.0, 1.0)
    catalog = [synthetic.sample_ce([11.9, 12.2], True)]   # 1-based (11.9, 12.2): 1.5 px from the candidate at 0-based (10, 10)
    table, entries = resid.missed_sources(_StubSearch(images, cand, maps), images, catalog, min_sep_px=2.0)
    assert len(table) == len(entries) == 1 and table["n_detections"][0] == 3
    assert np.allclose([table["ra"][0], table["dec"][0]], [21.1, 25.8])        # the first image's detection: 1-based (20 + 1 + 0.1, 25 + 1 - 0.2)
    s = [m[k][20, 25] for m in maps for k in range(3)]
    f, z = RR.band_sums([im.b for im in images], s[0::3], s[1::3], s[2::3], 0.8)
    assert np.array_equal(table["flux"][0], f) and np.array_equal(table["z"][0], z) and np.isfinite(f).all()
    assert f[2] == maps[2][0][20, 25] / maps[2][1][20, 25] and table["n_images"][0].tolist() == [1, 1, 1, 1, 1]
    e = entries[0]
    assert e.is_star and np.array_equal(e.star_fluxes, np.maximum(f, resid.DEFAULT_FLUX_FLOOR_NMGY)) and np.array_equal(e.pos, [table["ra"][0], table["dec"][0]])
    # with the catalog source moved away the first candidate stays: two objects
    table2, _ = resid.missed_sources(_StubSearch(images, cand, maps), images, [synthetic.sample_ce([30.0, 40.0], True)])
    assert len(table2) == 2 and table2["n_detections"].tolist() == [1, 3]
