"""The stack of the resid library without a GPU: its structures against the header (laid out by the C compiler), the refusals
that come back before any device is touched, the defaults that load nothing, and the numpy restatement
(tests/stack_reference.py) against properties that do not depend on it: its tangent plane against 50-digit arithmetic, a
one-band channel over one aligned image, noise-free point sources, the standard score on Poisson frames, cells off every
image; resid.grid_covering and resid.stacked_sources against their restatements on hand-made inputs."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_structures_are_laid_out_as_the_header_lays_them_out(lib, tmp_path):
    from celeste_jl_amd import resid
    names = ["celeste_resid_wcs_t", "celeste_resid_grid_t", "celeste_resid_stack_opts_t", "celeste_resid_stack_frame_t",
             "celeste_resid_stack_candidate_t"]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "celeste_resid.h"\nint main(void) {\n' +
                   "".join('printf("%%zu\\n", sizeof(%s));\n' % n for n in names) +
                   'printf("%zu %zu %zu\\n", offsetof(celeste_resid_grid_t, wcs), offsetof(celeste_resid_stack_candidate_t, dh), '
                   'offsetof(celeste_resid_stack_candidate_t, world));\n'
                   'printf("%d %d %d\\n", CELESTE_RESID_ABI_VERSION, CELESTE_RESID_STACK_MAX_CHANNELS, CELESTE_RESID_STACK_COUNT);\n'
                   "return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert [int(x) for x in out[:5]] == [C.sizeof(resid.WcsT), C.sizeof(resid.GridT), C.sizeof(resid.StackOptsT),
                                         resid.STACK_FRAME_DTYPE.itemsize, resid.STACK_CANDIDATE_DTYPE.itemsize] == [72, 80, 16, 32, 72]
    assert [int(x) for x in out[5].split()] == [resid.GridT.wcs.offset, resid.STACK_CANDIDATE_DTYPE.fields["dh"][1],
                                                resid.STACK_CANDIDATE_DTYPE.fields["world"][1]] == [8, 16, 56]
    assert [int(x) for x in out[6].split()] == [resid.ABI_VERSION, resid.STACK_MAX_CHANNELS, resid.STACK_COUNT] == [101, 8, 3]
    o = resid.StackOptsT()
    resid.load_library().celeste_resid_stack_opts_default(C.byref(o))
    assert (o.threshold, o.min_images) == (5.0, 1)


def _wcs(kind=0, world0=(0.0, 0.0), pix0=(0.0, 0.0), m=(1.0, 0.0, 0.0, 1.0)):
    from celeste_jl_amd import resid
    w = resid.WcsT()
    w.kind = kind
    w.world0[:], w.pix0[:], w.m[:] = world0, pix0, m
    return w


def test_wcs_check_and_the_refusals_before_any_device(lib):
    from celeste_jl_amd import cabi, resid
    f = resid.load_library()
    chk = lambda *ws: f.celeste_resid_wcs_check(len(ws), (resid.WcsT * max(len(ws), 1))(*ws))
    tan = dict(kind=1, world0=(10.0, 60.0), pix0=(5.0, 5.0), m=(0.0, 1e-4, 1e-4, 0.0))
    assert chk(_wcs()) == 0 and chk(_wcs(**tan)) == 0 and chk(_wcs(), _wcs(**tan)) == 0
    assert f.celeste_resid_wcs_check(0, (resid.WcsT * 1)()) == cabi.ERR_INVALID_ARG and f.celeste_resid_wcs_check(1, None) == cabi.ERR_INVALID_ARG
    bad = [_wcs(kind=2), _wcs(m=(1.0, 2.0, 2.0, 4.0)), _wcs(m=(0.0, 0.0, 0.0, 0.0)), _wcs(world0=(math.nan, 0.0)),
           _wcs(pix0=(0.0, math.inf)), _wcs(m=(1.0, math.nan, 0.0, 1.0)), _wcs(**dict(tan, world0=(10.0, 90.5))),
           _wcs(**dict(tan, world0=(10.0, -91.0))), _wcs(**dict(tan, m=(1e-4, 1e-4, 1e-4, 1e-4))), _wcs(m=(1e200, 0.0, 0.0, 1e200))]
    for w in bad:
        assert chk(w) == cabi.ERR_INVALID_ARG and chk(_wcs(), w) == cabi.ERR_INVALID_ARG
    assert chk(_wcs(**dict(tan, world0=(10.0, 90.0)))) == 0
    # without a context every call is INVALID_ARG (not NO_DEVICE, not a HIP error), and nothing is written
    g = resid.GridT()
    g.H, g.W, g.wcs = 4, 4, _wcs()
    wts = np.ones(5)
    frames, cand = np.full(8, -7.0), np.full(16, -7.0)
    nf, st = C.c_int64(-7), C.c_int32(-7)
    o = resid.StackOptsT(5.0, 1, 0)
    ws = (resid.WcsT * 1)(_wcs())
    assert f.celeste_resid_stack(None, C.byref(g), 1, ws, 1, resid._ptr(wts, cabi.c_double_p), C.byref(o), frames.ctypes.data,
                                 cand.ctypes.data, 1, C.byref(nf), C.byref(st)) == cabi.ERR_INVALID_ARG
    out = np.full(16, -7.0)
    assert f.celeste_resid_stack_get_map(None, 0, resid.STACK_Z, resid._ptr(out, cabi.c_double_p)) == cabi.ERR_INVALID_ARG
    assert f.celeste_resid_stack_last_ms(None, (C.c_float * 2)()) == cabi.ERR_INVALID_ARG
    f.celeste_resid_stack_opts_default(None)
    assert (frames == -7).all() and (cand == -7).all() and (out == -7).all() and (nf.value, st.value) == (-7, -7)


def test_no_device_no_stack(lib):
    """there is no CPU path: without a device no context exists to stack on"""
    import torch
    from celeste_jl_amd import cabi, resid, synthetic
    if torch.cuda.is_available():
        return
    f = synthetic.make_sample_dataset("two_body", seed=1)
    with pytest.raises(RuntimeError, match="no HIP device") as e:
        resid.ResidContext(cabi.Problem(f.images, f.patches, f.neighbors))
    assert "status %d" % cabi.ERR_NO_DEVICE in str(e.value)


def test_the_defaults_do_not_import_resid_and_refine_stack_needs_refine():
    code = r"""
import sys, inspect
import celeste_jl_amd as cel
from celeste_jl_amd import synthetic
assert inspect.signature(cel.infer_box).parameters["refine_stack"].default is False
f = synthetic.make_sample_dataset("two_body", seed=1)
assert cel.infer_box(f.images, cel.BoundingBox(-9.0, -8.0, -9.0, -8.0), f.catalog) == []
assert cel.infer_box(f.images, cel.BoundingBox(-9.0, -8.0, -9.0, -8.0), f.catalog, refine=1, refine_stack=True) == []
try:
    cel.infer_box(f.images, cel.BoundingBox(0.0, 30.0, 0.0, 30.0), f.catalog, refine_stack=True)
except ValueError as e:
    assert "refine" in str(e)
else:
    raise AssertionError("refine_stack=True with refine=0 must raise")
assert "celeste_jl_amd.resid" not in sys.modules
print("ok")
"""
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


# ---- the restatement's tangent plane against 50 digits ---------------------------------------------------------------------------
def test_the_restated_tangent_plane_against_mpmath():
    import mp_wcs
    import stack_reference as SR
    import wcs_scene
    rng = np.random.Generator(np.random.PCG64(4))
    th = math.radians(30.0)
    s = wcs_scene.SCALE
    cd = np.array([[s * math.cos(th), -s * math.sin(th)], [-s * math.sin(th), -s * math.cos(th)]])     # turned, parity flipped
    crval, crpix = (359.9995, 60.0), (700.3, 1024.1)
    w, ref = SR.Wcs(SR.TAN, crval, crpix, cd), mp_wcs.MpTan(crval, crpix, cd)
    worst_px = worst_deg = 0.0
    for _ in range(40):
        h, v = rng.uniform(1, 1489), rng.uniform(1, 2048)
        ra, dec = w.pix_to_world(h, v)
        mra, mdec = ref.pix_to_world(h, v)
        worst_deg = max(worst_deg, abs(float(mp_wcs._m(float(ra)) - mra)), abs(float(mp_wcs._m(float(dec)) - mdec)))
        p = w.world_to_pix(float(ra), float(dec))
        worst_px = max(worst_px, mp_wcs.pix_error((float(p[0]), float(p[1])), ref.world_to_pix(float(ra), float(dec))))
    print("restated TAN against mpmath: %.3e px (bound %.2e), %.3e degrees (bound %.2e)" % (worst_px, wcs_scene.BOUND_PX, worst_deg, wcs_scene.BOUND_DEG))
    assert worst_px <= wcs_scene.BOUND_PX and worst_deg <= wcs_scene.BOUND_DEG
    assert all(np.isnan(x) for x in w.world_to_pix(crval[0] + 180.0, -60.0))                       # behind the plane
    # the affine kind: the adjugate inverse undoes the matrix
    a = SR.Wcs(SR.AFFINE, (3.0, -2.0), (10.0, 20.0), np.array([[0.8, -0.6], [0.6, 0.8]]))
    p = a.world_to_pix(*a.pix_to_world(17.25, 4.5))
    assert abs(p[0] - 17.25) <= 1e-13 and abs(p[1] - 4.5) <= 1e-13
    assert a.world_to_pix(4.0, -2.0) == (10.8, 20.6)                                               # pix = J (world - world0) + pix0


# ---- the restatement against properties that do not depend on it ---------------------------------------------------------------
def _psf():
    from celeste_jl_amd.model import make_psf
    return make_psf([0.7, 0.3], [(0.3, -0.2), (-0.4, 0.5)],
                    [np.array([[2.2, 0.6], [0.6, 1.1]]), np.array([[5.0, -1.0], [-1.0, 7.5]])])


def _frame(H, W, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    iota = (900.0 + 50.0 * rng.random(H)).astype(np.float32)
    lam = iota.astype(np.float64)[:, None] * (0.15 + 0.02 * rng.random((H, W)))
    return iota, lam


def _ident(shift=(0.0, 0.0)):
    import stack_reference as SR
    return SR.Wcs(SR.AFFINE, shift, (0.0, 0.0), np.eye(2))


def test_a_one_band_channel_over_one_aligned_image_is_that_image_and_off_image_cells_are_empty():
    import resid_reference as RR
    import stack_reference as SR
    H, W = 31, 27
    iota, lam = _frame(H, W, 3)
    x = np.random.Generator(np.random.PCG64(8)).poisson(lam).astype(np.float64)
    x[4, 5] = np.nan
    mp = RR.filter_maps(x, lam, iota, RR.phi_taps(_psf(), 8))
    maps = {0: (mp.N, mp.D, mp.z), 1: (mp.N + 1.0, mp.D, mp.z)}
    st = SR.Stack(maps, [0, 1], {0: 3, 1: 4}, {0: _ident(), 1: _ident()}, SR.Grid(H, W, _ident()), weights=[[0, 0, 1, 0, 0]])
    seen = ~np.isnan(mp.z)
    assert np.array_equal(st.z[0], mp.z, equal_nan=True) and np.array_equal(st.N[0][seen], mp.N[seen]) and np.array_equal(st.D[0][seen], mp.D[seen])
    assert np.array_equal(st.cnt[0], seen.astype(np.int32)) and (st.N[0][~seen] == 0).all() and seen.any() and (~seen).any()
    # a grid that reaches 6 cells past the frame on every side: cells outside every image are NaN with count 0
    big = SR.Grid(H + 12, W + 12, _ident().shifted(-6.0, -6.0))
    st = SR.Stack(maps, [0, 1], {0: 3, 1: 4}, {0: _ident(), 1: _ident()}, big)
    inside = np.zeros((H + 12, W + 12), dtype=bool)
    inside[6:6 + H, 6:6 + W] = True
    assert (st.cnt[0][~inside] == 0).all() and np.isnan(st.z[0][~inside]).all() and np.isnan(st.f[0][~inside]).all()
    assert np.array_equal(st.cnt[0][inside].reshape(H, W), 2 * seen) and st.frames[0][0] == int(seen.sum())
    # min_images above what a cell has empties it
    st3 = SR.Stack(maps, [0, 1], {0: 3, 1: 4}, {0: _ident(), 1: _ident()}, big, min_images=3)
    assert np.isnan(st3.z).all() and st3.frames[0] == (0,) + st3.frames[0][1:] and np.isnan(st3.frames[0][1])


@pytest.mark.parametrize("weights", [[1, 1, 1, 1, 1], [0.5, 2.0, 1.0, 0.25, 3.0]])
def test_noise_free_point_sources_in_aligned_frames_come_back_exactly(weights):
    """x_i = lam_i + iota_i (s_i f0) phi_i(. - p0): N_i = s_i f0 D_i at p0, so the channel with weights s has N = f0 sum s_i^2 D_i:
    f = f0 to 1e-12 and z = f0 sqrt(sum s_i^2 D_i)"""
    import resid_reference as RR
    import stack_reference as SR
    from celeste_jl_amd.synthetic import band_psf
    R, H, W, f0, p0 = 8, 41, 37, 0.37, (19, 17)
    maps, bands, wcs, want_D = {}, {}, {}, 0.0
    for i in range(5):
        iota, lam = _frame(H, W, 10 + i)
        phi = RR.phi_taps(_psf() if i % 2 else band_psf(i), R)
        x = lam.copy()
        for dh in range(-R, R + 1):
            for dw in range(-R, R + 1):
                x[p0[0] + dh, p0[1] + dw] += float(iota[p0[0] + dh]) * (weights[i] * f0) * phi[dh + R, dw + R]
        mp = RR.filter_maps(x, lam, iota, phi)
        maps[i], bands[i], wcs[i] = (mp.N, mp.D, mp.z), i + 1, _ident()
        want_D += weights[i] ** 2 * mp.D[p0]
    st = SR.Stack(maps, list(range(5)), bands, wcs, SR.Grid(H, W, _ident()), weights=[weights])
    print("f / f0 - 1 = %.3e, z / (f0 sqrt(sum D)) - 1 = %.3e" % (st.f[0][p0] / f0 - 1, st.z[0][p0] / (f0 * math.sqrt(want_D)) - 1))
    assert abs(st.f[0][p0] / f0 - 1) <= 1e-12 and abs(st.z[0][p0] / (f0 * math.sqrt(want_D)) - 1) <= 1e-12 and st.cnt[0][p0] == 5
    assert [(int(c["h"]), int(c["w"])) for c in st.candidates] == [p0] and st.candidates["n_images"][0] == 5


def test_the_stacked_z_is_a_standard_score_on_independent_poisson_frames():
    """K independent frames drawn from their models: Var N = D in each, so the stacked z has mean 0 and variance 1.  Its
    correlation over the window is the D-weighted mean of the frames' (one PSF here: the single frame's rho); the standard
    errors as tests/test_resid_host.py corrects them."""
    import resid_reference as RR
    import stack_reference as SR
    R, H, W, K = 8, 200, 200, 4
    phi = RR.phi_taps(_psf(), R)
    maps = {}
    for i in range(K):
        iota, lam = _frame(H, W, 30 + i)
        x = np.random.Generator(np.random.PCG64([20261020, i])).poisson(lam).astype(np.float64)
        mp = RR.filter_maps(x, lam, iota, phi)
        maps[i] = (mp.N, mp.D, mp.z)
    st = SR.Stack(maps, list(range(K)), {i: 1 + i % 5 for i in range(K)}, {i: _ident() for i in range(K)}, SR.Grid(H, W, _ident()),
                  weights=[[1.0, 0.5, 2.0, 1.5, 1.0]])
    z = st.z[0][R:H - R, R:W - R]
    assert np.isfinite(z).all() and (st.cnt[0][R:H - R, R:W - R] == K).all()
    T = 2 * R + 1
    pad = np.zeros((3 * T, 3 * T))
    pad[T:2 * T, T:2 * T] = phi
    rho = np.array([[(pad[T:2 * T, T:2 * T] * pad[T + a:2 * T + a, T + b:2 * T + b]).sum() for b in range(-T + 1, T)]
                    for a in range(-T + 1, T)]) / (phi * phi).sum()
    n = z.size
    se_mean, se_var = math.sqrt(rho.sum() / n), math.sqrt(2 * (rho * rho).sum() / n)
    print("stacked: mean z = %.4f (5 se = %.4f), var z - 1 = %.4f (5 se = %.4f), n = %d" % (z.mean(), 5 * se_mean, z.var() - 1, 5 * se_var, n))
    assert abs(z.mean()) <= 5 * se_mean and abs(z.var() - 1) <= 5 * se_var


# ---- grid_covering and stacked_sources ---------------------------------------------------------------------------------------
def _same_grid(g, r):
    return (g.H, g.W, g.wcs.kind, list(g.wcs.world0), list(g.wcs.pix0)) == (r.H, r.W, r.wcs.kind, r.wcs.w0, r.wcs.p0)


def test_grid_covering_against_its_restatement():
    import stack_reference as SR
    import wcs_scene
    import celeste_jl_amd as cel
    from celeste_jl_amd import resid, synthetic
    images = synthetic.blank_images(37, 41)
    images[4] = synthetic.blank_images(13, 9)[4]
    images[4].wcs_world0 = np.array([30.0, 38.0])            # reaches past the others' corner
    g = resid.grid_covering(images, [0, 4])
    assert (g.H, g.W) == (43, 47) and list(g.wcs.pix0) == [0.0, 0.0] and _same_grid(g, SR.grid_covering(images, [0, 4]))
    g = resid.grid_covering(images, [4, 0])                  # on the small image's plane: the others start 30, 38 cells before it
    assert (g.H, g.W) == (43, 47) and list(g.wcs.pix0) == [30.0, 38.0] and _same_grid(g, SR.grid_covering(images, [4, 0]))
    box = cel.BoundingBox(10.2, 20.4, 5.0, 100.0)
    g = resid.grid_covering(images, [0, 1], box)
    assert (g.H, g.W) == (11, 37) and list(g.wcs.pix0) == [-9.0, -4.0] and _same_grid(g, SR.grid_covering(images, [0, 1], box))
    with pytest.raises(ValueError):
        resid.grid_covering(images, [0], cel.BoundingBox(100.0, 120.0, 0.0, 10.0))
    with pytest.raises(ValueError):
        resid.grid_covering(images, [])
    f = wcs_scene.tan_multifield(perturb=False)
    which = list(range(15))
    g, r = resid.grid_covering(f.images, which), SR.grid_covering(f.images, which)
    assert g.wcs.kind == resid.WCS_TAN and _same_grid(g, r) and list(g.wcs.m) == r.wcs.inv and g.H > 64 and g.W > 80
    # every frame's corners lie on the grid
    for n in which:
        H, W = f.images[n].pixels.shape
        for c in ((1.0, 1.0), (H, 1.0), (1.0, W), (H, W)):
            p = r.wcs.world_to_pix(*SR.Wcs.of_image(f.images[n]).pix_to_world(*c))
            assert 0.5 <= p[0] <= g.H + 0.5 and 0.5 <= p[1] <= g.W + 0.5
    far = [f.images[0], synthetic.blank_images(8, 8)[0]]
    far[1].wcs_world0 = np.array([1e6, 1e6])
    far[0] = synthetic.blank_images(8, 8)[0]
    with pytest.raises(ValueError, match="too large"):
        resid.grid_covering(far, [0, 1])
    far[1].wcs_world0 = np.array([math.nan, 0.0])
    with pytest.raises(ValueError, match="finite"):
        resid.grid_covering(far, [0, 1])


class _Stub:
    pass


def test_stacked_sources_keeps_the_strongest_of_a_group_and_drops_catalog_neighbours():
    import resid_reference as RR
    import stack_reference as SR
    from celeste_jl_amd import resid, synthetic
    images = synthetic.blank_images(40, 50)
    rng = np.random.Generator(np.random.PCG64(5))
    maps = [(rng.normal(size=(40, 50)), 1.0 + rng.random((40, 50)), np.ones((40, 50))) for _ in images]
    search = _Stub()
    search.images, search.min_coverage = list(range(5)), 0.8
    search.sample = lambda image, h, w: tuple(np.array([maps[int(n)][k][hh, ww] for n, hh, ww in zip(image, h, w)]) for k in range(3))
    grid = resid.StackGrid.of_image(images[0])
    cand = np.zeros(5, dtype=resid.STACK_CANDIDATE_DTYPE)
    rows = [(0, 10, 10, 5, 0.0, 0.0, 6.0), (0, 20, 25, 5, 0.1, -0.2, 6.5), (1, 21, 25, 4, -0.3, 0.2, 7.5), (1, 30, 40, 3, 0.0, 0.0, 5.5),
            (2, 31, 41, 5, 0.2, 0.2, 5.5)]
    for k, (ch, h, w, n, dh, dw, z) in enumerate(rows):
        cand[k] = (ch, h, w, n, dh, dw, z, 1.0, 1.0, (h + 1 + dh, w + 1 + dw))
    stack = _Stub()
    stack.candidates, stack.grid = cand, grid
    catalog = [synthetic.sample_ce([11.9, 12.2], True)]      # 1.5 px from the first candidate
    table, entries = resid.stacked_sources(stack, search, images, catalog)
    kept = SR.kept_candidates(cand, SR.Grid.of_image(images[0]), [ce.pos for ce in catalog])
    assert kept == [2, 3]                                     # the strongest of the pair; of the tie, the first in the list
    assert len(entries) == 2 and [tuple(e.pos) for e in entries] == [tuple(cand["world"][i]) for i in kept]
    assert table["n_detections"].tolist() == [4, 3] and all(e.is_star for e in entries)
    s = [m[k][21, 25] for m in maps for k in range(3)]       # rint(21 + 1 - 0.3) - 1 = 21, rint(25 + 1 + 0.2) - 1 = 25
    f, z = RR.band_sums([im.b for im in images], s[0::3], s[1::3], s[2::3], 0.8)
    assert np.array_equal(table["flux"][0], f) and np.array_equal(table["z"][0], z)
    assert np.array_equal(entries[0].star_fluxes, np.maximum(f, resid.DEFAULT_FLUX_FLOOR_NMGY))
    t2, e2 = resid.stacked_sources(stack, search, images, [], min_sep_px=0.5)
    assert len(e2) == 5 and t2["n_detections"].tolist() == [4, 5, 5, 3, 5]
