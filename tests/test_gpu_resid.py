"""Whole-frame residuals on the device (libceleste_resid.so) against the numpy restatement (tests/resid_reference.py): the frame
model within 1e-12 of the plane's maximum (and against the engine's own expected image), the filter maps within 1e-11 of their
sum |term|, the NaN patterns and the candidate lists exactly; the peak rule on hand-made planes; determinism and independence
of the call's other images; the isolation of a non-finite row; the recovery of a source left out of the table, and
infer_box(..., refine=1)."""
import os

import numpy as np
import pytest

import resid_reference as RR

pytestmark = pytest.mark.gpu

LAM_TOL = 1e-12           # of the plane's maximum
MAP_TOL = 1e-11           # of sum |term|
KINDS = ("lam", "N", "D", "z", "coverage")


def _problem(f):
    from celeste_jl_amd import cabi
    return cabi.Problem(f.images, f.patches, f.neighbors)


def _run(f, vp=None, images=None, kinds=KINDS, problem=None, **kw):
    """a search and its maps {image: {kind: plane}}"""
    from celeste_jl_amd import resid
    with resid.ResidContext(problem or _problem(f)) as rc:
        s = rc.search(f.vp if vp is None else vp, images=images, **kw)
        maps = {n: {k: s.map(n, k) for k in kinds} for n in s.images}
    return s, maps


def _same_maps(a, b, images=None):
    return all(np.array_equal(a[n][k], b[n][k], equal_nan=True) for n in (images or a) for k in a[n])


def _compare_lam(f, maps, lam_ref, name):
    worst = 0.0
    for n, ref in lam_ref.items():
        got = maps[n]["lam"]
        assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref)), (name, n)
        ok = ~np.isnan(ref)
        worst = max(worst, float(np.abs(got - ref)[ok].max() / np.abs(ref[ok]).max()))
    print("resid parity %-28s lam %.3e of the plane's maximum (bound %.0e)" % (name, worst, LAM_TOL))
    assert worst <= LAM_TOL, (name, worst)


def _compare_engine(f, maps, name):
    """lam / iota - eps against celeste_render_expected, on the scale of the plane's maximum"""
    import celeste_jl_amd as cel
    ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
    try:
        planes = [ctx.render_expected(f.vp, n) for n in range(len(f.images))]
    finally:
        ctx.close()
    worst = 0.0
    for n, img in enumerate(f.images):
        mine = maps[n]["lam"] / img.nelec_per_nmgy.astype(np.float64)[:, None] - img.sky.astype(np.float64)
        scale = max(np.abs(planes[n]).max(), np.abs(img.sky).max())
        worst = max(worst, float(np.abs(mine - planes[n]).max() / scale))
    print("resid parity %-28s lam / iota - eps against celeste_render_expected %.3e (bound %.0e)" % (name, worst, LAM_TOL))
    assert worst <= LAM_TOL, (name, worst)


def _compare_maps(maps, ref, name):
    """N, D, coverage, z of every image against the restatement's Maps; the NaN patterns exactly"""
    worst = dict(N=0.0, D=0.0, cov=0.0, z=0.0)
    for n, mp in ref.items():
        g = maps[n]
        for k, r in (("N", mp.N), ("D", mp.D), ("coverage", mp.cov), ("z", mp.z)):
            assert np.array_equal(np.isnan(g[k]), np.isnan(r)), (name, n, k)
        if np.isnan(mp.N).all():
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            for k, err, scale in (("N", np.abs(g["N"] - mp.N), mp.abs_N), ("D", np.abs(g["D"] - mp.D), mp.D),
                                  ("cov", np.abs(g["coverage"] - mp.cov), np.ones_like(mp.cov)),
                                  ("z", np.abs(g["z"] - mp.z), mp.abs_N / np.sqrt(mp.D))):
                ok = np.isfinite(err)
                zero = ok & (scale == 0)
                assert (err[zero] == 0).all(), (name, n, k)
                if (ok & ~zero).any():
                    worst[k] = max(worst[k], float((err[ok & ~zero] / scale[ok & ~zero]).max()))
    print("resid parity %-28s N %.3e  D %.3e  cov %.3e  z %.3e of sum|term| (bound %.0e)" %
          (name, worst["N"], worst["D"], worst["cov"], worst["z"], MAP_TOL))
    assert max(worst.values()) <= MAP_TOL, (name, worst)


def _compare_candidates(s, ref, name, maps):
    """the list's (image, h, w) is the restatement's -- the scenes are chosen so that none of the restatement's peaks hangs on
    less than 1e-9 (asserted) -- and the records agree with its maps; the frame summaries: counts and statuses exactly, chi2
    within 1e-10 of itself (its terms are not negative), the z range is that of the device's own map"""
    fragile = sum(len(RR.fragile_peaks(ref.maps[n].z, ref.threshold)) for n in ref.images if not np.isnan(ref.maps[n].z).all())
    assert fragile == 0, (name, fragile)
    got = [(int(c["image"]), int(c["h"]), int(c["w"])) for c in s.candidates]
    want = [(int(c["image"]), int(c["h"]), int(c["w"])) for c in ref.candidates]
    assert got == want and s.n_found == len(want), (name, got, want)
    for c, r in zip(s.candidates, ref.candidates):
        mp = ref.maps[int(r["image"])]
        tol = MAP_TOL * mp.abs_N[r["h"], r["w"]]
        assert abs(c["z"] - r["z"]) <= tol / np.sqrt(r["D"]) and abs(c["f"] - r["f"]) <= 2 * tol / r["D"], (name, c, r)
        assert abs(c["D"] - r["D"]) <= MAP_TOL * r["D"] and abs(c["cov"] - r["cov"]) <= MAP_TOL
        g = maps[int(c["image"])]
        assert c["z"] == g["z"][c["h"], c["w"]] and c["D"] == g["D"][c["h"], c["w"]] and c["cov"] == g["coverage"][c["h"], c["w"]]
        assert abs(c["dh"]) <= 0.5 and abs(c["dw"]) <= 0.5
    for fr in s.frames:
        r = ref.frames[int(fr["image"])]
        assert (fr["status"], fr["n_px"], fr["n_bad"]) == (r["status"], r["n_px"], r["n_bad"]), (name, fr, r)
        if r["status"] == 0:
            assert abs(fr["chi2"] - r["chi2"]) <= 1e-10 * r["chi2"]
            z = maps[int(fr["image"])]["z"]
            if np.isfinite(z).any():
                assert fr["z_max"] == np.nanmax(z) and fr["z_min"] == np.nanmin(z)
            else:
                assert np.isnan(fr["z_max"]) and np.isnan(fr["z_min"])
        else:
            assert np.isnan(fr["chi2"]) and np.isnan(fr["z_max"]) and np.isnan(fr["z_min"])


# ---- the committed fixtures ------------------------------------------------------------------------------------------------
_FIX = {}


def _fixture(name):
    if name not in _FIX:
        import golden_util as G
        _FIX[name] = G.arrays_to_field(np.load(G.path(name)))
    return _FIX[name]


@pytest.mark.parametrize("name", ["sample_star", "sample_galaxy", "sample_two_body", "field_64x80_8src_nan",
                                  "field_72x88_9src_variable"])
def test_frame_model_of_a_fixture_against_the_restatement_and_the_engine(lib, name):
    f = _fixture(name)
    s, maps = _run(f, kinds=("lam",))
    assert (s.frames["status"] == 0).all() and s.frames["image"].tolist() == list(range(5))
    _compare_lam(f, maps, RR.frame_model(f.images, f.patches, f.vp), name)
    _compare_engine(f, maps, name)


# ---- a scene of edge cases ---------------------------------------------------------------------------------------------------
def _asym_psf():
    """neither centred nor symmetric: phi(dh, dw) != phi(dw, dh)"""
    from celeste_jl_amd.model import make_psf
    return make_psf([0.7, 0.3], [(0.3, -0.2), (-0.4, 0.5)],
                    [np.array([[2.2, 0.6], [0.6, 1.1]]), np.array([[5.0, -1.0], [-1.0, 7.5]])])


def _edge_scene():
    """Four 37 x 41 images (no multiple of the 32 x 8 and 32 x 16 tiles) and a fifth of 13 x 9 (smaller than a tile, narrower than
    2 R + 1 at R = 8 and 12), shifted by (20, 10).  Sources 0-2: patches of 9 x 9 = 81 pixels, 0 and 1 in a row so that the last
    column of 0's patch lies inside 1's, 2 clipped by the corner of the frame; 0 is off the fifth image.  Sources 3-5: patches of
    17 x 17 = 289 pixels, three that overlap one another, clipped by the fifth image.  NaN pixels inside and outside patches and
    a NaN block of 3 x 3.  The row calibration varies (iota by row is not iota by column).  After the patches are made, images 1
    and 3 get a filter PSF that is not symmetric (the patches keep theirs: the frame model does not change)."""
    if "edge" not in _FIX:
        from celeste_jl_amd import synthetic
        from celeste_jl_amd.model import get_sky_patches, neighbor_map
        from celeste_jl_amd.params import catalog_init_source
        rng = np.random.Generator(np.random.PCG64(7))
        images = synthetic.blank_images(37, 41)
        images[4] = synthetic.blank_images(13, 9)[4]
        images[4].wcs_world0 = np.array([20.0, 10.0])
        for im in images:
            im.nelec_per_nmgy = (im.nelec_per_nmgy * (1.0 + 0.2 * np.arange(im.H) / im.H)).astype(np.float32)
        small = [synthetic.sample_ce([8.2, 12.3], True), synthetic.sample_ce([8.3, 17.2], False),
                 synthetic.sample_ce([35.3, 38.2], True)]
        large = [synthetic.sample_ce([24.2, 16.3], False), synthetic.sample_ce([27.4, 20.1], True),
                 synthetic.sample_ce([22.3, 22.4], False)]
        catalog = small + large
        synthetic.gen_images(images, catalog, rng)
        for im in images[:4]:
            for h, w in ((7, 12), (25, 18), (1, 39), (36, 0)):
                im.pixels[h, w] = np.nan
            im.pixels[15:18, 30:33] = np.nan
        images[4].pixels[3, 5] = np.nan
        patches = get_sky_patches(images, small, radius_override_pix=4.0) + get_sky_patches(images, large, radius_override_pix=8.0)
        vp = np.stack([catalog_init_source(ce) for ce in catalog])
        for n in (1, 3):
            images[n].psf = _asym_psf()
        _FIX["edge"] = synthetic.Field(images, catalog, patches, neighbor_map(patches), vp, "edge")
        _FIX["edge_lam"] = RR.frame_model(images, patches, vp)
    return _FIX["edge"], _FIX["edge_lam"]


def test_edge_scene_frame_model(lib):
    f, lam = _edge_scene()
    sizes = [[p.active_pixel_bitmap.shape for p in row] for row in f.patches]
    assert sizes[0][0] == (9, 9) and sizes[3][0] == (17, 17) and 0 in sizes[0][4] and 0 not in sizes[3][4]
    assert sizes[2][0] != (9, 9) and 0 not in sizes[2][0] and sizes[3][4] != (17, 17)            # clipped by a frame edge
    assert 1 in f.neighbors[0] and {4, 5} <= set(f.neighbors[3]) and 5 in f.neighbors[4]
    p0, p1 = f.patches[0][0], f.patches[1][0]
    last = p0.bitmap_offset[1] + 8                                       # 0's last column, 0-based: inside 1's patch
    assert p1.bitmap_offset[1] <= last < p1.bitmap_offset[1] + 8
    s, maps = _run(f, kinds=("lam",))
    assert (s.frames["status"] == 0).all() and [m["lam"].shape for m in maps.values()] == [(37, 41)] * 4 + [(13, 9)]
    _compare_lam(f, maps, lam, "edge scene")
    _compare_engine(f, maps, "edge scene")
    # a tile no patch touches holds the sky alone
    img = f.images[0]
    assert np.array_equal(maps[0]["lam"][32:, 0:8], (img.nelec_per_nmgy.astype(np.float64)[:, None] * img.sky.astype(np.float64))[32:, 0:8])


def test_explicit_bitmaps_in_the_frame_model(lib):
    """patches whose bitmaps leave pixels unset that are not NaN reach the library as explicit bitmaps: an ellipse and a disc that
    overlap (the scene of the fit library's bitmap test)"""
    from celeste_jl_amd import synthetic
    from celeste_jl_amd.model import ImagePatch, neighbor_map
    from celeste_jl_amd.params import catalog_init_source
    images = synthetic.blank_images(48, 60)
    catalog = [synthetic.sample_ce([20.2, 20.3], False), synthetic.sample_ce([22.3, 27.2], True)]
    synthetic.gen_images(images, catalog, np.random.Generator(np.random.PCG64(13)))
    boxes = [((16, 24), (14, 26)), ((18, 26), (23, 31))]
    hh, ww = np.arange(1, 49)[:, None], np.arange(1, 61)[None, :]
    masks = [((hh - 20) / 4.6) ** 2 + ((ww - 20) / 6.6) ** 2 <= 1.0, (hh - 22) ** 2 + (ww - 27) ** 2 <= 4.3 ** 2]
    patches = [[ImagePatch.from_box(img, box) for img in images] for box in boxes]
    for row, box, mask in zip(patches, boxes, masks):
        for p in row:
            p.active_pixel_bitmap = p.active_pixel_bitmap & mask[box[0][0] - 1:box[0][1], box[1][0] - 1:box[1][1]]
    assert not patches[0][0].active_pixel_bitmap.all() and not np.isnan(images[0].pixels).any()
    f = synthetic.Field(images, catalog, patches, neighbor_map(patches), np.stack([catalog_init_source(ce) for ce in catalog]), "bitmaps")
    s, maps = _run(f, kinds=("lam",))
    _compare_lam(f, maps, RR.frame_model(f.images, f.patches, f.vp), "explicit bitmaps")
    _compare_engine(f, maps, "explicit bitmaps")
    sky = images[2].nelec_per_nmgy.astype(np.float64)[:, None] * images[2].sky.astype(np.float64)
    assert maps[2]["lam"][15, 13] == sky[15, 13] and maps[2]["lam"][19, 19] > 1.01 * sky[19, 19]   # a corner of 0's box, outside its ellipse; its centre


@pytest.mark.parametrize("radius", [1, 8, 12])
def test_edge_scene_filter_maps(lib, radius):
    f, lam = _edge_scene()
    s, maps = _run(f, radius=radius, threshold=6.0)
    ref = RR.Search(f.images, f.patches, f.vp, threshold=6.0, radius=radius, lam=lam)
    _compare_maps(maps, ref.maps, "edge scene, radius %d" % radius)
    if radius > 1:
        assert 2 * radius + 1 > 9 and np.isnan(ref.maps[4].z).any()            # the small frame: windows hang over every edge
    assert (ref.maps[0].cov[15:18, 30:33] < 1).all()                             # the NaN block
    _compare_candidates(s, ref, "edge scene, radius %d" % radius, maps)


def test_sparse_and_dense_multifield_agree_bit_for_bit(lib):
    from celeste_jl_amd import synthetic
    fs = synthetic.make_multifield((2, 2), 96, 96, 0.10, 30, seed=11, sparse=True)
    fd = synthetic.make_multifield((2, 2), 96, 96, 0.10, 30, seed=11, sparse=False)
    ss, ms = _run(fs, kinds=("lam", "z"))
    sd, md = _run(fd, kinds=("lam", "z"))
    assert len(ms) == 20 and _same_maps(ms, md)
    assert ss.frames.tobytes() == sd.frames.tobytes() and ss.candidates.tobytes() == sd.candidates.tobytes()
    sub = [0, 7, 19]
    _compare_lam(fs, {n: ms[n] for n in sub}, RR.frame_model(fs.images, fs.patches, fs.vp, which=sub), "multifield (sparse)")


# ---- the peak rule on hand-made planes -----------------------------------------------------------------------------------------
def _check_peaks(z, thr, name):
    from celeste_jl_amd import resid
    want = RR.find_peaks(z, thr)
    cov = np.random.Generator(np.random.PCG64(1)).random(z.shape)
    c, n, st = resid.find_peaks(z, cov, threshold=thr, max_candidates=max(len(want), 1))
    assert n == len(want) and st == 0, (name, n, len(want))
    assert [(int(r["h"]), int(r["w"])) for r in c] == [(h, w) for h, w, _, _ in want], name
    if want:
        err = max(max(abs(r["dh"] - w[2]), abs(r["dw"] - w[3])) for r, w in zip(c, want))
        print("peaks %-24s %d candidates, sub-pixel offsets within %.3e (bound 1e-12)" % (name, n, err))
        assert err <= 1e-12
        assert all(r["z"] == z[r["h"], r["w"]] and r["cov"] == cov[r["h"], r["w"]] and np.isnan(r["f"]) and np.isnan(r["D"])
                   and r["image"] == 0 for r in c)
    return want


def test_find_peaks_ties_plateaus_nan_borders_and_overflow(lib):
    from celeste_jl_amd import resid
    z = np.zeros((9, 8))
    z[3:6, 2:5] = 7.0                      # a 3 x 3 plateau
    z[7, 6] = 5.0                          # threshold equality
    z[0, 7] = 6.0                          # a corner, next to a NaN
    z[1, 7] = np.nan
    z[8, 0] = 9.0                          # another corner
    z[8, 3], z[8, 4] = 6.5, 6.5            # a tie of two on the border: the lower raster index (8, 3)
    want = _check_peaks(z, 5.0, "hand-made")
    assert [(h, w) for h, w, _, _ in want] == [(8, 0), (3, 2), (8, 3), (7, 6), (0, 7)]
    # whole numbers with NaNs sprinkled in: ties, plateaus and NaN neighbours everywhere; 1517 pixels are 6 workgroups
    rng = np.random.Generator(np.random.PCG64(2))
    zi = rng.integers(0, 8, (37, 41)).astype(np.float64)
    zi[rng.random(zi.shape) < 0.1] = np.nan
    want = _check_peaks(zi, 5.0, "whole numbers 37 x 41")
    assert len(want) > 40
    # smooth values: the sub-pixel step away from 0 and from its clamp
    zs = 4.0 * rng.random((23, 19)) + 3.0
    want = _check_peaks(zs, 5.0, "uniform 23 x 19")
    assert any(0 < abs(w[2]) < 0.5 for w in want)
    # more than 1024 workgroups: the scan's lanes add runs of counts
    zl = rng.integers(0, 8, (613, 431)).astype(np.float64)
    want = _check_peaks(zl, 7.0, "whole numbers 613 x 431")
    assert 613 * 431 > 1024 * 256 and len(want) > 1000
    # overflow: the first max_candidates of the list, the true count, the status
    full = RR.find_peaks(zi, 5.0)
    c, n, st = resid.find_peaks(zi, threshold=5.0, max_candidates=7)
    assert n == len(full) and st == resid.TRUNCATED and [(int(r["h"]), int(r["w"])) for r in c] == [(h, w) for h, w, _, _ in full[:7]]
    assert np.isnan(c["cov"]).all()
    c, n, st = resid.find_peaks(zi, threshold=5.0, max_candidates=0)
    assert n == len(full) and st == resid.TRUNCATED and len(c) == 0
    c, n, st = resid.find_peaks(zi, threshold=50.0)
    assert n == 0 and st == 0 and len(c) == 0


# ---- determinism -------------------------------------------------------------------------------------------------------------
def test_determinism_and_independence_of_the_other_images(lib):
    from celeste_jl_amd import resid
    f, _ = _edge_scene()
    with resid.ResidContext(_problem(f)) as rc:
        a = rc.search(f.vp, threshold=3.0)
        ma = {n: {k: a.map(n, k) for k in KINDS} for n in a.images}
        b = rc.search(f.vp, threshold=3.0)
        mb = {n: {k: b.map(n, k) for k in KINDS} for n in b.images}
        assert _same_maps(ma, mb) and a.frames.tobytes() == b.frames.tobytes() and a.candidates.tobytes() == b.candidates.tobytes()
        assert len(a.candidates) > 0
        with pytest.raises(RuntimeError):
            a.map(0, "z")                                                # the context has searched again
        c = rc.search(f.vp, images=[1, 3], threshold=3.0)
        mc = {n: {k: c.map(n, k) for k in KINDS} for n in c.images}
        assert c.images == [1, 3] and _same_maps(mc, ma, [1, 3])
        assert c.frames.tobytes() == a.frames[[1, 3]].tobytes()
        assert c.candidates.tobytes() == a.candidates[np.isin(a.candidates["image"], [1, 3])].tobytes()
        # sample reads the same maps
        hh, ww = np.array([0, 12, 36, 40, -1, 5]), np.array([0, 14, 40, 3, 2, 41])
        sN, sD, sc = c.sample([1, 3, 1, 3, 1, 3], hh, ww)
        assert (sN[3:] == 0).all() and (sD[3:] == 0).all() and (sc[3:] == 0).all()        # outside the frame
        for i, n in enumerate([1, 3, 1]):
            masked = np.isnan(ma[n]["z"][hh[i], ww[i]])
            assert sc[i] == ma[n]["coverage"][hh[i], ww[i]]
            assert np.isnan(sN[i]) and np.isnan(sD[i]) if masked else (sN[i] == ma[n]["N"][hh[i], ww[i]] and sD[i] == ma[n]["D"][hh[i], ww[i]])
        assert np.isnan(ma[1]["z"][0, 0]) and np.isfinite(ma[3]["z"][12, 14])
        with pytest.raises(RuntimeError):
            c.sample([0], [1], [1])                                      # image 0 was not in the last search
        ms = rc.last_ms()
        assert len(ms) == 4 and all(x >= 0 for x in ms) and ms[1] > 0 and ms[2] > 0
    old = os.environ.get("CELESTE_CHUNK_PX")
    for chunk in ("64", "256"):
        os.environ["CELESTE_CHUNK_PX"] = chunk
        try:
            s, m = _run(f, threshold=3.0)
            assert _same_maps(m, ma) and s.frames.tobytes() == a.frames.tobytes() and s.candidates.tobytes() == a.candidates.tobytes(), chunk
        finally:
            if old is None:
                del os.environ["CELESTE_CHUNK_PX"]
            else:
                os.environ["CELESTE_CHUNK_PX"] = old


def test_a_non_finite_row_flags_the_frames_it_touches_and_no_others(lib):
    from celeste_jl_amd import cabi
    f, lam = _edge_scene()
    clean, mclean = _run(f, threshold=3.0)
    vp = f.vp.copy()
    vp[0] = np.nan                                                       # source 0 has no patch in the fifth image
    s, m = _run(f, vp=vp, threshold=3.0)
    assert s.frames["status"].tolist() == [cabi.ERR_NONFINITE_INPUT] * 4 + [0] and s.status == cabi.ERR_NONFINITE_INPUT
    for n in range(4):
        assert all(np.isnan(m[n][k]).all() for k in ("N", "D", "z", "coverage")) and np.isnan(s.frames["chi2"][n])
        assert np.isnan(m[n]["lam"]).any() and s.frames["n_bad"][n] > 0 and s.frames["n_px"][n] == clean.frames["n_px"][n]
    assert _same_maps(m, mclean, [4]) and s.frames[4:].tobytes() == clean.frames[4:].tobytes()
    assert not (s.candidates["image"] < 4).any()
    assert s.candidates.tobytes() == clean.candidates[clean.candidates["image"] == 4].tobytes()
    ref = RR.Search(f.images, f.patches, vp, threshold=3.0)
    assert [ref.frames[n]["status"] for n in range(5)] == s.frames["status"].tolist()
    assert [ref.frames[n]["n_bad"] for n in range(5)] == s.frames["n_bad"].tolist()


def test_refusals_with_a_context(lib):
    import ctypes as C
    from celeste_jl_amd import cabi, resid
    f = _fixture("sample_two_body")
    dp, ip = cabi.c_double_p, cabi.c_int32_p
    p = resid._ptr
    with resid.ResidContext(_problem(f)) as rc:
        vp = np.ascontiguousarray(f.vp)
        psf = rc._psf
        frames = np.zeros(5, dtype=resid.FRAME_DTYPE)
        cand = np.zeros(8, dtype=resid.CANDIDATE_DTYPE)
        nf, st = C.c_int64(-7), C.c_int32(-7)
        out = np.full(20 * 23, -7.0)
        assert rc.lib.celeste_resid_get_map(rc.handle, 0, resid.Z, p(out, dp)) == cabi.ERR_INVALID_ARG     # before any search
        one = np.zeros(1, dtype=np.int32)
        assert rc.lib.celeste_resid_sample(rc.handle, 1, p(one, ip), p(one, ip), p(one, ip), p(out, dp), p(out, dp), p(out, dp)) == cabi.ERR_INVALID_ARG

        def search(images, radius=8, mx=8, K=2):
            o = resid.OptsT(5.0, 0.8, radius, K, p(psf, dp))
            ia = None if images is None else np.array(images, dtype=np.int32)
            return rc.lib.celeste_resid_search(rc.handle, p(vp, dp), 0 if images is None else len(images), p(ia, ip), C.byref(o),
                                               frames.ctypes.data, cand.ctypes.data, mx, C.byref(nf), C.byref(st))
        for bad in ([5], [-1], [0, 5], [1, 1]):                           # out of range, listed twice
            assert search(bad) == cabi.ERR_INVALID_ARG
        assert search([0], radius=13) == cabi.ERR_INVALID_ARG and search([0], radius=0) == cabi.ERR_INVALID_ARG
        assert search([0], mx=-1) == cabi.ERR_INVALID_ARG and search([0], K=0) == cabi.ERR_INVALID_ARG
        assert nf.value == -7 and st.value == -7 and (out == -7).all()
        assert search([2]) == 0 and st.value == 0 and nf.value >= 0 and frames["image"][0] == 2
        assert rc.lib.celeste_resid_get_map(rc.handle, 2, resid.Z, p(out, dp)) == 0 and not (out == -7).any()
        for image, which in ((0, resid.Z), (5, resid.Z), (2, 5), (2, -1)):   # not in the last search, out of range, no such map
            assert rc.lib.celeste_resid_get_map(rc.handle, image, which, p(out, dp)) == cabi.ERR_INVALID_ARG
        assert search(None) == 0 and frames["image"].tolist() == [0, 1, 2, 3, 4]
        with pytest.raises(ValueError):
            rc.search(f.vp, images=[5])
        with pytest.raises(ValueError):
            rc.search(f.vp, radius=13)
        with pytest.raises(ValueError):
            rc.search(f.vp, max_candidates=-1)


# ---- recovery ----------------------------------------------------------------------------------------------------------------
SEED, THRESHOLD, OMIT = 2, 6.0, 9          # make_field(160, 170, 12, seed=SEED): the restatement has no peak at 6 with every source in the table


def _recovery():
    """make_field(160, 170, 12, SEED) with every source at its catalog row, and the same with source OMIT left out of the table"""
    if "recovery" not in _FIX:
        from celeste_jl_amd import synthetic
        from celeste_jl_amd.model import neighbor_map
        from celeste_jl_amd.params import catalog_init_source
        f = synthetic.make_field(160, 170, 12, seed=SEED, perturb=False)
        vp = np.stack([catalog_init_source(ce) for ce in f.catalog])
        full = synthetic.Field(f.images, f.catalog, f.patches, f.neighbors, vp, "recovery")
        keep = [i for i in range(12) if i != OMIT]
        patches = [f.patches[i] for i in keep]
        part = synthetic.Field(f.images, [f.catalog[i] for i in keep], patches, neighbor_map(patches), vp[keep], "recovery, one left out")
        _FIX["recovery"] = (full, part, f.catalog[OMIT])
    return _FIX["recovery"]


def test_the_complete_table_is_silent_and_a_source_left_out_is_found(lib):
    from celeste_jl_amd import resid
    full, part, missing = _recovery()
    flux_r = (missing.star_fluxes if missing.is_star else missing.gal_fluxes)[2]
    assert flux_r > 1.0
    ref_full = RR.Search(full.images, full.patches, full.vp, threshold=THRESHOLD)
    assert len(ref_full.candidates) == 0
    s, maps = _run(full, threshold=THRESHOLD)
    _compare_maps(maps, ref_full.maps, "recovery, complete")
    _compare_candidates(s, ref_full, "recovery, complete", maps)
    assert s.n_found == 0 and s.status == 0
    ref = RR.Search(part.images, part.patches, part.vp, threshold=THRESHOLD)
    pc = [img.world_to_pix(missing.pos) - 1.0 for img in part.images]              # 0-based
    near = lambda c: np.hypot(c["h"] + c["dh"] - pc[c["image"]][0], c["w"] + c["dw"] - pc[c["image"]][1]) <= 1.0
    bands_ref = sorted(int(c["image"]) for c in ref.candidates if near(c))
    assert 2 in bands_ref
    with resid.ResidContext(_problem(part)) as rc:
        s = rc.search(part.vp, threshold=THRESHOLD)
        maps = {n: {k: s.map(n, k) for k in KINDS} for n in s.images}
        table, entries = resid.missed_sources(s, part.images, part.catalog)
    _compare_maps(maps, ref.maps, "recovery, one left out")
    _compare_candidates(s, ref, "recovery, one left out", maps)
    assert sorted(int(c["image"]) for c in s.candidates if near(c)) == bands_ref
    print("recovery: r flux %.3f nmgy, candidates in images %s, f = %s" % (flux_r, bands_ref, [round(float(c["f"]), 3) for c in s.candidates if near(c)]))
    assert len(entries) == 1 and np.hypot(*(part.images[2].world_to_pix(entries[0].pos) - part.images[2].world_to_pix(missing.pos))) <= 1.0
    rt, _ = resid.missed_sources(ref, part.images, part.catalog)
    assert len(rt) == 1 and np.allclose(rt["flux"], table["flux"], rtol=1e-9, equal_nan=True)


@pytest.mark.parametrize("prep", ["host", "device"])
def test_infer_box_refine_adds_the_missing_source(lib, prep):
    import celeste_jl_amd as cel
    from celeste_jl_amd import cabi, model, resid
    from celeste_jl_amd.catalog import celeste_to_rows
    from celeste_jl_amd.params import init_source_table
    full, part, missing = _recovery()
    box = cel.BoundingBox(0.0, 160.0, 0.0, 170.0)
    cfg = cel.ElboConfig(max_iters=8)
    kw = dict(catalog=part.catalog, method="joint_vi", cfg=cfg, prep=prep)
    plain = cel.infer_box(part.images, box, **kw)
    res = cel.infer_box(part.images, box, refine=1, refine_threshold=THRESHOLD, **kw)
    assert len(plain) == 11 and len(res) == 12 and [r.refined for r in res] == [None] * 11 + [1]
    new = res[-1]
    truth = part.images[2].world_to_pix(missing.pos)
    assert np.hypot(*(part.images[2].world_to_pix(new.vs[0:2]) - truth)) <= 1.0
    assert np.hypot(*(part.images[2].world_to_pix([new.init_ra, new.init_dec]) - truth)) <= 1.0
    rows = celeste_to_rows(res, refined=True)
    assert [r["refine_round"] for r in rows] == [r.refined for r in res if not r.is_sky_bad]

    def chi2(catalog, results, second=None):
        table = model.table_for(part.images, catalog, False, prep_device=0 if prep == "device" else None)
        vp = init_source_table(catalog)
        vp[:len(results)] = np.stack([r.vs for r in results])
        with resid.ResidContext(cabi.problem_from_table(part.images, table, table.neighbors())) as rc:
            s = rc.search(vp, threshold=THRESHOLD)
            assert (s.frames["status"] == 0).all()
            if second is not None:
                second.append(s)
                second.append(resid.missed_sources(s, part.images, catalog)[1])
            return float(s.frames["chi2"].sum())
    first = []
    before = chi2(part.catalog, plain, first)
    assert len(first[1]) == 1 and (new.init_ra, new.init_dec) == tuple(first[1][0].pos)      # the entry the first search found
    again = []
    after = chi2(list(part.catalog) + first[1], res, again)
    print("refine (%s): summed chi2 %.1f -> %.1f" % (prep, before, after))
    assert after < before
    pcs = [img.world_to_pix(new.vs[0:2]) - 1.0 for img in part.images]
    assert not any(np.hypot(c["h"] + c["dh"] - pcs[c["image"]][0], c["w"] + c["dw"] - pcs[c["image"]][1]) <= 2.0 for c in again[0].candidates)


def test_infer_box_refine_with_the_complete_catalog_adds_nothing(lib):
    import celeste_jl_amd as cel
    from celeste_jl_amd.catalog import celeste_to_rows
    full, _, _ = _recovery()
    box = cel.BoundingBox(0.0, 160.0, 0.0, 170.0)
    kw = dict(catalog=full.catalog, method="joint_vi", cfg=cel.ElboConfig(max_iters=8))
    plain = cel.infer_box(full.images, box, **kw)
    res = cel.infer_box(full.images, box, refine=1, refine_threshold=THRESHOLD, **kw)
    assert len(res) == len(plain) == 12 and all(r.refined is None for r in res)
    assert all(a.vs.tobytes() == b.vs.tobytes() for a, b in zip(plain, res)) and celeste_to_rows(res) == celeste_to_rows(plain)
    with pytest.raises(ValueError, match="mcmc"):
        cel.infer_box(full.images, box, catalog=full.catalog, method="mcmc", refine=1)


@pytest.mark.parametrize("prep", ["host", "device"])
def test_infer_box_refine_after_detection(lib, prep):
    """without a catalog the first inference runs over the detections' catalog and patches; a round that finds nothing returns
    what refine=0 returns, bit for bit; a round that finds something appends it after the old targets, inside the box"""
    import celeste_jl_amd as cel
    full, _, _ = _recovery()
    box = cel.BoundingBox(20.0, 140.0, 20.0, 150.0)
    kw = dict(catalog=None, method="joint_vi", cfg=cel.ElboConfig(max_iters=8), match_radius=2.5, prep=prep)
    plain = cel.infer_box(full.images, box, **kw)
    quiet = cel.infer_box(full.images, box, refine=2, refine_threshold=1e9, **kw)
    assert len(plain) == len(quiet) >= 5 and all(r.refined is None for r in quiet)
    assert all(a.vs.tobytes() == b.vs.tobytes() and (a.init_ra, a.init_dec) == (b.init_ra, b.init_dec) for a, b in zip(plain, quiet))
    res = cel.infer_box(full.images, box, refine=1, refine_threshold=4.0, **kw)
    n_new = len(res) - len(plain)
    print("refine after detection (%s): %d targets, %d added at threshold 4" % (prep, len(plain), n_new))
    assert n_new >= 0 and [r.refined for r in res] == [None] * len(plain) + [1] * n_new
    assert [(r.init_ra, r.init_dec) for r in res[:len(plain)]] == [(r.init_ra, r.init_dec) for r in plain]
    assert all(box.contains((r.init_ra, r.init_dec)) and np.isfinite(r.vs).all() for r in res)
