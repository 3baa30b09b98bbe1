"""The stack of a search's maps across images on the device (celeste_resid_stack) against the numpy restatement
(tests/stack_reference.py), fed the device's own per-image maps so that the stack step is isolated: counts and NaN patterns
exactly, N, D and z within 1e-11 of their sum |term|, the candidate lists, the sub-pixel offsets and the world positions; an
aligned scene of edge cases and a tangent-plane scene of turned frames; culling off against on, bit for bit; determinism and
isolation; truncation; refusals; and the recovery of a star too faint for every single image, through infer_box(...,
refine_stack=True)."""
import ctypes as C
import os

import numpy as np
import pytest

import resid_reference as RR
import stack_reference as SR
import test_gpu_resid as TG

pytestmark = pytest.mark.gpu

MAP_TOL = 1e-11           # of sum |term|: the project's bound for the filter maps (exact agreement is expected)
FLAT = [1.0] * 5
ONE = [[1.0 if b == k else 0.0 for b in range(5)] for k in range(5)]
TWO = [0.0, 2.0, 0.5, 0.0, 0.0]
PLANES = ("N", "D", "z", "count")


def _device_maps(s):
    return {n: (s.map(n, "N"), s.map(n, "D"), s.map(n, "z")) for n in s.images}


def _restate(images, s, maps, grid, weights, threshold=5.0, min_images=1):
    ok = {int(fr["image"]): int(fr["status"]) == 0 for fr in s.frames}
    return SR.Stack(maps, s.images, {n: images[n].b for n in s.images}, {n: SR.Wcs.of_image(images[n]) for n in s.images}, grid,
                    weights, threshold, min_images, ok)


def _planes(st):
    return {k: np.stack([st.map(c, k) for c in range(len(st.weights))]) for k in PLANES}


def _compare(st, ref, name, planes=None, max_left_out=0.0):
    """the device's stack against the restatement's, in the cells that are not within reach of a rounding tie"""
    g = planes or _planes(st)
    use = ~ref.tie
    left = 1.0 - use.mean()
    assert left <= max_left_out, (name, left)
    worst = dict(N=0.0, D=0.0, z=0.0)
    for k in range(len(ref.z)):
        assert np.array_equal(g["count"][k][use], ref.cnt[k][use]), (name, k)
        assert np.array_equal(np.isnan(g["z"][k][use]), np.isnan(ref.z[k][use])), (name, k)
        with np.errstate(invalid="ignore", divide="ignore"):
            for key, got, want, scale in (("N", g["N"][k], ref.N[k], ref.abs_N[k]), ("D", g["D"][k], ref.D[k], ref.D[k]),
                                          ("z", g["z"][k], ref.z[k], ref.abs_N[k] / np.sqrt(ref.D[k]))):
                err = np.abs(got - want)
                okc = use & np.isfinite(err)
                zero = okc & (scale == 0)
                assert (err[zero] == 0).all(), (name, k, key)
                if (okc & ~zero).any():
                    worst[key] = max(worst[key], float((err[okc & ~zero] / scale[okc & ~zero]).max()))
        fr = st.frames[k]
        zk = g["z"][k]
        assert fr["channel"] == k and fr["n_cells"] == int((~np.isnan(zk)).sum())
        if fr["n_cells"]:
            assert fr["z_max"] == np.nanmax(zk) and fr["z_min"] == np.nanmin(zk)
        else:
            assert np.isnan(fr["z_max"]) and np.isnan(fr["z_min"])
    print("stack parity %-34s N %.3e  D %.3e  z %.3e of sum|term| (bound %.0e), %.3f %% of the cells left out" %
          (name, worst["N"], worst["D"], worst["z"], MAP_TOL, 100 * left))
    assert max(worst.values()) <= MAP_TOL, (name, worst)
    return g


def _compare_candidates(st, ref, name, g):
    """the lists agree except at peaks that hang on less than 1e-9 or that touch a cell left out; the records agree with the
    restatement's and with the device's own planes"""
    unsafe = set()
    tie = np.argwhere(ref.tie)
    for k in range(len(ref.z)):
        unsafe |= {(k, h, w) for h, w in RR.fragile_peaks(ref.z[k], ref.threshold, 1e-9)}
        unsafe |= {(k, int(h) + a, int(w) + b) for h, w in tie for a in (-1, 0, 1) for b in (-1, 0, 1)}
    key = lambda c: (int(c["channel"]), int(c["h"]), int(c["w"]))
    got = [c for c in st.candidates if key(c) not in unsafe]
    want = [c for c in ref.candidates if key(c) not in unsafe]
    assert [key(c) for c in got] == [key(c) for c in want], (name, len(got), len(want))
    assert st.n_found == len(st.candidates) and st.status == 0 and abs(st.n_found - len(ref.candidates)) <= len(unsafe)
    off = wd = 0.0
    for c, r in zip(got, want):
        k, h, w = key(c)
        off = max(off, abs(c["dh"] - r["dh"]), abs(c["dw"] - r["dw"]))
        wd = max(wd, float(np.abs(c["world"] - r["world"]).max()))
        assert c["z"] == g["z"][k][h, w] and c["D"] == g["D"][k][h, w] and c["n_images"] == g["count"][k][h, w] == r["n_images"]
        assert c["f"] == g["N"][k][h, w] / g["D"][k][h, w] and abs(c["z"] - r["z"]) <= MAP_TOL * ref.abs_N[k][h, w] / np.sqrt(r["D"])
    print("stack candidates %-30s %d compared (%d unsafe cells), offsets within %.3e (bound 1e-12), world within %.3e degrees "
          "(bound 1e-10)" % (name, len(got), len(unsafe), off, wd))
    assert off <= 1e-12 and wd <= 1e-10
    return len(got)


# ---- the aligned scene of edge cases -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge(lib):
    from celeste_jl_amd import resid
    f, _ = TG._edge_scene()
    with resid.ResidContext(TG._problem(f)) as rc:
        yield f, rc


@pytest.mark.parametrize("min_images", [1, 3])
@pytest.mark.parametrize("which", [0, 4])
def test_edge_scene_against_the_restatement(edge, which, min_images):
    """four 37 x 41 frames and a 13 x 9 frame shifted by (20, 10); on the grid of image 0 and on that of image 4, smaller than a
    tile; the flat channel, every one-band channel and a two-band channel with weights that are neither 0 nor 1"""
    from celeste_jl_amd import resid
    f, rc = edge
    s = rc.search(f.vp, threshold=3.0)
    maps = _device_maps(s)
    weights = [FLAT] + ONE + [TWO]
    st = s.stack(resid.StackGrid.of_image(f.images[which]), weights, threshold=3.0, min_images=min_images)
    ref = _restate(f.images, s, maps, SR.Grid.of_image(f.images[which]), weights, 3.0, min_images)
    assert not ref.tie.any()
    name = "edge, grid %d, min_images %d" % (which, min_images)
    g = _compare(st, ref, name)
    n = _compare_candidates(st, ref, name, g)
    assert ref.cnt[0].max() == 5 and (which == 4 or (ref.cnt[0].min() < 3 and np.isnan(ref.z[0]).any()))
    if min_images == 1:
        assert n > 0
        if which == 0:
            # a one-band channel is the image's own map, bit for bit; image 4 (band 5) lands at its shift
            for n_img in range(4):
                N, D, z = maps[n_img]
                seen = ~np.isnan(z)
                k = 1 + n_img
                assert np.array_equal(g["z"][k], z, equal_nan=True) and np.array_equal(g["N"][k][seen], N[seen]) and np.array_equal(g["D"][k][seen], D[seen])
            assert np.array_equal(g["z"][5][20:33, 10:19], maps[4][2], equal_nan=True) and g["count"][5].sum() == (~np.isnan(maps[4][2])).sum()
    else:
        assert np.isnan(g["z"][1:6]).all() and (g["count"][1:6] <= 1).all()      # a one-band channel never has three images


def test_determinism_isolation_and_a_frame_that_is_not_ok(edge):
    from celeste_jl_amd import cabi, resid
    f, rc = edge
    grid = resid.grid_covering(f.images, list(range(5)))
    weights = [FLAT, TWO]
    s = rc.search(f.vp, threshold=3.0)
    a = s.stack(grid, weights, threshold=3.0)
    pa = _planes(a)
    b = s.stack(grid, weights, threshold=3.0)
    pb = _planes(b)
    assert all(np.array_equal(pa[k], pb[k], equal_nan=True) for k in PLANES)
    assert a.frames.tobytes() == b.frames.tobytes() and a.candidates.tobytes() == b.candidates.tobytes() and len(a.candidates) > 0
    with pytest.raises(RuntimeError):
        a.map(0, "z")                                                    # the context has stacked again
    ms = rc.stack_last_ms()
    assert len(ms) == 2 and ms[0] > 0 and ms[1] >= 0
    # a search of two images, then a stack: the other images' planes are not read
    c = rc.search(f.vp, images=[1, 3], threshold=3.0)
    with pytest.raises(RuntimeError):
        s.stack(grid, weights)                                           # a stale search
    st = c.stack(grid, weights, threshold=3.0)
    ref = _restate(f.images, c, _device_maps(c), SR.grid_covering(f.images, list(range(5))), weights, 3.0)
    g = _compare(st, ref, "edge, images [1, 3]")
    _compare_candidates(st, ref, "edge, images [1, 3]", g)
    assert ref.cnt.max() == 2
    # the non-finite-row scene: frames 0 .. 3 are not OK and add nothing, image 4 stands
    vp = f.vp.copy()
    vp[0] = np.nan
    d = rc.search(vp, threshold=3.0)
    assert d.frames["status"].tolist() == [cabi.ERR_NONFINITE_INPUT] * 4 + [0]
    st = d.stack(grid, [FLAT], threshold=3.0)
    maps = _device_maps(d)
    ref = _restate(f.images, d, maps, SR.grid_covering(f.images, list(range(5))), [FLAT], 3.0)
    g = _compare(st, ref, "edge, non-finite row")
    seen = ~np.isnan(maps[4][2])
    assert g["count"][0].max() == 1 and g["count"][0].sum() == seen.sum() and np.array_equal(g["z"][0][20:33, 10:19], maps[4][2], equal_nan=True)


def test_truncation_gives_the_true_count(edge):
    from celeste_jl_amd import resid
    f, rc = edge
    s = rc.search(f.vp, threshold=3.0)
    grid = resid.StackGrid.of_image(f.images[0])
    ref = _restate(f.images, s, _device_maps(s), SR.Grid.of_image(f.images[0]), [FLAT, TWO], 1.5)
    assert len(ref.candidates) > 8 and not any(RR.fragile_peaks(ref.z[k], 1.5) for k in range(2))
    full = s.stack(grid, [FLAT, TWO], threshold=1.5)
    cut = s.stack(grid, [FLAT, TWO], threshold=1.5, max_candidates=5)
    none = s.stack(grid, [FLAT, TWO], threshold=1.5, max_candidates=0)
    assert full.n_found == cut.n_found == none.n_found == len(ref.candidates) and full.status == 0
    assert cut.status == none.status == resid.TRUNCATED and len(none.candidates) == 0
    assert cut.candidates.tobytes() == full.candidates[:5].tobytes()
    assert len(set(full.candidates["channel"].tolist())) == 2 and (np.diff(full.candidates["channel"]) >= 0).all()


def test_refusals_with_a_context(lib):
    from celeste_jl_amd import cabi, resid
    f = TG._fixture("sample_two_body")
    p, dp = resid._ptr, cabi.c_double_p
    with resid.ResidContext(TG._problem(f)) as rc:
        frames = np.zeros(8, dtype=resid.STACK_FRAME_DTYPE)
        cand = np.zeros(8, dtype=resid.STACK_CANDIDATE_DTYPE)
        nf, st = C.c_int64(-7), C.c_int32(-7)
        good_grid = resid.StackGrid.of_image(f.images[0])

        def stack(H=20, W=23, n_images=5, n_ch=1, wts=FLAT, min_images=1, mx=8, grid_wcs=None, img_wcs=None, out=cand, grid=True, opts=True):
            g = good_grid.c_struct()
            g.H, g.W = H, W
            if grid_wcs is not None:
                g.wcs = grid_wcs
            ws = (resid.WcsT * 5)(*[resid.wcs_of(im) for im in f.images])
            if img_wcs is not None:
                ws[3] = img_wcs
            w = np.ascontiguousarray(np.asarray(wts, dtype=np.float64).reshape(-1))
            o = resid.StackOptsT(5.0, min_images, 0)
            return rc.lib.celeste_resid_stack(rc.handle, C.byref(g) if grid else None, n_images, ws, n_ch, p(w, dp),
                                              C.byref(o) if opts else None, frames.ctypes.data, None if out is None else out.ctypes.data, mx,
                                              C.byref(nf), C.byref(st))
        out = np.full(20 * 23, -7.0)
        assert stack() == cabi.ERR_INVALID_ARG                           # no search yet
        assert rc.lib.celeste_resid_stack_get_map(rc.handle, 0, resid.STACK_Z, p(out, dp)) == cabi.ERR_INVALID_ARG
        s = rc.search(f.vp)
        assert rc.lib.celeste_resid_stack_get_map(rc.handle, 0, resid.STACK_Z, p(out, dp)) == cabi.ERR_INVALID_ARG     # no stack yet
        sing = resid.wcs_of(f.images[0])
        sing.m[:] = [1.0, 2.0, 2.0, 4.0]
        nanw = resid.wcs_of(f.images[0])
        nanw.pix0[0] = np.nan
        pole = resid.WcsT()
        pole.kind = resid.WCS_TAN
        pole.world0[:], pole.pix0[:], pole.m[:] = (0.0, 91.0), (1.0, 1.0), (1e-4, 0.0, 0.0, 1e-4)
        nan_w, neg_w = list(FLAT), list(FLAT)
        nan_w[2], neg_w[4] = np.nan, -1.0
        for kw in (dict(n_images=4), dict(n_images=6), dict(H=0), dict(W=0), dict(H=65536, W=32768), dict(n_ch=0), dict(n_ch=9, wts=[FLAT] * 9),
                   dict(wts=nan_w), dict(wts=neg_w), dict(wts=[0.0] * 5), dict(n_ch=2, wts=[FLAT, [0.0] * 5]), dict(min_images=0),
                   dict(grid_wcs=sing), dict(grid_wcs=nanw), dict(grid_wcs=pole), dict(img_wcs=sing), dict(img_wcs=nanw), dict(img_wcs=pole),
                   dict(mx=-1), dict(out=None), dict(grid=False), dict(opts=False)):
            assert stack(**kw) == cabi.ERR_INVALID_ARG, kw
        assert nf.value == -7 and st.value == -7 and not frames.view(np.uint8).any() and not cand.view(np.uint8).any()
        assert stack() == 0 and st.value in (0, resid.TRUNCATED) and nf.value >= 0
        assert stack(out=None, mx=0) == 0
        assert rc.lib.celeste_resid_stack_get_map(rc.handle, 0, resid.STACK_Z, p(out, dp)) == 0 and not (out == -7).any()
        for ch, which in ((1, resid.STACK_Z), (-1, resid.STACK_Z), (0, 4), (0, -1)):
            assert rc.lib.celeste_resid_stack_get_map(rc.handle, ch, which, p(out, dp)) == cabi.ERR_INVALID_ARG
        for kw in (dict(weights=[FLAT] * 9), dict(weights=[neg_w]), dict(min_images=0), dict(max_candidates=-1), dict(grid=resid.StackGrid(0, 4, sing))):
            with pytest.raises(ValueError):
                s.stack(**kw)
        with pytest.raises(RuntimeError):
            s.stack(grid=resid.StackGrid(4, 4, sing))                    # a singular WCS reaches the library, which refuses


# ---- the tangent-plane scene ---------------------------------------------------------------------------------------------------
TAN_W = [FLAT, TWO, ONE[2]]
TAN_COV = 0.3             # the frames' border pixels keep their z: a sample at a frame's very edge counts


@pytest.fixture(scope="module")
def tan(lib):
    import wcs_scene
    from celeste_jl_amd import resid
    f = wcs_scene.tan_multifield(perturb=False)
    assert len(f.images) == 15 and all(im.wcs is not None for im in f.images)
    with resid.ResidContext(TG._problem(f)) as rc:
        yield f, rc


def _tan_grids(f):
    """(name, the product's grid, the restatement's): images 0, 5, 10, the covering grid, and image 0's plane moved 55 rows up --
    mostly off every image"""
    from celeste_jl_amd import resid
    out = [("image %d" % n, resid.StackGrid.of_image(f.images[n]), SR.Grid.of_image(f.images[n])) for n in (0, 5, 10)]
    out.append(("covering", resid.grid_covering(f.images, list(range(15))), SR.grid_covering(f.images, list(range(15)))))
    off = resid.StackGrid.of_image(f.images[0])
    off.wcs.pix0[0] += 55.0
    out.append(("mostly off", off, SR.Grid(64, 80, SR.Wcs.of_image(f.images[0]).shifted(-55.0, 0.0))))
    return out


@pytest.mark.parametrize("gi", range(5), ids=["image0", "image5", "image10", "covering", "mostly_off"])
def test_tan_scene_against_the_restatement(tan, gi):
    """15 frames of 64 x 80 turned by 0, 30 and 90 degrees, one field with flipped parity, straddling RA 0"""
    f, rc = tan
    name, grid, rgrid = _tan_grids(f)[gi]
    s = rc.search(f.vp, threshold=3.0, min_coverage=TAN_COV)
    assert (s.frames["status"] == 0).all()
    maps = _device_maps(s)
    st = s.stack(grid, TAN_W, threshold=3.0)
    ref = _restate(f.images, s, maps, rgrid, TAN_W, 3.0)
    g = _compare(st, ref, "tan, " + name, max_left_out=0.01)
    n = _compare_candidates(st, ref, "tan, " + name, g)
    print("tan, %s: %d x %d cells, images per cell %d .. %d" % (name, grid.H, grid.W, ref.cnt[0].min(), ref.cnt[0].max()))
    if gi < 3:
        assert ref.cnt[0].max() >= 5 and n > 0
    if gi == 3:
        assert ref.cnt[0].min() == 0 and ref.cnt[0].max() >= 10 and n > 0        # corners of the mosaic's box hold no frame
    if gi == 4:
        assert (ref.cnt[0] == 0).mean() > 0.5 and ref.cnt[0].max() >= 1


def test_culling_changes_no_bit(tan, edge):
    from celeste_jl_amd import resid
    old = os.environ.pop("CELESTE_STACK_NO_CULL", None)
    try:
        runs = []
        f, rc = tan
        s = rc.search(f.vp, threshold=3.0, min_coverage=TAN_COV)
        for name, grid, _ in _tan_grids(f):
            runs.append(("tan, " + name, s, grid, TAN_W))
        fe, rce = edge
        se = rce.search(fe.vp, threshold=3.0)
        runs.append(("edge, covering", se, resid.grid_covering(fe.images, list(range(5))), [FLAT] + ONE + [TWO]))
        runs.append(("edge, image 4", se, resid.StackGrid.of_image(fe.images[4]), [FLAT] + ONE + [TWO]))
        for name, srch, grid, w in runs:
            os.environ.pop("CELESTE_STACK_NO_CULL", None)
            on = srch.stack(grid, w, threshold=3.0)
            pon = _planes(on)
            os.environ["CELESTE_STACK_NO_CULL"] = "1"
            offr = srch.stack(grid, w, threshold=3.0)
            poff = _planes(offr)
            assert all(pon[k].tobytes() == poff[k].tobytes() for k in PLANES), name
            assert on.frames.tobytes() == offr.frames.tobytes() and on.candidates.tobytes() == offr.candidates.tobytes(), name
    finally:
        os.environ.pop("CELESTE_STACK_NO_CULL", None)
        if old is not None:
            os.environ["CELESTE_STACK_NO_CULL"] = old


# ---- a star too faint for every single image -------------------------------------------------------------------------------------
STAR_POS, STAR_FLUX, STAR_SEED, THRESHOLD = (53.3, 78.6), 0.55, 20261020, 5.0      # chosen on the CPU with the restatement
_REC = {}


def _faint():
    """make_field(160, 170, 12, seed=2) with every source at its catalog row; the same pixels plus one star of STAR_FLUX nmgy in
    every band at STAR_POS, Poisson-drawn from STAR_SEED, that the catalog does not have"""
    if not _REC:
        from celeste_jl_amd import synthetic
        from celeste_jl_amd.params import CatalogEntry, catalog_init_source
        f = synthetic.make_field(160, 170, 12, seed=2, perturb=False)
        vp = np.stack([catalog_init_source(ce) for ce in f.catalog])
        star = CatalogEntry(np.array(STAR_POS), True, np.full(5, STAR_FLUX), np.full(5, STAR_FLUX), 0.5, 0.8, 0.0, 0.2)
        lam = RR.frame_model(f.images, f.patches, vp)
        before = RR.Search(f.images, f.patches, vp, threshold=THRESHOLD, lam=lam)
        for n, im in enumerate(f.images):
            el = (synthetic.render_expected_image(im, [star]) - im.sky.astype(np.float64)) * im.nelec_per_nmgy.astype(np.float64)[:, None]
            im.pixels = (im.pixels.astype(np.float64) + np.random.Generator(np.random.PCG64([STAR_SEED, n])).poisson(el)).astype(np.float32)
        after = RR.Search(f.images, f.patches, vp, threshold=THRESHOLD, lam=lam)
        _REC.update(f=synthetic.Field(f.images, f.catalog, f.patches, f.neighbors, vp, "faint star"), star=star, before=before, after=after)
    return _REC["f"], _REC["star"], _REC["before"], _REC["after"]


def _flat_stack(f, search):
    simgs = list(range(5))
    return SR.Stack({n: (search.maps[n].N, search.maps[n].D, search.maps[n].z) for n in simgs}, simgs, {n: f.images[n].b for n in simgs},
                    {n: SR.Wcs.of_image(f.images[n]) for n in simgs}, SR.Grid.of_image(f.images[0]), [FLAT], THRESHOLD)


def test_a_star_below_every_single_image_is_found_by_the_stack(lib):
    from celeste_jl_amd import resid
    f, star, before, after = _faint()
    # the fixture's conditions, on the restatement alone
    hh, ww = np.mgrid[0:160, 0:170]
    d = np.hypot(hh + 1 - STAR_POS[0], ww + 1 - STAR_POS[1])
    z0, z1 = _flat_stack(f, before).z[0], _flat_stack(f, after).z[0]
    assert np.nanmax(np.abs(z0[d <= 3])) < 1                              # a quiet spot
    assert len(after.candidates) == 0                                     # no single image sees the star
    assert np.nanmax(z1[d <= 1]) >= 6 and np.nanmax(z1[d > 6]) < 5
    print("faint star: stacked z without it %.2f within 3 px; with it %.2f within 1 px, %.2f beyond 6 px; single images at most %.2f" %
          (np.nanmax(np.abs(z0[d <= 3])), np.nanmax(z1[d <= 1]), np.nanmax(z1[d > 6]), max(np.nanmax(after.maps[n].z) for n in range(5))))
    with resid.ResidContext(TG._problem(f)) as rc:
        s = rc.search(f.vp, threshold=THRESHOLD)
        assert s.n_found == 0 and resid.missed_sources(s, f.images, f.catalog)[1] == []
        st = s.stack(threshold=THRESHOLD)
        table, entries = resid.stacked_sources(st, s, f.images, f.catalog)
    assert st.n_found == 1 and len(st.candidates) == 1 and len(entries) == 1
    c = st.candidates[0]
    assert np.hypot(c["h"] + 1 + c["dh"] - STAR_POS[0], c["w"] + 1 + c["dw"] - STAR_POS[1]) <= 1.0 and c["n_images"] == 5 and c["z"] >= 6
    assert np.hypot(*(entries[0].pos - np.array(STAR_POS))) <= 1.0 and table["n_detections"][0] == 5
    print("faint star: candidate z %.2f, f %.3f nmgy (true %.2f), per-band fluxes %s" % (c["z"], c["f"], STAR_FLUX, np.round(table["flux"][0], 3)))


@pytest.mark.parametrize("prep", ["host", "device"])
def test_infer_box_refine_stack_adds_the_faint_star(lib, prep):
    import celeste_jl_amd as cel
    f, star, _, _ = _faint()
    box = cel.BoundingBox(0.0, 160.0, 0.0, 170.0)
    kw = dict(catalog=f.catalog, method="joint_vi", cfg=cel.ElboConfig(max_iters=8), prep=prep, refine=1, refine_threshold=THRESHOLD)
    plain = cel.infer_box(f.images, box, **kw)
    assert len(plain) == 12 and all(r.refined is None for r in plain)            # as today: the single-image search finds nothing
    res = cel.infer_box(f.images, box, refine_stack=True, **kw)
    assert len(res) == 13 and [r.refined for r in res] == [None] * 12 + [1]
    new = res[-1]
    d_init, d_fit = np.hypot(*(np.array([new.init_ra, new.init_dec]) - STAR_POS)), np.hypot(*(new.vs[0:2] - np.array(STAR_POS)))
    print("refine_stack (%s): the new source %.2f px from the star as found, %.2f px as fitted" % (prep, d_init, d_fit))
    assert d_init <= 1.0 and d_fit <= 1.0
    assert [(r.init_ra, r.init_dec) for r in res[:12]] == [(r.init_ra, r.init_dec) for r in plain]


def test_infer_box_refine_stack_with_the_star_in_the_catalog_adds_nothing(lib):
    import celeste_jl_amd as cel
    f, star, _, _ = _faint()
    box = cel.BoundingBox(0.0, 160.0, 0.0, 170.0)
    res = cel.infer_box(f.images, box, catalog=list(f.catalog) + [star], method="joint_vi", cfg=cel.ElboConfig(max_iters=8), refine=1,
                        refine_threshold=THRESHOLD, refine_stack=True)
    assert len(res) == 13 and all(r.refined is None for r in res)
