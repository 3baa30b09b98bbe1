"""Per-source goodness of fit on the device (libceleste_fit.so) against the numpy restatement (tests/fit_reference.py):
stamps within 1e-12 relative per pixel, every statistic within 1e-10 of its sum |term|, n_pix, statuses and the NaN pattern
of the stamps exactly; determinism and batch invariance; the isolation of a non-finite row; the engine's own expected image;
infer_box(..., diagnostics=True)."""
import os

import numpy as np
import pytest

import fit_reference as FR

pytestmark = pytest.mark.gpu

STAMP_RTOL = 1e-12
STAT_TOL = 1e-10          # of sum |term|: the parity level the README states for the engine against its oracle


def _problem(f):
    from celeste_jl_amd import cabi
    return cabi.Problem(f.images, f.patches, f.neighbors)


def _same(a, b):
    """equal bit for bit, NaNs included"""
    return (np.array_equal(a.n_pix, b.n_pix) and np.array_equal(a.status, b.status) and
            np.array_equal(a.stats, b.stats, equal_nan=True) and
            (a.stamps is None or b.stamps is None or
             all(na == nb and np.array_equal(sa, sb, equal_nan=True)
                 for ra, rb in zip(a.stamps, b.stamps) for (na, sa), (nb, sb) in zip(ra, rb))))


def _compare(got, ref, name):
    """stamps, statistics, and n_pix / statuses / NaN pattern; prints the measured figures before it asserts them"""
    worst_stamp, worst_stat = 0.0, 0.0
    for i in range(len(ref.status)):
        assert np.array_equal(got.n_pix[i], ref.n_pix[i]), (name, i)
        assert got.status[i] == ref.status[i], (name, i, got.status[i], ref.status[i])
        if got.stamps is not None:
            assert [n for n, _ in got.stamps[i]] == [n for n, _ in ref.stamps[i]], (name, i)
            for (n, a), (_, b) in zip(got.stamps[i], ref.stamps[i]):
                assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), (name, i, n)
                ok = np.isfinite(b)
                if ok.any():
                    worst_stamp = max(worst_stamp, float((np.abs(a[ok] - b[ok]) / np.abs(b[ok])).max()))
        if ref.status[i] != 0:
            assert np.isnan(got.stats[i]).all(), (name, i)
            continue
        err = np.abs(got.stats[i] - ref.stats[i])
        zero = ref.abs_sums[i] == 0
        assert (got.stats[i][zero] == 0).all(), (name, i)
        if (~zero).any():
            worst_stat = max(worst_stat, float((err[~zero] / ref.abs_sums[i][~zero]).max()))
    print("fit parity %-28s stamps %.3e (bound %.0e)  statistics %.3e of sum|term| (bound %.0e)" %
          (name, worst_stamp, STAMP_RTOL, worst_stat, STAT_TOL))
    assert worst_stamp <= STAMP_RTOL, (name, worst_stamp)
    assert worst_stat <= STAT_TOL, (name, worst_stat)


def _run(f, targets=None, stamps=True, vp=None):
    from celeste_jl_amd import fit
    targets = list(range(len(f.catalog))) if targets is None else targets
    with fit.FitContext(_problem(f)) as fc:
        return fc.stats(f.vp if vp is None else vp, targets, stamps=stamps)


# ---- the committed fixtures ------------------------------------------------------------------------------------------------
_FIX = {}


def _fixture(name):
    if name not in _FIX:
        import golden_util as G
        f = G.arrays_to_field(np.load(G.path(name)))
        targets = list(range(len(f.catalog)))
        _FIX[name] = (f, FR.fit_reference(f.images, f.patches, f.neighbors, f.vp, targets))
    return _FIX[name]


@pytest.mark.parametrize("name", ["sample_star", "sample_galaxy", "sample_two_body", "field_64x80_8src_nan",
                                  "field_72x88_9src_variable"])
def test_fixture_against_the_restatement(lib, name):
    f, ref = _fixture(name)
    got = _run(f)
    assert (ref.status == 0).all() and ref.n_pix.sum() > 0
    _compare(got, ref, name)
    if name == "field_64x80_8src_nan":        # NaN pixels are not visited; patches are clipped at the image edge
        assert any(np.isnan(s).any() for row in got.stamps for _, s in row)
        shapes = {s.shape for row in got.stamps for _, s in row}
        assert len(shapes) > 1
    if name == "sample_star":
        assert np.array_equal(got.purity(), np.ones((1, 5)))
    if name == "sample_two_body":
        assert (got.purity() < 1).all()


# ---- a scene of edge cases ---------------------------------------------------------------------------------------------------
def _edge_scene():
    """48 x 60 images, the fifth shifted by 20 rows.  Sources 0-2: patches of 9 x 9 = 81 pixels (not a multiple of 64), 0 and 1
    in a row so that the last column of 0's patch lies inside 1's; 0 is off the fifth image.  Sources 3-5: patches of
    17 x 17 = 289 pixels (across the 256-pixel chunk), three that overlap one another."""
    if "edge" not in _FIX:
        from celeste_jl_amd import synthetic
        from celeste_jl_amd.model import get_sky_patches, neighbor_map
        from celeste_jl_amd.params import catalog_init_source
        rng = np.random.Generator(np.random.PCG64(7))
        images = synthetic.blank_images(48, 60)
        images[4].wcs_world0 = np.array([20.0, 0.0])
        small = [synthetic.sample_ce([8.2, 12.3], True), synthetic.sample_ce([8.3, 17.2], False),
                 synthetic.sample_ce([40.3, 50.2], True)]
        large = [synthetic.sample_ce([30.2, 24.3], False), synthetic.sample_ce([33.4, 28.1], True),
                 synthetic.sample_ce([28.3, 30.4], False)]
        catalog = small + large
        synthetic.gen_images(images, catalog, rng)
        patches = get_sky_patches(images, small, radius_override_pix=4.0) + get_sky_patches(images, large, radius_override_pix=8.0)
        vp = np.stack([catalog_init_source(ce) for ce in catalog])
        f = synthetic.Field(images, catalog, patches, neighbor_map(patches), vp, "edge")
        _FIX["edge"] = (f, FR.fit_reference(f.images, f.patches, f.neighbors, f.vp, list(range(6))))
    return _FIX["edge"]


def test_edge_scene_against_the_restatement(lib):
    f, ref = _edge_scene()
    sizes = [[p.active_pixel_bitmap.shape for p in row] for row in f.patches]
    assert sizes[0][0] == (9, 9) and sizes[3][0] == (17, 17) and 0 in sizes[0][4] and 0 not in sizes[3][4]
    assert 1 in f.neighbors[0] and {4, 5} <= set(f.neighbors[3]) and 5 in f.neighbors[4]
    got = _run(f)
    _compare(got, ref, "edge scene")
    assert [n for n, _ in got.stamps[0]] == [0, 1, 2, 3]                       # source 0 has no patch in the fifth image
    assert got.n_pix[0].tolist() == [81, 81, 81, 81, 0] and (got.stats[0, 4] == 0).all()
    assert got.n_pix[3, 0] == 289
    # the last column of 0's patch: its own light is 0 there, its neighbour's is not, and the pixels count
    n, visited, E, m, B = FR.expected_nmgy(f.images, f.patches, f.neighbors, f.vp, 0)[2]
    assert (m[:, -1] == 0).all() and (B[:, -1] > 0).all() and visited[:, -1].all()
    lam_last = got.stamps[0][2][1][:, -1]
    h0, w0 = f.patches[0][2].bitmap_offset
    sky = f.images[2].sky[h0:h0 + 9, w0 + 8].astype(np.float64)
    iota = f.images[2].nelec_per_nmgy[h0:h0 + 9].astype(np.float64)
    assert (lam_last > iota * sky).all()
    # the crowd: every one of 3, 4, 5 sees the light of the other two
    for s in (3, 4, 5):
        assert (got.purity()[s] < 1).all()


def test_explicit_bitmaps_against_the_restatement(lib):
    """Patches whose bitmaps leave pixels unset that are not NaN, so that the library gets them as explicit bitmaps (a bitmap
    equal to the NaN mask is not passed at all, and no other test here has another).  Source 0: a 9 x 13 patch, an ellipse with
    one more pixel unset; source 1: a 9 x 9 patch that overlaps it, a disc.  Rows 18 .. 24, columns 23 .. 26 (1-based) are
    shared; of these (18, 23), (18, 24), (18, 25), (19, 23) are set in 0's bitmap and unset in 1's, and (24, 26) the other way.
    For CELESTE_CLIENT_MUTANT 3 (the neighbour's bitmap ignored: 1's light at those four pixels of 0's stamps) and 4 (the
    target's bitmap read transposed: wrong on a patch that is not square)."""
    from celeste_jl_amd import synthetic
    from celeste_jl_amd.model import ImagePatch, neighbor_map
    from celeste_jl_amd.params import catalog_init_source
    images = synthetic.blank_images(48, 60)
    catalog = [synthetic.sample_ce([20.2, 20.3], False), synthetic.sample_ce([22.3, 27.2], True)]
    synthetic.gen_images(images, catalog, np.random.Generator(np.random.PCG64(13)))
    boxes = [((16, 24), (14, 26)), ((18, 26), (23, 31))]
    hh, ww = np.arange(1, 49)[:, None], np.arange(1, 61)[None, :]
    masks = [((hh - 20) / 4.6) ** 2 + ((ww - 20) / 6.6) ** 2 <= 1.0, (hh - 22) ** 2 + (ww - 27) ** 2 <= 4.3 ** 2]
    masks[0][17, 16] = False                                      # (18, 17): off both axes of the ellipse
    patches = [[ImagePatch.from_box(img, box) for img in images] for box in boxes]
    for row, box, mask in zip(patches, boxes, masks):
        for p in row:
            p.active_pixel_bitmap = p.active_pixel_bitmap & mask[box[0][0] - 1:box[0][1], box[1][0] - 1:box[1][1]]
    assert [p.active_pixel_bitmap.shape for p in (patches[0][0], patches[1][0])] == [(9, 13), (9, 9)]
    assert not np.isnan(images[0].pixels).any() and not patches[0][0].active_pixel_bitmap.all() and not patches[1][0].active_pixel_bitmap.all()
    for h, w in ((18, 23), (18, 24), (18, 25), (19, 23)):
        assert masks[0][h - 1, w - 1] and not masks[1][h - 1, w - 1]
    assert masks[1][23, 25] and not masks[0][23, 25]
    assert not np.array_equal(patches[0][0].active_pixel_bitmap[:, :9], patches[0][0].active_pixel_bitmap[:, :9].T)
    f = synthetic.Field(images, catalog, patches, neighbor_map(patches), np.stack([catalog_init_source(ce) for ce in catalog]),
                        "bitmaps")
    assert f.neighbors == [[1], [0]]
    ref = FR.fit_reference(f.images, f.patches, f.neighbors, f.vp, [0, 1])
    got = _run(f)
    _compare(got, ref, "explicit bitmaps")
    assert got.n_pix[0, 0] == int(patches[0][0].active_pixel_bitmap.sum()) < 9 * 13 and (got.status == 0).all()
    # 1's light at a shared pixel it does not cover would be seen: it is far above the stamps' tolerance there
    n, visited, E, m, B = FR.expected_nmgy(f.images, f.patches, f.neighbors, f.vp, 0)[2]
    assert visited[2, 9] and B[2, 9] == 0 and B[3, 10] > 1e-6 * E[3, 10]     # (18, 23) unset in 1's disc; (19, 24) set


def test_determinism_and_batch_invariance(lib):
    """the same bits for every target: the call made twice, the targets reversed, one target repeated, one call per target,
    another CELESTE_CHUNK_PX on a fresh context"""
    from celeste_jl_amd import fit
    f, _ = _edge_scene()
    targets = list(range(6))
    with fit.FitContext(_problem(f)) as fc:
        a = fc.stats(f.vp, targets, stamps=True)
        assert _same(a, fc.stats(f.vp, targets, stamps=True))
        r = fc.stats(f.vp, targets[::-1], stamps=True)
        for k, t in enumerate(targets[::-1]):
            assert _same(r[k:k + 1], a[t:t + 1]), t
        rep = fc.stats(f.vp, [3, 0, 3, 5, 3], stamps=True)
        for k, t in enumerate([3, 0, 3, 5, 3]):
            assert _same(rep[k:k + 1], a[t:t + 1]), t
        for t in targets:
            assert _same(fc.stats(f.vp, [t], stamps=True), a[t:t + 1]), t
        assert _same(fc.stats(f.vp, targets), a)                 # without stamps
    old = os.environ.get("CELESTE_CHUNK_PX")
    for chunk in ("64", "128"):
        os.environ["CELESTE_CHUNK_PX"] = chunk
        try:
            with fit.FitContext(_problem(f)) as fc:
                assert _same(fc.stats(f.vp, targets, stamps=True), a), chunk
        finally:
            if old is None:
                del os.environ["CELESTE_CHUNK_PX"]
            else:
                os.environ["CELESTE_CHUNK_PX"] = old


def test_a_non_finite_row_fails_its_target_alone(lib):
    from celeste_jl_amd import cabi
    f, ref = _edge_scene()
    S = len(f.catalog)
    clean = _run(f)
    t = 0
    assert f.neighbors[t] == [1]
    vp = f.vp.copy()
    vp[t] = np.nan
    got = _run(f, vp=vp)
    ref2 = FR.fit_reference(f.images, f.patches, f.neighbors, vp, list(range(S)))
    _compare(got, ref2, "non-finite row")
    assert got.status[t] == cabi.ERR_NONFINITE_INPUT and np.isnan(got.stats[t]).all()
    assert np.array_equal(got.n_pix, clean.n_pix)
    seen = [s for s in range(S) if t in f.neighbors[s]]
    assert seen == [1] and got.status[1] == cabi.ERR_NONFINITE_RESULT      # its light is part of its neighbour's lam
    others = [s for s in range(S) if s != t and s not in seen]
    assert others
    for s in others:
        assert _same(got[s:s + 1], clean[s:s + 1]), s


def test_refusals_with_a_context(lib):
    from celeste_jl_amd import cabi, fit
    f, _ = _fixture("sample_two_body")
    dp, ip, lp = cabi.c_double_p, cabi.c_int32_p, cabi.c_int64_p
    p = fit._ptr
    with fit.FitContext(_problem(f)) as fc:
        vp = np.ascontiguousarray(f.vp)
        tg = np.array([0, 1], dtype=np.int32)
        n_pix = np.full((2, 5), -7, dtype=np.int64)
        st = np.full((2, 5, 7), -7.0)
        status = np.full(2, -7, dtype=np.int32)
        buf = np.full(8, -7.0)
        h = fc.handle
        good = [h, p(vp, dp), 2, p(tg, ip), p(n_pix, lp), p(st, dp), p(status, ip), None, None]
        for pos in (1, 3, 4, 5, 6):                               # a NULL pointer
            args = list(good)
            args[pos] = None
            assert fc.lib.celeste_fit_stats(*args) == cabi.ERR_INVALID_ARG, pos
        for bad in ([0, 2], [-1, 0]):                             # a target out of range
            args = list(good)
            args[3] = p(np.array(bad, dtype=np.int32), ip)
            assert fc.lib.celeste_fit_stats(*args) == cabi.ERR_INVALID_ARG
        args = list(good)
        args[2] = -1
        assert fc.lib.celeste_fit_stats(*args) == cabi.ERR_INVALID_ARG
        args = list(good)
        args[8] = p(buf, dp)                                      # stamps without stamp_offsets
        assert fc.lib.celeste_fit_stats(*args) == cabi.ERR_INVALID_ARG
        args = list(good)
        args[2] = 0                                               # no target: OK, nothing touched
        assert fc.lib.celeste_fit_stats(*args) == 0
        assert fc.lib.celeste_fit_stats(h, p(vp, dp), 0, None, None, None, None, None, None) == 0
        assert (n_pix == -7).all() and (st == -7).all() and (status == -7).all() and (buf == -7).all()
        with pytest.raises(ValueError):
            fc.stats(f.vp, [2])
        e = fc.stats(f.vp, [], stamps=True)
        assert e.n_pix.shape == (0, 5) and e.stats.shape == (0, 5, 7) and e.stamps == []
        assert fc.lib.celeste_fit_stats(*good) == 0 and (status == 0).all() and (n_pix >= 0).all()
        ms = fc.last_ms()
        assert len(ms) == 3 and all(x >= 0 for x in ms) and ms[1] > 0


# ---- several fields ----------------------------------------------------------------------------------------------------------
def test_sparse_and_dense_multifield_agree_bit_for_bit(lib):
    """visit lists against the dense S x N table; a band with several images sums over them; a source that is absent from an
    image contributes nothing"""
    from celeste_jl_amd import synthetic
    fs = synthetic.make_multifield((2, 3), 160, 160, 0.10, 70, seed=11, sparse=True)
    fd = synthetic.make_multifield((2, 3), 160, 160, 0.10, 70, seed=11, sparse=False)
    S = len(fs.catalog)
    gs, gd = _run(fs), _run(fd)
    assert _same(gs, gd)
    n_vis = [len(row) for row in gs.stamps]
    assert max(n_vis) >= 10 and min(n_vis) == 5                   # some sources lie where fields overlap
    for s in range(S):                                            # (no NaN pixels: every pixel of every patch is visited)
        want = np.zeros(5, dtype=np.int64)
        for n, st in gs.stamps[s]:
            want[fs.images[n].b - 1] += st.size
        assert np.array_equal(gs.n_pix[s], want)
    order = np.argsort(n_vis, kind="stable")
    sub = sorted({int(s) for s in order[-4:]} | {int(s) for s in order[:2]} |
                 {int(s) for s in np.argsort([len(x) for x in fs.neighbors])[-3:]})
    ref = FR.fit_reference(fs.images, fs.patches, fs.neighbors, fs.vp, sub)
    _compare(gs[sub], ref, "multifield (sparse)")


# ---- against the engine ------------------------------------------------------------------------------------------------------
def test_stamps_against_the_engine_expected_image(lib):
    """lam / iota - eps at a target's visited pixels is what celeste_render_expected puts there (every source on its own patch:
    equal because the neighbour lists are complete)"""
    import celeste_jl_amd as cel
    from celeste_jl_amd import synthetic
    from celeste_jl_amd.model import find_neighbors
    f = synthetic.make_field(160, 200, 30, seed=11, nan_fraction=0.004)
    S = len(f.catalog)
    assert f.neighbors == [find_neighbors(f.patches, s) for s in range(S)]
    got = _run(f)
    assert (got.status == 0).all()
    ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
    try:
        planes = [ctx.render_expected(f.vp, n) for n in range(len(f.images))]
    finally:
        ctx.close()
    worst = 0.0
    for s in range(S):
        for n, lam in got.stamps[s]:
            h0, w0 = f.patches[s][n].bitmap_offset
            H2, W2 = lam.shape
            ok = ~np.isnan(lam)
            iota = f.images[n].nelec_per_nmgy[h0:h0 + H2].astype(np.float64)[:, None]
            eps = f.images[n].sky[h0:h0 + H2, w0:w0 + W2].astype(np.float64)
            mine = (lam / iota - eps)[ok]
            theirs = planes[n][h0:h0 + H2, w0:w0 + W2][ok]
            scale = np.abs(planes[n]).max()
            worst = max(worst, abs(mine.sum() - theirs.sum()) / scale, float(np.abs(mine - theirs).max()) / scale)
    print("stamps against celeste_render_expected: %.3e of the plane's maximum (bound 1e-12)" % worst)
    assert worst <= 1e-12


# ---- infer_box ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["catalog", "catalog, prep on the device", "no catalog"])
def test_infer_box_attaches_the_fit(lib, case):
    import celeste_jl_amd as cel
    from celeste_jl_amd import cabi, fit, model, synthetic
    from celeste_jl_amd.params import init_source_table
    if case == "no catalog":
        from celeste_jl_amd import detect
        f = synthetic.make_field(200, 200, 40, seed=31, stars_only=True)
        box = cel.BoundingBox(20.0, 180.0, 20.0, 180.0)
        kw = dict(catalog=None, match_radius=2.5)
        catalog, patches = detect.detect_sources(f.images, match_radius=2.5)
        problem = cabi.Problem(f.images, patches, model.neighbor_map(patches))
    else:
        f = synthetic.make_field(200, 240, 40, seed=4)
        box = cel.BoundingBox(0.0, 200.0, 0.0, 240.0)
        device = case.endswith("device")
        kw = dict(catalog=f.catalog, prep="device" if device else "host")
        catalog = f.catalog
        table = model.table_for(f.images, catalog, False, prep_device=0 if device else None)
        problem = cabi.problem_from_table(f.images, table, table.neighbors())
    cfg = cel.ElboConfig(max_iters=8)
    plain = cel.infer_box(f.images, box, method="joint_vi", cfg=cfg, **kw)
    res = cel.infer_box(f.images, box, method="joint_vi", cfg=cfg, diagnostics=True, **kw)
    targets = [i for i, ce in enumerate(catalog) if box.contains(ce.pos)]
    assert len(res) == len(plain) == len(targets) >= 10
    assert all(p.fit is None for p in plain) and all(isinstance(r.fit, fit.FitStats) for r in res)
    for p, r in zip(plain, res):
        assert p.vs.tobytes() == r.vs.tobytes() and (p.init_ra, p.init_dec, p.is_sky_bad, p.failed) == (r.init_ra, r.init_dec, r.is_sky_bad, r.failed)
    vp = init_source_table(catalog)
    vp[targets] = np.stack([r.vs for r in res])
    with fit.FitContext(problem) as fc:
        want = fc.stats(vp, targets)
    for k, r in enumerate(res):
        assert r.fit.n_pix.shape == (5,) and r.fit.stats.shape == (5, 7)
        assert np.array_equal(r.fit.n_pix, want.n_pix[k]) and np.array_equal(r.fit.stats, want.stats[k], equal_nan=True)
        assert r.fit.status == want.status[k]
    assert (want.status == 0).all() and (want.n_pix.sum(axis=1) > 0).all()
    from celeste_jl_amd.catalog import DIAGNOSTIC_COLUMNS, celeste_to_rows
    rows = celeste_to_rows(res, diagnostics=True)
    assert len(rows) == sum(not r.is_sky_bad for r in res) and all(isinstance(row[c], (int, float)) for row in rows for c in DIAGNOSTIC_COLUMNS)
    assert celeste_to_rows(res) == celeste_to_rows(plain)


def test_mcmc_with_diagnostics_raises(lib):
    import celeste_jl_amd as cel
    f, _ = _fixture("sample_two_body")
    with pytest.raises(ValueError, match="mcmc"):
        cel.infer_box(f.images, cel.BoundingBox(0.0, 30.0, 0.0, 30.0), f.catalog, method="mcmc", diagnostics=True)
