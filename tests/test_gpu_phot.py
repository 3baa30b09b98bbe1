"""Per-exposure forced photometry on the device (libceleste_phot.so) against the numpy / scipy restatement
(tests/phot_reference.py): entries, images, n_pix, flags, statuses and the NaN pattern exactly; the root judged at the device's
own alpha; I and chi2 within 1e-10 of their sum |term|; the two solve paths, determinism and batch invariance bit for bit; the
isolation of a non-finite row; a scene with a variable source; infer_box(..., light_curves=True)."""
import os

import numpy as np
import pytest

import phot_reference as PR

pytestmark = pytest.mark.gpu

ROOT_TOL = 1e-8           # |g| / sqrt(I) at the device's alpha, and |alpha_dev - alpha_ref| / sigma.  Derived, not tuned: the
                          # fit library measured 2.5e-14 of sum |term| for such sums; g's sum |term| is about 2 sum a, and
                          # sum a / sqrt(I) is at most 3.3e3 on these scenes (about 2e3 typically): an error of about
                          # 1e-10 sigma, a margin of 50 to 100
SUM_TOL = 1e-10           # I and chi2, of their sum |term|: the parity level the README states
BOUND_RTOL = 1e-12        # AT_BOUND: alpha is -b / a of one pixel, a and b each a few roundings from the restatement's
SUMMARY_RTOL = 1e-9
ENTRY = ("image", "band", "alpha", "sigma", "chi2", "n_pix", "iters", "flag")


def _problem(f):
    from celeste_jl_amd import cabi
    return cabi.Problem(f.images, f.patches, f.neighbors)


def _run(f, targets=None, vp=None, **kw):
    from celeste_jl_amd import phot
    targets = list(range(len(f.catalog))) if targets is None else targets
    with phot.PhotContext(_problem(f)) as pc:
        return pc.light_curves(f.vp if vp is None else vp, targets, **kw)


def _same(a, b):
    """equal bit for bit, NaNs included"""
    return (np.array_equal(a.offsets, b.offsets) and all(np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True) for k in ENTRY) and
            np.array_equal(a.n_epochs, b.n_epochs) and np.array_equal(a.summary, b.summary, equal_nan=True) and
            np.array_equal(a.status, b.status))


def _compare(got, ref, name):
    """prints the measured maxima before it asserts them"""
    assert np.array_equal(got.offsets, ref.offsets), name
    assert np.array_equal(got.status, ref.status), (name, got.status, ref.status)
    worst = dict(g=0.0, alpha=0.0, I=0.0, chi2=0.0, bound=0.0, summary=0.0)
    for i, e in enumerate(ref.flat):
        at = (name, i, e.image)
        assert (got.image[i], got.band[i], got.n_pix[i], got.flag[i]) == (e.image, e.band, e.n_pix, e.flag), at + (got.flag[i], e.flag)
        al, sg, c2 = float(got.alpha[i]), float(got.sigma[i]), float(got.chi2[i])
        assert (np.isnan(al), np.isnan(sg), np.isnan(c2)) == (np.isnan(e.alpha), np.isnan(e.sigma), np.isnan(e.chi2)), at
        if e.flag == PR.OK:
            assert 1 <= got.iters[i] <= 50, at
            (g, I, chi2), (_, aI, ac) = e.evaluate(al)
            worst["g"] = max(worst["g"], abs(float(g)) / np.sqrt(float(I)))
            worst["alpha"] = max(worst["alpha"], abs(al - e.alpha) / e.sigma)
            worst["I"] = max(worst["I"], abs(1 / sg ** 2 - float(I)) / float(aI))
            worst["chi2"] = max(worst["chi2"], abs(c2 - float(chi2)) / float(ac))
        else:
            assert got.iters[i] == 0, at
        if e.flag == PR.NO_LIGHT and e.n_pix:
            worst["chi2"] = max(worst["chi2"], abs(c2 - e.chi2) / e.chi2)
        if e.flag == PR.AT_BOUND:
            worst["bound"] = max(worst["bound"], abs(al - e.alpha_min) / abs(e.alpha_min))
    # the summaries: the restatement's over the device's own entries (alpha, sigma, flag), so that what is compared is the
    # summation; chi2_var has the floor its cancellation leaves: 16 eps^2 sum w alpha^2 (wmean is rounded to eps |wmean|)
    assert np.array_equal(got.n_epochs, ref.n_epochs), name
    for t in range(len(ref.status)):
        sl = slice(got.offsets[t], got.offsets[t + 1])
        dev = [PR.Entry(int(n), int(b), 0, None, None, None, int(fl), float(al), np.nan, float(sg))
               for n, b, fl, al, sg in zip(got.image[sl], got.band[sl], got.flag[sl], got.alpha[sl], got.sigma[sl])]
        ne, sm = PR.band_summaries(dev)
        assert np.array_equal(ne, got.n_epochs[t]) and np.array_equal(np.isnan(sm), np.isnan(got.summary[t])), (name, t)
        for b in range(5):
            if ne[b] == 0:
                continue
            ok = [e for e in dev if e.flag == PR.OK and e.band == b]
            floor = 16 * np.finfo(float).eps ** 2 * sum((e.alpha / e.sigma) ** 2 for e in ok)
            err = np.abs(got.summary[t, b] - sm[b]) - np.array([0, 0, floor])
            worst["summary"] = max(worst["summary"], float((err / np.abs(np.where(sm[b] == 0, 1, sm[b]))).max()))
    print("phot parity %-26s |g|/sqrt(I) %.2e  |d alpha|/sigma %.2e (bound %.0e)  I %.2e  chi2 %.2e of sum|term| (bound %.0e)  "
          "at bound %.2e  summaries %.2e" % (name, worst["g"], worst["alpha"], ROOT_TOL, worst["I"], worst["chi2"], SUM_TOL,
                                             worst["bound"], worst["summary"]))
    assert worst["g"] <= ROOT_TOL and worst["alpha"] <= ROOT_TOL, (name, worst)
    assert worst["I"] <= SUM_TOL and worst["chi2"] <= SUM_TOL, (name, worst)
    assert worst["bound"] <= BOUND_RTOL and worst["summary"] <= SUMMARY_RTOL, (name, worst)
    return worst


# ---- the committed fixtures ------------------------------------------------------------------------------------------------
_FIX = {}


def _fixture(name):
    if name not in _FIX:
        import golden_util as G
        f = G.arrays_to_field(np.load(G.path(name)))
        _FIX[name] = (f, PR.phot_reference(f.images, f.patches, f.neighbors, f.vp, list(range(len(f.catalog)))))
    return _FIX[name]


@pytest.mark.parametrize("name", ["sample_star", "sample_galaxy", "sample_two_body", "field_64x80_8src_nan",
                                  "field_72x88_9src_variable"])
def test_fixture_against_the_restatement(lib, name):
    f, ref = _fixture(name)
    got = _run(f)
    assert (ref.status == 0).all() and all(e.flag == PR.OK for e in ref.flat) and len(ref.flat) == 5 * len(f.catalog)
    _compare(got, ref, name)
    assert (got.n_epochs == 1).all() and np.isfinite(got.flux_nmgy()).all()
    print("   mean Newton iterations %.2f, largest %d" % (got.iters.mean(), got.iters.max()))


# ---- a scene of edge cases ---------------------------------------------------------------------------------------------------
def _box(img, ce, up, down, left, right):
    from celeste_jl_amd.model import ImagePatch, julia_round
    pc = img.world_to_pix(ce.pos)
    h, w = julia_round(pc[0]), julia_round(pc[1])
    return ImagePatch.from_box(img, ((h - up, h + down), (w - left, w + right)))


SHAPES = [(4, 4, 4, 4), (4, 4, 4, 4), (3, 3, 4, 4),                   # 0, 1: 9 x 9 in a row; 2: 7 x 9
          (8, 8, 8, 8), (8, 8, 8, 8), (8, 8, 8, 8),                   # 3, 4, 5: 17 x 17, three that overlap one another
          (4, 3, 4, 3), (2, 2, 6, 6), (3, 3, 0, 0)]                   # 6: 8 x 8 (one tile); 7: 5 x 13 (65 pixels); 8: 7 x 1


def _edge_scene():
    """48 x 60 images, the fifth shifted by 20 rows (sources 0 and 1 are off it).  The last column of 0's patch lies inside 1's
    patch; NaN pixels inside the patches of 0 / 1 and of the crowd 3 / 4 / 5; source 8's patch is one column wide (only its
    last column: NO_LIGHT); the pixels of source 2's patch in the first image, its last column excepted, are 0 (AT_BOUND)."""
    if "edge" not in _FIX:
        from celeste_jl_amd import synthetic
        from celeste_jl_amd.model import neighbor_map
        from celeste_jl_amd.params import catalog_init_source
        rng = np.random.Generator(np.random.PCG64(7))
        images = synthetic.blank_images(48, 60)
        images[4].wcs_world0 = np.array([20.0, 0.0])
        catalog = [synthetic.sample_ce([8.2, 12.3], True), synthetic.sample_ce([8.3, 17.2], False),
                   synthetic.sample_ce([40.3, 50.2], True),
                   synthetic.sample_ce([30.2, 24.3], False), synthetic.sample_ce([33.4, 28.1], True),
                   synthetic.sample_ce([28.3, 30.4], False),
                   synthetic.sample_ce([40.4, 8.3], True), synthetic.sample_ce([24.2, 50.3], False),
                   synthetic.sample_ce([44.3, 30.2], True)]
        synthetic.gen_images(images, catalog, rng)
        images[0].pixels[7, 13] = np.nan
        images[1].pixels[30, 25] = np.nan
        images[1].pixels[31, 27] = np.nan
        images[0].pixels[36:43, 45:53] = 0.0                      # source 2: rows 37..43, columns 46..54 (1-based), not the last
        patches = [[_box(img, ce, *sh) for img in images] for ce, sh in zip(catalog, SHAPES)]
        vp = np.stack([catalog_init_source(ce) for ce in catalog])
        f = synthetic.Field(images, catalog, patches, neighbor_map(patches), vp, "edge")
        _FIX["edge"] = (f, PR.phot_reference(f.images, f.patches, f.neighbors, f.vp, list(range(len(catalog)))))
    return _FIX["edge"]


def test_edge_scene_against_the_restatement(lib):
    f, ref = _edge_scene()
    sizes = [[p.active_pixel_bitmap.shape for p in row] for row in f.patches]
    assert [s[0] for s in sizes] == [(9, 9), (9, 9), (7, 9), (17, 17), (17, 17), (17, 17), (8, 8), (5, 13), (7, 1)]
    assert 0 in sizes[0][4] and 0 in sizes[1][4] and 0 not in sizes[3][4]
    assert f.patches[2][0].box == ((37, 43), (46, 54)) and (f.images[0].pixels[36:43, 45:53] == 0).all()
    assert 1 in f.neighbors[0] and {4, 5} <= set(f.neighbors[3]) and 5 in f.neighbors[4]
    got = _run(f)
    _compare(got, ref, "edge scene")
    assert np.diff(got.offsets).tolist() == [4, 4, 5, 5, 5, 5, 5, 5, 5]           # sources 0 and 1 have no patch in the fifth image
    assert got[0].image.tolist() == [0, 1, 2, 3] and got[2].image.tolist() == [0, 1, 2, 3, 4]
    assert got.n_epochs[0].tolist() == [1, 1, 1, 1, 0] and np.isnan(got.summary[0, 4]).all()
    assert got[0].n_pix.tolist() == [80, 81, 81, 81] and got[3].n_pix.tolist() == [289, 287, 289, 289, 289]   # the NaN pixels
    # the last column of 0's patch: its own light is 0 there, its neighbour's is not
    import fit_reference as FR
    n, visited, E, m, B = FR.expected_nmgy(f.images, f.patches, f.neighbors, f.vp, 0)[2]
    assert (m[:, -1] == 0).all() and (B[:, -1] > 0).all() and visited[:, -1].all()
    # one column: no light of its own, the pixels counted, chi2 at lam = b
    assert (got[8].flag == PR.NO_LIGHT).all() and got[8].n_pix.tolist() == [7] * 5 and np.isnan(got[8].alpha).all()
    assert np.isfinite(got[8].chi2).all() and (got.n_epochs[8] == 0).all() and got.status[8] == 0
    # no electrons where the source has light: the edge of the domain, exactly one pixel's -b / a
    two = got[2]
    assert two.flag.tolist() == [PR.AT_BOUND, 0, 0, 0, 0] and ref.entries[2][0].flag == PR.AT_BOUND
    assert two.alpha[0] < 0 and np.isnan(two.sigma[0]) and np.isnan(two.chi2[0]) and got.n_epochs[2].tolist() == [0, 1, 1, 1, 1]
    assert (got.status == 0).all()


def test_the_streaming_path_gives_the_same_bits(lib):
    """lds_max_pixels = 64: every patch of more than one tile is read from device memory on every iteration"""
    f, _ = _edge_scene()
    a = _run(f)
    assert _same(_run(f, lds_max_pixels=64), a)
    assert _same(_run(f, lds_max_pixels=1), a) and _same(_run(f, lds_max_pixels=100), a)


def test_a_patch_above_the_capacity_of_lds(lib):
    """one 90 x 90 patch (8100 pixels > CELESTE_PHOT_LDS_PIXELS, 127 tiles) per image: streamed"""
    from celeste_jl_amd import phot, synthetic
    from celeste_jl_amd.model import ImagePatch, neighbor_map
    from celeste_jl_amd.params import catalog_init_source
    images = synthetic.blank_images(100, 100)
    catalog = [synthetic.sample_ce([50.3, 49.6], False)]
    synthetic.gen_images(images, catalog, np.random.Generator(np.random.PCG64(90)))
    patches = [[ImagePatch.from_box(img, ((6, 95), (6, 95))) for img in images]]
    assert patches[0][0].active_pixel_bitmap.shape == (90, 90) and 90 * 90 > phot.LDS_PIXELS
    f = synthetic.Field(images, catalog, patches, neighbor_map(patches), np.stack([catalog_init_source(catalog[0])]), "large")
    ref = PR.phot_reference(f.images, f.patches, f.neighbors, f.vp, [0])
    got = _run(f)
    _compare(got, ref, "90 x 90")
    assert (got.flag == 0).all() and (got.n_pix == 8100).all()
    assert _same(_run(f, lds_max_pixels=64), got)
    # and 70 x 70 = 4900 pixels: the largest size class of the LDS path (one workgroup per CU)
    patches = [[ImagePatch.from_box(img, ((16, 85), (16, 85))) for img in images]]
    f = synthetic.Field(images, catalog, patches, neighbor_map(patches), f.vp, "70 x 70")
    got = _run(f)
    _compare(got, PR.phot_reference(f.images, f.patches, f.neighbors, f.vp, [0]), "70 x 70")
    assert (got.flag == 0).all() and (got.n_pix == 4900).all() and 3072 < 4900 <= phot.LDS_PIXELS
    assert _same(_run(f, lds_max_pixels=64), got)


def _boxed_field(H, W, boxes, seed, name):
    """one source at the centre of each 1-based inclusive box ((h_lo, h_hi), (w_lo, w_hi)), galaxies and stars in turn, on
    blank_images(H, W); returns (Field, restatement)"""
    from celeste_jl_amd import synthetic
    from celeste_jl_amd.model import ImagePatch, neighbor_map
    from celeste_jl_amd.params import catalog_init_source
    images = synthetic.blank_images(H, W)
    catalog = [synthetic.sample_ce([(h[0] + h[1]) / 2 + 0.2, (w[0] + w[1]) / 2 - 0.3], k % 2 == 1) for k, (h, w) in enumerate(boxes)]
    synthetic.gen_images(images, catalog, np.random.Generator(np.random.PCG64(seed)))
    patches = [[ImagePatch.from_box(img, box) for img in images] for box in boxes]
    f = synthetic.Field(images, catalog, patches, neighbor_map(patches), np.stack([catalog_init_source(ce) for ce in catalog]), name)
    return f, PR.phot_reference(f.images, f.patches, f.neighbors, f.vp, list(range(len(catalog))))


def test_two_rounds_of_tiles_against_the_restatement(lib):
    """one 91 x 91 patch (8281 pixels, 130 tiles) per image: phot_pass takes tiles in rounds of 128, so the second round
    (t0 = 128: pixels 8192 .. 8280, the other LDS buffer, the sums carried across rounds) runs in every pass.  For
    CELESTE_PHOT_MUTANT 1 (t0 dropped), which no patch of at most 128 tiles can see."""
    f, ref = _boxed_field(100, 100, [((5, 95), (5, 95))], 91, "91 x 91")
    assert f.patches[0][0].active_pixel_bitmap.shape == (91, 91) and (91 * 91 + 63) // 64 == 130
    got = _run(f)
    _compare(got, ref, "91 x 91")
    assert (got.flag == 0).all() and (got.n_pix == 8281).all() and len(got.n_pix) == 5
    assert _same(_run(f, lds_max_pixels=64), got)


# the LDS path's size classes end at 704, 1664 and 3072 pixels: a patch on each end, one just above it, and two small ones
CLASS_BOXES = [((1, 53), (1, 58)),        # 0: 53 x 58 = 3074, the first size of the last class
               ((53, 100), (1, 64)),      # 1: 48 x 64 = 3072; shares row 53 with 0
               ((1, 26), (37, 100)),      # 2: 26 x 64 = 1664; shares columns 37 .. 58 with 0
               ((27, 63), (56, 100)),     # 3: 37 x 45 = 1665; overlaps 0 and 1
               ((64, 85), (65, 96)),      # 4: 22 x 32 = 704
               ((86, 100), (54, 100)),    # 5: 15 x 47 = 705; overlaps 1
               ((30, 38), (20, 28)),      # 6: 9 x 9, inside 0's patch
               ((70, 86), (20, 36))]      # 7: 17 x 17, inside 1's
CLASS_PIXELS = [3074, 3072, 1664, 1665, 704, 705, 81, 289]


def test_size_classes_of_the_lds_path_against_the_restatement(lib):
    """One call whose entries fall into every size class of the LDS path, on both sides of every class end, so that every class
    launch but the last holds patches smaller than the one its dynamic LDS was sized for (the staging's `pad` is then the
    entry's own, not the launch's); lds_max_pixels of 64, 704 and 1664 moves the class ends and streams what lies above."""
    from celeste_jl_amd import phot
    f, ref = _boxed_field(100, 100, CLASS_BOXES, 17, "size classes")
    assert [[p.active_pixel_bitmap.size for p in row] for row in f.patches] == [[n] * 5 for n in CLASS_PIXELS]
    assert 3074 <= phot.LDS_PIXELS and 0 in f.neighbors[6] and {0, 3, 5, 7} <= set(f.neighbors[1]) and f.neighbors[4] == []
    got = _run(f)
    _compare(got, ref, "size classes")
    assert got.n_pix.tolist() == [n for n in CLASS_PIXELS for _ in range(5)] and (got.status == 0).all()
    assert (got.flag == 0).all()
    for cap in (64, 704, 1664):
        assert _same(_run(f, lds_max_pixels=cap), got), cap


def test_determinism_and_batch_invariance(lib):
    """the same bits for every entry: the call made twice, the targets reversed, one target repeated, one call per target,
    another CELESTE_CHUNK_PX on a fresh context"""
    from celeste_jl_amd import phot
    f, _ = _edge_scene()
    targets = list(range(len(f.catalog)))
    with phot.PhotContext(_problem(f)) as pc:
        a = pc.light_curves(f.vp, targets)
        assert _same(a, pc.light_curves(f.vp, targets))
        r = pc.light_curves(f.vp, targets[::-1])
        for k, t in enumerate(targets[::-1]):
            assert _same(r[k], a[t]), t
        rep = pc.light_curves(f.vp, [3, 0, 3, 8, 3])
        for k, t in enumerate([3, 0, 3, 8, 3]):
            assert _same(rep[k], a[t]), t
        for t in targets:
            assert _same(pc.light_curves(f.vp, [t]), a[t]), t
        ms = pc.last_ms()
        assert len(ms) == 4 and all(x >= 0 for x in ms) and ms[1] > 0 and ms[2] > 0
    old = os.environ.get("CELESTE_CHUNK_PX")
    os.environ["CELESTE_CHUNK_PX"] = "64"
    try:
        with phot.PhotContext(_problem(f)) as pc:
            assert _same(pc.light_curves(f.vp, targets), a)
    finally:
        if old is None:
            del os.environ["CELESTE_CHUNK_PX"]
        else:
            os.environ["CELESTE_CHUNK_PX"] = old


def test_max_iters_and_tolerance(lib):
    f, _ = _edge_scene()
    a = _run(f)
    one = _run(f, max_iters=1)
    solved = ~np.isin(a.flag, [PR.NO_LIGHT, PR.AT_BOUND])
    assert (one.iters[solved] == 1).all() and (one.flag[solved] == PR.NOT_CONVERGED).all() and np.isfinite(one.alpha[solved]).all()
    assert np.isfinite(one.sigma[solved]).all() and (one.n_epochs == 0).all() and np.isnan(one.summary).all()
    assert np.array_equal(one.flag[~solved], a.flag[~solved]) and np.array_equal(one.n_pix, a.n_pix)
    loose = _run(f, tol_sigma=1e-3)
    assert (loose.iters <= a.iters).all() and (loose.iters[solved] < a.iters[solved]).any() and (loose.flag == a.flag).all()
    assert (np.abs(loose.alpha - a.alpha)[solved] <= 1e-3 * a.sigma[solved]).all()


def test_newton_step_counts_against_the_restatement(lib):
    """iters is the number of Newton steps the header's rule takes: |step| <= tol_sigma / sqrt(I(alpha_k)), restated in extended
    precision (phot_reference.newton_iters).  On this scene sigma is below 1e-2, so a threshold that is not scaled by sigma is
    at least 100 times looser and stops a step earlier; alpha is then still within ROOT_TOL of the root (Newton converges
    quadratically), which is why the parity of alpha alone did not see CELESTE_PHOT_MUTANT 5.  An entry with a step within
    0.1 % of its threshold is left out: there the count may depend on rounding."""
    f, ref = _edge_scene()
    ok = [i for i, e in enumerate(ref.flat) if e.flag == PR.OK]
    assert len(ok) >= 30 and all(ref.flat[i].sigma < 1e-2 for i in ok)
    for tol in (1e-3, 1e-6):
        got = _run(f, tol_sigma=tol)
        n = 0
        for i in ok:
            want, margin = PR.newton_iters(ref.flat[i], tol)
            if margin < 1e-3:
                continue
            n += 1
            assert got.flag[i] == PR.OK and got.iters[i] == want, (tol, i, got.iters[i], want, margin)
        print("Newton step counts at tol_sigma %.0e: %d entries compared, %d to %d steps" % (tol, n, got.iters[ok].min(), got.iters[ok].max()))
        assert n >= 30, (tol, n)


def test_a_non_finite_row_fails_its_target_alone(lib):
    from celeste_jl_amd import cabi
    f, _ = _edge_scene()
    S = len(f.catalog)
    clean = _run(f)
    t = 0
    assert f.neighbors[t] == [1]
    vp = f.vp.copy()
    vp[t] = np.nan
    got = _run(f, vp=vp)
    _compare(got, PR.phot_reference(f.images, f.patches, f.neighbors, vp, list(range(S))), "non-finite row")
    assert got.status[t] == cabi.ERR_NONFINITE_INPUT and (got[t].flag == PR.BAD_MODEL).all()
    assert np.isnan(got[t].alpha).all() and np.isnan(got[t].sigma).all() and np.isnan(got[t].chi2).all()
    assert np.array_equal(got.n_pix, clean.n_pix) and (got.n_epochs[t] == 0).all()
    seen = [s for s in range(S) if t in f.neighbors[s]]
    assert seen == [1] and got.status[1] == cabi.ERR_NONFINITE_RESULT and (got[1].flag == PR.BAD_MODEL).all()
    for s in range(S):
        if s != t and s not in seen:
            assert _same(got[s], clean[s]), s


def test_refusals_with_a_context(lib):
    import ctypes as C
    from celeste_jl_amd import cabi, phot
    from test_phot_host import _call_args
    f, _ = _fixture("sample_two_body")
    with phot.PhotContext(_problem(f)) as pc:
        for pos in (1, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15):         # a NULL pointer
            args, arrays = _call_args(ctx=pc.handle)
            args[pos] = None
            assert pc.lib.celeste_phot_light_curves(*args) == cabi.ERR_INVALID_ARG, pos
            assert all((a == -7).all() for a in arrays[2:])
        for kw in (dict(n=-1), dict(params=phot.ParamsT(np.nan, 50, 0)), dict(params=phot.ParamsT(1e-9, 50, -1))):
            args, arrays = _call_args(ctx=pc.handle, **kw)
            assert pc.lib.celeste_phot_light_curves(*args) == cabi.ERR_INVALID_ARG, kw
            assert all((a == -7).all() for a in arrays[2:])
        args, arrays = _call_args(ctx=pc.handle)
        arrays[1][0] = 2                                              # a target out of range
        assert pc.lib.celeste_phot_light_curves(*args) == cabi.ERR_INVALID_ARG
        args, arrays = _call_args(ctx=pc.handle, n=0)                 # no target: OK, nothing touched
        assert pc.lib.celeste_phot_light_curves(*args) == 0 and all((a == -7).all() for a in arrays[2:])
        with pytest.raises(ValueError):
            pc.light_curves(f.vp, [2])
        e = pc.light_curves(f.vp, [])
        assert len(e) == 0 and e.alpha.shape == (0,) and e.summary.shape == (0, 5, 3) and e.offsets.tolist() == [0]
        args, arrays = _call_args(ctx=pc.handle)                      # and a good call through the same lists: NULL params
        arrays[0][:] = f.vp
        assert pc.lib.celeste_phot_light_curves(*args) == 0
        off, image, flag, status = arrays[2], arrays[3], arrays[6], arrays[8]
        assert off.tolist() == [0, 5] and image[:5].tolist() == [0, 1, 2, 3, 4] and (flag[:5] == 0).all() and status[0] == 0
        assert (image[5:] == -7).all()


# ---- several exposures -------------------------------------------------------------------------------------------------------
def test_variability_scene_against_the_restatement(lib):
    """three exposures of five bands; the variable source is the one the device flags, summaries included"""
    from scipy.stats import chi2
    f, var = PR.variability_scene()
    ref = PR.phot_reference(f.images, f.patches, f.neighbors, f.vp, list(range(6)))
    got = _run(f)
    _compare(got, ref, "variability scene")
    assert (got.n_epochs == 3).all() and got[var].image.tolist() == list(range(15))
    rel = np.abs(got.summary - ref.summary) / np.abs(ref.summary)
    print("   against the restatement's own roots: wmean %.2e, wmean_sigma %.2e, chi2_var %.2e relative" %
          tuple(rel[:, :, k].max() for k in range(3)))
    assert rel.max() <= SUMMARY_RTOL
    v, q = got.chi2_var[:, 2], chi2.ppf(0.999, 2)
    assert int(np.argmax(v)) == var and v[var] > q and (np.delete(v, var) < q).all()
    assert np.array_equal(got.reduced_chi2_var(), got.chi2_var / 2)
    fl = got[var].flux_nmgy()[got[var].band == 2]
    assert fl[1] > 1.3 * fl[0] and fl[1] > 1.3 * fl[2]


def test_sparse_and_dense_multifield_agree_bit_for_bit(lib):
    """visit lists against the dense S x N table; a source has one entry per image it lies in, several per band where fields
    overlap"""
    from celeste_jl_amd import synthetic
    fs = synthetic.make_multifield((2, 3), 160, 160, 0.10, 70, seed=11, sparse=True)
    fd = synthetic.make_multifield((2, 3), 160, 160, 0.10, 70, seed=11, sparse=False)
    gs, gd = _run(fs), _run(fd)
    assert _same(gs, gd)
    n_ent = np.diff(gs.offsets)
    assert n_ent.max() >= 10 and n_ent.min() == 5 and gs.n_epochs.max() >= 2
    assert np.array_equal(gs.n_epochs.sum(axis=1), np.array([(gs[s].flag == 0).sum() for s in range(len(fs.catalog))]))
    order = np.argsort(n_ent, kind="stable")
    sub = sorted({int(s) for s in order[-3:]} | {int(s) for s in order[:1]})
    ref = PR.phot_reference(fs.images, fs.patches, fs.neighbors, fs.vp, sub)
    _compare(gs[sub], ref, "multifield (sparse)")


# ---- infer_box ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["catalog", "catalog, prep on the device", "no catalog"])
def test_infer_box_attaches_the_light_curves(lib, case):
    import celeste_jl_amd as cel
    from celeste_jl_amd import cabi, model, phot, synthetic
    from celeste_jl_amd.catalog import LIGHT_CURVE_COLUMNS, celeste_to_rows
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
    res = cel.infer_box(f.images, box, method="joint_vi", cfg=cfg, light_curves=True, **kw)
    targets = [i for i, ce in enumerate(catalog) if box.contains(ce.pos)]
    assert len(res) == len(plain) == len(targets) >= 10
    assert all(p.light_curve is None for p in plain) and all(isinstance(r.light_curve, phot.LightCurves) for r in res)
    assert all(r.fit is None for r in res)
    for p, r in zip(plain, res):
        assert p.vs.tobytes() == r.vs.tobytes() and (p.init_ra, p.init_dec, p.is_sky_bad, p.failed) == (r.init_ra, r.init_dec, r.is_sky_bad, r.failed)
    vp = init_source_table(catalog)
    vp[targets] = np.stack([r.vs for r in res])
    with phot.PhotContext(problem) as pc:
        want = pc.light_curves(vp, targets)
    for k, r in enumerate(res):
        assert len(r.light_curve) == 1 and r.light_curve.n_epochs.shape == (1, 5) and _same(r.light_curve, want[k]), k
    assert (want.status == 0).all() and (np.diff(want.offsets) == 5).all() and (want.flag == 0).mean() > 0.9
    rows = celeste_to_rows(res, light_curves=True)
    assert len(rows) == sum(not r.is_sky_bad for r in res) and all(row["n_epochs_r"] in (0, 1) for row in rows)
    assert all(isinstance(row["var_chi2_r"], float) for row in rows if row["n_epochs_r"])
    assert celeste_to_rows(res) == celeste_to_rows(plain)
    assert [{k: v for k, v in row.items() if k not in LIGHT_CURVE_COLUMNS} for row in rows] == celeste_to_rows(plain)


def test_mcmc_with_light_curves_raises(lib):
    import celeste_jl_amd as cel
    f, _ = _fixture("sample_two_body")
    with pytest.raises(ValueError, match="mcmc"):
        cel.infer_box(f.images, cel.BoundingBox(0.0, 30.0, 0.0, 30.0), f.catalog, method="mcmc", light_curves=True)
