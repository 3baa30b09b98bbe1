"""Per-exposure astrometry on the device (libceleste_astrom.so) against the numpy / torch restatement
(tests/astrom_reference.py): entries, images, n_pix, flags, pass counts, statuses and the NaN pattern exactly (an entry whose
decisions the restatement finds within 1e-3 of a threshold is left out of the exact comparisons); the fixed point judged at the
device's own theta; F, chi2 and the likelihood within 1e-10 of their sum |term|; the covariance against mpmath; the summaries
over the device's own entries; determinism and batch invariance bit for bit; the isolation of a non-finite row; a scene with a
moved source and one with a linear motion under a rotated tangent-plane WCS; infer_box(..., astrometry=True)."""
import os

import numpy as np
import pytest

import astrom_reference as AR

pytestmark = pytest.mark.gpu

DEC_FLOOR = 1e-8          # the restatement's dec at the device's theta is at most tol_sigma + DEC_FLOOR.  Phot's derivation: the
                          # fit library measured 2.5e-14 of sum |term| for such sums; the score's sum |term| is about 2 sum a
                          # (and sum |D_d| of the same order per pixel of gradient), and sum a / sqrt(I) is at most 3.3e3 on
                          # these scenes: an error of about 1e-10 standard errors, a margin of about 100
SUM_TOL = 1e-10           # every entry of F, chi2 and loglik, of its sum |term|
COV_TOL = 1e-12           # cov against inv(F) of the device's sums in mpmath, of cond(R) max |inv(R)| (as the info library's)
SUMMARY_RTOL = 1e-9
MARGIN = 1e-3             # an entry with a decision this close to its threshold is left out of the exact comparisons
R_MAX = 0.9               # every OK entry of a test scene contracts at least this fast
ENTRY = ("image", "delta", "alpha", "fisher", "cov", "chi2", "loglik", "n_pix", "iters", "flag")
TARGET = ("n_epochs", "summary_flag", "summary", "status")


def _problem(f):
    from celeste_jl_amd import cabi
    return cabi.Problem(f.images, f.patches, f.neighbors)


def _run(f, targets=None, vp=None, **kw):
    from celeste_jl_amd import astrom
    targets = list(range(len(f.catalog))) if targets is None else targets
    with astrom.AstromContext(_problem(f)) as ac:
        return ac.offsets(f.vp if vp is None else vp, targets, **kw)


def _same(a, b):
    """equal bit for bit, NaNs included"""
    return (np.array_equal(a.offsets, b.offsets) and all(np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True) for k in ENTRY + TARGET))


def _cov_error(F6, cov6):
    """|cov s s' - inv(R)| over cond(R) max |inv(R)|, inv(R) of the device's own F in mpmath at 50 digits"""
    import mpmath as mp
    mp.mp.dps = 50
    F = AR.full3(np.asarray(F6, dtype=np.float64))
    s = [mp.sqrt(mp.mpf(float(F[k, k]))) for k in range(3)]
    R = mp.matrix(3, 3)
    for k in range(3):
        for l in range(3):
            R[k, l] = mp.mpf(1) if k == l else mp.mpf(float(F[k, l])) / (s[k] * s[l])
    Ri = R ** -1
    kappa = float(np.linalg.cond(np.array([[float(R[k, l]) for l in range(3)] for k in range(3)])))
    rmax = max(abs(float(Ri[k, l])) for k in range(3) for l in range(3))
    C = AR.full3(np.asarray(cov6, dtype=np.float64))
    err = max(abs(float(mp.mpf(float(C[k, l])) * s[k] * s[l] - Ri[k, l])) for k in range(3) for l in range(3))
    return err / (kappa * rmax)


def _summary_error(got, t, epochs):
    """the device's summary of target t against the restatement's over the device's own entries; chi2_const and chi2_lin have
    the floor their cancellation leaves, 64 eps^2 sum Delta' W Delta (each residual is rounded to eps |Delta|)"""
    sl = slice(got.offsets[t], got.offsets[t + 1])
    rows = [(int(n), int(fl), d, F, J) for n, fl, d, F, J in zip(got.image[sl], got.flag[sl], got.delta[sl], got.fisher[sl], got.jac[sl])]
    n, fl, want = AR.summarise(rows, epochs)
    assert n == got.n_epochs[t] and fl == got.summary_flag[t], (t, n, fl, got.n_epochs[t], got.summary_flag[t])
    have = got.summary[t]
    assert np.array_equal(np.isnan(want), np.isnan(have)), (t, want, have)
    if n == 0:
        return 0.0
    ok = [r for r in rows if r[1] == AR.OK]
    floor = 64 * np.finfo(float).eps ** 2 * sum(float(D @ W @ D) for D, W in (AR.entry_weight(r[4], r[2], r[3]) for r in ok))
    worst = 0.0
    for lo, hi, fl_ in ((0, 2, 0), (2, 5, 0), (5, 6, floor), (6, 8, 0), (8, 10, 0), (10, 20, 0), (20, 21, floor), (21, 22, 0)):
        if np.isnan(want[lo]):
            continue
        scale = np.abs(want[lo:hi]).max()
        if lo == 10:                                          # the covariance of (Delta_0, mu): each entry against its own diagonal pair
            d = np.sqrt(np.abs(want[[10, 14, 17, 19]]))
            sc = np.array([d[k] * d[l] for k in range(4) for l in range(k, 4)])
            worst = max(worst, float((np.abs(have[lo:hi] - want[lo:hi]) / sc).max()))
            continue
        err = np.abs(have[lo:hi] - want[lo:hi]).max() - fl_
        worst = max(worst, float(err / scale) if scale > 0 else float(err > 0))
    return worst


def _compare(got, ref, name, epochs=None, tol_sigma=1e-6, min_exact=0.8):
    """prints the measured maxima before it asserts them; returns them"""
    assert np.array_equal(got.offsets, ref.offsets), name
    assert np.array_equal(got.status, ref.status), (name, got.status, ref.status)
    w = dict(dec=0.0, F=0.0, chi2=0.0, loglik=0.0, root=0.0, r=0.0, cov=0.0, summary=0.0)
    n_exact, iters_ok = 0, []
    for i, e in enumerate(ref.flat):
        r = e.result
        at = (name, i, e.image)
        assert (got.image[i], got.n_pix[i]) == (e.image, e.n_pix), at
        fl = int(got.flag[i])
        th = np.array([got.delta[i, 0], got.delta[i, 1], got.alpha[i]])
        if r.margin >= MARGIN:
            n_exact += 1
            assert (fl, int(got.iters[i])) == (r.flag, r.iters), at + (fl, got.iters[i], r.flag, r.iters, r.margin)
            for have, want in ((th, r.theta), (got.fisher[i], r.F), (got.cov[i], r.cov), (got.chi2[i], r.chi2), (got.loglik[i], r.loglik)):
                assert np.array_equal(np.isnan(np.asarray(have, dtype=np.float64)), np.isnan(np.asarray(want, dtype=np.float64))), at
        # the NaN pattern the header gives the device's own flag
        nan_theta = fl in (AR.NO_LIGHT, AR.TOO_FAINT, AR.BAD_MODEL)
        assert np.isnan(th).all() == nan_theta and np.isnan(th).any() == nan_theta, at
        assert np.isnan(got.fisher[i]).all() == (fl in (AR.NO_LIGHT, AR.BAD_MODEL)), at
        assert np.isnan(got.chi2[i]) == np.isnan(got.loglik[i]) == (fl == AR.BAD_MODEL), at
        if fl == AR.BAD_MODEL:
            continue
        # the sums at the device's own theta (theta_0 where the device reports none)
        p = e.evaluate(np.array([0.0, 0.0, 1.0]) if nan_theta else th)
        w["chi2"] = max(w["chi2"], abs(got.chi2[i] - p.chi2) / p.abs_chi2)
        w["loglik"] = max(w["loglik"], abs(got.loglik[i] - p.l) / p.abs_l)
        if fl == AR.NO_LIGHT:
            continue
        w["F"] = max(w["F"], float((np.abs(got.fisher[i] - p.F.astype(np.float64)) / p.abs_F.astype(np.float64)).max()))
        if not np.isnan(got.cov[i]).any():
            w["cov"] = max(w["cov"], _cov_error(got.fisher[i], got.cov[i]))
        if fl == AR.OK:
            iters_ok.append(int(got.iters[i]))
            assert 1 <= got.iters[i] <= 50, at
            st = AR.step_of(p.F, p.U)
            assert st.ok, at
            w["dec"] = max(w["dec"], st.dec)
            root, size = e.root(th)
            rr = e.contraction(root)
            F = AR.full3(np.asarray(p.F, dtype=np.float64))
            d = th - root
            w["r"] = max(w["r"], rr)
            assert rr <= R_MAX and size <= 1e-9, at + (rr, size)
            w["root"] = max(w["root"], float(np.sqrt(d @ F @ d)) * (1 - rr) / (2 * (tol_sigma + DEC_FLOOR)))
    for t in range(len(ref.status)):
        w["summary"] = max(w["summary"], _summary_error(got, t, epochs))
    frac = n_exact / max(len(ref.flat), 1)
    print("astrom parity %-24s exact %d of %d; dec %.2e (bound %.2e); F %.2e chi2 %.2e loglik %.2e of sum|term| (bound %.0e); "
          "root distance %.2f of its bound, r <= %.3f; cov %.2e (bound %.0e); summaries %.2e; passes of OK entries %s" %
          (name, n_exact, len(ref.flat), w["dec"], tol_sigma + DEC_FLOOR, w["F"], w["chi2"], w["loglik"], SUM_TOL, w["root"], w["r"],
           w["cov"], COV_TOL, w["summary"], ("%d to %d, mean %.1f" % (min(iters_ok), max(iters_ok), np.mean(iters_ok))) if iters_ok else "-"))
    assert frac >= min_exact, (name, frac)
    assert w["dec"] <= tol_sigma + DEC_FLOOR, (name, w)
    assert max(w["F"], w["chi2"], w["loglik"]) <= SUM_TOL, (name, w)
    assert w["root"] <= 1.0 and w["cov"] <= COV_TOL and w["summary"] <= SUMMARY_RTOL, (name, w)
    return w


# ---- the committed fixtures ------------------------------------------------------------------------------------------------
_FIX = {}


def _fixture(name):
    if name not in _FIX:
        import golden_util as G
        f = G.arrays_to_field(np.load(G.path(name)))
        _FIX[name] = (f, AR.astrom_reference(f.images, f.patches, f.neighbors, f.vp, list(range(len(f.catalog)))))
    return _FIX[name]


@pytest.mark.parametrize("name", ["sample_star", "sample_galaxy", "sample_two_body", "field_64x80_8src_nan",
                                  "field_72x88_9src_variable"])
def test_fixture_against_the_restatement(lib, name):
    f, ref = _fixture(name)
    got = _run(f)
    assert (ref.status == 0).all() and len(ref.flat) == 5 * len(f.catalog)
    _compare(got, ref, name)
    flags = np.bincount(got.flag, minlength=7)
    print("   flags (OK, NO_LIGHT, TOO_FAINT, OUT_OF_RANGE, STALLED, NOT_CONVERGED, BAD_MODEL): %s" % flags.tolist())
    assert flags[AR.OK] >= 2 and flags[AR.BAD_MODEL] == 0


# ---- a scene of edge cases ---------------------------------------------------------------------------------------------------
def _box(img, ce, up, down, left, right):
    from celeste_jl_amd.model import ImagePatch, julia_round
    pc = img.world_to_pix(ce.pos)
    h, w = julia_round(pc[0]), julia_round(pc[1])
    return ImagePatch.from_box(img, ((h - up, h + down), (w - left, w + right)))


SHAPES = [(4, 4, 4, 4), (4, 4, 4, 4), (3, 3, 4, 4),                   # 0, 1: 9 x 9 in a row; 2: 7 x 9
          (8, 8, 8, 8), (8, 8, 8, 8), (8, 8, 8, 8),                   # 3, 4, 5: 17 x 17, three that overlap one another
          (4, 3, 4, 3), (2, 2, 6, 6), (3, 3, 0, 0)]                   # 6: 8 x 8 (one tile); 7: 5 x 13 (65 pixels); 8: 7 x 1
FAINT = 6                 # the source of the 8 x 8 patch is rendered and catalogued 30000 times fainter: above the gate


def _edge_scene():
    """48 x 60 images, the fifth shifted by 20 rows (sources 0 and 1 are off it).  The last column of 0's patch lies inside 1's
    patch; NaN pixels inside the patches of 0 / 1 and of the crowd 3 / 4 / 5; source 8's patch is one column wide (only its
    last column: NO_LIGHT); the pixels of source 2's patch in the first image, its last column excepted, are 0; source 6 is too
    faint for a position (TOO_FAINT in every image)."""
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
        catalog[FAINT].star_fluxes = np.asarray(catalog[FAINT].star_fluxes) / 30000.0
        catalog[FAINT].gal_fluxes = np.asarray(catalog[FAINT].gal_fluxes) / 30000.0
        synthetic.gen_images(images, catalog, rng)
        images[0].pixels[7, 13] = np.nan
        images[1].pixels[30, 25] = np.nan
        images[1].pixels[31, 27] = np.nan
        images[0].pixels[36:43, 45:53] = 0.0                      # source 2: rows 37..43, columns 46..54 (1-based), not the last
        patches = [[_box(img, ce, *sh) for img in images] for ce, sh in zip(catalog, SHAPES)]
        vp = np.stack([catalog_init_source(ce) for ce in catalog])
        f = synthetic.Field(images, catalog, patches, neighbor_map(patches), vp, "edge")
        _FIX["edge"] = (f, AR.astrom_reference(f.images, f.patches, f.neighbors, f.vp, list(range(len(catalog)))))
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
    assert got[0].n_pix.tolist() == [80, 81, 81, 81] and got[3].n_pix.tolist() == [289, 287, 289, 289, 289]   # the NaN pixels
    # one column: no light of its own, the pixels counted, chi2 and the likelihood at lam = b
    assert (got[8].flag == AR.NO_LIGHT).all() and got[8].n_pix.tolist() == [7] * 5 and np.isnan(got[8].alpha).all()
    assert np.isfinite(got[8].chi2).all() and np.isfinite(got[8].loglik).all() and got.n_epochs[8] == 0 and got.status[8] == 0
    assert got.summary_flag[8] == AR.NO_EPOCHS | AR.NO_MOTION and np.isnan(got.summary[8]).all() and (got[8].iters == 1).all()
    # no electrons where the source has light: never OK (the header); what it ends with is the restatement's
    zero = got[2]
    want = ref.entries[2][0].result
    print("   the patch of zeros: flag %d after %d passes (restatement: %d after %d, margin %.1e), alpha %.3g" %
          (zero.flag[0], zero.iters[0], want.flag, want.iters, want.margin, zero.alpha[0]))
    assert zero.flag[0] in (AR.STALLED, AR.NOT_CONVERGED, AR.OUT_OF_RANGE) and (zero.flag[1:] == AR.OK).all()
    # above the gate: not iterated, the covariance of theta_0 reported
    faint = got[FAINT]
    assert (faint.flag == AR.TOO_FAINT).all() and (faint.iters == 1).all() and np.isnan(faint.delta).all()
    assert (faint.pos_stderr_px().max(axis=1) > 0.2).all() and got.n_epochs[FAINT] == 0
    assert (got.status == 0).all() and (got.flag == AR.OK).sum() >= 25
    assert got.n_epochs.tolist() == [int((got[s].flag == AR.OK).sum()) for s in range(9)]


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
    return f, AR.astrom_reference(f.images, f.patches, f.neighbors, f.vp, list(range(len(catalog))))


def test_one_tile_more_than_a_round_against_the_restatement(lib):
    """one 32 x 65 patch (2080 pixels, 33 tiles) per image: the solve takes tiles in rounds of 32, so the second round (one
    tile, the other LDS buffer, the sums carried across rounds) runs in every pass"""
    if "round" not in _FIX:
        _FIX["round"] = _boxed_field(40, 80, [((4, 35), (8, 72))], 33, "32 x 65")
    f, ref = _FIX["round"]
    assert f.patches[0][0].active_pixel_bitmap.shape == (32, 65) and (32 * 65 + 63) // 64 == 33
    got = _run(f)
    _compare(got, ref, "32 x 65")
    assert (got.flag == AR.OK).all() and (got.n_pix == 2080).all() and len(got.n_pix) == 5


# ---- parameters ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol", [1e-9, 1e-3])
def test_pass_counts_at_other_tolerances(lib, tol):
    """iters is the number of passes the header's rule makes, restated in extended precision, at a tight and a loose tol_sigma"""
    f, _ = _fixture("sample_two_body")
    key = ("two_body", tol)
    if key not in _FIX:
        _FIX[key] = AR.astrom_reference(f.images, f.patches, f.neighbors, f.vp, [0, 1], tol_sigma=tol)
    got = _run(f, tol_sigma=tol)
    _compare(got, _FIX[key], "two_body at %.0e" % tol, tol_sigma=tol)
    base = _run(f)
    ok = (got.flag == AR.OK) & (base.flag == AR.OK)
    assert ok.sum() >= 6
    assert ((got.iters[ok] >= base.iters[ok]) if tol < 1e-6 else (got.iters[ok] <= base.iters[ok])).all()
    assert (got.iters[ok] != base.iters[ok]).any()


def test_max_iters_and_max_shift(lib):
    f, _ = _edge_scene()
    a = _run(f)
    one = _run(f, max_iters=1)
    solved = ~np.isin(a.flag, [AR.NO_LIGHT, AR.TOO_FAINT])
    assert (one.iters[solved] == 1).all() and (one.flag[solved] == AR.NOT_CONVERGED).all()
    assert (one.delta[solved] == 0).all() and (one.alpha[solved] == 1).all() and np.isfinite(one.cov[solved]).all()
    assert (one.n_epochs == 0).all() and np.isnan(one.summary).all()
    assert np.array_equal(one.flag[~solved], a.flag[~solved]) and np.array_equal(one.n_pix, a.n_pix)
    # the fixtures' rows are perturbed by most of a pixel: a range of a quarter of a pixel is left by an accepted iterate
    g, _ = _fixture("sample_star")
    wide, tight = _run(g), _run(g, max_shift_px=0.25)
    assert (wide.flag == AR.OK).all() and (np.abs(wide.delta).max(axis=1) > 0.5).all()
    assert (tight.flag == AR.OUT_OF_RANGE).all() and (np.abs(tight.delta).max(axis=1) > 0.25).all() and (tight.n_epochs == 0).all()
    assert (tight.iters < wide.iters).all() and np.isfinite(tight.cov).all()


# ---- equal bits ------------------------------------------------------------------------------------------------------------
def test_determinism_and_batch_invariance(lib):
    """the same bits for every entry: the call made twice, the targets reversed, one target repeated, one call per target,
    a second context, another CELESTE_CHUNK_PX on a fresh context"""
    from celeste_jl_amd import astrom
    f, _ = _edge_scene()
    targets = list(range(len(f.catalog)))
    with astrom.AstromContext(_problem(f)) as ac:
        a = ac.offsets(f.vp, targets)
        assert _same(a, ac.offsets(f.vp, targets))
        r = ac.offsets(f.vp, targets[::-1])
        for k, t in enumerate(targets[::-1]):
            assert _same(r[k], a[t]), t
        rep = ac.offsets(f.vp, [3, 0, 3, 8, 3])
        for k, t in enumerate([3, 0, 3, 8, 3]):
            assert _same(rep[k], a[t]), t
        for t in targets:
            assert _same(ac.offsets(f.vp, [t]), a[t]), t
        ms = ac.last_ms()
        assert len(ms) == 4 and all(x >= 0 for x in ms) and ms[1] > 0 and ms[2] > 0
        with astrom.AstromContext(_problem(f)) as other:
            assert _same(other.offsets(f.vp, targets), a)
    old = os.environ.get("CELESTE_CHUNK_PX")
    os.environ["CELESTE_CHUNK_PX"] = "64"
    try:
        with astrom.AstromContext(_problem(f)) as ac:
            assert _same(ac.offsets(f.vp, targets), a)
    finally:
        if old is None:
            del os.environ["CELESTE_CHUNK_PX"]
        else:
            os.environ["CELESTE_CHUNK_PX"] = old


def test_a_non_finite_row_fails_its_target_and_its_neighbours_alone(lib):
    from celeste_jl_amd import cabi
    f, _ = _edge_scene()
    S = len(f.catalog)
    clean = _run(f)
    t = 0
    assert f.neighbors[t] == [1]
    vp = f.vp.copy()
    vp[t] = np.nan
    got = _run(f, vp=vp)
    assert got.status[t] == cabi.ERR_NONFINITE_INPUT and (got[t].flag == AR.BAD_MODEL).all() and (got[t].iters == 0).all()
    for k in ("delta", "alpha", "fisher", "cov", "chi2", "loglik"):
        assert np.isnan(getattr(got[t], k)).all(), k
    assert np.array_equal(got.n_pix, clean.n_pix) and got.n_epochs[t] == 0 and np.isnan(got.summary[t]).all()
    seen = [s for s in range(S) if t in f.neighbors[s]]
    assert seen == [1] and got.status[1] == cabi.ERR_NONFINITE_RESULT and (got[1].flag == AR.BAD_MODEL).all()
    assert (got[1].iters == 0).all() and np.isnan(got[1].delta).all() and got.n_epochs[1] == 0
    for s in range(S):
        if s != t and s not in seen:
            assert _same(got[s], clean[s]), s


def test_refusals_with_a_context(lib):
    from celeste_jl_amd import astrom, cabi
    from test_astrom_host import BAD_PARAMS, _call_args
    f, _ = _fixture("sample_two_body")
    with astrom.AstromContext(_problem(f)) as ac:
        for pos in [1, 3] + list(range(6, 21)):                          # a NULL pointer (4: params and 5: epochs may be NULL)
            args, arrays = _call_args(ctx=ac.handle)
            args[pos] = None
            assert ac.lib.celeste_astrom_offsets(*args) == cabi.ERR_INVALID_ARG, pos
            assert all((a == -7).all() for a in arrays[2:])
        cases = [dict(n=-1)] + [dict(params=astrom.ParamsT(*p, 0)) for p in BAD_PARAMS]
        cases += [dict(epochs=np.array([0.0, 1.0, np.nan, 3.0, 4.0])), dict(epochs=np.array([0.0, 1.0, 2.0, 3.0, np.inf]))]
        for kw in cases:
            args, arrays = _call_args(ctx=ac.handle, **kw)
            assert ac.lib.celeste_astrom_offsets(*args) == cabi.ERR_INVALID_ARG, kw
            assert all((a == -7).all() for a in arrays[2:])
        args, arrays = _call_args(ctx=ac.handle)
        arrays[1][0] = 2                                              # a target out of range
        assert ac.lib.celeste_astrom_offsets(*args) == cabi.ERR_INVALID_ARG
        args, arrays = _call_args(ctx=ac.handle, n=0)                 # no target: OK, nothing touched
        assert ac.lib.celeste_astrom_offsets(*args) == 0 and all((a == -7).all() for a in arrays[2:])
        with pytest.raises(ValueError):
            ac.offsets(f.vp, [2])
        with pytest.raises(ValueError):
            ac.offsets(f.vp, [0], epochs=[0.0, 1.0])
        e = ac.offsets(f.vp, [])
        assert len(e) == 0 and e.alpha.shape == (0,) and e.delta.shape == (0, 2) and e.summary.shape == (0, 22) and e.offsets.tolist() == [0]
        args, arrays = _call_args(ctx=ac.handle)                      # and a good call through the same lists: NULL params and epochs
        arrays[0][:] = f.vp
        assert ac.lib.celeste_astrom_offsets(*args) == 0
        off, image, flag, status = arrays[2], arrays[3], arrays[6], arrays[9]
        assert off.tolist() == [0, 5] and image[:5].tolist() == [0, 1, 2, 3, 4] and (flag[:5] != AR.BAD_MODEL).all() and status[0] == 0
        assert (image[5:] == -7).all()
        want = ac.offsets(f.vp, [0])
        assert np.array_equal(arrays[10][:10].reshape(5, 2), want.delta, equal_nan=True) and np.array_equal(flag[:5], want.flag)


# ---- several exposures -------------------------------------------------------------------------------------------------------
def test_moved_scene_against_the_restatement(lib):
    """three exposures of five bands; the moved source is the one the device flags, its displaced entries at the truth"""
    from scipy.stats import chi2
    import test_astrom_host as TH
    f, mv = AR.moved_scene()
    ref = TH._CACHE.get("moved") or AR.astrom_reference(f.images, f.patches, f.neighbors, f.vp, list(range(6)))
    TH._CACHE["moved"] = ref
    got = _run(f)
    _compare(got, ref, "moved scene")
    one = got[mv]
    TH.check_moved(f, mv, [(int(n), int(fl), np.array([d[0], d[1], a]), c) for n, fl, d, a, c in
                           zip(one.image, one.flag, one.delta, one.alpha, one.cov)], got.n_epochs, got.chi2_const, chi2)
    rel = np.abs(got.summary[:, :6] - ref.summary[:, :6]) / np.abs(ref.summary[:, :6])
    print("   against the restatement's own estimates: mean, mean_cov, chi2_const %.2e relative; chi2_const %s" %
          (np.nanmax(rel), np.round(got.chi2_const, 1).tolist()))
    assert got[mv].image.tolist() == list(range(15))


LINEAR_SEED = 3
LINEAR_EPOCHS = [0.0, 1.0, 2.5, 4.0]
LINEAR_MU_PX = (0.15, -0.1)        # pixels (rows, columns) per unit of the epochs


def _linear_scene():
    """four exposures of five bands at epochs 0, 1, 2.5, 4 under a rotated tangent-plane WCS; the brightest source moves by
    LINEAR_MU_PX pixels per unit time from its catalog position at t = 0.  Returns (Field, moving source, epochs per image,
    mu in the units of pos)."""
    if "linear" not in _FIX:
        import copy
        import math
        import wcs_scene
        from celeste_jl_amd import synthetic
        from celeste_jl_amd.model import TanWCS, get_sky_patches, neighbor_map, with_tan_wcs
        t = math.radians(30.0)                                    # the scene's sky and pixel scale, the grid turned by 30 degrees
        cd = wcs_scene.SCALE * np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]])
        wcs = TanWCS(wcs_scene.CRVAL, ((64 + 1) / 2.0, (80 + 1) / 2.0), cd)
        f0 = synthetic.make_field(64, 80, 5, seed=LINEAR_SEED, margin=14, perturb=False, wcs=wcs)
        catalog = f0.catalog
        mv = AR._brightest(catalog)
        img0 = f0.images[0]
        pix0 = np.asarray(img0.world_to_pix(catalog[mv].pos), dtype=np.float64)
        images, epochs = [], []
        for k, t in enumerate(LINEAR_EPOCHS):
            cat = copy.deepcopy(catalog)
            cat[mv].pos = np.asarray(img0.pix_to_world(pix0 + t * np.array(LINEAR_MU_PX)), dtype=np.float64)
            if k == 0:
                more = list(f0.images)
            else:
                more = synthetic.blank_images(64, 80)
                for im in more:
                    with_tan_wcs(im, wcs)
                synthetic.gen_images(more, cat, np.random.Generator(np.random.PCG64([LINEAR_SEED, k])))
            images += more
            epochs += [t] * 5
        patches = get_sky_patches(images, catalog)
        f = synthetic.Field(images, catalog, patches, neighbor_map(patches), f0.vp.copy(), "linear")
        J = np.asarray(patches[mv][0].wcs_jacobian, dtype=np.float64)
        _FIX["linear"] = (f, mv, np.array(epochs), np.linalg.solve(J, np.array(LINEAR_MU_PX)))
    return _FIX["linear"]


def test_linear_motion_scene_under_a_rotated_wcs(lib):
    """mu within 4 sigma of the truth; chi2_lin below the 0.999 quantile of its 2 n - 4 degrees of freedom and chi2_const above
    that of its 2 (n - 1); the summaries against the restatement over the device's own entries"""
    from scipy.stats import chi2
    f, mv, epochs, mu = _linear_scene()
    J = np.asarray(f.patches[mv][0].wcs_jacobian, dtype=np.float64)
    assert abs(J[0, 1]) > 0.1 * abs(J[0, 0]) and len(f.images) == 20                 # rotated: the axes mix
    got = _run(f, targets=[mv], epochs=epochs)
    n = int(got.n_epochs[0])
    assert got.summary_flag[0] == 0 and n >= 10 and got.status[0] == 0
    worst = _summary_error(got, 0, epochs)
    z = (got.motion[0] - mu) / np.sqrt(np.diag(got.motion_cov[0])[2:])
    print("linear motion: %d epochs, mu %s (truth %s), pulls %s; chi2_lin %.1f (quantile %.1f), chi2_const %.1f (quantile %.1f); "
          "summaries %.2e" % (n, got.motion[0], mu, np.round(z, 2), got.chi2_lin[0], chi2.ppf(0.999, 2 * n - 4), got.chi2_const[0],
                              chi2.ppf(0.999, 2 * n - 2), worst))
    assert worst <= SUMMARY_RTOL
    assert (np.abs(z) <= 4).all()
    assert got.chi2_lin[0] < chi2.ppf(0.999, 2 * n - 4) and got.chi2_const[0] > chi2.ppf(0.999, 2 * n - 2)
    assert got.t_ref[0] == np.mean([epochs[i] for i, fl in zip(got.image, got.flag) if fl == AR.OK])
    # NULL epochs: the image index is the time; a constant index step per exposure it is not, so the motion differs
    idx = _run(f, targets=[mv])
    assert idx.summary_flag[0] == 0 and not np.array_equal(idx.motion, got.motion) and np.array_equal(idx.delta, got.delta, equal_nan=True)
    assert np.array_equal(idx.mean, got.mean) and idx.chi2_const[0] == got.chi2_const[0]


def test_sparse_and_dense_multifield_agree_bit_for_bit(lib):
    """visit lists against the dense S x N table; a source has one entry per image it lies in"""
    from celeste_jl_amd import synthetic
    fs = synthetic.make_multifield((2, 3), 160, 160, 0.10, 70, seed=11, sparse=True)
    fd = synthetic.make_multifield((2, 3), 160, 160, 0.10, 70, seed=11, sparse=False)
    gs, gd = _run(fs), _run(fd)
    assert _same(gs, gd)
    n_ent = np.diff(gs.offsets)
    assert n_ent.max() >= 10 and n_ent.min() == 5 and gs.n_epochs.max() >= 2
    assert np.array_equal(gs.n_epochs, np.array([(gs[s].flag == 0).sum() for s in range(len(fs.catalog))]))
    assert (gs.flag == AR.OK).sum() >= 20 and (gs.status == 0).all()


# ---- infer_box ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["catalog", "catalog, prep on the device", "no catalog"])
def test_infer_box_attaches_the_astrometry(lib, case):
    import celeste_jl_amd as cel
    from celeste_jl_amd import astrom, cabi, model, synthetic
    from celeste_jl_amd.catalog import ASTROMETRY_COLUMNS, celeste_to_rows
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
    epochs = [0.0, 0.5, 1.0, 2.0, 4.0]
    plain = cel.infer_box(f.images, box, method="joint_vi", cfg=cfg, **kw)
    res = cel.infer_box(f.images, box, method="joint_vi", cfg=cfg, astrometry=True, epochs=epochs, **kw)
    targets = [i for i, ce in enumerate(catalog) if box.contains(ce.pos)]
    assert len(res) == len(plain) == len(targets) >= 10
    assert all(p.astrometry is None for p in plain) and all(isinstance(r.astrometry, astrom.Astrometry) for r in res)
    assert all(r.fit is None and r.light_curve is None for r in res)
    for p, r in zip(plain, res):
        assert p.vs.tobytes() == r.vs.tobytes() and (p.init_ra, p.init_dec, p.is_sky_bad, p.failed) == (r.init_ra, r.init_dec, r.is_sky_bad, r.failed)
    vp = init_source_table(catalog)
    vp[targets] = np.stack([r.vs for r in res])
    with astrom.AstromContext(problem) as ac:
        want = ac.offsets(vp, targets, epochs=epochs)
    for k, r in enumerate(res):
        assert len(r.astrometry) == 1 and r.astrometry.summary.shape == (1, 22) and _same(r.astrometry, want[k]), k
    assert (want.status == 0).all() and (np.diff(want.offsets) == 5).all() and (want.flag == 0).mean() > 0.3
    rows = celeste_to_rows(res, astrometry=True)
    assert len(rows) == sum(not r.is_sky_bad for r in res) and all(0 <= row["n_epochs_astrom"] <= 5 for row in rows)
    assert any(isinstance(row["pm_ra"], float) and row["pm_ra_stderr"] > 0 for row in rows)
    assert celeste_to_rows(res) == celeste_to_rows(plain)
    assert [{k: v for k, v in row.items() if k not in ASTROMETRY_COLUMNS} for row in rows] == celeste_to_rows(plain)


def test_mcmc_with_astrometry_raises(lib):
    import celeste_jl_amd as cel
    f, _ = _fixture("sample_two_body")
    with pytest.raises(ValueError, match="mcmc"):
        cel.infer_box(f.images, cel.BoundingBox(0.0, 30.0, 0.0, 30.0), f.catalog, method="mcmc", astrometry=True)
