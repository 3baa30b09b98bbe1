"""Position and shape standard errors on the device (libceleste_info.so) against the restatement (tests/info_reference.py):
every sum within 1e-10 of its sum |term|; n_pix, flags, statuses and NaN patterns exactly; the covariance step against mpmath
on the device's own sums; doubling, a bright neighbour, determinism and batch invariance; the isolation of a non-finite row;
the refusals; infer_box(..., uncertainties=True)."""
import os

import numpy as np
import pytest

import info_reference as IR

pytestmark = pytest.mark.gpu

SUM_TOL = 1e-10           # of sum |term|: the parity level the README states for the engine against its oracle
SOLVE_TOL = 1e-12         # times cond_2(R) max |inv(R)|: c n eps cond of a Cholesky inverse, n <= 6, 10 - 100 over n^2 eps
END_TO_END = 1e-6         # C from the device's sums against C from the restatement's, of sqrt(C_kk C_ll)
FIELDS = ("n_pix", "sums_star", "sums_gal", "cov_star", "cov_gal", "flag", "status")


def _problem(f, **kw):
    from celeste_jl_amd import cabi
    return cabi.Problem(f.images, f.patches, f.neighbors, **kw)


def _same(a, b):
    """equal bit for bit, NaNs included"""
    return all(np.array_equal(getattr(a, n), getattr(b, n), equal_nan=True) for n in FIELDS)


def _run(f, targets=None, vp=None, **kw):
    from celeste_jl_amd import info
    targets = list(range(len(f.catalog))) if targets is None else targets
    with info.InfoContext(_problem(f, **kw)) as ic:
        return ic.bounds(f.vp if vp is None else vp, targets)


def _compare(got, ref, name, conditioned=False):
    """sums, n_pix / flags / statuses / NaN patterns, the covariance step against mpmath on the device's sums, and C end to end;
    prints the measured figures before it asserts them.  conditioned: the reference flags no block ILL_CONDITIONED or
    NOT_POSITIVE (asserted)."""
    from celeste_jl_amd import info
    worst_sum = worst_solve = worst_e2e = 0.0
    worst_kappa = 0.0
    gsums, gcov = (got.sums_star, got.sums_gal), (got.cov_star, got.cov_gal)
    for ti in range(len(ref.status)):
        assert np.array_equal(got.n_pix[ti], ref.n_pix[ti]), (name, ti)
        assert got.status[ti] == ref.status[ti], (name, ti, got.status[ti], ref.status[ti])
        assert np.array_equal(got.flag[ti], ref.flag[ti]), (name, ti, got.flag[ti], ref.flag[ti])
        for i in range(2):
            g = IR.G[i]
            S, C = gsums[i][ti], gcov[i][ti]
            assert np.array_equal(np.isnan(C), np.isnan(ref.cov[i][ti])) and np.array_equal(np.isinf(C), np.isinf(ref.cov[i][ti])), (name, ti, i)
            if ref.status[ti] != 0:
                assert np.isnan(S).all() and np.isnan(C).all() and got.flag[ti, i] == info.NOT_POSITIVE, (name, ti, i)
                continue
            if conditioned:
                assert not ref.flag[ti, i] & (IR.ILL_CONDITIONED | IR.NOT_POSITIVE), (name, ti, i, ref.flag[ti, i], ref.kappa[ti, i])
            err, scale = np.abs(S - ref.sums[i][ti]), ref.abs_sums[i][ti]
            zero = scale == 0
            assert (S[zero] == 0).all(), (name, ti, i)
            if (~zero).any():
                worst_sum = max(worst_sum, float((err[~zero] / scale[~zero]).max()))
            # the covariance step on the device's own sums
            r = IR.solve(S, g)
            assert r.flag == got.flag[ti, i], (name, ti, i, r.flag, got.flag[ti, i])
            if r.rinv is None:
                continue
            Cf, Cr = info.unpack(C, g), info.unpack(ref.cov[i][ti], g)
            s = np.array([float(x) for x in r.s])
            keep = np.flatnonzero(np.isfinite(np.diag(Cf)))
            for k in keep:
                for l in keep:
                    e = abs(Cf[k, l] * s[k] * s[l] - float(r.rinv[int(k), int(l)])) / (r.kappa * r.rinv_max)
                    worst_solve = max(worst_solve, e)
                    worst_e2e = max(worst_e2e, abs(Cf[k, l] - Cr[k, l]) / np.sqrt(Cr[k, k] * Cr[l, l]))
            worst_kappa = max(worst_kappa, r.kappa)
    print("info parity %-24s sums %.3e of sum|term| (bound %.0e)  solve %.3e of cond max|inv R| (bound %.0e; largest cond %.3e)  "
          "C end to end %.3e (bound %.0e)" % (name, worst_sum, SUM_TOL, worst_solve, SOLVE_TOL, worst_kappa, worst_e2e, END_TO_END))
    assert worst_sum <= SUM_TOL, (name, worst_sum)
    assert worst_solve <= SOLVE_TOL, (name, worst_solve)
    assert worst_e2e <= END_TO_END, (name, worst_e2e)


# ---- the committed fixtures ------------------------------------------------------------------------------------------------
_FIX = {}


def _fixture(name):
    if name not in _FIX:
        import golden_util as G
        f = G.arrays_to_field(np.load(G.path(name)))
        _FIX[name] = (f, IR.info_reference(f.images, f.patches, f.neighbors, f.vp, list(range(len(f.catalog)))))
    return _FIX[name]


@pytest.mark.parametrize("name", ["sample_star", "sample_galaxy", "sample_two_body", "field_64x80_8src_nan",
                                  "field_72x88_9src_variable"])
def test_fixture_against_the_restatement(lib, name):
    f, ref = _fixture(name)
    got = _run(f)
    assert (ref.status == 0).all() and ref.n_pix.sum() > 0
    _compare(got, ref, name, conditioned=True)
    assert (got.flag == 0).all()
    for i in range(2):
        assert (got.pos_stderr(i) > 0).all() and np.isfinite(got.pos_stderr(i)).all() and (np.abs(got.pos_corr(i)) < 1).all()
    assert (got.shape_stderr() > 0).all()


# ---- a scene of edge cases ---------------------------------------------------------------------------------------------------
def _edge_field():
    """the edge scene of tests/test_gpu_fit.py, from the same recipe: 48 x 60 images, the fifth shifted by 20 rows.  Sources 0-2:
    patches of 9 x 9 = 81 pixels (not a multiple of 64), 0 and 1 in a row so that the last column of 0's patch lies inside 1's;
    0 is off the fifth image.  Sources 3-5: patches of 17 x 17 = 289 pixels (across the 256-pixel chunk), three that overlap
    one another."""
    if "edge field" not in _FIX:
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
        _FIX["edge field"] = synthetic.Field(images, catalog, patches, neighbor_map(patches), vp, "edge")
    return _FIX["edge field"]


def _edge_scene():
    if "edge" not in _FIX:
        f = _edge_field()
        _FIX["edge"] = (f, IR.info_reference(f.images, f.patches, f.neighbors, f.vp, list(range(6))))
    return _FIX["edge"]


def _edge_device():
    """the device's numbers of the edge scene's six targets, once per module"""
    if "edge device" not in _FIX:
        _FIX["edge device"] = _run(_edge_field())
    return _FIX["edge device"]


def test_edge_scene_against_the_restatement(lib):
    f, ref = _edge_scene()
    sizes = [[p.active_pixel_bitmap.shape for p in row] for row in f.patches]
    assert sizes[0][0] == (9, 9) and sizes[3][0] == (17, 17) and 0 in sizes[0][4] and 0 not in sizes[3][4]
    assert 1 in f.neighbors[0] and {4, 5} <= set(f.neighbors[3]) and 5 in f.neighbors[4]
    got = _edge_device()
    _compare(got, ref, "edge scene", conditioned=True)
    assert got.n_pix[0].tolist() == [81, 81, 81, 81, 0] and got.n_pix[3, 0] == 289
    assert (got.sums_star[0, 4] == 0).all() and (got.sums_gal[0, 4] == 0).all()      # source 0 has no patch in the fifth image
    assert (got.sums_star[0, :4, 5] > 0).all() and (got.flag == 0).all()


def test_rotated_tangent_plane_scene_against_the_restatement(lib):
    """the scene of tests/test_gpu_wcs.py (fields turned by 0, 30 and 90 degrees, one flipped): the position chain through a
    Jacobian that is not diagonal.  Three targets: the ones with the most patches in the turned fields.  The table is the
    catalog's (the scene's own perturbation moves a position by pixels' worth of degrees)."""
    import wcs_scene
    f = wcs_scene.tan_multifield(perturb=False)
    S = len(f.catalog)

    def turned(s):
        return sum(1 for n in range(5, 15) if 0 not in f.patches[s][n].active_pixel_bitmap.shape)
    targets = sorted(range(S), key=lambda s: -turned(s))[:3]
    assert all(turned(s) >= 5 for s in targets)
    J = [np.asarray(f.patches[s][n].wcs_jacobian) for s in targets for n in range(5, 10)
         if 0 not in f.patches[s][n].active_pixel_bitmap.shape]
    assert J and all(abs(j[0, 1]) > 0.3 * abs(j[0, 0]) for j in J)                      # 30 degrees: tan = 0.58
    ref = IR.info_reference(f.images, f.patches, f.neighbors, f.vp, targets)
    got = _run(f, targets)
    assert (ref.status == 0).all()
    _compare(got, ref, "rotated tangent planes")
    assert (np.abs(got.pos_corr(0)) > 0).all()


def test_three_psf_components_against_the_restatement(lib):
    """psf_K = 3: 42 galaxy components per source (test_gpu_parity.py's recipe on the two-body sample)"""
    from celeste_jl_amd import synthetic
    from celeste_jl_amd.model import ConstantPSFMap, get_sky_patches, neighbor_map, render_psf
    K = 3
    f = synthetic.make_sample_dataset("two_body")
    rng = np.random.default_rng(K)
    for img in f.images:
        w = rng.dirichlet(np.ones(K) * 4)
        comps = []
        for k in range(K):
            s = 1.1 + 0.9 * k + 0.2 * rng.random()
            comps.append([w[k], 0.3 * rng.normal(), 0.3 * rng.normal(), s * s, 0.1 * s * s * rng.normal(), s * s * (1 + 0.2 * rng.random())])
        img.psf = np.array(comps)
        img.psfmap = ConstantPSFMap(render_psf(img.psf, (51, 51)))
    patches = get_sky_patches(f.images, f.catalog)
    f = synthetic.Field(f.images, f.catalog, patches, neighbor_map(patches), f.vp, "psf_K=3")
    assert patches[0][0].psf.shape == (3, 6)
    ref = IR.info_reference(f.images, f.patches, f.neighbors, f.vp, [0, 1])
    got = _run(f, psf_K=K)
    assert (ref.status == 0).all()
    _compare(got, ref, "psf_K = 3")


def test_round_galaxy_and_pure_profiles_against_the_restatement(lib):
    """gal_axis_ratio = 1 exactly leaves gal_angle without any information (UNCONSTRAINED: inf and zeros, the rest solved
    without it); gal_frac_dev at 0 and at 1 (one profile has no weight; its derivative has)"""
    from celeste_jl_amd import info
    from celeste_jl_amd.params import ids
    f = _edge_field()
    vp = f.vp.copy()
    vp[1, ids.gal_axis_ratio] = 1.0
    vp[3, ids.gal_frac_dev] = 0.0
    vp[5, ids.gal_frac_dev] = 1.0
    targets = [1, 3, 5]
    ref = IR.info_reference(f.images, f.patches, f.neighbors, vp, targets)
    got = _run(f, targets, vp=vp)
    assert (ref.status == 0).all()
    _compare(got, ref, "round galaxy, pure profiles")
    assert got.flag.tolist() == [[0, info.UNCONSTRAINED], [0, 0], [0, 0]]
    C = got.cov(1)[0]
    assert C[4, 4] == np.inf and (np.delete(C[4], 4) == 0).all() and np.isfinite(np.delete(np.delete(C, 4, 0), 4, 1)).all()
    assert (got.sums_gal[0][:, [4, 9, 13, 16, 18, 19, 25]] == 0).all()                 # A[., 4] and c[4]: exact zeros
    assert np.isfinite(got.shape_stderr()[1:]).all() and (got.shape_stderr()[1:, 0] > 0).all()


# ---- the covariance step alone -----------------------------------------------------------------------------------------------
def test_solve_on_hand_made_matrices(lib):
    from celeste_jl_amd import info
    f, _ = _fixture("sample_star")
    cases = IR.hand_made()
    names = list(cases)
    s0, s1 = np.zeros((len(names), 5, 6)), np.zeros((len(names), 5, 28))
    for k, name in enumerate(names):
        rows = cases[name][0]
        (s0 if rows.shape[1] == 6 else s1)[k] = rows
    with info.InfoContext(_problem(f)) as ic:
        c0, c1, fl = ic.solve(s0, s1)
        assert _same_solve((c0, c1, fl), ic.solve(s0, s1))
        e0, e1, efl = ic.solve(np.zeros((0, 5, 6)), np.zeros((0, 5, 28)))
        assert e0.shape == (0, 3) and e1.shape == (0, 21) and efl.shape == (0, 2)
    for k, name in enumerate(names):
        rows, flag, want = cases[name]
        i = 0 if rows.shape[1] == 6 else 1
        g = IR.G[i]
        C = info.unpack((c0, c1)[i][k], g)
        assert fl[k, i] == flag and fl[k, 1 - i] == info.NO_PIXELS, (name, fl[k])
        assert np.isnan((c0, c1)[1 - i][k]).all()
        r = IR.solve(rows, g)
        assert np.array_equal(np.isnan(C), np.isnan(info.unpack(r.cov, g))) and np.array_equal(np.isinf(C), np.isinf(info.unpack(r.cov, g))), name
        if want is None:
            assert np.isnan(C).all(), name
            continue
        s = np.array([float(x) for x in r.s])
        keep = np.flatnonzero(np.isfinite(np.diag(C)))
        err = max(abs(C[a, b] * s[a] * s[b] - float(r.rinv[int(a), int(b)])) for a in keep for b in keep) / (r.kappa * r.rinv_max)
        print("solve %-18s cond %.3e  error %.3e of cond max|inv R| (bound %.0e)" % (name, r.kappa, err, SOLVE_TOL))
        assert err <= SOLVE_TOL, (name, err)
        drop = [a for a in range(g) if a not in keep]
        for a in drop:
            assert C[a, a] == np.inf and (np.delete(C[a], a) == 0).all(), name
    assert np.array_equal(c1[names.index("diagonal")][[0, 6, 11]], [1.0, 0.25, 1.0 / 9.0])


def _same_solve(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


# ---- properties of the device's own output -----------------------------------------------------------------------------------
def _full_sums(rows, g):
    """[5, NSUM] -> [5, g + 1, g + 1]: the information of (geometry, the band's scale) per band"""
    from celeste_jl_amd import info
    na = g * (g + 1) // 2
    M = np.zeros((5, g + 1, g + 1))
    M[:, :g, :g] = info.unpack(rows[:, :na], g)
    M[:, :g, g] = M[:, g, :g] = rows[:, na:na + g]
    M[:, g, g] = rows[:, na + g]
    return M


def test_doubling_every_exposure_doubles_the_sums_and_halves_the_covariances(lib):
    """the image list twice: every sum doubles and every covariance halves, to 1e-12 of sqrt(M_kk M_ll) -- the size of an
    entry of a positive semi-definite matrix (an off-diagonal sum cancels and can be far smaller than its terms)"""
    from celeste_jl_amd import synthetic
    f, _ = _fixture("sample_two_body")
    f2 = synthetic.Field(f.images + f.images, f.catalog, [row + row for row in f.patches], f.neighbors, f.vp, "twice")
    a, b = _run(f), _run(f2)
    assert np.array_equal(b.n_pix, 2 * a.n_pix) and (a.status == 0).all() and (b.status == 0).all() and (b.flag == 0).all()
    worst = 0.0
    for i, (sa, sb, ca, cb) in enumerate(((a.sums_star, b.sums_star, a.cov_star, b.cov_star), (a.sums_gal, b.sums_gal, a.cov_gal, b.cov_gal))):
        g = IR.G[i]
        for t in range(2):
            Ma, Mb = _full_sums(sa[t], g), _full_sums(sb[t], g)
            d = np.sqrt(np.einsum("bk,bl->bkl", np.einsum("bkk->bk", Ma), np.einsum("bkk->bk", Ma)))
            worst = max(worst, float((np.abs(Mb - 2 * Ma) / (2 * d)).max()))
        Ca, Cb = a.cov(i), b.cov(i)
        d = np.sqrt(np.einsum("tk,tl->tkl", np.einsum("tkk->tk", Ca), np.einsum("tkk->tk", Ca)))
        worst = max(worst, float((np.abs(2 * Cb - Ca) / d).max()))
    print("doubling: worst %.3e (bound 1e-12)" % worst)
    assert worst <= 1e-12


def test_a_bright_overlapping_neighbour_costs_position_information(lib):
    """sources 0 and 2 of the edge scene alone, then with source 1 (whose patch overlaps 0's) in the table, ten times as bright:
    both position variances of 0 grow, in both blocks; 2 overlaps nobody and keeps its bits"""
    import math
    from celeste_jl_amd import synthetic
    from celeste_jl_amd.model import neighbor_map
    from celeste_jl_amd.params import ids
    f = _edge_field()
    pa = [f.patches[0], f.patches[2]]
    alone = synthetic.Field(f.images, [f.catalog[0], f.catalog[2]], pa, neighbor_map(pa), f.vp[[0, 2]], "alone")
    pb = [f.patches[0], f.patches[1], f.patches[2]]
    vp = f.vp[[0, 1, 2]].copy()
    vp[1, ids.flux_loc] += math.log(10.0)
    crowd = synthetic.Field(f.images, f.catalog[:3], pb, neighbor_map(pb), vp, "crowd")
    assert alone.neighbors == [[], []] and crowd.neighbors == [[1], [0], []]
    a, b = _run(alone), _run(crowd, [0, 2])
    assert (a.status == 0).all() and (b.status == 0).all() and (a.flag == 0).all() and (b.flag == 0).all()
    for i in range(2):
        va, vb = a.pos_stderr(i)[0] ** 2, b.pos_stderr(i)[0] ** 2
        print("type %d: position variances alone %s, with the neighbour %s" % (i, va, vb))
        assert (vb > va).all()
    assert _same(a[1:2], b[1:2])


def test_determinism_and_batch_invariance(lib):
    """the same bits for every target: the call made twice, the targets shuffled, one target repeated, the call cut in two,
    CELESTE_CHUNK_PX = 64 on a fresh context"""
    from celeste_jl_amd import info
    f = _edge_field()
    targets = list(range(6))
    with info.InfoContext(_problem(f)) as ic:
        a = ic.bounds(f.vp, targets)
        assert _same(a, ic.bounds(f.vp, targets))
        order = [4, 0, 5, 2, 1, 3]
        r = ic.bounds(f.vp, order)
        for k, t in enumerate(order):
            assert _same(r[k:k + 1], a[t:t + 1]), t
        rep = ic.bounds(f.vp, [3, 0, 3, 5, 3])
        for k, t in enumerate([3, 0, 3, 5, 3]):
            assert _same(rep[k:k + 1], a[t:t + 1]), t
        assert _same(ic.bounds(f.vp, targets[:2]), a[:2]) and _same(ic.bounds(f.vp, targets[2:]), a[2:])
    assert _same(a, _edge_device())                               # another context
    old = os.environ.get("CELESTE_CHUNK_PX")
    os.environ["CELESTE_CHUNK_PX"] = "64"
    try:
        with info.InfoContext(_problem(f)) as ic:
            assert _same(ic.bounds(f.vp, targets), a)
    finally:
        if old is None:
            del os.environ["CELESTE_CHUNK_PX"]
        else:
            os.environ["CELESTE_CHUNK_PX"] = old


def test_a_non_finite_row_fails_its_target_alone(lib):
    from celeste_jl_amd import cabi, info
    f, ref = _edge_scene()
    S = len(f.catalog)
    clean = _edge_device()
    t = 0
    assert f.neighbors[t] == [1]
    vp = f.vp.copy()
    vp[t] = np.nan
    got = _run(f, vp=vp)
    assert got.status[t] == cabi.ERR_NONFINITE_INPUT
    seen = [s for s in range(S) if t in f.neighbors[s]]
    assert seen == [1] and got.status[1] == cabi.ERR_NONFINITE_RESULT      # its light is part of its neighbour's lam
    for s in (t, 1):
        assert np.isnan(got.sums_star[s]).all() and np.isnan(got.sums_gal[s]).all() and np.isnan(got.cov_star[s]).all() and \
            np.isnan(got.cov_gal[s]).all() and (got.flag[s] == info.NOT_POSITIVE).all()
    assert np.array_equal(got.n_pix, clean.n_pix)
    others = [s for s in range(S) if s != t and s not in seen]
    assert others
    for s in others:
        assert _same(got[s:s + 1], clean[s:s + 1]), s
    # the restatement says the same of the two it touches
    ref2 = IR.info_reference(f.images, f.patches, f.neighbors, vp, [0, 1])
    assert ref2.status.tolist() == [cabi.ERR_NONFINITE_INPUT, cabi.ERR_NONFINITE_RESULT] and (ref2.flag == IR.NOT_POSITIVE).all()
    assert np.array_equal(ref2.n_pix, got.n_pix[:2])


def test_refusals_with_a_context(lib):
    from celeste_jl_amd import cabi, info
    f, _ = _fixture("sample_two_body")
    dp, ip, lp = cabi.c_double_p, cabi.c_int32_p, cabi.c_int64_p
    p = info._ptr
    with info.InfoContext(_problem(f)) as ic:
        vp = np.ascontiguousarray(f.vp)
        tg = np.array([0, 1], dtype=np.int32)
        n_pix = np.full((2, 5), -7, dtype=np.int64)
        s0, s1, c0, c1 = np.full((2, 5, 6), -7.0), np.full((2, 5, 28), -7.0), np.full((2, 3), -7.0), np.full((2, 21), -7.0)
        fl, status = np.full((2, 2), -7, dtype=np.int32), np.full(2, -7, dtype=np.int32)
        outs = [n_pix, s0, s1, c0, c1, fl, status]
        h = ic.handle
        good = [h, p(vp, dp), 2, p(tg, ip), p(n_pix, lp), p(s0, dp), p(s1, dp), p(c0, dp), p(c1, dp), p(fl, ip), p(status, ip)]
        for pos in (1, 3, 4, 5, 6, 7, 8, 9, 10):                  # a NULL pointer
            args = list(good)
            args[pos] = None
            assert ic.lib.celeste_info_bounds(*args) == cabi.ERR_INVALID_ARG, pos
        for bad in ([0, 2], [-1, 0]):                             # a target out of range
            args = list(good)
            args[3] = p(np.array(bad, dtype=np.int32), ip)
            assert ic.lib.celeste_info_bounds(*args) == cabi.ERR_INVALID_ARG
        args = list(good)
        args[2] = -1
        assert ic.lib.celeste_info_bounds(*args) == cabi.ERR_INVALID_ARG
        args = list(good)
        args[2] = 0                                               # no target: OK, nothing touched
        assert ic.lib.celeste_info_bounds(*args) == 0
        assert ic.lib.celeste_info_bounds(h, p(vp, dp), 0, None, None, None, None, None, None, None, None) == 0
        sgood = [h, 2, p(s0, dp), p(s1, dp), p(c0, dp), p(c1, dp), p(fl, ip)]
        for pos in (2, 3, 4, 5, 6):
            args = list(sgood)
            args[pos] = None
            assert ic.lib.celeste_info_solve(*args) == cabi.ERR_INVALID_ARG, pos
        args = list(sgood)
        args[1] = -1
        assert ic.lib.celeste_info_solve(*args) == cabi.ERR_INVALID_ARG
        assert ic.lib.celeste_info_solve(h, 0, None, None, None, None, None) == 0
        assert all((a == -7).all() for a in outs)
        with pytest.raises(ValueError):
            ic.bounds(f.vp, [2])
        e = ic.bounds(f.vp, [])
        assert e.n_pix.shape == (0, 5) and e.sums_gal.shape == (0, 5, 28) and e.cov_gal.shape == (0, 21) and e.flag.shape == (0, 2)
        assert ic.lib.celeste_info_bounds(*good) == 0 and (status == 0).all() and (n_pix >= 0).all() and (fl == 0).all()
        ms = ic.last_ms()
        assert len(ms) == 4 and all(x >= 0 for x in ms) and ms[1] > 0


# ---- infer_box ---------------------------------------------------------------------------------------------------------------
def test_infer_box_attaches_the_uncertainty(lib):
    import celeste_jl_amd as cel
    from celeste_jl_amd import cabi, info, model, synthetic
    from celeste_jl_amd.catalog import UNCERTAINTY_COLUMNS, celeste_to_rows
    from celeste_jl_amd.params import init_source_table
    f = synthetic.make_field(200, 240, 40, seed=4)
    box = cel.BoundingBox(0.0, 200.0, 0.0, 240.0)
    cfg = cel.ElboConfig(max_iters=8)
    plain = cel.infer_box(f.images, box, f.catalog, method="joint_vi", cfg=cfg)
    res = cel.infer_box(f.images, box, f.catalog, method="joint_vi", cfg=cfg, uncertainties=True)
    targets = [i for i, ce in enumerate(f.catalog) if box.contains(ce.pos)]
    assert len(res) == len(plain) == len(targets) >= 10
    assert all(p.uncertainty is None for p in plain) and all(isinstance(r.uncertainty, info.InfoBounds) for r in res)
    for p, r in zip(plain, res):
        assert p.vs.tobytes() == r.vs.tobytes() and (p.init_ra, p.init_dec, p.is_sky_bad, p.failed) == (r.init_ra, r.init_dec, r.is_sky_bad, r.failed)
    table = model.table_for(f.images, f.catalog, False)
    problem = cabi.problem_from_table(f.images, table, table.neighbors())
    vp = init_source_table(f.catalog)
    vp[targets] = np.stack([r.vs for r in res])
    with info.InfoContext(problem) as ic:
        want = ic.bounds(vp, targets)
    for k, r in enumerate(res):
        assert r.uncertainty.n_pix.shape == (5,) and r.uncertainty.cov_gal.shape == (21,) and r.uncertainty.flag.shape == (2,)
        assert _same(r.uncertainty, want[k])
    assert (want.status == 0).all() and (want.n_pix.sum(axis=1) > 0).all()
    rows = celeste_to_rows(res, uncertainties=True)
    kept = [r for r in res if not r.is_sky_bad]
    assert len(rows) == len(kept)
    for row, r in zip(rows, kept):
        assert all(c in row for c in UNCERTAINTY_COLUMNS)
        t = int(r.uncertainty.chosen(r.vs))
        if not r.uncertainty.flag[t] & (info.NO_PIXELS | info.NOT_POSITIVE):
            assert row["ra_stderr"] > 0 and row["dec_stderr"] > 0 and abs(row["ra_dec_corr"]) < 1
        assert (row["gal_radius_px_stderr"] is None) == (t == 0) or row["gal_radius_px_stderr"] is None
    assert sum(row["ra_stderr"] is not None for row in rows) >= len(rows) - 2
    assert celeste_to_rows(res) == celeste_to_rows(plain)


def test_mcmc_with_uncertainties_raises(lib):
    import celeste_jl_amd as cel
    f, _ = _fixture("sample_two_body")
    with pytest.raises(ValueError, match="mcmc"):
        cel.infer_box(f.images, cel.BoundingBox(0.0, 30.0, 0.0, 30.0), f.catalog, method="mcmc", uncertainties=True)
