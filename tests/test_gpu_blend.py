"""maximize! with several active sources on the device (libceleste_blend.so): the multi-active ElboArgs path of
celeste_jl_amd.maximize, the batched evaluation against celeste_elbo_eval_multi and the CPU restatement, the
general-dimension trust-region sub-problem, Sa = 1 blends against celeste_maximize_batch, determinism and batch
invariance, the refusals and the isolation of a failing blend."""
import ctypes as C

import numpy as np
import pytest

import tr_reference as R

pytestmark = pytest.mark.gpu


def rel_err(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(np.asarray(b))), 1e-300))


def symmetric_neighbors(neighbors, S):
    nb = [set(neighbors[s]) for s in range(S)]
    for s in range(S):
        for t in neighbors[s]:
            nb[t].add(s)
    return nb


def conflict_free_blends(neighbors, S, rng, max_sa=4, min_sa=2):
    """groups of 2..max_sa overlapping sources, no member of one group a neighbour of a member of another"""
    nb = symmetric_neighbors(neighbors, S)
    owner = {}
    blends = []
    for s in rng.permutation(S):
        s = int(s)
        if s in owner or any(t in owner for t in nb[s]):
            continue
        bl = [s]
        for t in sorted(nb[s]):
            if len(bl) >= max_sa:
                break
            if t in owner or any(u in owner and u not in bl for u in nb[t]):
                continue
            bl.append(int(t))
        if len(bl) < min_sa:
            continue
        b = len(blends)
        for t in bl:
            owner[t] = b
        blends.append(bl)
    return blends


def crowded(seed, S=14, H=110, W=130, nan_fraction=0.02, punch=True):
    from celeste_jl_amd import synthetic
    rng = np.random.default_rng(seed)
    f = synthetic.make_field(H, W, S, seed=seed, nan_fraction=nan_fraction, margin=10)
    if punch:
        for s in range(S):
            if rng.random() < 0.4:
                p = f.patches[s][int(rng.integers(5))]
                p.active_pixel_bitmap &= rng.random(p.active_pixel_bitmap.shape) > 0.15
    return f, rng


def test_maximize_with_several_active_sources():
    """maximize!(ElboArgs(..., active_sources=[0, 1])) on three_body: both sources move, the ELBO rises, source 2 stays"""
    import celeste_jl_amd as cel
    from celeste_jl_amd import synthetic
    f = synthetic.make_sample_dataset("three_body")
    ea = cel.ElboArgs(f.images, f.patches, [0, 1])
    vp0 = f.vp.copy()
    before = cel.elbo(ea, vp0, calculate_gradient=False).v
    evals, value, vp = cel.maximize(ea, vp0.copy(), cel.ElboConfig(max_iters=20))
    after = cel.elbo(ea, vp, calculate_gradient=False).v
    assert evals >= 2 and after > before
    assert abs(value - after) <= 1e-10 * abs(after)
    assert not np.array_equal(vp[0], vp0[0]) and not np.array_equal(vp[1], vp0[1])
    assert np.array_equal(vp[2], vp0[2])


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_batched_evaluation_matches_eval_multi_and_the_oracle(oracle, seed):
    import celeste_jl_amd as cel
    f, rng = crowded(seed)
    S = len(f.patches)
    blends = conflict_free_blends(f.neighbors, S, rng)
    assert len(blends) >= 2
    ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
    for flags in (7, 5, 4):
        v, d, h, cnt, st = ctx.blend_context().eval_blends(f.vp, blends, flags)
        assert (st == 0).all()
        for b, bl in enumerate(blends):
            mv, md, mh, mcnt = ctx.eval_multi(f.vp, bl, flags)
            assert np.array_equal(cnt[b], mcnt)
            assert abs(v[b] - mv) <= 1e-12 * abs(mv)
            if flags & 3:
                assert np.all(np.abs(d[b] - md) <= 1e-12 * np.abs(md) + 1e-300), (b, rel_err(d[b], md))
            if flags & 2:
                assert np.array_equal(h[b], h[b].T)
                assert np.all(np.abs(h[b] - mh) <= 1e-12 * np.abs(mh) + 1e-300), (b, rel_err(h[b], mh))
            ov, od, oh, ocnt, ost = oracle.elbo_multi(ctx.problem, f.vp, bl, flags)
            assert ost == 0 and np.array_equal(cnt[b], ocnt)
            assert abs(v[b] - ov) <= 1e-8 * abs(ov)
            if flags & 3:
                assert max(rel_err(d[b][:, k], od[k]) for k in range(len(bl))) <= 1e-8
            if flags & 2:
                assert rel_err(h[b], oh) <= 1e-8


def blend_problems(oracle, sa):
    """(name, H, g, delta): -ELBO's free-space gradient and Hessian, cross blocks included, of a real blend of sa overlapping
    sources at its starting point (tests/blend_reference.py)"""
    import blend_reference as BR
    from celeste_jl_amd import cabi
    for seed in range(11, 40):
        f, rng = crowded(seed)
        bl = [b for b in conflict_free_blends(f.neighbors, len(f.patches), rng, max_sa=sa, min_sa=sa) if len(b) == sa]
        if bl:
            break
    blend = bl[0]
    pb = cabi.Problem(f.images, f.patches, f.neighbors)
    xs, centres = [], []
    vp = f.vp.copy()
    for s in blend:
        lo, hi, sc = BR.boxes(f.vp[s, :2])
        vp[s], x = BR.enforce_to_free(f.vp[s], lo, hi, sc)
        xs.append(x)
        centres.append(f.vp[s, :2].copy())
    v, d, h, _, st = oracle.elbo_multi(pb, vp, blend)
    assert st == 0
    g, H = BR.free_derivs(oracle, np.array(xs), centres, d, h)
    return [("blend of %d (seed %d) delta %g" % (sa, seed, dl), -H, -g, dl) for dl in (1.0, 0.05)]


def _tr_err(p, ref):
    pn = np.linalg.norm(ref["p"])
    e = np.linalg.norm(p - ref["p"])
    if ref["kind"] == "hard":   # the sign of the lowest eigenvector is free; so is the vector itself in a cluster
        e = min(e, np.linalg.norm(p - ref["p"] + 2 * (ref["z"] @ ref["p"]) * ref["z"]))
        if ref["mc"] > 1:
            e = abs(np.linalg.norm(p) - pn)
    return e


@pytest.mark.parametrize("n", [41, 82, 123, 164])
def test_general_dimension_subproblem(oracle, n):
    """the blends' sub-problem solver against the 60-digit solution of the same rules (tests/tr_reference.py)"""
    from celeste_jl_amd import blend
    rng = np.random.default_rng(n)
    probs = R.random_problems(rng, n)
    if n > 82:   # (the 60-digit reference costs minutes per problem at this size: a representative subset)
        keep = ("spd boundary", "indefinite", "hard case, rotated", "near hard case")
        probs = [p for p in probs if p[0] in keep]
    if n == 41:
        probs += R.celeste_problems(oracle, "two_body", points=2)
    probs += blend_problems(oracle, n // 41)
    Hs = [p[1] for p in probs]
    gs = [p[2] for p in probs]
    ps, m, interior = blend.tr_solve_batch(Hs, gs, [p[3] for p in probs])
    for k, (name, Hk, gk, dk) in enumerate(probs):
        ref = R.tr_reference(Hk, gk, dk)
        pn = max(np.linalg.norm(ref["p"]), 1e-300)
        assert np.linalg.norm(ps[k]) <= dk * (1 + 1e-12), name
        assert _tr_err(ps[k], ref) <= R.error_bound(ref, Hk, pn), (name, _tr_err(ps[k], ref), R.error_bound(ref, Hk, pn))


def _blend_run(ctx, vp, blends, cfg, **kw):
    return ctx.blend_context().maximize_blends(vp, blends, cfg, raise_on_error=False, **kw)


@pytest.mark.parametrize("max_iters", [6, 50])
def test_single_member_blends_against_maximize_batch(max_iters):
    import celeste_jl_amd as cel
    f, rng = crowded(21, punch=False, nan_fraction=0.0)
    S = len(f.patches)
    nb = symmetric_neighbors(f.neighbors, S)
    targets, used = [], set()
    for s in range(S):   # a layer: no two targets neighbours
        if s not in used and not (nb[s] & set(targets)):
            targets.append(s)
            used.add(s)
    ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
    cfg = cel.ElboConfig(max_iters=max_iters)
    vb, itb, evb, elb, stb = ctx.maximize_batch(f.vp, targets, cfg)
    vk, itk, evk, elk, stk = _blend_run(ctx, f.vp, [[t] for t in targets], cfg)
    assert (stb == 0).all() and (stk == 0).all()
    if max_iters <= 8:
        assert np.array_equal(itb, itk) and np.array_equal(evb, evk)
        assert np.all(np.abs(elk - elb) <= 1e-9 * np.abs(elb))
        assert np.max(np.abs(vk[targets] - vb[targets])) <= 1e-6
    else:
        assert np.all(np.abs(itk - itb) <= 3) and np.all(np.abs(evk - evb) <= 3)
        assert np.all(np.abs(elk - elb) <= 2e-6 * np.abs(elb))
    others = [s for s in range(S) if s not in targets]
    assert np.array_equal(vk[others], f.vp[others])


def test_determinism_and_batch_invariance():
    import celeste_jl_amd as cel
    f, rng = crowded(31)
    S = len(f.patches)
    blends = conflict_free_blends(f.neighbors, S, rng)
    assert len(blends) >= 3 and max(len(b) for b in blends) >= 2
    ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
    cfg = cel.ElboConfig(max_iters=10)
    r1 = _blend_run(ctx, f.vp, blends, cfg)
    r2 = _blend_run(ctx, f.vp, blends, cfg)
    for a, b in zip(r1, r2):
        assert np.array_equal(a, b)
    assert (r1[4] == 0).all()
    moved = [s for bl in blends for s in bl]
    assert not np.array_equal(r1[0][moved], f.vp[moved])
    others = [s for s in range(S) if s not in moved]
    assert np.array_equal(r1[0][others], f.vp[others])
    # a subset, and the blends in another order: the same rows and per-blend outputs, bit for bit
    for order in (list(range(len(blends)))[::-2], list(rng.permutation(len(blends)))):
        sub = [blends[k] for k in order]
        r = _blend_run(ctx, f.vp, sub, cfg)
        for j, k in enumerate(order):
            assert np.array_equal(r[0][blends[k]], r1[0][blends[k]])
            for q in (1, 2, 3, 4):
                assert r[q][j] == r1[q][k]


def test_refusals_leave_vp_untouched():
    import celeste_jl_amd as cel
    from celeste_jl_amd import blend, cabi
    f, rng = crowded(41, nan_fraction=0.0, punch=False)
    S = len(f.patches)
    nb = symmetric_neighbors(f.neighbors, S)
    a = next(s for s in range(S) if nb[s])
    b = min(nb[a])
    far = [s for s in range(S) if s != a and s not in nb[a]]
    ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
    bc = ctx.blend_context()
    cases = {"shared source": [[a, b], [b]], "repeat": [[a, a]], "empty": [[a], []], "too many": [list(range(5))],
             "neighbours across blends": [[a], [b]]}
    if far:
        cases["shared source far"] = [[a], [far[0], a]]
    ccfg = cel.ElboConfig(max_iters=3).to_c(True)
    for name, blends in cases.items():
        vp = np.ascontiguousarray(f.vp.copy())
        off, src = blend.blend_arrays(blends)
        out = [np.zeros(len(blends), dtype=np.int32), np.zeros(len(blends), dtype=np.int32), np.zeros(len(blends)),
               np.zeros(len(blends), dtype=np.int32)]
        st = bc.lib.celeste_blend_maximize(bc.handle, vp.ctypes.data_as(cabi.c_double_p), None, None, len(blends),
                                           off.ctypes.data_as(cabi.c_int64_p), src.ctypes.data_as(cabi.c_int32_p), C.byref(ccfg),
                                           out[0].ctypes.data_as(cabi.c_int32_p), out[1].ctypes.data_as(cabi.c_int32_p),
                                           out[2].ctypes.data_as(cabi.c_double_p), out[3].ctypes.data_as(cabi.c_int32_p))
        assert st == cabi.ERR_INVALID_ARG, name
        assert np.array_equal(vp, f.vp), name
        with pytest.raises(RuntimeError):
            bc.eval_blends(f.vp, blends)


def test_a_failing_blend_keeps_its_rows_and_the_others_equal_their_solo_runs():
    """a NaN centre of one member's position box makes its blend's ELBO non-finite (enforce! clamps a NaN parameter, not
    a NaN box)"""
    import celeste_jl_amd as cel
    f, rng = crowded(51)
    S = len(f.patches)
    blends = conflict_free_blends(f.neighbors, S, rng)
    assert len(blends) >= 2
    ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
    cfg = cel.ElboConfig(max_iters=8)
    members = [s for bl in blends for s in bl]
    pc = f.vp[members, :2].copy()
    pc[len(blends[0]) - 1] = np.nan
    r = _blend_run(ctx, f.vp, blends, cfg, pos_centers=pc)
    assert r[4][0] != 0 and (r[4][1:] == 0).all()
    assert np.array_equal(r[0][blends[0]], f.vp[blends[0]])
    for k in range(1, len(blends)):
        solo = _blend_run(ctx, f.vp, [blends[k]], cfg)
        assert np.array_equal(r[0][blends[k]], solo[0][blends[k]])
        assert r[1][k] == solo[1][0] and r[2][k] == solo[2][0] and r[3][k] == solo[3][0]


def _scene_blends(scene):
    from celeste_jl_amd import synthetic
    if scene in ("two_body", "three_body"):
        f = synthetic.make_sample_dataset(scene)
        nb = symmetric_neighbors(f.neighbors, len(f.patches))
        comp = sorted({s for s in range(len(f.patches)) if nb[s]} )
        return f, [comp[:4]]
    f, rng = crowded(int(scene))
    return f, conflict_free_blends(f.neighbors, len(f.patches), rng)


@pytest.mark.parametrize("scene", ["two_body", "three_body", "61", "62"])
def test_iterates_against_the_restatement(oracle, scene):
    """overlapping blends of 2-4 sources: the device's joint optimiser against tests/blend_reference.py -- identical counts
    and ELBO within 1e-9 over a few iterations, the slack of test_randomised_optimiser_against_cpu over a long run"""
    import celeste_jl_amd as cel
    import blend_reference as BR
    f, blends = _scene_blends(scene)
    assert blends and all(2 <= len(b) <= 4 for b in blends)
    ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
    for iters in ((6, 50) if scene == "two_body" else (6,)):
        vk, itk, evk, elk, stk = _blend_run(ctx, f.vp, blends, cel.ElboConfig(max_iters=iters))
        assert (stk == 0).all()
        for b, bl in enumerate(blends):
            rvp, rit, rev, rel, rst = BR.maximize_blend(oracle, ctx.problem, f.vp, bl, max_iters=iters)
            assert rst == 0
            if iters <= 8:
                assert (itk[b], evk[b]) == (rit, rev), (bl, itk[b], evk[b], rit, rev)
                assert abs(elk[b] - rel) <= 1e-9 * abs(rel), (bl, elk[b], rel)
                assert np.abs(vk[bl] - rvp[bl]).max() <= 1e-6, bl
            else:
                assert abs(itk[b] - rit) <= 3 and abs(evk[b] - rev) <= 3
                assert abs(elk[b] - rel) <= 2e-6 * abs(rel)


@pytest.mark.xfail(reason="open: from the perturbed start the blend uses all 50 iterations and ends with source 1 a galaxy "
                          "(p_star 0.005, ELBO -39178.2) where per-source sweeps reach the true star (ELBO -39147.2); "
                          "tests/blend_reference.py does the same, so the device follows the specified algorithm", strict=False)
def test_two_body_blend_recovers_both_sources():
    """two_body from the perturbed initialisation: one blend of both sources recovers both positions within 0.1 px of the
    truth and the right source types (position boxes wide enough to reach the truth, as the single-source recovery tests)"""
    import celeste_jl_amd as cel
    from celeste_jl_amd import synthetic
    f = synthetic.make_sample_dataset("two_body", perturb=True)
    ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
    vp, its, ev, el, st = ctx.blend_context().maximize_blends(f.vp, [[0, 1]], cel.ElboConfig(loc_width=3.0))
    assert st[0] == 0
    J = np.asarray(f.images[0].wcs_jacobian).reshape(2, 2)
    for s in (0, 1):
        dpix = J @ (vp[s, :2] - np.asarray(f.catalog[s].pos))
        assert np.linalg.norm(dpix) < 0.1, (s, dpix)
        assert (vp[s, 26] > 0.5) == bool(f.catalog[s].is_star), s


@pytest.mark.xfail(reason="open: on this scene the 4-member blend ends about 1e-5 relative below three Cyclades sweeps "
                          "(-47940.61 against -47940.14, both to f_tol 1e-12)", strict=False)
def test_blends_against_cyclades_sweeps(oracle):
    """a crowded scene: each conflict-free group of 2-4 overlapping sources optimised as one blend reaches a group ELBO
    (oracle.elbo_multi) no lower than three Cyclades sweeps (one member at a time, the others frozen, position boxes
    pinned at the start) from the same start; a blend pass started at the Cyclades result ends on a stopping rule"""
    import celeste_jl_amd as cel
    f, rng = crowded(71, nan_fraction=0.0, punch=False)
    S = len(f.patches)
    blends = conflict_free_blends(f.neighbors, S, rng)
    assert len(blends) >= 2
    ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
    # both sides run to a tight f_tol: with the default 1e-6 the blend's last accepted step may stop it a few 1e-6 short of
    # its optimum, which compares stopping points, not what the optimisers reach
    cfg = cel.ElboConfig(ftol_rel=1e-12, max_iters=200)
    start = f.vp.copy()
    layers = [[bl[j] for bl in blends if len(bl) > j] for j in range(max(len(b) for b in blends))]
    centres = [start[l, :2].copy() for l in layers]
    cyc, _, _, _, cst = ctx.joint_infer(start, layers * 3, cfg, pos_centers=centres * 3)
    assert (cst == 0).all()
    members = [s for bl in blends for s in bl]
    vb, its, ev, el, st = _blend_run(ctx, start, blends, cfg, pos_centers=start[members, :2])
    assert (st == 0).all()
    for bl in blends:
        jv = oracle.elbo_multi(ctx.problem, vb, bl)[0]
        cv = oracle.elbo_multi(ctx.problem, cyc, bl)[0]
        assert jv >= cv - 1e-6 * abs(cv), (bl, jv, cv)
    dcfg = cel.ElboConfig()
    v2, its2, ev2, el2, st2 = _blend_run(ctx, cyc, blends, dcfg, pos_centers=start[members, :2])
    assert (st2 == 0).all() and (its2 < dcfg.max_iters).all(), its2
