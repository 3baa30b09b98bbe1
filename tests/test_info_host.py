"""libceleste_info.so without a GPU: its C ABI (header, exports, Python binding), the refusals that come back before any
device is touched, the restatement of its sums (tests/info_reference.py) -- its autograd gradients against finite differences,
its sums against the covariance of the score over Poisson pixels it drew itself -- the covariance step in mpmath on hand-made
matrices, and the Python side (the block a row picks, the catalog columns)."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import info_reference as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _protos():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "celeste_info.h")).read(), flags=re.S)
    return {n: (0 if a.strip() in ("", "void") else len(a.split(","))) for n, a in
            re.findall(r"\b(celeste_info_\w+)\s*\(([^)]*)\)\s*;", hdr)}


def test_the_info_library_exports_its_c_abi_and_nothing_else(lib):
    from celeste_jl_amd import info
    protos = _protos()
    assert set(protos) == set(info.EXPORTED_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", info.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip()) == sorted(info.EXPORTED_SYMBOLS)
    emap = open(os.path.join(ROOT, "celeste.jl_amd", "csrc", "info", "exports.map")).read()
    assert re.search(r"global:\s*celeste_info_\*;\s*local:\s*\*;", emap)
    f = info.load_library()
    for name, n_args in protos.items():                       # the ctypes signatures
        at = getattr(f, name).argtypes
        assert (0 if at is None else len(at)) == n_args, name
    assert f.celeste_info_version() == info.ABI_VERSION
    assert b"no CPU fallback" in f.celeste_info_strerror(5)


def test_header_constants_match_the_binding_and_the_restatement():
    from celeste_jl_amd import info
    hdr = open(os.path.join(ROOT, "include", "celeste_info.h")).read()
    defs = dict(re.findall(r"#define CELESTE_INFO_(\w+) (\S+)", hdr))
    assert int(defs["ABI_VERSION"]) == info.ABI_VERSION and int(defs["BANDS"]) == info.BANDS == IR.NB
    assert (int(defs["G_STAR"]), int(defs["G_GAL"])) == info.G == IR.G
    assert (int(defs["NSUM_STAR"]), int(defs["NSUM_GAL"])) == info.NSUM == IR.NSUM
    assert (int(defs["NCOV_STAR"]), int(defs["NCOV_GAL"])) == info.NCOV == IR.NCOV
    assert float(defs["PIVOT_MIN"]) == info.PIVOT_MIN == IR.PIVOT_MIN
    for g, ns, nc in zip(info.G, info.NSUM, info.NCOV):
        assert nc == g * (g + 1) // 2 and ns == nc + g + 1
    flags = dict(re.findall(r"CELESTE_INFO_(NO_PIXELS|UNCONSTRAINED|NOT_POSITIVE|ILL_CONDITIONED) = (\d+)", hdr))
    for name, v in flags.items():
        assert int(v) == getattr(info, name) == getattr(IR, name), name
    assert len(flags) == 4


def test_refusals_come_back_before_any_device_is_touched(lib):
    import ctypes as C
    from celeste_jl_amd import cabi, info
    f = info.load_library()
    vp = np.zeros((2, 44))
    tg = np.zeros(1, dtype=np.int32)
    n_pix = np.full((1, 5), -7, dtype=np.int64)
    s0, s1, c0, c1 = np.full((1, 5, 6), -7.0), np.full((1, 5, 28), -7.0), np.full((1, 3), -7.0), np.full((1, 21), -7.0)
    fl, status = np.full((1, 2), -7, dtype=np.int32), np.full(1, -7, dtype=np.int32)
    p = info._ptr
    dp, ip, lp = cabi.c_double_p, cabi.c_int32_p, cabi.c_int64_p
    outs = (p(n_pix, lp), p(s0, dp), p(s1, dp), p(c0, dp), p(c1, dp), p(fl, ip), p(status, ip))
    for args in ((None, p(vp, dp), 1, p(tg, ip)) + outs, (None, p(vp, dp), -1, p(tg, ip)) + outs,
                 (None, None, 0, None) + (None,) * 7):
        assert f.celeste_info_bounds(*args) == cabi.ERR_INVALID_ARG
    assert f.celeste_info_solve(None, 1, p(s0, dp), p(s1, dp), p(c0, dp), p(c1, dp), p(fl, ip)) == cabi.ERR_INVALID_ARG
    for a in (n_pix, s0, s1, c0, c1, fl, status):
        assert (a == -7).all()
    assert f.celeste_info_last_ms(None, (C.c_float * 4)()) == cabi.ERR_INVALID_ARG
    assert f.celeste_info_ctx_create(None, 0, None) == cabi.ERR_INVALID_ARG
    h = C.c_void_p(1234)
    assert f.celeste_info_ctx_create(None, 0, C.byref(h)) == cabi.ERR_INVALID_ARG and not h.value
    f.celeste_info_ctx_destroy(None)


# ---- the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sample_star", "sample_galaxy", "sample_two_body"])
def test_autograd_gradients_against_central_differences(name):
    """d f_i / d theta on every patch of every source, forward-mode autograd against (f(theta + h e_k) - f(theta - h e_k)) / 2h
    with h = 1e-5 max(1, |theta_k|): within 1e-6 of the largest |derivative| of the parameter over the patch's grid.  (Truncation
    h^2 f''' / 6 and rounding eps f / h are both near 1e-10 of that scale.)"""
    import torch
    import fit_reference as FR
    import golden_util as GU
    f = GU.arrays_to_field(np.load(GU.path(name)))
    light = FR._Light(f.images, f.patches, f.vp)
    worst = 0.0
    for s in range(len(f.catalog)):
        vs = torch.tensor(np.asarray(f.vp[s], dtype=np.float64))
        pas = [p for p in f.patches[s] if 0 not in p.active_pixel_bitmap.shape]
        assert len(pas) == 5
        for i in range(2):
            fn = IR.density_fn(pas, [light.coef(p.stamp) for p in pas], i)
            theta = vs[0:IR.G[i]].clone()
            _, jac = IR.value_and_jacobian(fn, theta)
            for k in range(IR.G[i]):
                h = 1e-5 * max(1.0, abs(float(theta[k])))
                e = torch.zeros_like(theta)
                e[k] = h
                fd = ((fn(theta + e) - fn(theta - e)) / (2 * h)).numpy()
                for q in range(len(pas)):
                    scale = np.abs(jac[k][q]).max()
                    assert scale > 0
                    worst = max(worst, float(np.abs(jac[k][q] - fd[q]).max() / scale))
    print("autograd against central differences, %s: %.3e (bound 1e-6)" % (name, worst))
    assert worst <= 1e-6


MC_SEED, MC_DRAWS = 20261020, 4000


def test_the_sums_are_the_fisher_information_of_poisson_pixels():
    """One star, 9 x 9 patches in 5 bands.  x ~ Poisson(lam_0) at every visited pixel, 4000 draws (PCG64 seed 20261020); the
    score of (pos1, pos2, five band scales) is sum D (x - lam) / lam; its second moments (the score has mean 0) must equal
    the 7 x 7 information assembled from the restatement's sums within 4 standard errors of each entry's sample mean."""
    from celeste_jl_amd import synthetic
    from celeste_jl_amd.model import get_sky_patches, neighbor_map
    from celeste_jl_amd.params import catalog_init_source
    images = synthetic.blank_images(20, 23)
    catalog = [synthetic.sample_ce([10.1, 12.2], True)]
    synthetic.gen_images(images, catalog, np.random.Generator(np.random.PCG64(3)))
    patches = get_sky_patches(images, catalog, radius_override_pix=4.0)
    assert all(p.active_pixel_bitmap.shape == (9, 9) for p in patches[0])
    vp = np.stack([catalog_init_source(ce) for ce in catalog])
    recs = IR.pixel_terms(images, patches, neighbor_map(patches), vp, 0)
    assert len(recs) == 5
    want = IR.full_information(recs, 0)
    # the information from the packed sums is the same matrix
    ref = IR.info_reference(images, patches, neighbor_map(patches), vp, [0])
    packed = np.zeros((7, 7))
    for b in range(5):
        A00, A01, A11, c0, c1, d = ref.sums[0][0, b]
        packed[:2, :2] += [[A00, A01], [A01, A11]]
        packed[0, 2 + b] = packed[2 + b, 0] = c0
        packed[1, 2 + b] = packed[2 + b, 1] = c1
        packed[2 + b, 2 + b] = d
    assert np.allclose(packed, want, rtol=1e-12, atol=0)
    rng = np.random.Generator(np.random.PCG64(MC_SEED))
    score = np.zeros((MC_DRAWS, 7))
    for rec in recs:
        v, b = rec["visited"], rec["band"]
        lam = rec["lam"][0][v]
        x = rng.poisson(lam, size=(MC_DRAWS, lam.size)).astype(np.float64)
        z = (x - lam) / lam
        for k in range(2):
            score[:, k] += z @ rec["D"][0][k][v]
        score[:, 2 + b] += z @ rec["a"][0][v]
    prod = score[:, :, None] * score[:, None, :]
    got = prod.mean(axis=0)
    se = prod.std(axis=0, ddof=1) / math.sqrt(MC_DRAWS)
    dev = np.abs(got - want) / se
    print("score covariance against the information: worst %.2f standard errors (bound 4), seed %d" % (dev.max(), MC_SEED))
    assert (dev <= 4).all()
    assert np.abs(score.mean(axis=0) / (score.std(axis=0) / math.sqrt(MC_DRAWS))).max() <= 4


# ---- the covariance step ---------------------------------------------------------------------------------------------------
def _full(cov, g):
    from celeste_jl_amd import info
    return info.unpack(cov, g)


def test_solve_on_hand_made_matrices():
    cases = IR.hand_made()
    for name, (rows, flag, want) in cases.items():
        g = 2 if rows.shape[1] == 6 else 6
        r = IR.solve(rows, g)
        assert r.flag == flag, (name, r.flag)
        if want is None:
            assert np.isnan(r.cov).all(), name
            continue
        C = _full(r.cov, g)
        fin = np.isfinite(want)
        assert np.array_equal(np.isposinf(C), np.isposinf(want)), name
        assert np.allclose(C[fin], want[fin], rtol=1e-5 if name == "nearly singular" else 1e-12, atol=0), name
    # the diagonal's answer is known exactly; the zero row leaves the smaller problem's answer and inf / zeros
    assert np.array_equal(IR.solve(cases["diagonal"][0], 6).cov[[0, 6, 11]], [1.0, 0.25, 1.0 / 9.0])
    z = _full(IR.solve(cases["zero row"][0], 6).cov, 6)
    assert z[4, 4] == np.inf and (np.delete(z[4], 4) == 0).all() and (np.delete(z[:, 4], 4) == 0).all()
    keep = [0, 1, 2, 3, 5]
    Z = _full(cases["zero row"][0][0, :21], 6)
    small = IR.solve(IR.rows_of(Z[np.ix_(keep, keep)]), 5)
    assert small.flag == 0 and np.array_equal(z[np.ix_(keep, keep)], _full(small.cov, 5))
    # the nearly singular pair: written, flagged, kappa = (1 + r) / (1 - r)
    ns = IR.solve(cases["nearly singular"][0], 2)
    assert np.isfinite(ns.cov).all() and 1e9 < ns.kappa < 4e9
    # non-finite sums: S is not finite
    bad = cases["schur"][0].copy()
    bad[3, 0] = np.nan
    assert IR.solve(bad, 2).flag == IR.NOT_POSITIVE
    assert IR.solve(np.full((5, 28), np.nan), 6).flag == IR.NOT_POSITIVE


# ---- the Python side -------------------------------------------------------------------------------------------------------
def _bounds(flag=(0, 0)):
    from celeste_jl_amd import info
    cs = np.array([[4e-4, 1e-4], [1e-4, 1e-4]])
    rng = np.random.Generator(np.random.PCG64(9))
    X = rng.normal(size=(10, 6))
    cg = X.T @ X * 1e-3
    cg[3, 3], cg[5, 5], cg[3, 5] = 0.01, 0.04, 0.005
    cg[5, 3] = cg[3, 5]
    iu0, iu1 = np.triu_indices(2), np.triu_indices(6)
    return info.InfoBounds(np.zeros(5, dtype=np.int64), np.zeros((5, 6)), np.zeros((5, 28)), cs[iu0], cg[iu1],
                           np.array(flag, dtype=np.int32), np.int32(0)), cs, cg


def test_chosen_follows_the_rows_type_rule_and_the_columns_follow_it():
    from celeste_jl_amd import catalog, info, infer
    from celeste_jl_amd.params import ids
    ub, cs, cg = _bounds()
    vs = np.zeros(44)
    vs[ids.gal_axis_ratio], vs[ids.gal_radius_px] = 0.49, 4.0
    for is_star, t in ((0.9, 0), (0.5, 1), (0.1, 1)):
        vs[ids.is_star[0]], vs[ids.is_star[1]] = is_star, 1 - is_star
        assert int(ub.chosen(vs)) == t == (0 if catalog.variational_parameters_to_row(vs)["is_star"] > 0.5 else 1)
    assert np.array_equal(ub.cov(0), cs) and np.array_equal(ub.cov(1), cg)
    assert np.allclose(ub.pos_stderr(0), [0.02, 0.01]) and abs(ub.pos_corr(0) - 0.5) < 1e-15
    assert np.allclose(ub.shape_stderr(), np.sqrt([cg[2, 2], 0.01, cg[4, 4], 0.04]))
    # a star row: the star block's positions, no shape columns
    vs[ids.is_star[0]], vs[ids.is_star[1]] = 0.9, 0.1
    cols = catalog.uncertainty_columns(ub, vs)
    assert tuple(cols) == catalog.UNCERTAINTY_COLUMNS
    assert abs(cols["ra_stderr"] - 0.02) < 1e-15 and abs(cols["dec_stderr"] - 0.01) < 1e-15 and abs(cols["ra_dec_corr"] - 0.5) < 1e-15
    assert all(cols[c] is None for c in catalog.UNCERTAINTY_COLUMNS[3:])
    # a galaxy row: the galaxy block; radius sqrt(q) by the delta method, by hand:
    # (4 / (2 * 0.7))^2 * 0.01 + 2 * (4 / 1.4) * 0.7 * 0.005 + 0.49 * 0.04 = 0.0816326530612245 + 0.02 + 0.0196
    vs[ids.is_star[0]], vs[ids.is_star[1]] = 0.1, 0.9
    cols = catalog.uncertainty_columns(ub, vs)
    assert abs(cols["ra_stderr"] - math.sqrt(cg[0, 0])) < 1e-15 and abs(cols["ra_dec_corr"] - cg[0, 1] / math.sqrt(cg[0, 0] * cg[1, 1])) < 1e-14
    assert abs(cols["gal_radius_px_stderr"] - math.sqrt(0.1212326530612245)) < 1e-12
    assert abs(cols["gal_axis_ratio_stderr"] - 0.1) < 1e-15
    assert abs(cols["gal_angle_deg_stderr"] - math.degrees(math.sqrt(cg[4, 4]))) < 1e-12
    assert abs(cols["gal_frac_dev_stderr"] - math.sqrt(cg[2, 2])) < 1e-15
    # flags: NO_PIXELS and NOT_POSITIVE give None; UNCONSTRAINED gives None for the infinite value only
    for fl in (info.NO_PIXELS, info.NOT_POSITIVE, info.NOT_POSITIVE | info.UNCONSTRAINED):
        ub2, _, _ = _bounds((0, fl))
        assert all(v is None for v in catalog.uncertainty_columns(ub2, vs).values())
        vs_star = vs.copy()
        vs_star[ids.is_star[0]] = 0.9
        assert catalog.uncertainty_columns(ub2, vs_star)["ra_stderr"] is not None          # the star block is not flagged
    ub3, _, _ = _bounds((0, info.UNCONSTRAINED))
    ub3.cov_gal = ub3.cov_gal.copy()
    ub3.cov_gal[18] = np.inf                                   # (4, 4): gal_angle
    cols = catalog.uncertainty_columns(ub3, vs)
    assert cols["gal_angle_deg_stderr"] is None and cols["gal_axis_ratio_stderr"] is not None
    # through celeste_to_rows; a result without `uncertainty` gets None
    res = [infer.OptimizedSource(1.0, 2.0, vs, False, uncertainty=ub),
           infer.OptimizedSource(1.0, 2.0, vs, False)]
    rows = catalog.celeste_to_rows(res, uncertainties=True)
    assert rows[0]["ra_stderr"] is not None and all(rows[1][c] is None for c in catalog.UNCERTAINTY_COLUMNS)
    assert res[1].uncertainty is None


def test_the_defaults_do_not_import_info_and_return_what_they_returned():
    code = r"""
import sys, inspect
import numpy as np
import celeste_jl_amd as cel
from celeste_jl_amd import catalog, synthetic
assert inspect.signature(cel.infer_box).parameters["uncertainties"].default is False
assert inspect.signature(catalog.celeste_to_rows).parameters["uncertainties"].default is False
f = synthetic.make_sample_dataset("two_body", seed=1)
res = [cel.OptimizedSource(1.0, 2.0, f.vp[0].copy(), False), cel.OptimizedSource(3.0, 4.0, f.vp[1].copy(), True)]
rows = catalog.celeste_to_rows(res)
assert rows == [catalog.variational_parameters_to_row(f.vp[0])] and list(rows[0]) == catalog.COLUMNS
assert not set(catalog.UNCERTAINTY_COLUMNS) & set(rows[0])
u = catalog.celeste_to_rows(res, uncertainties=True)
assert list(u[0]) == catalog.COLUMNS + list(catalog.UNCERTAINTY_COLUMNS)
assert {k: v for k, v in u[0].items() if k not in catalog.UNCERTAINTY_COLUMNS} == rows[0]
try:
    cel.infer_box(f.images, cel.BoundingBox(0.0, 30.0, 0.0, 30.0), f.catalog, method="mcmc", uncertainties=True)
except ValueError as e:
    assert "mcmc" in str(e)
else:
    raise AssertionError("method='mcmc' with uncertainties=True must raise")
assert "celeste_jl_amd.info" not in sys.modules
print("ok")
"""
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
