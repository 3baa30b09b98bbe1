"""Shared helpers for the HIP-vs-oracle parity tests (test infrastructure)."""
import numpy as np

# Stated fp64 tolerance (BASELINE.json north_star: "within 1e-8 relative of the reference").
# Entry-wise criterion: |gpu - ref| <= RTOL * max(|ref|, FLOOR * ||ref||_inf of the block), i.e. relative
# 1e-8 on every entry that is not itself below 1e-6 of the block's largest entry (entries that small are
# sums of cancelling O(||.||) terms).
RTOL = 1e-8
FLOOR = 1e-6


def rel_err(a, ref):
    a = np.asarray(a, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    scale = np.maximum(np.abs(ref), FLOOR * np.abs(ref).max() if ref.size else 0.0)
    scale = np.where(scale == 0, 1.0, scale)
    return float((np.abs(a - ref) / scale).max()) if ref.size else 0.0


def assert_parity(gpu, ref, what=""):
    v, d, h, cnt, st = gpu
    ov, od, oh, ocnt, ost = ref
    assert np.array_equal(st, ost), (what, st, ost)
    assert np.array_equal(cnt, ocnt), (what, "pixel counters", cnt, ocnt)
    ev = float(np.max(np.abs(v - ov) / np.abs(ov)))
    assert ev <= RTOL, (what, "value", ev)
    errs = {"v": ev}
    if d is not None:
        for t in range(len(v)):
            e = rel_err(d[t], od[t]); errs["d"] = max(errs.get("d", 0), e)
            assert e <= RTOL, (what, "gradient", t, e)
    if h is not None:
        for t in range(len(v)):
            assert np.array_equal(h[t], h[t].T), (what, "Hessian not exactly symmetric")
            e = rel_err(h[t], oh[t]); errs["h"] = max(errs.get("h", 0), e)
            assert e <= RTOL, (what, "hessian", t, e)
    return errs


# ---- single-precision mode (CELESTE_FLAG_FP32): an entry-wise criterion -------------------------------------------------------
# The mode's stated tolerance (1e-4 on v and on ||.||inf-scaled d and h) says nothing about an entry far below the largest one
# of its target.  Each entry is measured here as well, on a scale that does not change when one parameter is rescaled, built
# from the fp64 Hessian h64 of the same target (always with CELESTE_FLAG_HESS, also for a gradient-only evaluation):
#   Hessian (i, j):  |h32 - h64| <= FP32_T_H * max(|h64_ij|, FP32_F * sqrt(|h64_ii h64_jj|))
#   gradient i:      |d32 - d64| <= FP32_T_D * max(|d64_i|,  FP32_F * sqrt(|h64_ii|))
#   value:           |v32 - v64| <= FP32_T_V * |v64|
# An entry whose reference and scale are both exactly 0 (the k block without CELESTE_FLAG_KL) must be exactly 0.  A non-finite
# fp32 entry (NaN, +-inf) fails whatever its reference.
# FP32_T_D * FP32_F bounds how far the gradient error moves a Newton step, in posterior standard deviations
# (1 / sqrt(h_ii)) of that parameter.
# The thresholds are 4x or more above the worst ratio measured on the MI355X over every fixture the suite checks this way --
# the fp32 fuzz seeds, the 200 x 240 field, the 2 x 2 and 2 x 4 multifields, the variable fields, the randomised fuzz and
# the variable golden (tools/gpu_fp32_entry_errors.py, profiles/fp32_entry_errors_mi355x.json).
# Measured worst ratios (F = 1e-2, all fixtures above): v 1.02e-5, d 4.9e-4, h 2.13e-2 (a star-flux row of one configs[4]
# source; the same 2.1e-2 with F = 1e-1, i.e. on an entry that is not floor-scaled).  Thresholds: 4.9x, 4.1x, 4.7x that.
FP32_F = 1e-2
FP32_T_V = 5e-5
FP32_T_D = 2e-3
FP32_T_H = 1e-1
# The two criteria are meant to be used TOGETHER: T_h = 0.1 lets a 10 % error through on the largest Hessian entries, which
# the norm-scaled 1e-4 does not (norm_scaled_fp32_errors).  The entry-wise check adds power on the small entries; it does not
# replace the norm-scaled one, and the suite keeps both wherever fp32 results are compared.

# parameter blocks of the 44 canonical parameters (params.ids_names())
FP32_BLOCKS = {"position": [0, 1], "shape": [2, 3, 4, 5], "star_flux": [6, 8], "galaxy_flux": [7, 9],
               "colour": list(range(10, 26)), "type": [26, 27], "k": list(range(28, 44))}


def _ratio(err, scale):
    out = np.zeros_like(err)
    nz = scale > 0
    out[nz] = err[nz] / scale[nz]
    out[~nz & (err != 0)] = np.inf     # reference and scale exactly 0: only an exact 0 passes
    out[~np.isfinite(err)] = np.inf    # a NaN or infinite entry fails (a NaN ratio would compare false against any bound)
    return out


def fp32_errors(gpu, ref, ref_h, F=None):
    """Entry-wise error ratios of an fp32 result against an fp64 reference (see FP32_* above): a dict with "v" [n] (relative),
    "d" [n, 44] and "h" [n, 44, 44] (each |error| / scale; d, h are None when gpu has none).  gpu / ref: (v, d, h, ...);
    ref_h: the fp64 Hessians [n, 44, 44] of the same targets."""
    F = FP32_F if F is None else F
    v, d, h = gpu[0], gpu[1], gpu[2]
    ov, od, oh = ref[0], ref[1], ref[2]
    v = np.asarray(v, np.float64); ov = np.asarray(ov, np.float64)
    ev = np.abs(v - ov) / np.abs(ov)
    out = {"v": np.where(np.isfinite(ev), ev, np.inf), "d": None, "h": None}
    if d is None and h is None:
        return out
    diag = np.sqrt(np.abs(np.diagonal(np.asarray(ref_h, np.float64), axis1=1, axis2=2)))      # [n, 44]
    if d is not None:
        od = np.asarray(od, np.float64)
        out["d"] = _ratio(np.abs(np.asarray(d, np.float64) - od), np.maximum(np.abs(od), F * diag))
    if h is not None:
        oh = np.asarray(oh, np.float64)
        out["h"] = _ratio(np.abs(np.asarray(h, np.float64) - oh),
                          np.maximum(np.abs(oh), F * diag[:, :, None] * diag[:, None, :]))
    return out


def norm_scaled_fp32_errors(gpu, ref):
    """the mode's stated (norm-scaled) tolerance: max over targets of max|dx| / max|ref x|, x = v (relative), d, h"""
    def worst(a):      # (a NaN anywhere is inf: Python's max() and a > comparison would both step over it)
        a = np.asarray(a, dtype=np.float64)
        return float(a.max()) if a.size and np.isfinite(a).all() else (0.0 if not a.size else np.inf)
    out = {"v": worst(np.abs(gpu[0] - ref[0]) / np.abs(ref[0]))}
    for k, x in ((1, "d"), (2, "h")):
        if gpu[k] is not None:
            out[x] = worst([worst(np.abs(gpu[k][t] - ref[k][t])) / np.abs(ref[k][t]).max() for t in range(len(gpu[0]))])
    return out


def assert_fp32_parity(gpu, ref, ref_h, what=""):
    """fp32_errors within FP32_T_V / FP32_T_D / FP32_T_H; a failure names the target and the parameter(s).  Returns the worst
    ratio of each of v, d, h."""
    from celeste_jl_amd.params import ids_names
    names = ids_names()
    e = fp32_errors(gpu, ref, ref_h)
    worst = {"v": float(e["v"].max()) if e["v"].size else 0.0}
    t = int(np.argmax(e["v"])) if e["v"].size else 0
    assert worst["v"] <= FP32_T_V, (what, "value", "target %d" % t, worst["v"], gpu[0][t], ref[0][t])
    for x, tol in (("d", FP32_T_D), ("h", FP32_T_H)):
        r = e[x]
        if r is None:
            continue
        worst[x] = float(r.max()) if r.size else 0.0
        if not worst[x] <= tol:
            idx = np.unravel_index(int(np.argmax(r)), r.shape)
            k = {"d": 1, "h": 2}[x]
            raise AssertionError((what, "gradient" if x == "d" else "hessian", "target %d" % idx[0],
                                  " x ".join(names[i] for i in idx[1:]), "ratio %.3g > %.3g" % (worst[x], tol),
                                  "fp32 %r, fp64 %r" % (float(gpu[k][idx]), float(ref[k][idx]))))
    return worst
