"""MCMC inference of single sources on the device: the reference's method "mcmc" of infer_box.

  reference                                                  here
  ---------------------------------------------------------  ------------------------------------------------
  process_source_mcmc (ParallelRun.jl:504-543)               run_ais_batch (all targets of a call at once)
  run_ais (mcmc_infer.jl:10-135)                             celeste_mcmc_ais (libceleste_mcmc.so) + _finish
  ais_slicesample / bootstrap_lnZ (ais.jl:68-143)            device AIS; logmeanexp, bootstrap_lnz here
  sigmoid_schedule (ais.jl:99-107)                           sigmoid_schedule
  make_location_prior (mcmc_functions.jl:324-370)            location_box
  samples_to_dataframe(_row) (mcmc_misc.jl:105-168)          samples_to_rows, samples_to_row
  summarize_samples / consolidate_samples                    summarize_samples, consolidate_samples
      (mcmc_infer.jl:265-304)

The likelihoods, priors, the slice sampler and AIS run in HIP (csrc/mcmc/celeste_mcmc.hip); the bootstrap of lnZ,
type_chain and ave_pstar are cheap and run here, seeded from MCMCConfig.seed.  Random numbers come from Philox4x32-10
(DESIGN.md section 11): results match the reference function by function, not sample by sample.
"""
import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _binding, cabi

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "mcmc", "libceleste_mcmc.so")
ABI_VERSION = 100          # CELESTE_MCMC_ABI_VERSION of include/celeste_mcmc.h
D = 11                     # CELESTE_MCMC_D: the stride of a state vector
EXPORTED_SYMBOLS = ["celeste_mcmc_version", "celeste_mcmc_strerror", "celeste_mcmc_ctx_create", "celeste_mcmc_ctx_destroy",
                    "celeste_mcmc_loglike", "celeste_mcmc_ais", "celeste_mcmc_last_ms"]
CHAIN_STATUS = {0: "ok", 1: "NaN likelihood", 2: "acceptable caught in a loop", 3: "shrinkage cap", 4: "shrank to zero"}
STAR, GALAXY = 0, 1
LN_PSTAR, LN_PGAL = math.log(.28), math.log(.72)   # run_ais: is_star = [.28, .72] (mcmc_infer.jl:104-106)


class MCMCConfigT(C.Structure):
    _fields_ = [("num_temperatures", C.c_int32), ("num_ais_runs", C.c_int32), ("num_chain_samples", C.c_int32),
                ("max_shrink", C.c_int32), ("seed", C.c_uint64), ("temps_per_launch", C.c_int32),
                ("samples_per_launch", C.c_int32)]


class MCMCSourceT(C.Structure):
    _fields_ = [("pos", C.c_double * 2), ("is_star", C.c_int32), ("reserved", C.c_int32), ("star_fluxes", C.c_double * 5),
                ("gal_fluxes", C.c_double * 5), ("gal_frac_dev", C.c_double), ("gal_axis_ratio", C.c_double),
                ("gal_angle", C.c_double), ("gal_radius_px", C.c_double)]


@dataclass
class MCMCConfig:
    """Config (src/config.jl): num_ais_temperatures = 50, num_ais_samples = 10; run_ais's num_samples_per_chain = 25;
    num_bootstrap = 5000 (ais_slicesample).  seed keys the device's Philox streams and the host bootstrap.
    max_shrink bounds the slice sampler's shrinkage (the reference has no bound); temps_per_launch and
    samples_per_launch split the work into launches (results do not depend on them)."""
    num_ais_temperatures: int = 50
    num_ais_samples: int = 10
    num_samples_per_chain: int = 25
    num_bootstrap: int = 5000
    seed: int = 0
    max_shrink: int = 10000
    temps_per_launch: int = 10
    samples_per_launch: int = 5

    def to_c(self) -> MCMCConfigT:
        return MCMCConfigT(int(self.num_ais_temperatures), int(self.num_ais_samples), int(self.num_samples_per_chain),
                           int(self.max_shrink), int(self.seed) & (2 ** 64 - 1), int(self.temps_per_launch),
                           int(self.samples_per_launch))


@dataclass
class MCMCResult:
    """run_ais's result for one target (mcmc_infer.jl:122-131).  Samples are [n, 7] (star) and [n, 11] (galaxy) rows of
    [ln f_1..5, ra, dec (degrees)(, frac_dev, axis_ratio, angle_rad, radius_px)]; *_lls their log-posteriors."""
    source: int
    star_samples: np.ndarray
    star_lls: np.ndarray
    gal_samples: np.ndarray
    gal_lls: np.ndarray
    star_lnZ: float
    gal_lnZ: float
    star_bootstrap: np.ndarray
    gal_bootstrap: np.ndarray
    type_samples: np.ndarray
    ave_pstar: float               # ln of the mean posterior star probability, as the reference returns it
    ais_weights: np.ndarray        # [2, R]
    evals: np.ndarray              # [2, 2R] likelihood evaluations per AIS run, then per chain
    status: np.ndarray             # [2, 2R] CHAIN_STATUS codes
    failed: bool = False

    @property
    def p_star(self) -> float:
        return float(math.exp(self.ave_pstar))


# ---- host-side pieces of the reference ---------------------------------------------------------------------------
def sigmoid_schedule(num_steps: int, rad: float = 4.0) -> np.ndarray:
    """ais.jl:99-107"""
    if num_steps == 1:
        return np.array([0.0, 1.0])
    t = np.linspace(-rad, rad, num_steps)
    s = 1.0 / (1.0 + np.exp(-t))
    return (s - s.min()) / (s.max() - s.min())


def logsumexp(x) -> float:
    x = np.asarray(x, dtype=np.float64)
    m = np.max(x)
    if not np.isfinite(m):
        return float(m)
    return float(m + np.log(np.sum(np.exp(x - m))))


def logmeanexp(x) -> float:
    return logsumexp(x) - math.log(len(x))


def bootstrap_lnz(w: np.ndarray, num_bootstrap: int, rng: np.random.Generator) -> np.ndarray:
    """bootstrap_lnZ (ais.jl:80-89): num_bootstrap resamples with replacement of the AIS log weights"""
    w = np.asarray(w, dtype=np.float64)
    n = len(w)
    x = w[rng.integers(0, n, size=(num_bootstrap, n))]
    m = x.max(axis=1)
    with np.errstate(invalid="ignore"):
        s = m + np.log(np.sum(np.exp(x - m[:, None]), axis=1))
    return np.where(np.isfinite(m), s, m) - math.log(n)


def type_chain(star_boot: np.ndarray, gal_boot: np.ndarray) -> np.ndarray:
    """run_ais (mcmc_infer.jl:103-114): ln p(star | data) for each bootstrap pair"""
    a = np.asarray(star_boot) + LN_PSTAR
    b = np.asarray(gal_boot) + LN_PGAL
    return a - np.logaddexp(a, b)


def location_box(wcs_jacobian, wcs_world0, wcs_pix0, pos0, pos_pixel_delta=(2.0, 2.0)) -> np.ndarray:
    """make_location_prior (mcmc_functions.jl:324-370) under the affine WCS pix = J (world - w0) + p0:
    the corners pos0_pix -/+ delta / 2 mapped to world coordinates and sorted per coordinate.
    Returns [ra_lo, ra_hi, dec_lo, dec_hi]."""
    J = np.asarray(wcs_jacobian, dtype=np.float64).reshape(2, 2)
    w0, p0 = np.asarray(wcs_world0, dtype=np.float64), np.asarray(wcs_pix0, dtype=np.float64)
    pix = J @ (np.asarray(pos0, dtype=np.float64) - w0) + p0
    half = 0.5 * np.asarray(pos_pixel_delta, dtype=np.float64)
    lo = np.linalg.solve(J, pix - half - p0) + w0
    hi = np.linalg.solve(J, pix + half - p0) + w0
    ra = sorted([lo[0], hi[0]])
    dec = sorted([lo[1], hi[1]])
    return np.array([ra[0], ra[1], dec[0], dec[1]])


def image_location_box(img, pos0, pos_pixel_delta=(2.0, 2.0)) -> np.ndarray:
    """location_box through the image's own WCS (make_location_prior maps its corners with the image's wcs)"""
    if img.wcs is None:
        return location_box(img.wcs_jacobian, img.wcs_world0, img.wcs_pix0, pos0, pos_pixel_delta)
    pix = img.world_to_pix(np.asarray(pos0, dtype=np.float64))
    half = 0.5 * np.asarray(pos_pixel_delta, dtype=np.float64)
    lo, hi = img.pix_to_world(pix - half), img.pix_to_world(pix + half)
    ra = sorted([lo[0], hi[0]])
    dec = sorted([lo[1], hi[1]])
    return np.array([ra[0], ra[1], dec[0], dec[1]])


def samples_to_rows(chain: np.ndarray, is_star: bool) -> Dict[str, np.ndarray]:
    """samples_to_dataframe (mcmc_misc.jl:105-136): columns of the sample table"""
    chain = np.asarray(chain, dtype=np.float64)
    df = {"log_flux_r": chain[:, 2], "flux_r_nmgy": np.exp(chain[:, 2]), "color_ug": chain[:, 1] - chain[:, 0],
          "color_gr": chain[:, 2] - chain[:, 1], "color_ri": chain[:, 3] - chain[:, 2], "color_iz": chain[:, 4] - chain[:, 3],
          "ra": chain[:, 5], "dec": chain[:, 6]}
    if not is_star:
        df["gal_frac_dev"] = chain[:, 7]
        df["gal_axis_ratio"] = chain[:, 8]
        df["gal_angle_deg"] = chain[:, 9] * 360 / (2 * math.pi)
        df["gal_radius_px"] = chain[:, 10] * np.sqrt(chain[:, 8])
    return df


def samples_to_row(df: Dict[str, np.ndarray], is_star: bool) -> Dict[str, float]:
    """samples_to_dataframe_row (mcmc_misc.jl:139-168); std is the sample standard deviation (Julia's std)"""
    def sd(x):
        return float(np.std(x, ddof=1)) if len(x) > 1 else float("nan")
    row = {"ra": float(np.mean(df["ra"])), "dec": float(np.mean(df["dec"])), "is_star": True,
           "gal_frac_dev": float("nan"), "gal_axis_ratio": float("nan"), "gal_radius_px": float("nan"),
           "gal_angle_deg": float("nan"), "flux_r_nmgy": float(np.mean(df["flux_r_nmgy"])),
           "log_flux_r": float(np.mean(df["log_flux_r"])), "log_flux_r_stderr": sd(df["log_flux_r"])}
    for c in ("color_ug", "color_gr", "color_ri", "color_iz"):
        row[c] = float(np.mean(df[c]))
    for c in ("color_ug", "color_gr", "color_ri", "color_iz"):
        row[c + "_stderr"] = sd(df[c])
    if not is_star:
        row["is_star"] = False
        for c in ("gal_frac_dev", "gal_axis_ratio", "gal_radius_px", "gal_angle_deg"):
            row[c] = float(np.mean(df[c]))
    return row


def summarize_samples(res: MCMCResult, objid: str = "") -> Dict[str, Dict[str, float]]:
    """summarize_samples (mcmc_infer.jl:265-287): the star row, the galaxy row and p_star"""
    star = samples_to_row(samples_to_rows(res.star_samples, True), True)
    gal = samples_to_row(samples_to_rows(res.gal_samples, False), False)
    pstar = res.p_star
    for r in (star, gal):
        r["objid"] = objid
        r["prob_star"] = pstar
    return {"star": star, "gal": gal, "pstar": pstar}


def consolidate_samples(summary: Dict[str, Dict[str, float]]) -> Dict[str, float]:
    """consolidate_samples (mcmc_infer.jl:290-304): the star row if p_star > 0.5, else the galaxy row"""
    row = dict(summary["star"] if summary["pstar"] > 0.5 else summary["gal"])
    row["is_star"] = summary["pstar"] > 0.5
    return row


# ---- the library ----------------------------------------------------------------------------------------------------
def _declare(lib):
    vp, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lib.celeste_mcmc_strerror.restype = C.c_char_p
    lib.celeste_mcmc_strerror.argtypes = [C.c_int]
    lib.celeste_mcmc_ctx_create.restype = C.c_int
    lib.celeste_mcmc_ctx_create.argtypes = [C.POINTER(cabi.ProblemT), C.c_int, C.POINTER(vp)]
    lib.celeste_mcmc_ctx_destroy.restype = None
    lib.celeste_mcmc_ctx_destroy.argtypes = [vp]
    lib.celeste_mcmc_loglike.restype = C.c_int
    lib.celeste_mcmc_loglike.argtypes = [vp, C.POINTER(MCMCSourceT), C.c_int32, ip, dp, C.c_int32, C.c_int32, ip, dp, dp, dp]
    lib.celeste_mcmc_ais.restype = C.c_int
    lib.celeste_mcmc_ais.argtypes = [vp, C.POINTER(MCMCConfigT), C.POINTER(MCMCSourceT), C.c_int32, ip, dp, dp, dp, dp, dp,
                                     C.POINTER(C.c_int64), ip]
    lib.celeste_mcmc_last_ms.restype = C.c_int
    lib.celeste_mcmc_last_ms.argtypes = [vp, C.POINTER(C.c_float)]


def load_library(path: Optional[str] = None) -> C.CDLL:
    """libceleste_mcmc.so; CELESTE_MI355X_MCMC_LIB overrides its path (_binding.open_library)"""
    return _binding.open_library("mcmc", LIB_PATH, "CELESTE_MI355X_MCMC_LIB", ABI_VERSION, "celeste_mcmc_version", _declare, path)


def _dp(a: np.ndarray):
    return _binding.ptr(a, C.POINTER(C.c_double))


def _ip(a: np.ndarray):
    return _binding.ptr(a, C.POINTER(C.c_int32))


_check = _binding.checker("mcmc")


def source_table(catalog) -> "C.Array":
    arr = (MCMCSourceT * len(catalog))()
    for i, ce in enumerate(catalog):
        s = arr[i]
        s.pos[:] = [float(x) for x in ce.pos]
        s.is_star = 1 if ce.is_star else 0
        s.star_fluxes[:] = [float(x) for x in ce.star_fluxes]
        s.gal_fluxes[:] = [float(x) for x in ce.gal_fluxes]
        s.gal_frac_dev, s.gal_axis_ratio = float(ce.gal_frac_dev), float(ce.gal_axis_ratio)
        s.gal_angle, s.gal_radius_px = float(ce.gal_angle), float(ce.gal_radius_px)
    return arr


class MCMCContext(_binding.Context):
    """The device copy of a problem for MCMC (celeste_mcmc_ctx_t), built from a marshalled celeste_problem_t."""
    _name, _load = "mcmc", staticmethod(load_library)

    def loglike(self, catalog, targets: Sequence[int], boxes: np.ndarray, model: int, which: Sequence[int], theta: np.ndarray):
        """celeste_mcmc_loglike: (ll, lp) of the points theta[k] (7 or 11 entries) of targets[which[k]]"""
        targets = np.ascontiguousarray(targets, dtype=np.int32)
        boxes = np.ascontiguousarray(boxes, dtype=np.float64).reshape(len(targets), 4)
        theta = np.asarray(theta, dtype=np.float64)
        th = np.zeros((len(theta), D))
        th[:, :theta.shape[1]] = theta
        which = np.ascontiguousarray(which, dtype=np.int32)
        ll, lp = np.zeros(len(th)), np.zeros(len(th))
        src = source_table(catalog)
        _check(self.lib, self.lib.celeste_mcmc_loglike(self.handle, src, len(targets), _ip(targets), _dp(boxes), int(model),
                                                       len(th), _ip(which), _dp(th), _dp(ll), _dp(lp)))
        return ll, lp

    def ais(self, catalog, targets: Sequence[int], boxes: np.ndarray, cfg: MCMCConfig) -> dict:
        """celeste_mcmc_ais: the raw device outputs, arrays [n_targets, 2, ...]"""
        targets = np.ascontiguousarray(targets, dtype=np.int32)
        n, R, L = len(targets), cfg.num_ais_samples, cfg.num_samples_per_chain
        boxes = np.ascontiguousarray(boxes, dtype=np.float64).reshape(n, 4)
        out = {"ais_state": np.zeros((n, 2, R, D)), "ais_weight": np.zeros((n, 2, R)),
               "samples": np.zeros((n, 2, R * L, D)), "sample_lp": np.zeros((n, 2, R * L)),
               "evals": np.zeros((n, 2, 2 * R), dtype=np.int64), "status": np.zeros((n, 2, 2 * R), dtype=np.int32)}
        c = cfg.to_c()
        src = source_table(catalog)
        _check(self.lib, self.lib.celeste_mcmc_ais(
            self.handle, C.byref(c), src, n, _ip(targets), _dp(boxes), _dp(out["ais_state"]),
            _dp(out["ais_weight"]), _dp(out["samples"]), _dp(out["sample_lp"]),
            out["evals"].ctypes.data_as(C.POINTER(C.c_int64)), _ip(out["status"])))
        ms = (C.c_float * 3)()
        self.lib.celeste_mcmc_last_ms(self.handle, ms)
        out["device_ms"] = [float(x) for x in ms]
        return out


def _finish(t: int, k: int, out: dict, box: np.ndarray, cfg: MCMCConfig, rng: np.random.Generator) -> MCMCResult:
    st = out["status"][k]
    failed = bool(np.any(st != 0))
    w = out["ais_weight"][k]
    lnz = [logmeanexp(w[m]) for m in (STAR, GALAXY)]
    boots = [bootstrap_lnz(w[m], cfg.num_bootstrap, rng) for m in (STAR, GALAXY)]
    tc = type_chain(boots[0], boots[1])
    samples = []
    for m, dim in ((STAR, 7), (GALAXY, 11)):
        s = out["samples"][k, m, :, :dim].copy()
        s[:, 5] = (box[1] - box[0]) * s[:, 5] + box[0]        # uniform_to_deg
        s[:, 6] = (box[3] - box[2]) * s[:, 6] + box[2]
        samples.append(s)
    return MCMCResult(int(t), samples[0], out["sample_lp"][k, STAR].copy(), samples[1], out["sample_lp"][k, GALAXY].copy(),
                      lnz[0], lnz[1], boots[0], boots[1], tc, logmeanexp(tc), w.copy(), out["evals"][k].copy(), st.copy(), failed)


def target_boxes(images, catalog, targets: Sequence[int]) -> np.ndarray:
    """the location box of every target in the WCS of images[1] (make_location_prior on imgs[1])"""
    return np.array([image_location_box(images[0], catalog[t].pos) for t in targets]).reshape(len(targets), 4)


def run_ais_batch(ctx, catalog, targets: Sequence[int], cfg: Optional[MCMCConfig] = None) -> List[MCMCResult]:
    """run_ais for every target (the background of each from the catalog point parameters of its neighbours);
    ctx: a FieldContext (its problem) or an MCMCContext.  One MCMCResult per target, in target order; a target whose chains
    failed has failed = True (the reference throws)."""
    cfg = cfg or MCMCConfig()
    mc = ctx if isinstance(ctx, MCMCContext) else ctx.mcmc_context()
    targets = [int(t) for t in targets]
    if not targets:
        return []
    boxes = target_boxes(mc.problem.images, catalog, targets)
    out = mc.ais(catalog, targets, boxes, cfg)
    # the bootstrap of a target draws from its own stream (seed, source index): independent of the other targets
    return [_finish(t, k, out, boxes[k], cfg, np.random.default_rng([int(cfg.seed) & (2 ** 64 - 1), t]))
            for k, t in enumerate(targets)]
