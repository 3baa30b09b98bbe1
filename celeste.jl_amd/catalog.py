"""Output side of the path: optimised variational parameters -> catalog rows.

  reference (src/AccuracyBenchmark.jl)                         here
  ----------------------------------------------------------  ---------------------------------------
  canonical_angle (:162), color_from_fluxes (:150-156)         canonical_angle, color_from_fluxes
  fluxes_from_colors (:325-335), get_median_fluxes (:337-342)  fluxes_from_colors, get_median_fluxes
  variational_parameters_to_data_frame_row (:344-372)          variational_parameters_to_row
  celeste_to_df (:378-387)                                     celeste_to_rows
  flux_to_mag / mag_to_flux (:140-148), get_error_df,          flux_to_mag, mag_to_flux, get_error_row, is_good_row,
  is_good_row, get_scores_df, score_predictions (:795-977)     score_predictions
"""
import math
from typing import Dict, List, Optional, Sequence

import numpy as np

from .params import ids

COLUMNS = ["ra", "dec", "is_star", "gal_frac_dev", "gal_axis_ratio", "gal_radius_px", "gal_angle_deg", "flux_r_nmgy",
           "color_ug", "color_gr", "color_ri", "color_iz", "log_flux_r_stderr", "color_ug_stderr", "color_gr_stderr",
           "color_ri_stderr", "color_iz_stderr"]


def canonical_angle(gal_angle_deg: float) -> float:
    return gal_angle_deg - math.floor(gal_angle_deg / 180) * 180


def color_from_fluxes(flux1: float, flux2: float) -> Optional[float]:
    """log(flux2 / flux1); None (the reference's `missing`) for non-positive fluxes"""
    if flux1 <= 0 or flux2 <= 0:
        return None
    return math.log(flux2 / flux1)


def fluxes_from_colors(flux_r_nmgy: float, colors: Sequence[float]) -> np.ndarray:
    assert len(colors) == 4
    r = np.exp(np.asarray(colors, dtype=np.float64))
    f = np.zeros(5)
    f[2] = flux_r_nmgy
    f[3] = f[2] * r[2]
    f[4] = f[3] * r[3]
    f[1] = f[2] / r[1]
    f[0] = f[1] / r[0]
    return f


def get_median_fluxes(vs: np.ndarray, source_type: int) -> np.ndarray:
    """source_type 0 = star, 1 = galaxy (the reference's 1 / 2)"""
    return fluxes_from_colors(math.exp(vs[ids.flux_loc[source_type]]), vs[ids.color_mean[:, source_type]])


def variational_parameters_to_row(vs: np.ndarray) -> Dict[str, Optional[float]]:
    vs = np.asarray(vs, dtype=np.float64)
    row: Dict[str, Optional[float]] = {}
    row["ra"] = float(vs[ids.pos[0]])
    row["dec"] = float(vs[ids.pos[1]])
    row["is_star"] = float(vs[ids.is_star[0]])
    row["gal_frac_dev"] = float(vs[ids.gal_frac_dev])
    row["gal_axis_ratio"] = float(vs[ids.gal_axis_ratio])
    row["gal_radius_px"] = float(vs[ids.gal_radius_px] * math.sqrt(vs[ids.gal_axis_ratio]))
    row["gal_angle_deg"] = canonical_angle(180 / math.pi * float(vs[ids.gal_angle]))
    t = 0 if row["is_star"] > 0.5 else 1
    fl = get_median_fluxes(vs, t)
    row["flux_r_nmgy"] = float(fl[2])
    for name, a, b in (("color_ug", 0, 1), ("color_gr", 1, 2), ("color_ri", 2, 3), ("color_iz", 3, 4)):
        row[name] = color_from_fluxes(float(fl[a]), float(fl[b]))
    row["log_flux_r_stderr"] = math.sqrt(vs[ids.flux_scale[t]])
    for k, name in enumerate(("color_ug_stderr", "color_gr_stderr", "color_ri_stderr", "color_iz_stderr")):
        row[name] = math.sqrt(vs[ids.color_var[k, t]])
    return row


DIAGNOSTIC_COLUMNS = ("chi2_reduced", "flux_z_r", "purity_r", "max_z", "n_pix")


def fit_columns(fit) -> Dict[str, Optional[float]]:
    """the goodness-of-fit columns of one result (fit.FitStats of infer_box(..., diagnostics=True)): the reduced chi-square
    and the visited pixels over all bands, the standardised flux misfit and the purity in the r band, the largest pixel
    deviation; None where the result carries no `fit` or the quantity is undefined"""
    if fit is None:
        return {name: None for name in DIAGNOSTIC_COLUMNS}

    def num(x):
        x = float(x)
        return x if math.isfinite(x) else None
    return {"chi2_reduced": num(fit.reduced_chi2()[1]), "flux_z_r": num(fit.flux_z()[2]), "purity_r": num(fit.purity()[2]),
            "max_z": num(fit.max_z()), "n_pix": int(fit.n_pix.sum())}


LIGHT_CURVE_COLUMNS = ("n_epochs_r", "var_chi2_r")


def light_curve_columns(lc) -> Dict[str, Optional[float]]:
    """the variability columns of one result (phot.LightCurves of infer_box(..., light_curves=True)) in the r band: the number
    of exposures with a sound estimate and the chi-square of their scales about the weighted mean (n_epochs_r - 1 degrees of
    freedom for a source of constant light); None where the result carries no `light_curve` or the quantity is undefined"""
    if lc is None:
        return {name: None for name in LIGHT_CURVE_COLUMNS}
    n, v = int(lc.n_epochs[0, 2]), float(lc.chi2_var[0, 2])
    return {"n_epochs_r": n, "var_chi2_r": v if math.isfinite(v) else None}


UNCERTAINTY_COLUMNS = ("ra_stderr", "dec_stderr", "ra_dec_corr", "gal_frac_dev_stderr", "gal_axis_ratio_stderr",
                       "gal_angle_deg_stderr", "gal_radius_px_stderr")


def uncertainty_columns(ub, vs) -> Dict[str, Optional[float]]:
    """the Cramer-Rao columns of one result (info.InfoBounds of infer_box(..., uncertainties=True)) whose row is vs.  The
    positions come from the block of the row's type (is_star > 0.5: the star's), in the units of pos, without a cos(dec)
    factor; the four shape columns are the galaxy block's and None for a star row.  gal_radius_px_stderr is the delta-method
    error of the column's own quantity radius * sqrt(axis_ratio), from the (axis_ratio, radius) sub-block; gal_angle_deg_stderr
    is in degrees.  None where the result carries no `uncertainty`, where the value is not finite, or where the block is
    flagged NO_PIXELS or NOT_POSITIVE."""
    out: Dict[str, Optional[float]] = {name: None for name in UNCERTAINTY_COLUMNS}
    if ub is None:
        return out
    from . import info
    vs = np.asarray(vs, dtype=np.float64)
    t = int(ub.chosen(vs))
    if int(ub.flag[t]) & (info.NO_PIXELS | info.NOT_POSITIVE):
        return out

    def num(x):
        x = float(x)
        return x if math.isfinite(x) else None
    c = ub.cov(t)
    with np.errstate(invalid="ignore"):
        out["ra_stderr"], out["dec_stderr"] = num(np.sqrt(c[0, 0])), num(np.sqrt(c[1, 1]))
        out["ra_dec_corr"] = num(ub.pos_corr(t))
        if t == info.GALAXY:
            se = ub.shape_stderr()
            out["gal_frac_dev_stderr"], out["gal_axis_ratio_stderr"] = num(se[0]), num(se[1])
            out["gal_angle_deg_stderr"] = num(180 / math.pi * se[2])
            # d(radius sqrt(q)) / d(q, radius) = (radius / (2 sqrt(q)), sqrt(q))
            q, r = float(vs[ids.gal_axis_ratio]), float(vs[ids.gal_radius_px])
            if q > 0:
                gq, gr = r / (2 * math.sqrt(q)), math.sqrt(q)
                a, b = info.AXIS_RATIO, info.RADIUS
                out["gal_radius_px_stderr"] = num(np.sqrt(gq * gq * c[a, a] + 2 * gq * gr * c[a, b] + gr * gr * c[b, b]))
    return out


ASTROMETRY_COLUMNS = ("n_epochs_astrom", "pm_ra", "pm_dec", "pm_ra_stderr", "pm_dec_stderr", "astrom_chi2_const",
                      "astrom_chi2_lin")


def astrometry_columns(am) -> Dict[str, Optional[float]]:
    """the motion columns of one result (astrom.Astrometry of infer_box(..., astrometry=True)): the number of exposures with a
    converged offset, the linear motion of the position in the units of pos per unit of the epochs (without a cos(dec) factor)
    with its standard errors, and the chi-squares of the exposures' offsets about their weighted mean (2 (n - 1) degrees of
    freedom for a source at rest) and about the linear motion (2 n - 4); None where the result carries no `astrometry` or the
    quantity is undefined"""
    out: Dict[str, Optional[float]] = {name: None for name in ASTROMETRY_COLUMNS}
    if am is None:
        return out

    def num(x):
        x = float(x)
        return x if math.isfinite(x) else None
    out["n_epochs_astrom"] = int(am.n_epochs[0])
    mu, mc = am.motion[0], am.motion_cov[0]
    out["pm_ra"], out["pm_dec"] = num(mu[0]), num(mu[1])
    with np.errstate(invalid="ignore"):
        out["pm_ra_stderr"], out["pm_dec_stderr"] = num(np.sqrt(mc[2, 2])), num(np.sqrt(mc[3, 3]))
    out["astrom_chi2_const"], out["astrom_chi2_lin"] = num(am.chi2_const[0]), num(am.chi2_lin[0])
    return out


def celeste_to_rows(results, diagnostics: bool = False, light_curves: bool = False,
                    uncertainties: bool = False, refined: bool = False, astrometry: bool = False) -> List[Dict[str, Optional[float]]]:
    """one row per OptimizedSource whose sky is not flagged bad; diagnostics: each row also gets DIAGNOSTIC_COLUMNS;
    light_curves: each row also gets LIGHT_CURVE_COLUMNS; uncertainties: each row also gets UNCERTAINTY_COLUMNS; refined: each
    row also gets refine_round (infer_box(..., refine=k): the round of the residual search that added the source, else None);
    astrometry: each row also gets ASTROMETRY_COLUMNS"""
    rows = [variational_parameters_to_row(r.vs) for r in results if not r.is_sky_bad]
    if diagnostics:
        for row, r in zip(rows, [r for r in results if not r.is_sky_bad]):
            row.update(fit_columns(getattr(r, "fit", None)))
    if light_curves:
        for row, r in zip(rows, [r for r in results if not r.is_sky_bad]):
            row.update(light_curve_columns(getattr(r, "light_curve", None)))
    if uncertainties:
        for row, r in zip(rows, [r for r in results if not r.is_sky_bad]):
            row.update(uncertainty_columns(getattr(r, "uncertainty", None), r.vs))
    if refined:
        for row, r in zip(rows, [r for r in results if not r.is_sky_bad]):
            row["refine_round"] = getattr(r, "refined", None)
    if astrometry:
        for row, r in zip(rows, [r for r in results if not r.is_sky_bad]):
            row.update(astrometry_columns(getattr(r, "astrometry", None)))
    return rows


# ---- scoring against a ground-truth catalog (AccuracyBenchmark.jl:140-148, 795-931) -------------------------------

ASINH_SOFTENING_PARAMETERS = (1.4e-10, 0.9e-10, 1.2e-10, 1.8e-10, 7.4e-10)   # AccuracyBenchmark.jl, SDSS asinh magnitudes
COLOR_COLUMNS = ("color_ug", "color_gr", "color_ri", "color_iz")
ABSOLUTE_ERROR_COLUMNS = ("gal_frac_dev", "gal_axis_ratio", "gal_radius_px") + COLOR_COLUMNS


def flux_to_mag(flux_nmgy: float, band_index: int) -> float:
    """band_index 1..5 like the reference"""
    b = ASINH_SOFTENING_PARAMETERS[band_index - 1]
    return -2.5 / math.log(10) * (math.asinh(flux_nmgy * 1e-9 / (2 * b)) + math.log(b))


def mag_to_flux(mags: float, band_index: int) -> float:
    b = ASINH_SOFTENING_PARAMETERS[band_index - 1]
    return 1e9 * 2 * b * math.sinh(-math.log(10) / 2.5 * mags - math.log(b))


def degrees_to_diff(a: float, b: float) -> float:
    d = abs(a - b) % 180
    return min(d, 180 - d)


def catalog_entry_to_row(ce) -> Dict[str, Optional[float]]:
    """the ground-truth row of a CatalogEntry (the columns variational_parameters_to_row produces)"""
    fl = ce.star_fluxes if ce.is_star else ce.gal_fluxes
    row = {"ra": float(ce.pos[0]), "dec": float(ce.pos[1]), "is_star": 1.0 if ce.is_star else 0.0,
           "gal_frac_dev": ce.gal_frac_dev, "gal_axis_ratio": ce.gal_axis_ratio,
           "gal_radius_px": ce.gal_radius_px * math.sqrt(ce.gal_axis_ratio),
           "gal_angle_deg": canonical_angle(180 / math.pi * ce.gal_angle), "flux_r_nmgy": float(fl[2])}
    for k, name in enumerate(COLOR_COLUMNS):
        row[name] = color_from_fluxes(float(fl[k]), float(fl[k + 1]))
    return row


def get_error_row(truth: Dict, predicted: Dict) -> Dict[str, Optional[float]]:
    """get_error_df (:813-849) for one matched pair; positions are in pixels (world = pixel here)"""
    e: Dict[str, Optional[float]] = {}
    pg, tg = predicted["is_star"] < 0.5, truth["is_star"] < 0.5
    e["missed_stars"] = float(pg) if not tg else None
    e["missed_galaxies"] = float(not pg) if tg else None
    e["position"] = math.hypot(truth["ra"] - predicted["ra"], truth["dec"] - predicted["dec"])
    e["flux_r_mag"] = abs(flux_to_mag(truth["flux_r_nmgy"], 3) - flux_to_mag(predicted["flux_r_nmgy"], 3))
    e["flux_r_nmgy"] = abs(truth["flux_r_nmgy"] - predicted["flux_r_nmgy"])
    e["gal_angle_deg"] = degrees_to_diff(truth["gal_angle_deg"], predicted["gal_angle_deg"])
    for c in ABSOLUTE_ERROR_COLUMNS:
        e[c] = None if truth[c] is None or predicted[c] is None else abs(truth[c] - predicted[c])
    for c in COLOR_COLUMNS:
        if e[c] is not None:
            e[c] *= 2.5 / math.log(10)
    return e


def is_good_row(truth: Dict, error: Dict, column: str) -> bool:
    """:851-874"""
    if error[column] is None or math.isnan(error[column]):
        return False
    if truth["gal_radius_px"] is not None and truth["gal_radius_px"] > 20:
        return False
    if column in ("gal_axis_ratio", "gal_radius_px", "gal_angle_deg", "gal_frac_dev"):
        if truth["gal_frac_dev"] is not None and 0.05 < truth["gal_frac_dev"] < 0.95:
            return False
    if column == "gal_angle_deg" and truth["gal_axis_ratio"] is not None and truth["gal_axis_ratio"] > 0.6:
        return False
    return True


def score_predictions(truth_rows: List[Dict], predicted_rows: List[Dict]) -> Dict[str, Dict[str, float]]:
    """score_predictions / get_scores_df (:903-931, 967-977) for one set of predictions already matched row by row:
    {column: {"N": count of good rows, "first": mean error}}; columns with <= 1 good row are dropped."""
    assert len(truth_rows) == len(predicted_rows)
    errors = [get_error_row(t, p) for t, p in zip(truth_rows, predicted_rows)]
    out: Dict[str, Dict[str, float]] = {}
    for column in (errors[0].keys() if errors else []):
        good = [e[column] for t, e in zip(truth_rows, errors) if is_good_row(t, e, column)]
        if len(good) > 1:
            out[column] = {"N": len(good), "first": float(np.mean(good))}
    return out
