"""The per-exposure forced photometry of include/celeste_phot.h, restated in numpy / scipy -- test infrastructure.

Written from the header's text, not from the kernel: it sits on fit_reference.expected_nmgy (the visited pixels, m and B of
every patch of a target), forms a = iota m and b = iota (eps + B) on whole patches, brackets the root of g with
scipy.optimize.brentq (xtol 1e-14) instead of iterating Newton, and evaluates g, I and chi2 at any given alpha in
np.longdouble, together with sum |term| of each (which conditions a comparison of the sums).  It reproduces the flags, the
status rule and the band summaries.
"""
from dataclasses import dataclass, field

import numpy as np
from scipy.optimize import brentq

import fit_reference as FR
from celeste_jl_amd import cabi

NB = 5
OK, NO_LIGHT, AT_BOUND, NOT_CONVERGED, BAD_MODEL = range(5)
LD = np.longdouble


@dataclass
class Entry:
    """one (target, image) pair: the visited pixels' a, b, x as vectors"""
    image: int
    band: int                # 0-based
    n_pix: int
    a: np.ndarray
    b: np.ndarray
    x: np.ndarray
    flag: int = OK
    alpha: float = np.nan
    alpha_min: float = np.nan
    sigma: float = np.nan
    chi2: float = np.nan

    def evaluate(self, alpha):
        """g, I, chi2 at alpha in extended precision, and the sum |term| of each: (g, I, chi2), (|g|, |I|, |chi2|)"""
        a, b, x = self.a.astype(LD), self.b.astype(LD), self.x.astype(LD)
        lam = b + LD(alpha) * a
        tg, tI, tc = a * (x / lam - 1), a * a / lam, (x - lam) ** 2 / lam
        return (tg.sum(), tI.sum(), tc.sum()), (np.abs(tg).sum(), np.abs(tI).sum(), np.abs(tc).sum())

    def g(self, alpha):
        return float(self.evaluate(alpha)[0][0])


def patch_entries(images, patches, neighbors, vp, target, expected=None):
    """the entries of one target, in image order, not yet solved.  expected: fit_reference.expected_nmgy(...) of the target,
    computed earlier for the same vp and geometry (a and b do not depend on the pixel values)"""
    out = []
    for n, visited, E, m, B in (expected if expected is not None else FR.expected_nmgy(images, patches, neighbors, vp, target)):
        img = images[n]
        H2, W2 = visited.shape
        h0, w0 = patches[target][n].bitmap_offset
        iota = img.nelec_per_nmgy[h0:h0 + H2].astype(np.float64)[:, None]
        sky = img.sky[h0:h0 + H2, w0:w0 + W2].astype(np.float64)
        x = img.pixels[h0:h0 + H2, w0:w0 + W2].astype(np.float64)
        a, b = iota * m, iota * (sky + B)
        out.append(Entry(n, img.b - 1, int(visited.sum()), a[visited], b[visited], x[visited]))
    return out


def solve(e: Entry) -> Entry:
    """flag, alpha, sigma and chi2 of an entry, as the header defines them"""
    a, b, x = e.a, e.b, e.x
    with np.errstate(invalid="ignore"):
        sound = np.isfinite(a).all() and np.isfinite(b).all() and (a >= 0).all() and (b > 0).all()
    if not sound:
        e.flag = BAD_MODEL
        return e
    lit = a > 0
    if not lit.any():
        e.flag = NO_LIGHT
        e.chi2 = float(((x.astype(LD) - b.astype(LD)) ** 2 / b.astype(LD)).sum())
        return e
    e.alpha_min = float((-b[lit] / a[lit]).max())
    if not (x[lit] > 0).any():
        e.flag, e.alpha = AT_BOUND, e.alpha_min
        return e
    # a bracket: g -> +inf at alpha_min, g -> -sum a < 0 at infinity
    lo, d = None, 0.5 * (1.0 - e.alpha_min)
    while lo is None:
        cand = e.alpha_min + d
        if cand > e.alpha_min and e.g(cand) > 0:
            lo = cand
        d *= 0.25
        assert d > 0, "no point right of alpha_min where g > 0"
    hi = max(1.0, lo + 1.0)
    while e.g(hi) > 0:
        hi = lo + 2 * (hi - lo)
        assert np.isfinite(hi)
    e.alpha = brentq(e.g, lo, hi, xtol=1e-14, rtol=8.9e-16, maxiter=500)
    (_, I, chi2), _ = e.evaluate(e.alpha)
    e.sigma, e.chi2 = float(1 / np.sqrt(I)), float(chi2)
    return e


def newton_iters(e: Entry, tol_sigma, max_iters=50):
    """The header's iteration on a solved OK entry, in extended precision: alpha_0 = 1, alpha_{k+1} = alpha_k + g / D with
    D = sum x a^2 / lam^2, half of the way to alpha_min where a step would reach it, stopping once a step that stayed inside
    has |step| <= tol_sigma / sqrt(I(alpha_k)).  Returns (steps taken, the smallest |log(|step| / threshold)| over the steps
    tested: how far the count is from depending on rounding)."""
    a, b, x = e.a.astype(LD), e.b.astype(LD), e.x.astype(LD)
    alpha, margin = LD(1), np.inf
    for k in range(1, max_iters + 1):
        lam = b + alpha * a
        g, D, I = (a * (x / lam - 1)).sum(), (x * a * a / lam ** 2).sum(), (a * a / lam).sum()
        step = g / D
        inside = alpha + step > e.alpha_min
        alpha = alpha + step if inside else alpha + LD(0.5) * (LD(e.alpha_min) - alpha)
        thr = LD(tol_sigma) / np.sqrt(I)
        margin = min(margin, abs(float(np.log(abs(step) / thr))))
        if inside and abs(step) <= thr:
            return k, margin
    return max_iters, margin


def band_summaries(entries):
    """(n_epochs [5] int, summary [5, 3]) over the OK entries of every band in image order"""
    n_epochs, summary = np.zeros(NB, dtype=np.int32), np.full((NB, 3), np.nan)
    for band in range(NB):
        ok = [e for e in entries if e.flag == OK and e.band == band]
        n_epochs[band] = len(ok)
        if ok:
            al, w = np.array([e.alpha for e in ok]), np.array([1 / e.sigma ** 2 for e in ok])
            wmean = (w * al).sum() / w.sum()
            summary[band] = [wmean, 1 / np.sqrt(w.sum()), (w * (al - wmean) ** 2).sum()]
    return n_epochs, summary


@dataclass
class PhotReference:
    entries: list            # per target: [Entry]
    n_epochs: np.ndarray     # [T, 5]
    summary: np.ndarray      # [T, 5, 3]
    status: np.ndarray       # [T]
    flat: list = field(default_factory=list)    # every entry in (target, image) order

    @property
    def offsets(self):
        return np.concatenate([[0], np.cumsum([len(r) for r in self.entries])]).astype(np.int64)


def phot_reference(images, patches, neighbors, vp, targets, expected=None) -> PhotReference:
    vp = np.asarray(vp, dtype=np.float64)
    rows, n_epochs, summary, status = [], [], [], np.zeros(len(targets), dtype=np.int32)
    for ti, s in enumerate(targets):
        row = [solve(e) for e in patch_entries(images, patches, neighbors, vp, s, None if expected is None else expected[s])]
        if not np.isfinite(vp[s]).all():
            status[ti] = cabi.ERR_NONFINITE_INPUT
            for e in row:
                e.flag, e.alpha, e.sigma, e.chi2 = BAD_MODEL, np.nan, np.nan, np.nan
        elif any(e.flag == BAD_MODEL for e in row):
            status[ti] = cabi.ERR_NONFINITE_RESULT
        ne, sm = band_summaries(row)
        rows.append(row); n_epochs.append(ne); summary.append(sm)
    return PhotReference(rows, np.array(n_epochs).reshape(len(targets), NB), np.array(summary).reshape(len(targets), NB, 3),
                         status, [e for r in rows for e in r])


# ---- scenes shared by the host and the device tests -----------------------------------------------------------------------------
VARIABILITY_SEED = 3      # chosen so that the restatement alone separates the variable source (tests/test_phot_host.py)
_SCENES = {}


def variability_scene(seed=VARIABILITY_SEED):
    """Three exposures of five bands (15 images: image 5 e + band) of one 64 x 80 region with 6 prior-drawn sources; the
    brightest one in r is rendered 1.5 times brighter in the second exposure only.  Returns (Field, index of that source)."""
    if ("var", seed) not in _SCENES:
        import copy
        from celeste_jl_amd import synthetic
        from celeste_jl_amd.model import get_sky_patches, neighbor_map
        f0 = synthetic.make_field(64, 80, 6, seed=seed, margin=12, perturb=False)
        catalog = f0.catalog
        var = int(np.argmax([ce.star_fluxes[2] if ce.is_star else ce.gal_fluxes[2] for ce in catalog]))
        bright = copy.deepcopy(catalog)
        bright[var].star_fluxes = np.asarray(bright[var].star_fluxes) * 1.5
        bright[var].gal_fluxes = np.asarray(bright[var].gal_fluxes) * 1.5
        images = list(f0.images)
        for e, cat in ((1, bright), (2, catalog)):
            more = synthetic.blank_images(64, 80)
            synthetic.gen_images(more, cat, np.random.Generator(np.random.PCG64([seed, e])))
            images += more
        patches = get_sky_patches(images, catalog)
        _SCENES["var", seed] = (synthetic.Field(images, catalog, patches, neighbor_map(patches), f0.vp.copy(), "variability"), var)
    return _SCENES["var", seed]
