"""The stack of include/celeste_resid.h ("The stack"), restated in numpy (fp64) -- test infrastructure.

Written from the header's text: its own WCS formulas (the affine matrix and the tangent plane, inverses by the adjugate), the
nearest-pixel gather, the sums in the call's image order with each product rounded once (numpy never contracts), the peak rule of
tests/resid_reference.py on each channel's z plane, resid.grid_covering and steps 1 and 2 of resid.stacked_sources.  It takes the
per-image maps as input -- the device's own or resid_reference.Search's -- so that a comparison isolates the stack step.  It does
not call the product's stack code.
"""
import math
from dataclasses import dataclass

import numpy as np

import resid_reference as RR

D2R, R2D = math.pi / 180.0, 180.0 / math.pi
AFFINE, TAN = 0, 1
CAND_DTYPE = np.dtype([("channel", "<i4"), ("h", "<i4"), ("w", "<i4"), ("n_images", "<i4"), ("dh", "<f8"), ("dw", "<f8"),
                       ("z", "<f8"), ("f", "<f8"), ("D", "<f8"), ("world", "<f8", (2,))])


class Wcs:
    """kind AFFINE: pix = J (world - world0) + pix0; kind TAN: crval, crpix, cd.  The inverse matrix by the adjugate."""

    def __init__(self, kind, world0, pix0, mat):
        self.kind = kind
        self.w0 = [float(world0[0]), float(world0[1])]
        self.p0 = [float(pix0[0]), float(pix0[1])]
        a = [float(mat[0][0]), float(mat[0][1]), float(mat[1][0]), float(mat[1][1])]
        det = a[0] * a[3] - a[1] * a[2]
        ai = [a[3] / det, -a[1] / det, -a[2] / det, a[0] / det]
        # fwd: world -> pixel, inv: pixel -> world (TAN is given as cd: pixel -> world)
        self.fwd, self.inv = (ai, a) if kind == TAN else (a, ai)
        d0 = self.w0[1] * D2R
        self.sin0, self.cos0 = (math.sin(d0), math.cos(d0)) if kind == TAN else (0.0, 1.0)

    @classmethod
    def of_image(cls, img):
        if getattr(img, "wcs", None) is not None:
            return cls(TAN, img.wcs.crval, img.wcs.crpix, np.asarray(img.wcs.cd, dtype=np.float64))
        return cls(AFFINE, img.wcs_world0, img.wcs_pix0, np.asarray(img.wcs_jacobian, dtype=np.float64))

    def shifted(self, d1, d2):
        """the same plane with pixel coordinates lowered by (d1, d2)"""
        out = Wcs.__new__(Wcs)
        out.__dict__.update(self.__dict__)
        out.p0 = [self.p0[0] - d1, self.p0[1] - d2]
        return out

    def world_to_pix(self, w1, w2):
        w1, w2 = np.asarray(w1, dtype=np.float64), np.asarray(w2, dtype=np.float64)
        f = self.fwd
        if self.kind == AFFINE:
            d1, d2 = w1 - self.w0[0], w2 - self.w0[1]
            return (f[0] * d1 + f[1] * d2) + self.p0[0], (f[2] * d1 + f[3] * d2) + self.p0[1]
        da, dr = (w1 - self.w0[0]) * D2R, w2 * D2R
        sd, cd, sa, ca = np.sin(dr), np.cos(dr), np.sin(da), np.cos(da)
        l = cd * sa
        sh = np.sin(0.5 * da)
        m = np.sin((w2 - self.w0[1]) * D2R) + (2.0 * (cd * self.sin0)) * (sh * sh)
        n = sd * self.sin0 + (cd * self.cos0) * ca
        with np.errstate(divide="ignore", invalid="ignore"):
            x, y = (l / n) * R2D, (m / n) * R2D
        p1 = self.p0[0] + (f[0] * x + f[1] * y)
        p2 = self.p0[1] + (f[2] * x + f[3] * y)
        behind = ~(n > 0.0)
        return np.where(behind, np.nan, p1), np.where(behind, np.nan, p2)

    def pix_to_world(self, c1, c2):
        c1, c2 = np.asarray(c1, dtype=np.float64), np.asarray(c2, dtype=np.float64)
        u, v = c1 - self.p0[0], c2 - self.p0[1]
        g = self.inv
        if self.kind == AFFINE:
            return (g[0] * u + g[1] * v) + self.w0[0], (g[2] * u + g[3] * v) + self.w0[1]
        x, y = (g[0] * u + g[1] * v) * D2R, (g[2] * u + g[3] * v) * D2R
        den, num = self.cos0 - y * self.sin0, self.sin0 + y * self.cos0
        ra = self.w0[0] + np.arctan2(x, den) * R2D
        hyp = np.hypot(x, den)
        dec = self.w0[1] + np.arctan2(y - self.sin0 * ((x * x) / (hyp + den)), num * self.sin0 + hyp * self.cos0) * R2D
        return ra, dec


@dataclass
class Grid:
    H: int
    W: int
    wcs: Wcs

    @classmethod
    def of_image(cls, img):
        return cls(int(img.pixels.shape[0]), int(img.pixels.shape[1]), Wcs.of_image(img))


def grid_covering(images, which, box=None):
    """resid.grid_covering, restated"""
    ref = Wcs.of_image(images[which[0]])
    p1s, p2s = [], []
    for n in which:
        H, W = images[n].pixels.shape
        w = Wcs.of_image(images[n])
        for c1, c2 in ((1.0, 1.0), (H, 1.0), (1.0, W), (H, W)):
            a, b = w.pix_to_world(c1, c2)
            p1, p2 = ref.world_to_pix(a, b)
            p1s.append(float(p1)); p2s.append(float(p2))
    if not (np.isfinite(p1s).all() and np.isfinite(p2s).all()):
        raise ValueError("a corner is not finite")
    lo = [np.rint(min(p1s)), np.rint(min(p2s))]
    hi = [np.rint(max(p1s)), np.rint(max(p2s))]
    if box is not None:
        b1, b2 = [], []
        for ra in (box.ramin, box.ramax):
            for dec in (box.decmin, box.decmax):
                p1, p2 = ref.world_to_pix(ra, dec)
                b1.append(float(p1)); b2.append(float(p2))
        if not (np.isfinite(b1).all() and np.isfinite(b2).all()):
            raise ValueError("a corner of the box is not finite")
        lo = [max(lo[0], np.rint(min(b1))), max(lo[1], np.rint(min(b2)))]
        hi = [min(hi[0], np.rint(max(b1))), min(hi[1], np.rint(max(b2)))]
    H, W = int(hi[0] - lo[0]) + 1, int(hi[1] - lo[1]) + 1
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError("an empty grid or one that is too large")
    return Grid(H, W, ref.shifted(lo[0] - 1.0, lo[1] - 1.0))


class Stack:
    """The restated stack.  maps: {image: (N, D, z)} planes [H, W] of the search's images `simgs` (the call's order); bands:
    {image: 1 .. 5}; wcs: {image: Wcs}; ok: {image: bool} (None: all OK).  Per channel k: .N[k], .D[k], .z[k], .cnt[k], and
    .abs_N[k] = sum |term| of N; .tie: the cells in which some image's pixel coordinate lies within tie_eps of a rounding tie;
    .candidates (CAND_DTYPE) in (channel, raster index) order; .frames: per channel (n_cells, z_max, z_min)."""

    def __init__(self, maps, simgs, bands, wcs, grid, weights=((1.0,) * 5,), threshold=5.0, min_images=1, ok=None, tie_eps=1e-6):
        self.grid, self.threshold = grid, threshold
        wts = np.asarray(weights, dtype=np.float64).reshape(-1, 5)
        K, H, W = len(wts), grid.H, grid.W
        hh, ww = np.meshgrid(np.arange(1, H + 1, dtype=np.float64), np.arange(1, W + 1, dtype=np.float64), indexing="ij")
        w1, w2 = grid.wcs.pix_to_world(hh, ww)
        self.N, self.D, self.abs_N = np.zeros((K, H, W)), np.zeros((K, H, W)), np.zeros((K, H, W))
        self.cnt = np.zeros((K, H, W), dtype=np.int32)
        self.tie = np.zeros((H, W), dtype=bool)
        for n in simgs:
            if ok is not None and not ok[n]:
                continue
            Nn, Dn, zn = maps[n]
            Hn, Wn = zn.shape
            p1, p2 = wcs[n].world_to_pix(w1, w2)
            with np.errstate(invalid="ignore"):
                fin = np.isfinite(p1) & np.isfinite(p2)
                for p in (p1, p2):
                    self.tie |= fin & (np.abs((p - np.floor(p)) - 0.5) <= tie_eps)
                r1, r2 = np.rint(p1), np.rint(p2)
                use = fin & (r1 >= 1) & (r1 <= Hn) & (r2 >= 1) & (r2 <= Wn)
            qh = np.where(use, r1, 1).astype(np.int64) - 1
            qw = np.where(use, r2, 1).astype(np.int64) - 1
            use &= ~np.isnan(zn[qh, qw])
            Nv, Dv = np.where(use, Nn[qh, qw], 0.0), np.where(use, Dn[qh, qw], 0.0)
            for k in range(K):
                s = float(wts[k, bands[n] - 1])
                if not s > 0:
                    continue
                tN = s * Nv
                tD = (s * s) * Dv
                self.N[k] = np.where(use, self.N[k] + tN, self.N[k])
                self.D[k] = np.where(use, self.D[k] + tD, self.D[k])
                self.abs_N[k] += np.where(use, np.abs(tN), 0.0)
                self.cnt[k] += use
        with np.errstate(invalid="ignore", divide="ignore"):
            has = (self.cnt >= min_images) & (self.D > 0)
            self.z = np.where(has, self.N / np.sqrt(self.D), np.nan)
            self.f = np.where(has, self.N / self.D, np.nan)
        cands, self.frames = [], []
        for k in range(K):
            fin = self.z[k][~np.isnan(self.z[k])]
            self.frames.append((int(fin.size), float(fin.max()) if fin.size else np.nan, float(fin.min()) if fin.size else np.nan))
            for h, w, dh, dw in RR.find_peaks(self.z[k], threshold):
                a, b = grid.wcs.pix_to_world((h + 1.0) + dh, (w + 1.0) + dw)
                cands.append((k, h, w, int(self.cnt[k, h, w]), dh, dw, self.z[k, h, w], self.f[k, h, w], self.D[k, h, w], (float(a), float(b))))
        self.candidates = np.array(cands, dtype=CAND_DTYPE) if cands else np.zeros(0, dtype=CAND_DTYPE)


def kept_candidates(cand, grid, catalog_world, min_sep_px=2.0):
    """steps 1 and 2 of resid.stacked_sources: the indices of the candidates that stay, in descending z"""
    pix = [(c["h"] + 1.0 + c["dh"], c["w"] + 1.0 + c["dw"]) for c in cand]
    order = sorted(range(len(cand)), key=lambda i: (-cand["z"][i], i))
    kept = []
    for i in order:
        if all(math.hypot(pix[i][0] - pix[j][0], pix[i][1] - pix[j][1]) > min_sep_px for j in kept):
            kept.append(i)
    out = []
    for i in kept:
        near = False
        for ra, dec in catalog_world:
            p1, p2 = grid.wcs.world_to_pix(ra, dec)
            if np.isfinite(p1) and np.isfinite(p2) and math.hypot(float(p1) - pix[i][0], float(p2) - pix[i][1]) <= min_sep_px:
                near = True
        if not near:
            out.append(i)
    return out
