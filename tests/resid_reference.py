"""The whole-frame residual search of include/celeste_resid.h, restated in numpy (fp64) -- test infrastructure.

Written from the header's text, not from the kernels: the frame model from fit_reference._Light (the densities of
tests/torch_value_model.py) under the rule of the expected image (joint_objective.expected_planes: a source's light on its own
patch without the last column, where its bitmap is set), the matched filter as a direct loop over the taps (whole-plane
shifted slices, no FFT), the peak rule and the sub-pixel step pixel by pixel, and the band sums of resid.missed_sources.  For
N and D it also returns sum |term|, which conditions a comparison of the sums.
"""
import math
from dataclasses import dataclass

import numpy as np
import torch

import fit_reference as FR
from celeste_jl_amd import cabi

DT = torch.float64
CAND_DTYPE = np.dtype([("image", "<i4"), ("h", "<i4"), ("w", "<i4"), ("dh", "<f8"), ("dw", "<f8"), ("z", "<f8"), ("f", "<f8"),
                       ("D", "<f8"), ("cov", "<f8")])


def frame_model(images, patches, vp, which=None):
    """{image: lam [H, W]}: iota[h] * (eps + sum over sources, ascending, of their light where they cover the pixel)"""
    light = FR._Light(images, patches, vp)
    out = {}
    for n, img in enumerate(images):
        if which is not None and n not in which:
            continue
        H, W = img.pixels.shape
        m = np.zeros((H, W))
        for s in range(len(patches)):
            p = patches[s][n]
            H2, W2 = p.active_pixel_bitmap.shape
            if H2 == 0 or W2 < 2:
                continue
            h0, w0 = p.bitmap_offset
            hh = torch.arange(h0 + 1, h0 + H2 + 1, dtype=DT)[:, None].expand(H2, W2 - 1)
            ww = torch.arange(w0 + 1, w0 + W2, dtype=DT)[None, :].expand(H2, W2 - 1)
            cover = np.asarray(p.active_pixel_bitmap, dtype=bool)[:, :W2 - 1]
            sub = m[h0:h0 + H2, w0:w0 + W2 - 1]
            sub += np.where(cover, light(s, n, hh, ww), 0.0)
        out[n] = img.nelec_per_nmgy.astype(np.float64)[:, None] * (img.sky.astype(np.float64) + m)
    return out


def phi_taps(psf, R):
    """phi[dh + R, dw + R] = sum_k alpha_k N((dh, dw); xi_k, T_k), not renormalised"""
    d = np.arange(-R, R + 1, dtype=np.float64)
    dh, dw = d[:, None], d[None, :]
    out = np.zeros((2 * R + 1, 2 * R + 1))
    for a, x1, x2, t11, t12, t22 in np.asarray(psf, dtype=np.float64).reshape(-1, 6):
        det = t11 * t22 - t12 * t12
        d0, d1 = dh - x1, dw - x2
        q = (t22 * d0 * d0 - 2 * t12 * d0 * d1 + t11 * d1 * d1) / det
        out += a * np.exp(-0.5 * q) / (2 * math.pi * math.sqrt(det))
    return out


@dataclass
class Maps:
    lam: np.ndarray
    N: np.ndarray
    D: np.ndarray
    cov: np.ndarray
    z: np.ndarray
    abs_N: np.ndarray      # sum |term| of N (D's terms are not negative: its own value)


def filter_maps(x, lam, iota, phi, min_coverage=0.8):
    """the matched filter over a frame: x [H, W] pixels (NaN = masked), lam [H, W], iota [H], phi [2R + 1, 2R + 1]"""
    x = np.asarray(x, dtype=np.float64)
    H, W = x.shape
    R = (phi.shape[0] - 1) // 2
    io = np.asarray(iota, dtype=np.float64)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        good = ~np.isnan(x) & (lam > 0)
        a = np.where(good, io * (x - lam) / lam, 0.0)
        b = np.where(good, io * io / lam, 0.0)
    N, D, absN, cs = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    tot = 0.0
    for dw in range(-R, R + 1):
        for dh in range(-R, R + 1):
            p = phi[dh + R, dw + R]
            tot += p
            # outputs (h, w) whose tap (h + dh, w + dw) is inside the frame
            h_lo, h_hi = max(0, -dh), min(H, H - dh)
            w_lo, w_hi = max(0, -dw), min(W, W - dw)
            if h_lo >= h_hi or w_lo >= w_hi:
                continue
            src = (slice(h_lo + dh, h_hi + dh), slice(w_lo + dw, w_hi + dw))
            dst = (slice(h_lo, h_hi), slice(w_lo, w_hi))
            N[dst] += p * a[src]
            absN[dst] += np.abs(p * a[src])
            D[dst] += p * p * b[src]
            cs[dst] += np.where(good[src], p, 0.0)
    cov = cs / tot
    with np.errstate(invalid="ignore", divide="ignore"):
        z = np.where((cov < min_coverage) | (D == 0), np.nan, N / np.sqrt(D))
    return Maps(lam, N, D, cov, z, absN)


def subpixel(zm, z0, zp):
    if zm is None or zp is None or np.isnan(zm) or np.isnan(zp):
        return 0.0
    den = zm - 2 * z0 + zp
    if not den < 0:
        return 0.0
    return float(min(0.5, max(-0.5, 0.5 * (zm - zp) / den)))


def find_peaks(z, threshold=5.0):
    """[(h, w, dh, dw)] in raster order (index h + H w), by the header's rule, pixel by pixel"""
    z = np.asarray(z, dtype=np.float64)
    H, W = z.shape
    out = []
    with np.errstate(invalid="ignore"):
        cand = np.argwhere(z >= threshold)
    for h, w in sorted(((int(h), int(w)) for h, w in cand), key=lambda t: t[0] + H * t[1]):
        z0, ok = z[h, w], True
        for dw in (-1, 0, 1):
            for dh in (-1, 0, 1):
                qh, qw = h + dh, w + dw
                if (dh == 0 and dw == 0) or not (0 <= qh < H and 0 <= qw < W) or np.isnan(z[qh, qw]):
                    continue
                lower = qh + H * qw < h + H * w
                if (z0 <= z[qh, qw]) if lower else (z0 < z[qh, qw]):
                    ok = False
        if ok:
            out.append((h, w, subpixel(z[h - 1, w] if h > 0 else None, z0, z[h + 1, w] if h < H - 1 else None),
                        subpixel(z[h, w - 1] if w > 0 else None, z0, z[h, w + 1] if w < W - 1 else None)))
    return out


def fragile_peaks(z, threshold, eps=1e-9):
    """pixels whose candidacy hangs on less than eps: z within eps of the threshold, or of a neighbour's while at or above the
    threshold themselves (or the neighbour is) -- where two correct implementations may differ"""
    z = np.asarray(z, dtype=np.float64)
    H, W = z.shape
    out = set()
    with np.errstate(invalid="ignore"):
        near = np.argwhere(z >= threshold - eps)
    for h, w in near:
        h, w = int(h), int(w)
        if abs(z[h, w] - threshold) <= eps:
            out.add((h, w))
        for dw in (-1, 0, 1):
            for dh in (-1, 0, 1):
                qh, qw = h + dh, w + dw
                if (dh or dw) and 0 <= qh < H and 0 <= qw < W and abs(z[h, w] - z[qh, qw]) <= eps:
                    out.add((h, w))
                    out.add((qh, qw))
    return out


class Search:
    """the restatement's search: .maps {image: Maps}, .frames, .candidates, and what resid.missed_sources asks of a search"""

    def __init__(self, images, patches, vp, which=None, threshold=5.0, radius=8, min_coverage=0.8, lam=None):
        self.images = list(range(len(images))) if which is None else list(which)
        self.min_coverage = min_coverage
        self.threshold = threshold
        vp = np.asarray(vp, dtype=np.float64)
        lam = frame_model(images, patches, vp, self.images) if lam is None else lam
        bad_rows = [s for s in range(len(patches)) if not np.isfinite(vp[s]).all()]
        self.maps, self.frames, cands = {}, {}, []
        for n in self.images:
            img = images[n]
            x = img.pixels.astype(np.float64)
            L = lam[n]
            input_bad = any(0 not in patches[s][n].active_pixel_bitmap.shape for s in bad_rows)
            n_bad = int((~(np.isfinite(L) & (L > 0))).sum())
            status = cabi.ERR_NONFINITE_INPUT if input_bad else (cabi.ERR_NONFINITE_RESULT if n_bad else 0)
            seen = ~np.isnan(x)
            if status:
                nan = np.full(L.shape, np.nan)
                self.maps[n] = Maps(L, nan, nan, nan, nan, nan)
                self.frames[n] = dict(image=n, status=status, n_px=int(seen.sum()), n_bad=n_bad, chi2=np.nan, z_max=np.nan,
                                      z_min=np.nan, abs_chi2=np.nan)
                continue
            mp = filter_maps(x, L, img.nelec_per_nmgy, phi_taps(img.psf, radius), min_coverage)
            self.maps[n] = mp
            r = (x - L)[seen]
            fin = mp.z[np.isfinite(mp.z)]
            self.frames[n] = dict(image=n, status=0, n_px=int(seen.sum()), n_bad=0, chi2=float((r * r / L[seen]).sum()),
                                  z_max=float(fin.max()) if fin.size else np.nan, z_min=float(fin.min()) if fin.size else np.nan)
            for h, w, dh, dw in find_peaks(mp.z, threshold):
                cands.append((n, h, w, dh, dw, mp.z[h, w], mp.N[h, w] / mp.D[h, w], mp.D[h, w], mp.cov[h, w]))
        self.candidates = np.array(cands, dtype=CAND_DTYPE) if cands else np.zeros(0, dtype=CAND_DTYPE)
        self._shapes = {n: images[n].pixels.shape for n in self.images}

    def sample(self, image, h, w):
        oN, oD, oc = [], [], []
        for n, hh, ww in zip(image, h, w):
            H, W = self._shapes[int(n)]
            if not (0 <= hh < H and 0 <= ww < W):
                oN.append(0.0); oD.append(0.0); oc.append(0.0)
                continue
            mp = self.maps[int(n)]
            masked = np.isnan(mp.z[hh, ww])
            oN.append(np.nan if masked else mp.N[hh, ww]); oD.append(np.nan if masked else mp.D[hh, ww]); oc.append(mp.cov[hh, ww])
        return np.array(oN), np.array(oD), np.array(oc)


def band_sums(bands, sN, sD, scov, min_coverage):
    """f_b = sum N / sum D, z_b = sum N / sqrt(sum D) over the samples of band b with cov >= min_coverage"""
    bands, sN, sD, scov = (np.asarray(a) for a in (bands, sN, sD, scov))
    f, z = np.full(5, np.nan), np.full(5, np.nan)
    for b in range(1, 6):
        use = (bands == b) & (scov >= min_coverage) & np.isfinite(sN) & np.isfinite(sD)
        if use.any() and sD[use].sum() > 0:
            f[b - 1] = sN[use].sum() / sD[use].sum()
            z[b - 1] = sN[use].sum() / math.sqrt(sD[use].sum())
    return f, z
