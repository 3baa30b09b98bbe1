"""Whole-frame residuals on the device: the sources a catalog missed.

  the standard step                                          here
  ---------------------------------------------------------  ------------------------------------------------
  subtract the fitted model from every frame                  ResidContext.search: the deterministic model image lam of
  filter the residuals with the PSF, look for peaks               whole frames, the matched-filter maps N, D, coverage, z, one
                                                                  summary per frame and the list of peaks
  add what was found and fit again                            missed_sources: peaks away from catalog sources, joined across
                                                                  images (detect.match_detections), one star CatalogEntry each;
                                                                  infer_box(..., refine=k) runs the loop

The reference has no such step.  The frame model, the filter and the peak rule are HIP (csrc/resid/celeste_resid.hip,
libceleste_resid.so); include/celeste_resid.h states every expression.  fp64 only, one device; the context uploads its own copy
of the image planes, as the fit context does.  The filter uses each image's own mixture img.psf (with a variable PSF map: the
fit at the image centre).
"""
import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import _binding, cabi
from .cabi import P

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "resid", "libceleste_resid.so")
ABI_VERSION = 100          # CELESTE_RESID_ABI_VERSION of include/celeste_resid.h
MAX_RADIUS = 12
TRUNCATED = 100            # CELESTE_RESID_TRUNCATED
LAM, N, D, Z, COVERAGE = range(5)
KINDS = {"lam": LAM, "N": N, "D": D, "z": Z, "coverage": COVERAGE}
EXPORTED_SYMBOLS = ["celeste_resid_version", "celeste_resid_strerror", "celeste_resid_opts_default", "celeste_resid_ctx_create",
                    "celeste_resid_ctx_destroy", "celeste_resid_search", "celeste_resid_get_map", "celeste_resid_sample",
                    "celeste_resid_find_peaks", "celeste_resid_last_ms"]
FRAME_DTYPE = np.dtype([("image", "<i4"), ("status", "<i4"), ("n_px", "<i8"), ("n_bad", "<i8"), ("chi2", "<f8"),
                        ("z_max", "<f8"), ("z_min", "<f8")], align=True)
CANDIDATE_DTYPE = np.dtype([("image", "<i4"), ("h", "<i4"), ("w", "<i4"), ("reserved", "<i4"), ("dh", "<f8"), ("dw", "<f8"),
                            ("z", "<f8"), ("f", "<f8"), ("D", "<f8"), ("cov", "<f8")], align=True)
MISSED_DTYPE = np.dtype([("ra", "<f8"), ("dec", "<f8"), ("n_detections", "<i4"), ("flux", "<f8", (5,)), ("z", "<f8", (5,)),
                         ("n_images", "<i4", (5,))])
DEFAULT_MAX_CANDIDATES = 65536
DEFAULT_FLUX_FLOOR_NMGY = 1e-3

_dp, _ip, _lp = cabi.c_double_p, cabi.c_int32_p, cabi.c_int64_p
_ptr = _binding.ptr
_check = _binding.checker("resid")


class OptsT(C.Structure):
    _fields_ = [("threshold", C.c_double), ("min_coverage", C.c_double), ("radius", C.c_int32), ("psf_K", C.c_int32),
                ("psf", _dp)]


def _declare(lib):
    vp = C.c_void_p
    lib.celeste_resid_strerror.restype = C.c_char_p
    lib.celeste_resid_strerror.argtypes = [C.c_int]
    lib.celeste_resid_opts_default.restype = None
    lib.celeste_resid_opts_default.argtypes = [C.POINTER(OptsT)]
    lib.celeste_resid_ctx_create.argtypes = [C.POINTER(cabi.ProblemT), C.c_int, C.POINTER(C.c_void_p)]
    lib.celeste_resid_ctx_destroy.argtypes = [vp]
    lib.celeste_resid_ctx_destroy.restype = None
    lib.celeste_resid_search.argtypes = [vp, _dp, C.c_int32, _ip, C.POINTER(OptsT), vp, vp, C.c_int64, _lp, _ip]
    lib.celeste_resid_get_map.argtypes = [vp, C.c_int32, C.c_int32, _dp]
    lib.celeste_resid_sample.argtypes = [vp, C.c_int64, _ip, _ip, _ip, _dp, _dp, _dp]
    lib.celeste_resid_find_peaks.argtypes = [C.c_int, C.c_int32, C.c_int32, _dp, _dp, C.POINTER(OptsT), vp, C.c_int64, _lp, _ip]
    lib.celeste_resid_last_ms.argtypes = [vp, C.POINTER(C.c_float)]


def load_library(path: Optional[str] = None) -> C.CDLL:
    """libceleste_resid.so; CELESTE_MI355X_RESID_LIB overrides its path (_binding.open_library)"""
    return _binding.open_library("resid", LIB_PATH, "CELESTE_MI355X_RESID_LIB", ABI_VERSION, "celeste_resid_version", _declare, path)


def find_peaks(z, coverage=None, threshold: float = 5.0, max_candidates: int = DEFAULT_MAX_CANDIDATES, device: int = 0):
    """celeste_resid_find_peaks: the peak rule on the caller's H x W plane z (and coverage).  Returns (candidates, n_found,
    status): the structured records (f and D are NaN), the true count, 0 or TRUNCATED."""
    lib = load_library()
    z = np.asarray(z, dtype=np.float64)
    H, W = z.shape
    zf = np.ascontiguousarray(z.T).reshape(-1)                       # index h + H w
    cf = None if coverage is None else np.ascontiguousarray(np.asarray(coverage, dtype=np.float64).T).reshape(-1)
    opts = OptsT()
    lib.celeste_resid_opts_default(C.byref(opts))
    opts.threshold = float(threshold)
    out = np.zeros(max(int(max_candidates), 1), dtype=CANDIDATE_DTYPE)
    n_found, status = C.c_int64(0), C.c_int32(0)
    _check(lib, lib.celeste_resid_find_peaks(int(device), H, W, _ptr(zf, _dp), _ptr(cf, _dp), C.byref(opts), out.ctypes.data,
                                             int(max_candidates), C.byref(n_found), C.byref(status)))
    return out[:min(int(n_found.value), int(max_candidates))].copy(), int(n_found.value), int(status.value)


@dataclass
class ResidualSearch:
    """One search (include/celeste_resid.h).  frames: one FRAME_DTYPE record per image of the call; candidates:
    CANDIDATE_DTYPE records in (image, raster index) order; n_found: the true number of candidates; status: the first non-OK
    status of a frame, TRUNCATED, or 0.  map and sample read the context's device buffers: they are valid until the
    context's next search."""
    context: "ResidContext"
    images: List[int]
    frames: np.ndarray
    candidates: np.ndarray
    n_found: int
    status: int
    min_coverage: float
    serial: int

    def _live(self):
        if self.context._serial != self.serial:
            raise RuntimeError("the context has searched again: this search's maps are gone")

    def map(self, image: int, kind) -> np.ndarray:
        """the H x W map `kind` ("lam", "N", "D", "z", "coverage" or its number) of an image of this search"""
        self._live()
        return self.context._map(int(image), KINDS[kind] if isinstance(kind, str) else int(kind))

    def sample(self, image, h, w):
        """(N, D, cov) of this search's maps at the 0-based pixels (h, w) of the images `image` (arrays of one length): zeros
        with cov = 0 outside a frame, NaN in N and D where z is NaN"""
        self._live()
        return self.context._sample(image, h, w)


class ResidContext(_binding.Context):
    """The resid library's copy of a problem (celeste_resid_ctx_t), built from a marshalled celeste_problem_t."""
    _name, _load = "resid", staticmethod(load_library)

    def __init__(self, problem: "cabi.Problem", device: int = 0):
        super().__init__(problem, device)
        self._serial = 0
        self._shapes = [(int(im.pixels.shape[0]), int(im.pixels.shape[1])) for im in problem.images]
        psf = [np.asarray(im.psf, dtype=np.float64).reshape(-1, 6) for im in problem.images]
        if len({p.shape for p in psf}) != 1:
            raise ValueError("the images' PSF mixtures differ in their number of components")
        self._psf = np.ascontiguousarray(np.stack(psf))

    def search(self, vp, images: Optional[Sequence[int]] = None, threshold: float = 5.0, radius: int = 8,
               min_coverage: float = 0.8, max_candidates: int = DEFAULT_MAX_CANDIDATES) -> ResidualSearch:
        """celeste_resid_search at the table vp [S, 44] over `images` (None: all).  A frame whose model is not finite gets a
        non-zero status and NaN maps; nothing is raised for it."""
        vp = np.ascontiguousarray(np.asarray(vp, dtype=np.float64).reshape(self.S, P))
        n_all = len(self._shapes)
        imgs = list(range(n_all)) if images is None else [int(n) for n in images]
        if any(n < 0 or n >= n_all for n in imgs) or len(set(imgs)) != len(imgs):
            raise ValueError("image out of range or listed twice")
        if not 1 <= int(radius) <= MAX_RADIUS:
            raise ValueError("radius must be in 1 .. %d" % MAX_RADIUS)
        if int(max_candidates) < 0:
            raise ValueError("max_candidates must not be negative")
        ia = np.ascontiguousarray(imgs, dtype=np.int32)
        opts = OptsT(float(threshold), float(min_coverage), int(radius), int(self._psf.shape[1]), _ptr(self._psf, _dp))
        frames = np.zeros(max(len(imgs), 1), dtype=FRAME_DTYPE)
        cand = np.zeros(max(int(max_candidates), 1), dtype=CANDIDATE_DTYPE)
        n_found, status = C.c_int64(0), C.c_int32(0)
        self._serial += 1
        _check(self.lib, self.lib.celeste_resid_search(self.handle, _ptr(vp, _dp), len(imgs), _ptr(ia, _ip), C.byref(opts),
                                                       frames.ctypes.data, cand.ctypes.data, int(max_candidates),
                                                       C.byref(n_found), C.byref(status)))
        n = min(int(n_found.value), int(max_candidates))
        return ResidualSearch(self, imgs, frames[:len(imgs)].copy(), cand[:n].copy(), int(n_found.value), int(status.value),
                              float(min_coverage), self._serial)

    def _map(self, image: int, which: int) -> np.ndarray:
        H, W = self._shapes[image]
        out = np.zeros(H * W)
        _check(self.lib, self.lib.celeste_resid_get_map(self.handle, image, which, _ptr(out, _dp)))
        return out.reshape(W, H).T.copy()

    def _sample(self, image, h, w):
        image, h, w = (np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.int32) for a in (image, h, w))
        n = image.size
        assert h.size == n and w.size == n
        oN, oD, oc = np.zeros(max(n, 1)), np.zeros(max(n, 1)), np.zeros(max(n, 1))
        _check(self.lib, self.lib.celeste_resid_sample(self.handle, n, _ptr(image, _ip), _ptr(h, _ip), _ptr(w, _ip), _ptr(oN, _dp),
                                                       _ptr(oD, _dp), _ptr(oc, _dp)))
        return oN[:n], oD[:n], oc[:n]

    def last_ms(self):
        """device ms of the last search: (per-visit tables, frame model, filter, peaks)"""
        ms = (C.c_float * 4)()
        _check(self.lib, self.lib.celeste_resid_last_ms(self.handle, ms))
        return tuple(float(x) for x in ms)


# ---- from peaks to catalog entries (host, numpy) -----------------------------------------------------------------------------
def band_sums(bands, sN, sD, scov, min_coverage: float):
    """per band (1 .. 5) of the images whose samples are sN, sD, scov: f_b = sum N / sum D and z_b = sum N / sqrt(sum D) over the
    images of band b with cov >= min_coverage (and finite N, D), NaN where a band has none; and the number of such images"""
    f, z, cnt = np.full(5, np.nan), np.full(5, np.nan), np.zeros(5, dtype=np.int32)
    for b in range(1, 6):
        sn = sd = 0.0
        for bb, n_, d_, c_ in zip(bands, sN, sD, scov):
            if bb == b and c_ >= min_coverage and np.isfinite(n_) and np.isfinite(d_):
                sn += float(n_)
                sd += float(d_)
                cnt[b - 1] += 1
        if cnt[b - 1] and sd > 0:
            f[b - 1], z[b - 1] = sn / sd, sn / np.sqrt(sd)
    return f, z, cnt


def missed_sources(search, images, catalog, min_sep_px: float = 2.0, match_radius: Optional[float] = None,
                   flux_floor_nmgy: float = DEFAULT_FLUX_FLOOR_NMGY):
    """The sources the catalog missed, from a search's candidates.  `search` needs .candidates, .images, .min_coverage and
    .sample(image, h, w) (a ResidualSearch, or the restatement's).
      1. a candidate within min_sep_px of a catalog source's pixel position in its image is dropped;
      2. the rest are joined across images by detect.match_detections on their world positions (angular=True when an image
         has a TanWCS), match_radius in world units (None: two pixels of the first image);
      3. each joined object is sampled at its nearest pixel in every image of the search, and per band f_b = sum N / sum D,
         z_b = sum N / sqrt(sum D) over the band's images with cov >= min_coverage (band_sums).
    Returns (table [MISSED_DTYPE], one star CatalogEntry per object with fluxes max(f_b, flux_floor_nmgy); a band without a
    usable image gets the floor)."""
    from .detect import match_detections
    from .params import CatalogEntry
    cand = search.candidates
    simgs = list(search.images)
    worlds = []
    for n in simgs:
        img = images[n]
        c = cand[cand["image"] == n]
        pix = np.stack([c["h"] + 1.0 + c["dh"], c["w"] + 1.0 + c["dw"]], axis=1).reshape(-1, 2)
        if len(c) and len(catalog):
            cpix = np.asarray(img.world_to_pix(np.array([ce.pos for ce in catalog], dtype=np.float64).reshape(-1, 2)))
            cpix = cpix[np.isfinite(cpix).all(axis=1)]
            if len(cpix):
                d = np.hypot(pix[:, None, 0] - cpix[None, :, 0], pix[:, None, 1] - cpix[None, :, 1]).min(axis=1)
                pix = pix[~(d <= min_sep_px)]
        worlds.append(np.asarray(img.pix_to_world(pix)).reshape(-1, 2) if len(pix) else np.zeros((0, 2)))
    angular = any(images[n].wcs is not None for n in simgs)
    if match_radius is None:
        im0 = images[simgs[0]] if simgs else None
        match_radius = 0.0 if im0 is None else 2.0 / float(np.sqrt(abs(np.linalg.det(np.asarray(im0.wcs_jacobian, float)))))
    joined, dets = match_detections(worlds, match_radius, angular=angular)
    table = np.zeros(len(joined), dtype=MISSED_DTYPE)
    entries = []
    for k, pos in enumerate(joined):
        ii, hh, ww, bands = [], [], [], []
        for n in simgs:
            pc = np.asarray(images[n].world_to_pix(pos), dtype=np.float64)
            if not np.isfinite(pc).all():
                continue
            ii.append(n); hh.append(int(np.rint(pc[0])) - 1); ww.append(int(np.rint(pc[1])) - 1); bands.append(images[n].b)
        sN, sD, sc = search.sample(ii, hh, ww)
        f, z, cnt = band_sums(bands, sN, sD, sc, search.min_coverage)
        table[k] = (pos[0], pos[1], len(dets[k]), f, z, cnt)
        flux = np.where(np.isfinite(f), np.maximum(np.nan_to_num(f), flux_floor_nmgy), flux_floor_nmgy)
        entries.append(CatalogEntry(np.array(pos, dtype=np.float64), True, flux.copy(), flux.copy(), 0.5, 0.8, 0.0, 0.2))
    return table, entries
