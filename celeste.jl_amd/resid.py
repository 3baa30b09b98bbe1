"""Whole-frame residuals on the device: the sources a catalog missed.

  the standard step                                          here
  ---------------------------------------------------------  ------------------------------------------------
  subtract the fitted model from every frame                  ResidContext.search: the deterministic model image lam of
  filter the residuals with the PSF, look for peaks               whole frames, the matched-filter maps N, D, coverage, z, one
                                                                  summary per frame and the list of peaks
  add what was found and fit again                            missed_sources: peaks away from catalog sources, joined across
                                                                  images (detect.match_detections), one star CatalogEntry each;
                                                                  infer_box(..., refine=k) runs the loop
  coadd before looking: a source below the threshold in       ResidualSearch.stack: N and D of the search added across images on a
  every single image                                              sky grid (nearest pixel through each image's WCS, affine or
                                                                  tangent-plane), per channel of band weights; the peak rule on
                                                                  the stacked z; stacked_sources, infer_box(..., refine_stack=True)

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
ABI_VERSION = 101          # CELESTE_RESID_ABI_VERSION of include/celeste_resid.h
MAX_RADIUS = 12
TRUNCATED = 100            # CELESTE_RESID_TRUNCATED
LAM, N, D, Z, COVERAGE = range(5)
KINDS = {"lam": LAM, "N": N, "D": D, "z": Z, "coverage": COVERAGE}
EXPORTED_SYMBOLS = ["celeste_resid_version", "celeste_resid_strerror", "celeste_resid_opts_default", "celeste_resid_ctx_create",
                    "celeste_resid_ctx_destroy", "celeste_resid_search", "celeste_resid_get_map", "celeste_resid_sample",
                    "celeste_resid_find_peaks", "celeste_resid_last_ms", "celeste_resid_stack_opts_default",
                    "celeste_resid_wcs_check", "celeste_resid_stack", "celeste_resid_stack_get_map", "celeste_resid_stack_last_ms"]
FRAME_DTYPE = np.dtype([("image", "<i4"), ("status", "<i4"), ("n_px", "<i8"), ("n_bad", "<i8"), ("chi2", "<f8"),
                        ("z_max", "<f8"), ("z_min", "<f8")], align=True)
CANDIDATE_DTYPE = np.dtype([("image", "<i4"), ("h", "<i4"), ("w", "<i4"), ("reserved", "<i4"), ("dh", "<f8"), ("dw", "<f8"),
                            ("z", "<f8"), ("f", "<f8"), ("D", "<f8"), ("cov", "<f8")], align=True)
MISSED_DTYPE = np.dtype([("ra", "<f8"), ("dec", "<f8"), ("n_detections", "<i4"), ("flux", "<f8", (5,)), ("z", "<f8", (5,)),
                         ("n_images", "<i4", (5,))])
STACK_FRAME_DTYPE = np.dtype([("channel", "<i4"), ("reserved", "<i4"), ("n_cells", "<i8"), ("z_max", "<f8"), ("z_min", "<f8")],
                             align=True)
STACK_CANDIDATE_DTYPE = np.dtype([("channel", "<i4"), ("h", "<i4"), ("w", "<i4"), ("n_images", "<i4"), ("dh", "<f8"), ("dw", "<f8"),
                                  ("z", "<f8"), ("f", "<f8"), ("D", "<f8"), ("world", "<f8", (2,))], align=True)
WCS_AFFINE, WCS_TAN = 0, 1
STACK_N, STACK_D, STACK_Z, STACK_COUNT = range(4)
STACK_KINDS = {"N": STACK_N, "D": STACK_D, "z": STACK_Z, "count": STACK_COUNT}
STACK_MAX_CHANNELS = 8
FLAT_WEIGHTS = ((1.0, 1.0, 1.0, 1.0, 1.0),)      # a flat SED in nanomaggies
DEFAULT_MAX_CANDIDATES = 65536
DEFAULT_FLUX_FLOOR_NMGY = 1e-3

_dp, _ip, _lp = cabi.c_double_p, cabi.c_int32_p, cabi.c_int64_p
_ptr = _binding.ptr
_check = _binding.checker("resid")


class OptsT(C.Structure):
    _fields_ = [("threshold", C.c_double), ("min_coverage", C.c_double), ("radius", C.c_int32), ("psf_K", C.c_int32),
                ("psf", _dp)]


class WcsT(C.Structure):
    """celeste_resid_wcs_t"""
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("world0", C.c_double * 2), ("pix0", C.c_double * 2),
                ("m", C.c_double * 4)]


class GridT(C.Structure):
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("wcs", WcsT)]


class StackOptsT(C.Structure):
    _fields_ = [("threshold", C.c_double), ("min_images", C.c_int32), ("reserved", C.c_int32)]


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
    lib.celeste_resid_stack_opts_default.restype = None
    lib.celeste_resid_stack_opts_default.argtypes = [C.POINTER(StackOptsT)]
    lib.celeste_resid_wcs_check.argtypes = [C.c_int32, C.POINTER(WcsT)]
    lib.celeste_resid_stack.argtypes = [vp, C.POINTER(GridT), C.c_int32, C.POINTER(WcsT), C.c_int32, _dp, C.POINTER(StackOptsT), vp,
                                        vp, C.c_int64, _lp, _ip]
    lib.celeste_resid_stack_get_map.argtypes = [vp, C.c_int32, C.c_int32, _dp]
    lib.celeste_resid_stack_last_ms.argtypes = [vp, C.POINTER(C.c_float)]


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


# ---- the stack: WCS records and grids -------------------------------------------------------------------------------------------
def wcs_of(img) -> WcsT:
    """the celeste_resid_wcs_t of an image: TAN from its model.TanWCS, otherwise its affine matrix"""
    w = WcsT()
    if getattr(img, "wcs", None) is not None:
        t = img.wcs
        cd = np.asarray(t.cd, dtype=np.float64)
        w.kind = WCS_TAN
        w.world0[:] = [float(t.crval[0]), float(t.crval[1])]
        w.pix0[:] = [float(t.crpix[0]), float(t.crpix[1])]
        w.m[:] = [float(cd[0, 0]), float(cd[0, 1]), float(cd[1, 0]), float(cd[1, 1])]
    else:
        J = np.asarray(img.wcs_jacobian, dtype=np.float64)
        w.kind = WCS_AFFINE
        w.world0[:] = [float(x) for x in np.asarray(img.wcs_world0, dtype=np.float64)]
        w.pix0[:] = [float(x) for x in np.asarray(img.wcs_pix0, dtype=np.float64)]
        w.m[:] = [float(J[0, 0]), float(J[1, 0]), float(J[0, 1]), float(J[1, 1])]
    return w


def _copy_wcs(w: WcsT) -> WcsT:
    out = WcsT()
    C.memmove(C.byref(out), C.byref(w), C.sizeof(WcsT))
    return out


@dataclass
class StackGrid:
    """celeste_resid_grid_t: H x W cells, cell (h, w), 0-based, at the 1-based pixel (h + 1, w + 1) of wcs"""
    H: int
    W: int
    wcs: WcsT

    @classmethod
    def of_image(cls, img) -> "StackGrid":
        return cls(int(img.pixels.shape[0]), int(img.pixels.shape[1]), wcs_of(img))

    def c_struct(self) -> GridT:
        g = GridT()
        g.H, g.W, g.wcs = int(self.H), int(self.W), _copy_wcs(self.wcs)
        return g


def grid_covering(images, which, box=None) -> StackGrid:
    """The grid on the WCS of images[which[0]] that covers every listed frame: the corner pixels (1, 1), (H, 1), (1, W), (H, W) of
    each listed frame go through their own pix_to_world and the first image's world_to_pix; the cells that hold the smallest
    and the largest coordinate per axis (rint) bound the grid, and the WCS is re-origined so that they become pixels 1 .. H,
    1 .. W.  With a box (ramin, ramax, decmin, decmax) that range is first intersected with the range of the box's four
    corners, found the same way.  ValueError: a corner that is not finite, an empty grid, or H * W >= 2^31."""
    which = [int(n) for n in which]
    if not which:
        raise ValueError("grid_covering needs at least one image")
    ref = images[which[0]]
    pts = []
    for n in which:
        H, W = images[n].pixels.shape
        corners = np.array([[1.0, 1.0], [H, 1.0], [1.0, W], [H, W]], dtype=np.float64)
        pts.append(np.asarray(ref.world_to_pix(np.asarray(images[n].pix_to_world(corners))), dtype=np.float64).reshape(-1, 2))
    pts = np.concatenate(pts)
    if not np.isfinite(pts).all():
        raise ValueError("grid_covering: a frame corner has no finite position on the first image's plane")
    lo, hi = np.rint(pts.min(axis=0)), np.rint(pts.max(axis=0))
    if box is not None:
        bw = np.array([[box.ramin, box.decmin], [box.ramin, box.decmax], [box.ramax, box.decmin], [box.ramax, box.decmax]], dtype=np.float64)
        bp = np.asarray(ref.world_to_pix(bw), dtype=np.float64).reshape(-1, 2)
        if not np.isfinite(bp).all():
            raise ValueError("grid_covering: a corner of the box has no finite position on the first image's plane")
        lo, hi = np.maximum(lo, np.rint(bp.min(axis=0))), np.minimum(hi, np.rint(bp.max(axis=0)))
    H, W = int(hi[0] - lo[0]) + 1, int(hi[1] - lo[1]) + 1
    if H < 1 or W < 1:
        raise ValueError("grid_covering: the box and the frames do not meet")
    if H * W >= 2 ** 31:
        raise ValueError("grid_covering: a grid of %d x %d cells is too large" % (H, W))
    w = wcs_of(ref)
    w.pix0[0] = w.pix0[0] - (float(lo[0]) - 1.0)
    w.pix0[1] = w.pix0[1] - (float(lo[1]) - 1.0)
    return StackGrid(H, W, w)


@dataclass
class StackedSearch:
    """One stack (include/celeste_resid.h, "The stack").  frames: one STACK_FRAME_DTYPE record per channel; candidates:
    STACK_CANDIDATE_DTYPE records in (channel, raster index) order; n_found: the true count; status: TRUNCATED or 0.  map reads
    the context's device buffers: valid until the context's next search or stack."""
    search: "ResidualSearch"
    grid: StackGrid
    weights: np.ndarray
    frames: np.ndarray
    candidates: np.ndarray
    n_found: int
    status: int
    serial: int

    def map(self, channel: int, kind) -> np.ndarray:
        """the H x W plane `kind` ("N", "D", "z", "count" or its number) of a channel"""
        self.search._live()
        if self.search.context._stack_serial != self.serial:
            raise RuntimeError("the context has stacked again: this stack's planes are gone")
        return self.search.context._stack_map(int(channel), STACK_KINDS[kind] if isinstance(kind, str) else int(kind), self.grid)


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

    def stack(self, grid: Optional[StackGrid] = None, weights=None, threshold: float = 5.0, min_images: int = 1,
              max_candidates: int = DEFAULT_MAX_CANDIDATES) -> "StackedSearch":
        """celeste_resid_stack over this search's maps: grid (None: the grid of the search's first image), weights
        [n_channels, 5] per band (None: FLAT_WEIGHTS).  Valid while this search is the context's last one."""
        self._live()
        return self.context._stack(self, grid, weights, threshold, min_images, max_candidates)


class ResidContext(_binding.Context):
    """The resid library's copy of a problem (celeste_resid_ctx_t), built from a marshalled celeste_problem_t."""
    _name, _load = "resid", staticmethod(load_library)

    def __init__(self, problem: "cabi.Problem", device: int = 0):
        super().__init__(problem, device)
        self._serial = 0
        self._stack_serial = 0
        self._wcs = (WcsT * len(problem.images))(*[wcs_of(im) for im in problem.images])
        self._images = problem.images
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

    def _stack(self, search, grid, weights, threshold, min_images, max_candidates) -> StackedSearch:
        if grid is None:
            if not search.images:
                raise ValueError("a search of no image has no default grid")
            grid = StackGrid.of_image(self._images[search.images[0]])
        wts = np.ascontiguousarray(np.asarray(FLAT_WEIGHTS if weights is None else weights, dtype=np.float64).reshape(-1, 5))
        if not 1 <= len(wts) <= STACK_MAX_CHANNELS:
            raise ValueError("1 .. %d channels" % STACK_MAX_CHANNELS)
        if not (np.isfinite(wts).all() and (wts >= 0).all() and (wts > 0).any(axis=1).all()):
            raise ValueError("weights must be finite and not negative, with one above zero in every channel")
        if int(min_images) < 1 or int(max_candidates) < 0:
            raise ValueError("min_images must be at least 1 and max_candidates not negative")
        if int(grid.H) < 1 or int(grid.W) < 1 or int(grid.H) * int(grid.W) >= 2 ** 31:
            raise ValueError("a grid of %d x %d cells" % (grid.H, grid.W))
        g = grid.c_struct()
        opts = StackOptsT(float(threshold), int(min_images), 0)
        frames = np.zeros(len(wts), dtype=STACK_FRAME_DTYPE)
        cand = np.zeros(max(int(max_candidates), 1), dtype=STACK_CANDIDATE_DTYPE)
        n_found, status = C.c_int64(0), C.c_int32(0)
        self._stack_serial += 1
        _check(self.lib, self.lib.celeste_resid_stack(self.handle, C.byref(g), len(self._wcs), self._wcs, len(wts), _ptr(wts, _dp),
                                                      C.byref(opts), frames.ctypes.data, cand.ctypes.data, int(max_candidates),
                                                      C.byref(n_found), C.byref(status)))
        n = min(int(n_found.value), int(max_candidates))
        return StackedSearch(search, grid, wts, frames, cand[:n].copy(), int(n_found.value), int(status.value), self._stack_serial)

    def _stack_map(self, channel: int, which: int, grid: StackGrid) -> np.ndarray:
        out = np.zeros(int(grid.H) * int(grid.W))
        _check(self.lib, self.lib.celeste_resid_stack_get_map(self.handle, channel, which, _ptr(out, _dp)))
        return out.reshape(int(grid.W), int(grid.H)).T.copy()

    def stack_last_ms(self):
        """device ms of the last stack: (the gather and the z ranges, the peaks and their world positions)"""
        ms = (C.c_float * 2)()
        _check(self.lib, self.lib.celeste_resid_stack_last_ms(self.handle, ms))
        return tuple(float(x) for x in ms)

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
    return _band_fluxes(search, images, joined, [len(d) for d in dets], flux_floor_nmgy)


def _band_fluxes(search, images, positions, n_detections, flux_floor_nmgy):
    """step 3 of missed_sources for the world positions `positions`: the table and one star CatalogEntry per position"""
    from .params import CatalogEntry
    simgs = list(search.images)
    table = np.zeros(len(positions), dtype=MISSED_DTYPE)
    entries = []
    for k, pos in enumerate(positions):
        ii, hh, ww, bands = [], [], [], []
        for n in simgs:
            pc = np.asarray(images[n].world_to_pix(pos), dtype=np.float64)
            if not np.isfinite(pc).all():
                continue
            ii.append(n); hh.append(int(np.rint(pc[0])) - 1); ww.append(int(np.rint(pc[1])) - 1); bands.append(images[n].b)
        sN, sD, sc = search.sample(ii, hh, ww)
        f, z, cnt = band_sums(bands, sN, sD, sc, search.min_coverage)
        table[k] = (pos[0], pos[1], n_detections[k], f, z, cnt)
        flux = np.where(np.isfinite(f), np.maximum(np.nan_to_num(f), flux_floor_nmgy), flux_floor_nmgy)
        entries.append(CatalogEntry(np.array(pos, dtype=np.float64), True, flux.copy(), flux.copy(), 0.5, 0.8, 0.0, 0.2))
    return table, entries


def _grid_world_to_pix(grid: StackGrid, world) -> np.ndarray:
    """1-based grid pixel coordinates of world positions [n, 2], by the grid's WCS (host, numpy: model.TanWCS or the matrix)"""
    from .model import TanWCS
    w = grid.wcs
    world = np.asarray(world, dtype=np.float64).reshape(-1, 2)
    if w.kind == WCS_TAN:
        return TanWCS(list(w.world0), list(w.pix0), np.array(list(w.m)).reshape(2, 2)).world_to_pix(world).reshape(-1, 2)
    J = np.array([[w.m[0], w.m[2]], [w.m[1], w.m[3]]])
    return (world - np.array(list(w.world0))) @ J.T + np.array(list(w.pix0))


def stacked_sources(stack, search, images, catalog, min_sep_px: float = 2.0, flux_floor_nmgy: float = DEFAULT_FLUX_FLOOR_NMGY):
    """The sources a stack found, as catalog entries.  `stack` needs .candidates (STACK_CANDIDATE_DTYPE fields) and .grid,
    `search` what missed_sources asks of one.
      1. candidates are taken in descending z across channels (ties: the list's order); one within min_sep_px grid pixels of a
         kept one is dropped;
      2. one within min_sep_px grid pixels of a catalog source (its position on the grid's plane) is dropped;
      3. per-band fluxes as step 3 of missed_sources, at the candidate's world position.
    Returns (table [MISSED_DTYPE], star CatalogEntry list); n_detections is the number of images added at the candidate's cell."""
    cand = stack.candidates
    order = np.argsort(-cand["z"], kind="stable")
    pix = np.stack([cand["h"] + 1.0 + cand["dh"], cand["w"] + 1.0 + cand["dw"]], axis=1).reshape(-1, 2)
    cpix = np.zeros((0, 2))
    if len(catalog):
        cpix = _grid_world_to_pix(stack.grid, np.array([ce.pos for ce in catalog], dtype=np.float64))
        cpix = cpix[np.isfinite(cpix).all(axis=1)]
    kept = []
    for i in order:
        if any(np.hypot(*(pix[i] - pix[j])) <= min_sep_px for j in kept):
            continue
        kept.append(int(i))
    kept = [i for i in kept if not (len(cpix) and (np.hypot(cpix[:, 0] - pix[i, 0], cpix[:, 1] - pix[i, 1]) <= min_sep_px).any())]
    return _band_fluxes(search, images, [cand["world"][i].copy() for i in kept], [int(cand["n_images"][i]) for i in kept],
                        flux_floor_nmgy)
