"""A box's problem on the device: patches, neighbour lists, eigen-PSF stamps and the sky check (libceleste_prep.so).

  host function                                              here
  ---------------------------------------------------------  ------------------------------------------------
  model.patch_table (get_sky_patches as arrays)              patch_table          (celeste_prep_patches)
  PatchTable.neighbors (find_neighbors for every source)     table.neighbor_lists (the same call)
  SDSSPSFMap.__call__ at every patch centre                  table.stamp / table.stamps (the same call)
  infer.bad_sky per catalog entry                            bad_sky_flags        (celeste_prep_bad_sky)
  detect.build_detection_output + model.neighbor_map         detected_table       (celeste_prep_detected)
  model.TanWCS of an image (projection, patch Jacobians)     PrepImages           (celeste_prep_images_set_wcs)

`PrepImages` uploads the planes once (numpy's row-major H x W arrays as they are) and serves any number of calls;
patch_table and bad_sky_flags make one of their own when none is given.  include/celeste_prep.h and DESIGN.md section 14
and 16 state the arithmetic: boxes, centres, counts, neighbour lists and flags are the host functions', exactly; the stamps and a
non-trivial Jacobian's world centres agree with numpy's within rounding (their summation orders are not numpy's).
The kernels are HIP (csrc/prep/celeste_prep.hip); there is no CPU path.
"""
import ctypes as C
import math
import os
from typing import List, Optional, Sequence

import numpy as np

from . import _binding, cabi
from .model import PatchTable, SDSSPSFMap, get_psf_width
from .params import CatalogEntry

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "prep", "libceleste_prep.so")
ABI_VERSION = 100          # CELESTE_PREP_ABI_VERSION of include/celeste_prep.h
EXPORTED_SYMBOLS = ["celeste_prep_version", "celeste_prep_strerror", "celeste_prep_images_create", "celeste_prep_images_destroy",
                    "celeste_prep_patches", "celeste_prep_result_get", "celeste_prep_result_destroy", "celeste_prep_bad_sky",
                    "celeste_prep_last_ms", "celeste_prep_detected_check", "celeste_prep_detected",
                    "celeste_prep_result_get_catalog", "celeste_prep_detected_last_ms", "celeste_prep_wcs_check",
                    "celeste_prep_images_set_wcs", "celeste_prep_result_get_jacobians"]
ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_ALLOC = 1, 2, 3, 4
FLAG_DENSE, FLAG_STAMPS = 1, 2
STAMP = 51                 # CELESTE_PREP_STAMP
N_STAGES = 5               # CELESTE_PREP_N_STAGES
STAGES = ("geometry", "active_pixels", "neighbors", "stamps", "sky")
MATCH_TILE = 1024          # CELESTE_PREP_MATCH_TILE: joined positions per LDS tile of the match kernel
MATCH_BLOCK = 256          # CELESTE_PREP_MATCH_BLOCK: detections per workgroup of the match kernel
DETECTED_N_STAGES = 6      # CELESTE_PREP_DETECTED_N_STAGES
DETECTED_STAGES = ("join", "entries", "geometry", "active_pixels", "neighbors", "stamps")
MIN_RADIUS_PIX, DILATE = 5.0, 0.2     # detection.jl:152-167
WCS_AFFINE, WCS_TAN = 0, 1            # celeste_prep_wcs_t.kind

c_float_p, c_double_p = C.POINTER(C.c_float), C.POINTER(C.c_double)


class PrepImageT(C.Structure):
    """celeste_prep_image_t"""
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("band", C.c_int32), ("reserved", C.c_int32),
                ("pixels", c_float_p), ("stride_h", C.c_int64), ("stride_w", C.c_int64),
                ("sky", c_float_p), ("sky_stride_h", C.c_int64), ("sky_stride_w", C.c_int64),
                ("nelec_per_nmgy", c_float_p), ("wcs_jacobian", C.c_double * 4), ("wcs_world0", C.c_double * 2),
                ("wcs_pix0", C.c_double * 2), ("psf_width", C.c_double), ("epsilon", C.c_double),
                ("rnrow", C.c_int32), ("rncol", C.c_int32), ("ni", C.c_int32), ("nj", C.c_int32), ("nk", C.c_int32),
                ("reserved2", C.c_int32), ("rrows", c_double_p), ("cmat", c_double_p)]


class PrepWcsT(C.Structure):
    """celeste_prep_wcs_t"""
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("crval", C.c_double * 2), ("crpix", C.c_double * 2),
                ("cd", C.c_double * 4)]


class PrepSourceT(C.Structure):
    """celeste_prep_source_t"""
    _fields_ = [("pos", C.c_double * 2), ("is_star", C.c_int32), ("reserved", C.c_int32), ("flux", C.c_double * 5),
                ("gal_radius_px", C.c_double)]


SOURCE_DTYPE = np.dtype([("pos", "<f8", (2,)), ("is_star", "<i4"), ("reserved", "<i4"), ("flux", "<f8", (5,)),
                         ("gal_radius_px", "<f8")])   # celeste_prep_source_t, field for field


class PrepTableT(C.Structure):
    """celeste_prep_table_t"""
    _fields_ = [("n_entries", C.c_int64), ("n_sources", C.c_int64), ("n_neighbors", C.c_int64), ("n_stamps", C.c_int64),
                ("source", C.POINTER(C.c_int32)), ("image", C.POINTER(C.c_int32)), ("box", C.POINTER(C.c_int64)),
                ("pixel_center", c_double_p), ("world_center", c_double_p), ("active_pixels", C.POINTER(C.c_int64)),
                ("nbr_offsets", C.POINTER(C.c_int64)), ("nbr_index", C.POINTER(C.c_int32)), ("stamp", C.POINTER(C.c_int32)),
                ("stamps", c_double_p)]


class PrepDetectionT(C.Structure):
    """celeste_prep_detection_t"""
    _fields_ = [("npix", C.c_int32), ("xmin", C.c_int32), ("xmax", C.c_int32), ("ymin", C.c_int32), ("ymax", C.c_int32),
                ("reserved", C.c_int32), ("x", C.c_double), ("y", C.c_double), ("a", C.c_double), ("b", C.c_double),
                ("theta", C.c_double), ("flux", C.c_double)]


DETECTION_DTYPE = np.dtype([("npix", "<i4"), ("xmin", "<i4"), ("xmax", "<i4"), ("ymin", "<i4"), ("ymax", "<i4"), ("reserved", "<i4"),
                            ("x", "<f8"), ("y", "<f8"), ("a", "<f8"), ("b", "<f8"), ("theta", "<f8"),
                            ("flux", "<f8")])   # celeste_prep_detection_t, field for field


class PrepCatalogT(C.Structure):
    """celeste_prep_catalog_t"""
    _fields_ = [("n_objects", C.c_int64), ("n_detections", C.c_int64), ("pos", c_double_p), ("flux", c_double_p),
                ("gal_axis_ratio", c_double_p), ("gal_angle", c_double_p), ("gal_radius_px", c_double_p),
                ("det_offsets", C.POINTER(C.c_int64)), ("det_image", C.POINTER(C.c_int32)), ("det_object", C.POINTER(C.c_int32))]


class PrepError(RuntimeError):
    def __init__(self, status: int, text: str):
        super().__init__("libceleste_prep: %s (status %d)" % (text, status))
        self.status = status


def _declare(lib):
    assert SOURCE_DTYPE.itemsize == C.sizeof(PrepSourceT) and DETECTION_DTYPE.itemsize == C.sizeof(PrepDetectionT)
    vp = C.c_void_p
    lib.celeste_prep_strerror.restype = C.c_char_p
    lib.celeste_prep_strerror.argtypes = [C.c_int]
    lib.celeste_prep_images_create.restype = C.c_int
    lib.celeste_prep_images_create.argtypes = [C.c_int, C.c_int32, C.POINTER(PrepImageT), C.POINTER(vp)]
    lib.celeste_prep_images_destroy.restype = None
    lib.celeste_prep_images_destroy.argtypes = [vp]
    lib.celeste_prep_patches.restype = C.c_int
    lib.celeste_prep_patches.argtypes = [vp, C.c_int64, vp, C.c_double, C.c_uint32, C.POINTER(vp)]
    lib.celeste_prep_result_get.restype = C.c_int
    lib.celeste_prep_result_get.argtypes = [vp, C.POINTER(PrepTableT)]
    lib.celeste_prep_result_destroy.restype = None
    lib.celeste_prep_result_destroy.argtypes = [vp]
    lib.celeste_prep_bad_sky.restype = C.c_int
    lib.celeste_prep_bad_sky.argtypes = [vp, C.c_int64, c_double_p, C.POINTER(C.c_uint8)]
    lib.celeste_prep_last_ms.restype = C.c_int
    lib.celeste_prep_last_ms.argtypes = [c_float_p]
    lib.celeste_prep_detected_check.restype = C.c_int
    lib.celeste_prep_detected_check.argtypes = [C.c_int32, vp, vp, vp, C.c_double, C.c_double, C.c_double, C.c_uint32]
    lib.celeste_prep_detected.restype = C.c_int
    lib.celeste_prep_detected.argtypes = [vp, vp, vp, vp, C.c_double, C.c_double, C.c_double, C.c_uint32, C.POINTER(vp)]
    lib.celeste_prep_result_get_catalog.restype = C.c_int
    lib.celeste_prep_result_get_catalog.argtypes = [vp, C.POINTER(PrepCatalogT)]
    lib.celeste_prep_detected_last_ms.restype = C.c_int
    lib.celeste_prep_detected_last_ms.argtypes = [c_float_p]
    lib.celeste_prep_wcs_check.restype = C.c_int
    lib.celeste_prep_wcs_check.argtypes = [C.c_int32, C.POINTER(PrepWcsT)]
    lib.celeste_prep_images_set_wcs.restype = C.c_int
    lib.celeste_prep_images_set_wcs.argtypes = [vp, C.c_int32, C.POINTER(PrepWcsT)]
    lib.celeste_prep_result_get_jacobians.restype = C.c_int
    lib.celeste_prep_result_get_jacobians.argtypes = [vp, C.POINTER(c_double_p)]


def load_library(path: Optional[str] = None) -> C.CDLL:
    """libceleste_prep.so; CELESTE_MI355X_PREP_LIB overrides its path (_binding.open_library)"""
    return _binding.open_library("prep", LIB_PATH, "CELESTE_MI355X_PREP_LIB", ABI_VERSION, "celeste_prep_version", _declare, path)


_check = _binding.checker("prep", PrepError)


def last_ms() -> dict:
    """device milliseconds of the stages of the last call, by name (STAGES)"""
    ms = (C.c_float * N_STAGES)()
    load_library().celeste_prep_last_ms(ms)
    return {k: float(v) for k, v in zip(STAGES, ms)}


def detected_last_ms() -> dict:
    """device milliseconds of the stages of the last call, when it was detected_table, by name (DETECTED_STAGES)"""
    ms = (C.c_float * DETECTED_N_STAGES)()
    load_library().celeste_prep_detected_last_ms(ms)
    return {k: float(v) for k, v in zip(DETECTED_STAGES, ms)}


def _plane(a):
    """(float32 array, stride_h, stride_w in elements): the array as it is when it is a row-major or column-major float32
    plane, else a row-major copy"""
    a = np.asarray(a)
    if a.dtype != np.float32 or a.ndim != 2 or not (a.flags.c_contiguous or a.flags.f_contiguous):
        a = np.ascontiguousarray(a, dtype=np.float32)
    H, W = a.shape
    return (a, W, 1) if a.flags.c_contiguous else (a, 1, H)


def image_structs(images, keep: list):
    """Model.Image list -> celeste_prep_image_t array (`keep` holds the buffers alive)"""
    arr = (PrepImageT * max(len(images), 1))()
    sky_done = False
    for n, im in enumerate(images):
        a = arr[n]
        px, sh, sw = _plane(im.pixels)
        iota = np.ascontiguousarray(im.nelec_per_nmgy, dtype=np.float32)
        assert iota.shape == (px.shape[0],)
        keep += [px, iota]
        a.H, a.W, a.band = px.shape[0], px.shape[1], int(im.b)
        a.pixels, a.stride_h, a.stride_w = px.ctypes.data_as(c_float_p), sh, sw
        a.nelec_per_nmgy = iota.ctypes.data_as(c_float_p)
        if int(im.b) == 4 and not sky_done:      # the sky check reads the first band-4 image's sky plane
            sky, a.sky_stride_h, a.sky_stride_w = _plane(im.sky)
            assert sky.shape == px.shape
            keep.append(sky)
            a.sky = sky.ctypes.data_as(c_float_p)
            sky_done = True
        J = np.asarray(im.wcs_jacobian, dtype=np.float64)
        a.wcs_jacobian[0], a.wcs_jacobian[1], a.wcs_jacobian[2], a.wcs_jacobian[3] = J[0, 0], J[1, 0], J[0, 1], J[1, 1]
        a.wcs_world0[0], a.wcs_world0[1] = float(im.wcs_world0[0]), float(im.wcs_world0[1])
        a.wcs_pix0[0], a.wcs_pix0[1] = float(im.wcs_pix0[0]), float(im.wcs_pix0[1])
        # the two per-image scalars of choose_patch_radius (width_scale 1.2), as model.choose_patch_radius forms them
        a.psf_width = get_psf_width(im.psf, width_scale=1.2)
        a.epsilon = float(im.sky[a.H // 2 - 1, a.W // 2 - 1])
        if isinstance(im.psfmap, SDSSPSFMap):
            m = im.psfmap
            rrows = np.ascontiguousarray(m.rrows, dtype=np.float64)
            cmat = np.ascontiguousarray(m.cmat, dtype=np.float64)
            keep += [rrows, cmat]
            a.rnrow, a.rncol = int(m.rnrow), int(m.rncol)
            a.ni, a.nj, a.nk = cmat.shape
            a.rrows, a.cmat = rrows.ctypes.data_as(c_double_p), cmat.ctypes.data_as(c_double_p)
    return arr


def wcs_structs(images):
    """Model.Image list -> celeste_prep_wcs_t array: kind TAN for an image with a model.TanWCS, else AFFINE"""
    arr = (PrepWcsT * max(len(images), 1))()
    for n, im in enumerate(images):
        w = getattr(im, "wcs", None)
        if w is None:
            arr[n].kind = WCS_AFFINE
            continue
        arr[n].kind = WCS_TAN
        arr[n].crval[0], arr[n].crval[1] = float(w.crval[0]), float(w.crval[1])
        arr[n].crpix[0], arr[n].crpix[1] = float(w.crpix[0]), float(w.crpix[1])
        arr[n].cd[0], arr[n].cd[1], arr[n].cd[2], arr[n].cd[3] = (float(w.cd[0, 0]), float(w.cd[0, 1]), float(w.cd[1, 0]),
                                                                  float(w.cd[1, 1]))
    return arr


class PrepImages:
    """celeste_prep_images_t: the planes, calibrations, WCS and eigen-PSFs of `images` on `device`.  A context manager;
    `close()` releases the device memory."""

    def __init__(self, images, device: int = 0):
        self.lib = load_library()
        self.images = images
        self.device = int(device)
        self._keep: List[object] = []
        self.has_eigen_psf = any(isinstance(im.psfmap, SDSSPSFMap) for im in images)
        arr = image_structs(images, self._keep)
        h = C.c_void_p()
        _check(self.lib, self.lib.celeste_prep_images_create(self.device, len(images), arr, C.byref(h)))
        self.handle = h
        self.has_tan_wcs = any(getattr(im, "wcs", None) is not None for im in images)
        if self.has_tan_wcs:
            self.set_wcs(wcs_structs(images))

    def set_wcs(self, arr, n: Optional[int] = None):
        """celeste_prep_images_set_wcs with a celeste_prep_wcs_t array (wcs_structs)"""
        _check(self.lib, self.lib.celeste_prep_images_set_wcs(self.handle, len(self.images) if n is None else n, arr))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.celeste_prep_images_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Result:
    """celeste_prep_result_t: owns the page-locked arrays the table's `stamps` is a view of"""

    def __init__(self, lib, handle):
        self.lib, self.handle = lib, handle

    def __del__(self):
        try:
            if self.handle:
                self.lib.celeste_prep_result_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def source_table(catalog) -> np.ndarray:
    """the celeste_prep_source_t array of a catalog: position, kind, the fluxes choose_patch_radius reads, galaxy radius"""
    src = np.zeros(len(catalog), dtype=SOURCE_DTYPE)
    if len(catalog):
        src["pos"] = np.array([ce.pos for ce in catalog], dtype=np.float64).reshape(-1, 2)
        src["is_star"] = [1 if ce.is_star else 0 for ce in catalog]
        src["flux"] = np.array([ce.star_fluxes if ce.is_star else ce.gal_fluxes for ce in catalog], dtype=np.float64).reshape(-1, 5)
        src["gal_radius_px"] = [ce.gal_radius_px for ce in catalog]
    return src


def _view(ptr, shape, dtype):
    n = int(np.prod(shape))
    if n == 0:
        return np.zeros(shape, dtype=dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).view(dtype).reshape(shape)


def patch_table(images, catalog, radius_override_pix: float = math.nan, sparse: bool = False, device: int = 0,
                prep_images: Optional[PrepImages] = None) -> PatchTable:
    """model.patch_table on the device: the same PatchTable, plus `neighbor_lists` (what PatchTable.neighbors() returns)
    and, when an image has an SDSSPSFMap, `stamp` ([E] index into `stamps`, -1 for entries of constant-map images) and
    `stamps` ([n, 51 * 51] raw column-major stamps at the entries' pixel centres).  A tried pair without a positive
    flux raises PrepError (status ERR_INVALID_ARG), where the host function raises AssertionError."""
    own = prep_images is None
    pi = PrepImages(images, device) if own else prep_images
    try:
        lib = pi.lib
        assert len(pi.images) == len(images)
        src = source_table(catalog)
        flags = (0 if sparse else FLAG_DENSE) | (FLAG_STAMPS if pi.has_eigen_psf else 0)
        rh = C.c_void_p()
        _check(lib, lib.celeste_prep_patches(pi.handle, len(src), src.ctypes.data_as(C.c_void_p), float(radius_override_pix),
                                             flags, C.byref(rh)))
        res = _Result(lib, rh)
        table = _table_from_result(lib, rh, res, len(images), sparse, pi.has_eigen_psf)
        return table
    finally:
        if own:
            pi.close()


def _table_from_result(lib, rh, res, n_images: int, sparse: bool, with_stamps: bool) -> PatchTable:
    t = PrepTableT()
    _check(lib, lib.celeste_prep_result_get(rh, C.byref(t)))
    E, S = int(t.n_entries), int(t.n_sources)
    table = PatchTable(S, n_images, not sparse,
                       _view(t.source, (E,), np.int32).copy(), _view(t.image, (E,), np.int32).copy(),
                       _view(t.box, (E, 4), np.int64).copy(), _view(t.pixel_center, (E, 2), np.float64).copy(),
                       _view(t.world_center, (E, 2), np.float64).copy(), _view(t.active_pixels, (E,), np.int64).copy())
    off = _view(t.nbr_offsets, (S + 1,), np.int64).tolist()
    idx = _view(t.nbr_index, (int(t.n_neighbors),), np.int32).tolist()
    table.neighbor_lists = [idx[off[s]:off[s + 1]] for s in range(S)]
    jp = c_double_p()
    _check(lib, lib.celeste_prep_result_get_jacobians(rh, C.byref(jp)))
    if jp:       # some image has a TanWCS: per-patch Jacobians, [E][4] = J11, J21, J12, J22
        j = _view(jp, (E, 4), np.float64)
        table.wcs_jacobian = np.stack([j[:, 0], j[:, 2], j[:, 1], j[:, 3]], axis=1).reshape(E, 2, 2)
    if with_stamps:
        table.stamp = _view(t.stamp, (E,), np.int32).copy()
        table.stamps = _view(t.stamps, (int(t.n_stamps), STAMP * STAMP), np.float64)   # a view: no copy of the stamps
        table._prep_result = res      # (owns the memory of `stamps`)
    return table


def detection_table(catalogs):
    """(det_offsets [n_images + 1] int64, the celeste_prep_detection_t array) of per-image detect.Catalog objects"""
    off = np.zeros(len(catalogs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(c) for c in catalogs])
    det = np.zeros(int(off[-1]), dtype=DETECTION_DTYPE)
    for n, c in enumerate(catalogs):
        d = det[off[n]:off[n + 1]]
        for k in ("npix", "xmin", "xmax", "ymin", "ymax", "x", "y", "a", "b", "theta", "flux"):
            d[k] = getattr(c, k)
    return off, det


def detected_table(images, catalogs, match_radius: float, sparse: Optional[bool] = None, device: int = 0,
                   prep_images: Optional[PrepImages] = None):
    """detect.build_detection_output and model.neighbor_map on the device: (catalog, table) of the per-image detect.Catalog
    objects `catalogs`.  catalog: the CatalogEntry list of the joined objects (detect.match_detections, detect.catalog_entry);
    table: their model.PatchTable with the boxes of detect.detection_box, `neighbor_lists`, `stamp` / `stamps` when an image
    has an SDSSPSFMap (as patch_table returns them) and `detections`, one list of (image, object) per joined object.
    sparse=None: build_detection_output's rule, more than 8 images."""
    from .detect import x_vs_n_angle
    if len(catalogs) != len(images):
        raise ValueError("one catalog per image: %d catalogs, %d images" % (len(catalogs), len(images)))
    if sparse is None:
        sparse = len(images) > 8
    own = prep_images is None
    pi = PrepImages(images, device) if own else prep_images
    try:
        lib = pi.lib
        assert len(pi.images) == len(images)
        off, det = detection_table(catalogs)
        ang = np.array([x_vs_n_angle(im.wcs_jacobian) for im in images], dtype=np.float64)
        flags = (0 if sparse else FLAG_DENSE) | (FLAG_STAMPS if pi.has_eigen_psf else 0)
        rh = C.c_void_p()
        _check(lib, lib.celeste_prep_detected(pi.handle, off.ctypes.data_as(C.c_void_p), det.ctypes.data_as(C.c_void_p),
                                              ang.ctypes.data_as(C.c_void_p), float(match_radius), MIN_RADIUS_PIX, DILATE, flags,
                                              C.byref(rh)))
        res = _Result(lib, rh)
        table = _table_from_result(lib, rh, res, len(images), sparse, pi.has_eigen_psf)
        k = PrepCatalogT()
        _check(lib, lib.celeste_prep_result_get_catalog(rh, C.byref(k)))
        S, D = int(k.n_objects), int(k.n_detections)
        pos = _view(k.pos, (S, 2), np.float64).copy()
        flux = _view(k.flux, (S, 5), np.float64).copy()
        ratio = _view(k.gal_axis_ratio, (S,), np.float64).tolist()
        angle = _view(k.gal_angle, (S,), np.float64).tolist()
        radius = _view(k.gal_radius_px, (S,), np.float64).tolist()
        catalog = [CatalogEntry(pos[s], False, flux[s].copy(), flux[s], 0.5, ratio[s], angle[s], radius[s]) for s in range(S)]
        doff = _view(k.det_offsets, (S + 1,), np.int64).tolist()
        pairs = list(zip(_view(k.det_image, (D,), np.int32).tolist(), _view(k.det_object, (D,), np.int32).tolist()))
        table.detections = [pairs[doff[s]:doff[s + 1]] for s in range(S)]
        return catalog, table
    finally:
        if own:
            pi.close()


def bad_sky_flags(entries, images, device: int = 0, prep_images: Optional[PrepImages] = None) -> List[bool]:
    """infer.bad_sky for many catalog entries at once, one workgroup per entry"""
    entries = list(entries)
    if not entries or not any(im.b == 4 for im in images):
        return [False] * len(entries)
    own = prep_images is None
    pi = PrepImages(images, device) if own else prep_images
    try:
        pos = np.ascontiguousarray(np.array([ce.pos for ce in entries], dtype=np.float64).reshape(-1, 2))
        out = np.zeros(len(entries), dtype=np.uint8)
        _check(pi.lib, pi.lib.celeste_prep_bad_sky(pi.handle, len(entries), pos.ctypes.data_as(c_double_p),
                                                   out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return [bool(x) for x in out]
    finally:
        if own:
            pi.close()
