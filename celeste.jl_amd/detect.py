"""Source detection: SEP.extract on the device (libceleste_detect.so, include/celeste_detect.h) and the reference's
detect_sources (src/detection.jl:39-171) on top of it.

Axes: SEP's x is the ROW index (axis 0) of the H x W planes, SEP's y the column index; `x` and `y` of a catalog are
1-based like SEP.jl:384-385, the boxes xmin .. ymax stay 0-based (SEP.jl does not shift them).
"""
import ctypes as C
import math
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _binding
from .model import Image, ImagePatch, PatchRow, box_around_point, clamp_box, julia_round
from .params import CatalogEntry

OK, ERR_INVALID_ARG, ERR_HIP, ERR_NO_DEVICE, ERR_ALLOC = 0, 1, 4, 5, 6
WANT_MAPS, TIMING = 1, 2
ABI_VERSION = 100
STAGES = ("calibrate", "mesh", "filter_threshold", "labelling", "deblend", "moments")

EXPORTED_SYMBOLS = ["celeste_detect_version", "celeste_detect_strerror", "celeste_detect_run", "celeste_detect_result_free"]

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "detect", "libceleste_detect.so")


class ImageT(C.Structure):
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("pixels", C.POINTER(C.c_float)), ("sky", C.POINTER(C.c_float)),
                ("nelec_per_nmgy", C.POINTER(C.c_float))]


class ParamsT(C.Structure):
    _fields_ = [("thresh", C.c_float), ("minarea", C.c_int32), ("deblend_nthresh", C.c_int32), ("flags", C.c_int32),
                ("deblend_cont", C.c_double), ("lds_max_pixels", C.c_int32), ("reserved", C.c_int32)]


class ObjectT(C.Structure):
    _fields_ = [("npix", C.c_int32), ("xmin", C.c_int32), ("xmax", C.c_int32), ("ymin", C.c_int32), ("ymax", C.c_int32),
                ("parent", C.c_int32), ("reserved", C.c_int32), ("pix_offset", C.c_int64),
                ("x", C.c_double), ("y", C.c_double), ("x2", C.c_double), ("y2", C.c_double), ("xy", C.c_double),
                ("a", C.c_double), ("b", C.c_double), ("theta", C.c_double), ("flux", C.c_double), ("peak", C.c_double)]


class ImageResultT(C.Structure):
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("rms", C.c_float), ("thresh", C.c_float), ("n_objects", C.c_int32),
                ("n_parents", C.c_int32), ("n_pix", C.c_int64), ("objects", C.POINTER(ObjectT)),
                ("pix", C.POINTER(C.c_int64)), ("mask", C.POINTER(C.c_uint8)), ("segmap", C.POINTER(C.c_int32))]


class ResultT(C.Structure):
    _fields_ = [("n_images", C.c_int32), ("reserved", C.c_int32), ("stage_ms", C.c_double * 6),
                ("images", C.POINTER(ImageResultT))]


class DetectError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__("celeste_detect status %d: %s" % (status, msg))
        self.status = status


_check = _binding.checker("detect", DetectError)


def _declare(lib):
    lib.celeste_detect_strerror.restype = C.c_char_p
    lib.celeste_detect_strerror.argtypes = [C.c_int]
    lib.celeste_detect_run.restype = C.c_int
    lib.celeste_detect_run.argtypes = [C.c_int32, C.c_int32, C.POINTER(ImageT), C.POINTER(ParamsT),
                                       C.POINTER(C.POINTER(ResultT))]
    lib.celeste_detect_result_free.restype = None
    lib.celeste_detect_result_free.argtypes = [C.POINTER(ResultT)]


def load_library(path: Optional[str] = None) -> C.CDLL:
    """The detection library; CELESTE_MI355X_DETECT_LIB overrides its path (_binding.open_library).  It does not need the
    engine's library: torch's HIP runtime alone is loaded first, so that one runtime serves the process."""
    return _binding.open_library("detect", LIB_PATH, "CELESTE_MI355X_DETECT_LIB", ABI_VERSION, "celeste_detect_version", _declare,
                                 path, engine=False)


@dataclass
class Catalog:
    """SEP.Catalog of one image (SEP.jl:365-398) plus the rms and threshold used, the parent of each object and its
    pixels (0-based (row, column) pairs, in SEP's raster order)."""
    rms: float
    thresh: float
    npix: np.ndarray
    xmin: np.ndarray
    xmax: np.ndarray
    ymin: np.ndarray
    ymax: np.ndarray
    x: np.ndarray            # 1-based
    y: np.ndarray            # 1-based
    x2: np.ndarray
    y2: np.ndarray
    xy: np.ndarray
    a: np.ndarray
    b: np.ndarray
    theta: np.ndarray
    flux: np.ndarray
    peak: np.ndarray
    parent: np.ndarray
    pixels: List[np.ndarray] = field(default_factory=list)
    mask: Optional[np.ndarray] = None      # want_maps: conv > thresh
    segmap: Optional[np.ndarray] = None    # want_maps: object index + 1, 0 = none

    def __len__(self):
        return int(self.npix.size)


def _image_arrays(img):
    if isinstance(img, Image):
        return img.pixels, img.sky, img.nelec_per_nmgy
    return img   # (pixels, sky, nelec_per_nmgy)


def extract(images, device: int = 0, thresh: float = 1.3, minarea: int = 5, deblend_nthresh: int = 32,
            deblend_cont: float = 0.005, want_maps: bool = False, lds_max_pixels: int = 0,
            stage_ms: Optional[dict] = None, want_pixels: bool = True) -> List[Catalog]:
    """SEP.Background(cal; boxsize=(256, 256), filtersize=(3, 3)) + global_rms + SEP.extract(cal, thresh; noise=rms)
    (detection.jl:45-58) for every image, in one device call.  `images`: model.Image objects or (pixels, sky,
    nelec_per_nmgy) triples.  SEP's `clean` pass (removal of detections explained by a bright neighbour's wings) is not
    done.  lds_max_pixels > 0 lowers the size limit of the LDS deblending path (components above it take the
    global-memory path).  stage_ms: a dict that receives the device time of each stage.  want_pixels=False leaves
    Catalog.pixels empty (the per-object lists are built by a Python loop that callers of the moments alone do not need)."""
    lib = load_library()
    keep = []
    arr = (ImageT * max(len(images), 1))()
    for n, img in enumerate(images):
        px, sky, nelec = _image_arrays(img)
        px = np.ascontiguousarray(px, dtype=np.float32)
        sky = np.ascontiguousarray(sky, dtype=np.float32)
        nelec = np.ascontiguousarray(nelec, dtype=np.float32)
        if px.ndim != 2 or sky.shape != px.shape or nelec.shape != (px.shape[0],):
            raise ValueError("image %d: pixels and sky must be H x W and nelec_per_nmgy of length H" % n)
        keep += [px, sky, nelec]
        fp = C.POINTER(C.c_float)
        arr[n] = ImageT(px.shape[0], px.shape[1], px.ctypes.data_as(fp), sky.ctypes.data_as(fp), nelec.ctypes.data_as(fp))
    prm = ParamsT(thresh, minarea, deblend_nthresh, (WANT_MAPS if want_maps else 0) | (TIMING if stage_ms is not None else 0),
                  deblend_cont, lds_max_pixels, 0)
    res = C.POINTER(ResultT)()
    st = lib.celeste_detect_run(device, len(images), arr, C.byref(prm), C.byref(res))
    _check(lib, st)
    try:
        out = []
        if stage_ms is not None:
            stage_ms.update({k: float(res.contents.stage_ms[i]) for i, k in enumerate(STAGES)})
        for n in range(len(images)):
            R = res.contents.images[n]
            m = R.n_objects
            if m > 0:
                objs = np.ctypeslib.as_array(C.cast(R.objects, C.POINTER(C.c_uint8)), shape=(m * C.sizeof(ObjectT),))
                rec = np.frombuffer(objs.tobytes(), dtype=np.dtype({
                    "names": [f[0] for f in ObjectT._fields_],
                    "formats": ["<i4"] * 7 + ["<i8"] + ["<f8"] * 10,
                    "offsets": [getattr(ObjectT, f[0]).offset for f in ObjectT._fields_],
                    "itemsize": C.sizeof(ObjectT)}))
                pix = np.ctypeslib.as_array(R.pix, shape=(R.n_pix,)).copy() if want_pixels else None
            else:
                rec = np.zeros(0, dtype=[(f[0], "<f8") for f in ObjectT._fields_])
                pix = np.zeros(0, dtype=np.int64)
            H = R.H
            pixels = []
            for o in range(m if want_pixels else 0):
                s = pix[rec["pix_offset"][o]: rec["pix_offset"][o] + rec["npix"][o]]
                pixels.append(np.stack([s % H, s // H], axis=1))
            ints = {k: np.asarray(rec[k], dtype=np.int64) for k in ("npix", "xmin", "xmax", "ymin", "ymax", "parent")}
            dbl = {k: np.asarray(rec[k], dtype=np.float64) for k in ("x2", "y2", "xy", "a", "b", "theta", "flux", "peak")}
            cat = Catalog(rms=float(R.rms), thresh=float(R.thresh), x=np.asarray(rec["x"], dtype=np.float64) + 1.0,
                          y=np.asarray(rec["y"], dtype=np.float64) + 1.0, pixels=pixels, **ints, **dbl)
            if want_maps:
                cat.mask = np.ctypeslib.as_array(R.mask, shape=(R.H, R.W)).astype(bool)
                cat.segmap = np.ctypeslib.as_array(R.segmap, shape=(R.H, R.W)).copy()
            out.append(cat)
        return out
    finally:
        lib.celeste_detect_result_free(res)


# ---- detect_sources (detection.jl) --------------------------------------------------------------------------------

def x_vs_n_angle(wcs_jacobian) -> float:
    """_x_vs_n_angle (detection.jl:22-29) for an affine WCS: the CD matrix is the inverse of the pixel-per-world
    Jacobian, and Julia's cd[1, 2] is cd[0, 1] here."""
    cd = np.linalg.inv(np.asarray(wcs_jacobian, dtype=np.float64))
    sgn = float(np.sign(np.linalg.det(cd)))
    n_vs_y_rot = math.atan2(sgn * cd[0, 1], sgn * cd[0, 0])
    return -(n_vs_y_rot + math.pi / 2)


def dilate_box(box, factor: float):
    """dilate_box / _dilate_range (imaged_sources.jl:15-22), Julia's round (ties to even)."""
    def rng(r):
        delta = julia_round(factor * (r[1] - r[0] + 1) / 2)
        return (r[0] - delta, r[1] + delta)
    return (rng(box[0]), rng(box[1]))


def enclose_boxes(b1, b2):
    """enclose_boxes (imaged_sources.jl:24-28)"""
    return ((min(b1[0][0], b2[0][0]), max(b1[0][1], b2[0][1])), (min(b1[1][0], b2[1][0]), max(b1[1][1], b2[1][1])))


def world_coords(cat: Catalog, img: Image) -> np.ndarray:
    """_worldcoords (detection.jl:9-17): world position of every object, n x 2."""
    if len(cat) == 0:
        return np.zeros((0, 2))
    pix = np.stack([cat.x, cat.y], axis=1)
    if img.wcs is not None:
        return img.pix_to_world(pix)
    return np.linalg.solve(np.asarray(img.wcs_jacobian, float), (pix - img.wcs_pix0).T).T + img.wcs_world0


def angular_separation(lon1, lat1, lon2, lat2):
    """Coordinates.jl:15-26: the angle in degrees between two points of the sphere, longitudes and latitudes in degrees."""
    dl = np.radians(np.asarray(lon2, dtype=np.float64) - lon1)
    p1, p2 = np.radians(lat1), np.radians(lat2)
    s1, s2, c1, c2 = np.sin(p1), np.sin(p2), np.cos(p1), np.cos(p2)
    return np.degrees(np.arctan2(np.hypot(c2 * np.sin(dl), c1 * s2 - s1 * c2 * np.cos(dl)), s1 * s2 + c1 * c2 * np.cos(dl)))


def unit_vectors(world) -> np.ndarray:
    """_spherical_to_cartesian (Coordinates.jl:33-45): [n, 2] (lon, lat) in degrees -> [n, 3]"""
    w = np.radians(np.asarray(world, dtype=np.float64).reshape(-1, 2))
    cl = np.cos(w[:, 1])
    return np.stack([cl * np.cos(w[:, 0]), cl * np.sin(w[:, 0]), np.sin(w[:, 1])], axis=1)


def match_detections(worlds: Sequence[np.ndarray], match_radius: float, angular: bool = False):
    """detection.jl:67-98: the joined list starts as image 1's detections; each detection of a later image joins its
    nearest joined entry (as the list stood before that image) when closer than match_radius, else it is appended.
    angular=False: distances are planar in world coordinates (the affine WCS of model.Image).  angular=True: world
    coordinates are (ra, dec) in degrees and match_radius is in degrees, as in match_coordinates (Coordinates.jl:71-86):
    the nearest entry is the one with the shortest chord between unit vectors (the lowest index on a tie), and a
    detection joins it when 2 asind(chord / 2) < match_radius.
    Returns (joined positions, detections: one list of (image, object) per joined entry, 0-based)."""
    if len(worlds) == 0:
        return np.zeros((0, 2)), []
    joined = [w for w in np.asarray(worlds[0], float).reshape(-1, 2)]
    detections = [[(0, j)] for j in range(len(joined))]
    for i in range(1, len(worlds)):
        w = np.asarray(worlds[i], float).reshape(-1, 2)
        if w.shape[0] == 0:
            continue
        ref = np.array(joined) if joined else np.zeros((0, 2))
        if angular:
            uref, uw = unit_vectors(ref), unit_vectors(w)
        for j in range(w.shape[0]):
            if ref.shape[0] > 0:
                if angular:
                    e = uref - uw[j]
                    chord = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
                    k = int(np.argmin(chord))
                    d = 2.0 * np.degrees(np.arcsin(np.minimum(chord / 2.0, 1.0)))
                else:
                    d = np.hypot(ref[:, 0] - w[j, 0], ref[:, 1] - w[j, 1])
                    k = int(np.argmin(d))
                if d[k] < match_radius:
                    detections[k].append((i, j))
                    continue
            joined.append(w[j].copy())
            detections.append([(i, j)])
    return np.array(joined).reshape(-1, 2), detections


def catalog_entry(world_center, dets, catalogs: Sequence[Catalog], images, x_vs_n: Sequence[float],
                  n_bands: int = 5) -> CatalogEntry:
    """detection.jl:116-146: fluxes from the detection with the most pixels in each band (0 where a band has none),
    shape from the single best band."""
    best = [None] * n_bands
    npix = [0] * n_bands
    for j, c in dets:
        b = images[j].b - 1
        n = int(catalogs[j].npix[c])
        if n > npix[b]:
            best[b], npix[b] = (j, c), n
    gal_fluxes = np.array([float(catalogs[bc[0]].flux[bc[1]]) if bc is not None else 0.0 for bc in best])
    j, c = best[int(np.argmax(npix))]
    cat = catalogs[j]
    a, b = float(cat.a[c]), float(cat.b[c])
    return CatalogEntry(np.asarray(world_center, dtype=np.float64).copy(), False, gal_fluxes.copy(), gal_fluxes, 0.5,
                        b / a, float(cat.theta[c]) + x_vs_n[j], math.sqrt(a * b) * math.sqrt(2.0 * math.log(2.0)))


def detection_box(cat: Catalog, c: int, img: Image, world_center):
    """detection.jl:152-158: the 0-based bounds used as 1-based ranges (SEP.jl shifts x, y but not xmin .. ymax),
    dilated by 0.2 and enclosed with the 5-pixel box around the joined position."""
    box = ((int(cat.xmin[c]), int(cat.xmax[c])), (int(cat.ymin[c]), int(cat.ymax[c])))
    return enclose_boxes(dilate_box(box, 0.2), box_around_point(img, world_center, 5.0))


def build_detection_output(images, catalogs: Sequence[Catalog], match_radius: float):
    """detection.jl:61-171 given the per-image catalogs: (catalog entries, patches).  When any image has a TanWCS the join
    is angular and match_radius is in degrees (detection.jl:87 uses 1 / 3600); affine images keep the planar distance."""
    worlds = [world_coords(cat, img) for cat, img in zip(catalogs, images)]
    joined, detections = match_detections(worlds, match_radius, angular=any(img.wcs is not None for img in images))
    x_vs_n = [x_vs_n_angle(img.wcs_jacobian) for img in images]
    sparse = len(images) > 8
    catalog, patches = [], []
    for i in range(len(joined)):
        wc = joined[i]
        catalog.append(catalog_entry(wc, detections[i], catalogs, images, x_vs_n))
        boxes = {j: detection_box(catalogs[j], c, images[j], wc) for j, c in detections[i]}
        row = {}
        for j, img in enumerate(images):
            box = boxes[j] if j in boxes else box_around_point(img, wc, 5.0)
            if sparse:
                cb = clamp_box(box, (img.H, img.W))
                if cb[0][1] < cb[0][0] or cb[1][1] < cb[1][0]:
                    continue
            row[j] = ImagePatch.from_box(img, box)
        patches.append(PatchRow(images, row) if sparse else [row[j] for j in range(len(images))])
    return catalog, patches


def detect_sources(images, device: int = 0, match_radius: float = 1.0 / 3600.0, **extract_kw):
    """detect_sources (detection.jl:39-171): per-image SEP extraction on the device, duplicates merged across
    (overlapping) images, one CatalogEntry and one row of ImagePatches per joined object."""
    catalogs = extract(images, device=device, **extract_kw)
    return build_detection_output(images, catalogs, match_radius)


def detect_table(images, device: int = 0, match_radius: float = 1.0 / 3600.0, prep_images=None, **extract_kw):
    """detect_sources with everything behind the extraction on the device too (prep.detected_table): (catalog, table) -- the
    catalog of detect_sources and, in place of its ImagePatch rows, their model.PatchTable with neighbour lists (and the
    stamps of eigen-PSF images), which cabi.problem_from_table takes.  prep_images: a prep.PrepImages over `images`."""
    from . import prep
    catalogs = extract(images, device=device, want_pixels=False, **extract_kw)
    return prep.detected_table(images, catalogs, match_radius, device=device, prep_images=prep_images)
