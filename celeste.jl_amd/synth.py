"""Synthetic survey images on the device: the reference's Synthetic.gen_images! (Synthetic.jl:15-58).

  reference / host function                                  here
  ---------------------------------------------------------  ------------------------------------------------
  Synthetic.gen_image! with expectation (render_expected_    expected_electrons  (celeste_synth_generate, fp64 planes)
      image of synthetic.py, times nelec_per_nmgy)
  Poisson sampling of the expected electrons                 sample_poisson      (celeste_synth_sample)
  Synthetic.gen_images!                                      gen_images          (celeste_synth_generate, Float32 pixels)

The geometry stays here: entry_table forms, for every (source, image) pair whose clamped radius-25 box is not empty, the
box, the source's pixel position m = J (pos - world_center) + pixel_center (as ImagePatch.from_box and
render_expected_image form it), the flux of the image's band, the shape parameters and a stamp index -- vectorised over
the catalog.  The stamps are the raw psfmap(pixel_center): one per image for a ConstantPSFMap, one per star entry for an
SDSSPSFMap; the library conditions and prefilters them.  Rendering and sampling run in HIP
(csrc/synth/celeste_synth.hip); include/celeste_synth.h and DESIGN.md section 13 state the sampler and its Philox
streams.  Parity with the host function is per function: numpy's random stream is not reproduced.
"""
import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np

from . import _binding, cabi
from .model import ConstantPSFMap, SDSSPSFMap

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "synth", "libceleste_synth.so")
ABI_VERSION = 100          # CELESTE_SYNTH_ABI_VERSION of include/celeste_synth.h
EXPORTED_SYMBOLS = ["celeste_synth_version", "celeste_synth_strerror", "celeste_synth_generate", "celeste_synth_sample",
                    "celeste_synth_last_ms"]
ERR_INVALID_ARG, ERR_NO_DEVICE = 1, 2
FLAG_EXPECTATION = 1
PHILOX_TAG = 0x53594E54    # CELESTE_SYNTH_PHILOX_TAG
MAX_BLOCKS = 64            # CELESTE_SYNTH_MAX_BLOCKS
BOX_RADIUS = 25            # Synthetic.jl:22


class SynthImageT(C.Structure):
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("psf_K", C.c_int32), ("stream", C.c_uint32),
                ("sky", C.POINTER(C.c_float)), ("nelec_per_nmgy", C.POINTER(C.c_float)), ("psf", C.POINTER(C.c_double)),
                ("lambda_out", C.POINTER(C.c_double)), ("pixels_out", C.POINTER(C.c_float))]


ENTRY_DTYPE = np.dtype([("image", "<i4"), ("source", "<i4"), ("h0", "<i4"), ("h1", "<i4"), ("w0", "<i4"), ("w1", "<i4"),
                        ("is_star", "<i4"), ("stamp", "<i4"), ("m", "<f8", (2,)), ("flux", "<f8"), ("gal_frac_dev", "<f8"),
                        ("gal_axis_ratio", "<f8"), ("gal_angle", "<f8"), ("gal_radius_px", "<f8")])   # celeste_synth_entry_t


class SynthError(RuntimeError):
    def __init__(self, status: int, text: str):
        super().__init__("libceleste_synth: %s (status %d)" % (text, status))
        self.status = status


def _declare(lib):
    lib.celeste_synth_strerror.restype = C.c_char_p
    lib.celeste_synth_strerror.argtypes = [C.c_int]
    lib.celeste_synth_generate.restype = C.c_int
    lib.celeste_synth_generate.argtypes = [C.c_int, C.c_int32, C.POINTER(SynthImageT), C.c_int64, C.c_void_p, C.c_int32,
                                           C.POINTER(C.c_double), C.c_uint64, C.c_uint32, C.c_int32, C.POINTER(C.c_int64)]
    lib.celeste_synth_sample.restype = C.c_int
    lib.celeste_synth_sample.argtypes = [C.c_int, C.c_int64, C.POINTER(C.c_double), C.c_uint64, C.c_uint32, C.c_uint32,
                                         C.POINTER(C.c_float), C.POINTER(C.c_int64)]
    lib.celeste_synth_last_ms.restype = C.c_int
    lib.celeste_synth_last_ms.argtypes = [C.POINTER(C.c_float)]


def load_library(path: Optional[str] = None) -> C.CDLL:
    """libceleste_synth.so; CELESTE_MI355X_SYNTH_LIB overrides its path (_binding.open_library)"""
    return _binding.open_library("synth", LIB_PATH, "CELESTE_MI355X_SYNTH_LIB", ABI_VERSION, "celeste_synth_version", _declare, path)


_check = _binding.checker("synth", SynthError)


def last_ms() -> List[float]:
    """device milliseconds of the last call: stamp prefilter, galaxy tables, pixel kernel(s)"""
    ms = (C.c_float * 3)()
    load_library().celeste_synth_last_ms(ms)
    return [float(x) for x in ms]


# ---- geometry -------------------------------------------------------------------------------------------------------
def _catalog_columns(catalog):
    S = len(catalog)
    pos = np.array([ce.pos for ce in catalog], dtype=np.float64).reshape(S, 2)
    is_star = np.array([bool(ce.is_star) for ce in catalog], dtype=bool)
    sflux = np.array([ce.star_fluxes for ce in catalog], dtype=np.float64).reshape(S, 5)
    gflux = np.array([ce.gal_fluxes for ce in catalog], dtype=np.float64).reshape(S, 5)
    shape = np.array([[ce.gal_frac_dev, ce.gal_axis_ratio, ce.gal_angle, ce.gal_radius_px] for ce in catalog],
                     dtype=np.float64).reshape(S, 4)
    return pos, is_star, sflux, gflux, shape


def _column_major(stamp) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(stamp, dtype=np.float64).T).reshape(-1)


def entry_table(images, catalog):
    """(entries, stamps): the celeste_synth_entry_t table, sorted by (image, source), and the raw stamps [n, 51 * 51]
    (column-major) its star entries index."""
    pos, is_star, sflux, gflux, shape = _catalog_columns(catalog)
    parts, stamps, n_stamps = [], [], 0
    for n, img in enumerate(images):
        J = np.asarray(img.wcs_jacobian, dtype=np.float64).reshape(2, 2)
        w0, p0 = np.asarray(img.wcs_world0, dtype=np.float64), np.asarray(img.wcs_pix0, dtype=np.float64)
        d0, d1 = pos[:, 0] - w0[0], pos[:, 1] - w0[1]
        pc0 = J[0, 0] * d0 + J[0, 1] * d1 + p0[0]            # box_around_point: img.world_to_pix(pos)
        pc1 = J[1, 0] * d0 + J[1, 1] * d1 + p0[1]
        if img.wcs is not None:
            pc = img.world_to_pix(pos)
            pc0, pc1 = pc[:, 0], pc[:, 1]
        with np.errstate(invalid="ignore"):
            far = ~((np.abs(pc0) < 2.0 ** 30) & (np.abs(pc1) < 2.0 ** 30))   # (and NaN): no box anywhere near the image
        pc0, pc1 = np.where(far, -1e9, pc0), np.where(far, -1e9, pc1)
        # julia_round (ties to even) of pc -/+ 25, then clamp_box
        h0 = np.clip(np.rint(pc0 - BOX_RADIUS).astype(np.int64), 1, img.H + 1)
        h1 = np.clip(np.rint(pc0 + BOX_RADIUS).astype(np.int64), 0, img.H)
        v0 = np.clip(np.rint(pc1 - BOX_RADIUS).astype(np.int64), 1, img.W + 1)
        v1 = np.clip(np.rint(pc1 + BOX_RADIUS).astype(np.int64), 0, img.W)
        keep = np.flatnonzero((h1 >= h0) & (v1 >= v0))
        if keep.size == 0:
            continue
        h0, h1, v0, v1 = h0[keep], h1[keep], v0[keep], v1[keep]
        # ImagePatch.from_box: pixel_center, world_center = pix_to_world(pixel_center); m = J (pos - world_center) + pixel_center
        cen = np.stack([(h0 + h1) / 2, (v0 + v1) / 2], axis=1)
        wc = np.linalg.solve(J, (cen - p0).T).T + w0
        J00, J01, J10, J11 = J[0, 0], J[0, 1], J[1, 0], J[1, 1]
        if img.wcs is not None:     # the patch's own centre and Jacobian
            wc = img.pix_to_world(cen)
            Jp = img.jacobian_at(cen)
            J00, J01, J10, J11 = Jp[:, 0, 0], Jp[:, 0, 1], Jp[:, 1, 0], Jp[:, 1, 1]
        e0, e1 = pos[keep, 0] - wc[:, 0], pos[keep, 1] - wc[:, 1]
        ent = np.zeros(keep.size, dtype=ENTRY_DTYPE)
        ent["image"], ent["source"] = n, keep
        ent["h0"], ent["h1"], ent["w0"], ent["w1"] = h0, h1, v0, v1
        ent["m"][:, 0] = J00 * e0 + J01 * e1 + cen[:, 0]
        ent["m"][:, 1] = J10 * e0 + J11 * e1 + cen[:, 1]
        star = is_star[keep]
        ent["is_star"] = star
        ent["flux"] = np.where(star, sflux[keep, img.b - 1], gflux[keep, img.b - 1])
        for k, name in enumerate(("gal_frac_dev", "gal_axis_ratio", "gal_angle", "gal_radius_px")):
            ent[name] = shape[keep, k]
        ent["stamp"] = -1
        ks = np.flatnonzero(star)
        if ks.size:
            if isinstance(img.psfmap, ConstantPSFMap):
                ent["stamp"][ks] = n_stamps
                stamps.append(_column_major(img.psfmap.stamp)[None, :])
                n_stamps += 1
            else:
                if isinstance(img.psfmap, SDSSPSFMap):
                    # SDSSPSFMap.__call__ for all the centres at once: the weights, then rrows @ w (column-major stamps)
                    RCS, cm = 0.001, img.psfmap.cmat
                    px = (RCS * (cen[ks, 0] - 1.0))[:, None] ** np.arange(cm.shape[0])[None, :]
                    py = (RCS * (cen[ks, 1] - 1.0))[:, None] ** np.arange(cm.shape[1])[None, :]
                    st = np.einsum("ijk,ei,ej->ek", cm, px, py) @ img.psfmap.rrows.T
                else:
                    st = np.stack([_column_major(img.psfmap(c[0], c[1])) for c in cen[ks]])
                ent["stamp"][ks] = n_stamps + np.arange(ks.size)
                stamps.append(np.ascontiguousarray(st, dtype=np.float64))
                n_stamps += ks.size
        parts.append(ent)
    entries = np.concatenate(parts) if parts else np.zeros(0, dtype=ENTRY_DTYPE)
    stamp_arr = np.concatenate(stamps) if stamps else np.zeros((0, 51 * 51))
    return entries, np.ascontiguousarray(stamp_arr)


# ---- calls ----------------------------------------------------------------------------------------------------------
def generate_raw(images, entries: np.ndarray, stamps: np.ndarray, seed: int = 0, want_lambda: bool = False,
                 want_pixels: bool = True, expectation: bool = False, device: int = 0, streams: Optional[Sequence[int]] = None,
                 chunk_tiles: int = 0, lib=None):
    """celeste_synth_generate on a ready entry table.  Returns (lambda planes or None, pixel planes or None, n_capped);
    planes are H x W arrays (Fortran order: the library's column-major layout)."""
    lib = lib or load_library()
    N = len(images)
    arr = (SynthImageT * max(N, 1))()
    keep = []
    lams = [np.zeros((im.H, im.W), dtype=np.float64, order="F") for im in images] if want_lambda else None
    pixs = [np.zeros((im.H, im.W), dtype=np.float32, order="F") for im in images] if want_pixels else None
    for n, im in enumerate(images):
        sky = np.asfortranarray(im.sky, dtype=np.float32)
        iota = np.ascontiguousarray(im.nelec_per_nmgy, dtype=np.float32)
        psf = np.ascontiguousarray(im.psf, dtype=np.float64)
        keep += [sky, iota, psf]
        a = arr[n]
        a.H, a.W, a.psf_K = im.H, im.W, psf.shape[0]
        a.stream = (n if streams is None else int(streams[n])) & 0xffffffff
        a.sky = sky.ctypes.data_as(C.POINTER(C.c_float))
        a.nelec_per_nmgy = iota.ctypes.data_as(C.POINTER(C.c_float))
        a.psf = psf.ctypes.data_as(C.POINTER(C.c_double))
        if want_lambda:
            a.lambda_out = lams[n].ctypes.data_as(C.POINTER(C.c_double))
        if want_pixels:
            a.pixels_out = pixs[n].ctypes.data_as(C.POINTER(C.c_float))
    entries = np.ascontiguousarray(entries, dtype=ENTRY_DTYPE)
    stamps = np.ascontiguousarray(stamps, dtype=np.float64).reshape(-1, 51 * 51)
    capped = C.c_int64(0)
    _check(lib, lib.celeste_synth_generate(int(device), N, arr, len(entries), entries.ctypes.data_as(C.c_void_p), len(stamps),
                                           stamps.ctypes.data_as(C.POINTER(C.c_double)), int(seed) & (2 ** 64 - 1),
                                           FLAG_EXPECTATION if expectation else 0, int(chunk_tiles), C.byref(capped)))
    return lams, pixs, int(capped.value)


def expected_electrons(images, catalog, device: int = 0) -> List[np.ndarray]:
    """render_expected_image(img, catalog) * nelec_per_nmgy[:, None] for every image: fp64 planes"""
    entries, stamps = entry_table(images, catalog)
    lams, _, _ = generate_raw(images, entries, stamps, want_lambda=True, want_pixels=False, device=device)
    return lams


def sample_poisson(lam, seed: int, stream: int = 0, first_index: int = 0, device: int = 0, return_capped: bool = False):
    """Poisson pixels (Float32) of an fp64 array: element i, in memory order of the column-major plane, is pixel index
    first_index + i of stream `stream`.  The result has lam's shape."""
    lam = np.asarray(lam, dtype=np.float64)
    flat = np.ascontiguousarray(lam.reshape(-1, order="F"))
    out = np.zeros(flat.size, dtype=np.float32)
    capped = C.c_int64(0)
    lib = load_library()
    _check(lib, lib.celeste_synth_sample(int(device), flat.size, flat.ctypes.data_as(C.POINTER(C.c_double)),
                                         int(seed) & (2 ** 64 - 1), int(stream) & 0xffffffff, int(first_index) & 0xffffffff,
                                         out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(capped)))
    out = out.reshape(lam.shape, order="F")
    return (out, int(capped.value)) if return_capped else out


def gen_images(images, catalog, seed: int, expectation: bool = False, device: int = 0, streams: Optional[Sequence[int]] = None,
               chunk_tiles: int = 0) -> int:
    """Synthetic.gen_images!: fills img.pixels (Float32, H x W) of every image; image n draws from stream streams[n]
    (default n) of the Philox seed.  Returns n_capped, the number of pixels that ran out of random blocks (NaN; 0 on
    finite images)."""
    entries, stamps = entry_table(images, catalog)
    _, pixs, capped = generate_raw(images, entries, stamps, seed=seed, expectation=expectation, device=device, streams=streams,
                                   chunk_tiles=chunk_tiles)
    for im, px in zip(images, pixs):
        im.pixels = np.ascontiguousarray(px)
    return capped
