"""Per-exposure forced photometry on the device: how bright was each source in each single image?

  the catalog reduces every exposure to one flux per band    PhotContext.light_curves: per target and image the maximum-
  (the variational parameters of a source)                       likelihood scale alpha of the source's own light in that image,
                                                                 its standard error, chi-square and a flag; per target and band
                                                                 the weighted mean over the exposures and the chi-square of
                                                                 the exposures about it (a variability statistic)

Two passes in HIP (csrc/phot/celeste_phot.hip, libceleste_phot.so): the densities and the neighbour rule of the ELBO once per
pixel, then every Newton iteration of an entry inside one kernel.  include/celeste_phot.h states every expression.  fp64 only,
one device; the x-axis of a light curve is the image index (the library knows no observation times).
"""
import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _binding, cabi
from .cabi import P

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "phot", "libceleste_phot.so")
ABI_VERSION = 100          # CELESTE_PHOT_ABI_VERSION of include/celeste_phot.h
BANDS = 5
NSUMMARY = 3
LDS_PIXELS = 6400          # CELESTE_PHOT_LDS_PIXELS
OK, NO_LIGHT, AT_BOUND, NOT_CONVERGED, BAD_MODEL = range(5)
WMEAN, WMEAN_SIGMA, CHI2_VAR = range(NSUMMARY)
EXPORTED_SYMBOLS = ["celeste_phot_version", "celeste_phot_strerror", "celeste_phot_ctx_create", "celeste_phot_ctx_destroy",
                    "celeste_phot_light_curves", "celeste_phot_last_ms"]

_dp, _ip, _lp = cabi.c_double_p, cabi.c_int32_p, cabi.c_int64_p
_ptr = _binding.ptr
_check = _binding.checker("phot")


class ParamsT(C.Structure):
    """celeste_phot_params_t"""
    _fields_ = [("tol_sigma", C.c_double), ("max_iters", C.c_int32), ("lds_max_pixels", C.c_int32)]


def _declare(lib):
    vp = C.c_void_p
    lib.celeste_phot_strerror.restype = C.c_char_p
    lib.celeste_phot_strerror.argtypes = [C.c_int]
    lib.celeste_phot_ctx_create.argtypes = [C.POINTER(cabi.ProblemT), C.c_int, C.POINTER(C.c_void_p)]
    lib.celeste_phot_ctx_destroy.argtypes = [vp]
    lib.celeste_phot_ctx_destroy.restype = None
    lib.celeste_phot_light_curves.argtypes = [vp, _dp, C.c_int32, _ip, C.POINTER(ParamsT), _lp, _ip, _dp, _dp, _dp, _ip, _ip, _ip,
                                              _ip, _dp, _ip]
    lib.celeste_phot_last_ms.argtypes = [vp, C.POINTER(C.c_float)]


def load_library(path: Optional[str] = None) -> C.CDLL:
    """libceleste_phot.so; CELESTE_MI355X_PHOT_LIB overrides its path (_binding.open_library)"""
    return _binding.open_library("phot", LIB_PATH, "CELESTE_MI355X_PHOT_LIB", ABI_VERSION, "celeste_phot_version", _declare, path)


def expected_band_flux(vp) -> np.ndarray:
    """[..., 5]: the flux in nanomaggies a parameter row expects in every band, sum_i a_i E[l_b | i] (what alpha scales)"""
    vp = np.asarray(vp, dtype=np.float64)
    out = np.zeros(vp.shape[:-1] + (BANDS,))
    for i in range(2):
        r, v = vp[..., 6 + i], vp[..., 8 + i]
        cm, cv = vp[..., 10 + 4 * i:14 + 4 * i], vp[..., 18 + 4 * i:22 + 4 * i]
        for b in range(BANDS):
            l = r + v / 2
            for k in range(2, b):                 # redder than r: + the colours from r up to the band
                l = l + cm[..., k] + cv[..., k] / 2
            for k in range(b, 2):                 # bluer than r: - the colours from the band up to r
                l = l - cm[..., k] + cv[..., k] / 2
            out[..., b] += vp[..., 26 + i] * np.exp(l)
    return out


@dataclass
class LightCurves:
    """The light curves of one or more targets (include/celeste_phot.h).  Per entry = (target, image with a non-empty patch), in
    (target, image) order: image, band (0-based), alpha, sigma, chi2, n_pix, iters, flag; offsets [T + 1]: the entries of the
    k-th target are offsets[k]:offsets[k + 1].  Per target and band: n_epochs [T, 5] and summary [T, 5, 3] = (wmean,
    wmean_sigma, chi2_var) over the band's OK entries; status [T] int32 (the fit library's rule); band_flux [T, 5]: the flux in
    nanomaggies the target's row expects in every band."""
    offsets: np.ndarray
    image: np.ndarray
    band: np.ndarray
    alpha: np.ndarray
    sigma: np.ndarray
    chi2: np.ndarray
    n_pix: np.ndarray
    iters: np.ndarray
    flag: np.ndarray
    n_epochs: np.ndarray
    summary: np.ndarray
    status: np.ndarray
    band_flux: np.ndarray

    _ENTRY = ("image", "band", "alpha", "sigma", "chi2", "n_pix", "iters", "flag")

    def __len__(self):
        return len(self.status)

    def __getitem__(self, k) -> "LightCurves":
        """the light curves of the k-th target of the call (an index, a slice or a list of indices); an index keeps the
        target axis (length 1)"""
        T = len(self.status)
        if isinstance(k, (int, np.integer)):
            ks = [range(T)[k]]
        elif isinstance(k, slice):
            ks = list(range(T)[k])
        else:
            ks = [range(T)[int(i)] for i in k]
        idx = np.concatenate([np.arange(self.offsets[i], self.offsets[i + 1]) for i in ks] + [np.zeros(0, dtype=np.int64)])
        idx = idx.astype(np.int64)
        off = np.concatenate([[0], np.cumsum([self.offsets[i + 1] - self.offsets[i] for i in ks])]).astype(np.int64)
        ent = {name: getattr(self, name)[idx] for name in self._ENTRY}
        return LightCurves(offsets=off, n_epochs=self.n_epochs[ks], summary=self.summary[ks], status=self.status[ks],
                           band_flux=self.band_flux[ks], **ent)

    def entry_target(self) -> np.ndarray:
        """per entry, the index of its target in the call"""
        return np.repeat(np.arange(len(self.status)), np.diff(self.offsets))

    def flux_nmgy(self) -> np.ndarray:
        """per entry: alpha times the flux the target's row expects in the entry's band, in nanomaggies"""
        return self.alpha * self.band_flux[self.entry_target(), self.band]

    def flux_nmgy_sigma(self) -> np.ndarray:
        """per entry: sigma in the same units"""
        return self.sigma * self.band_flux[self.entry_target(), self.band]

    @property
    def wmean(self):
        return self.summary[..., WMEAN]

    @property
    def wmean_sigma(self):
        return self.summary[..., WMEAN_SIGMA]

    @property
    def chi2_var(self):
        return self.summary[..., CHI2_VAR]

    def reduced_chi2_var(self) -> np.ndarray:
        """[T, 5]: chi2_var / (n_epochs - 1), NaN with fewer than two epochs"""
        dof = (self.n_epochs - 1).astype(np.float64)
        out = np.full(self.n_epochs.shape, np.nan)
        np.divide(self.chi2_var, dof, out=out, where=dof > 0)
        return out


def entry_counts(problem: "cabi.Problem") -> np.ndarray:
    """per source, the number of its non-empty patches: what sizes the entry arrays of a call"""
    arr = np.frombuffer(problem.c_patches, dtype=cabi.PATCH_DTYPE)
    S, N = problem.n_sources, problem.n_images
    if problem.sparse:
        src = np.asarray(problem.patch_source)
    else:
        src = np.repeat(np.arange(S), N)
    ok = (arr["H2"][:len(src)] > 0) & (arr["W2"][:len(src)] > 0)
    return np.bincount(np.asarray(src)[ok], minlength=S).astype(np.int64)


class PhotContext(_binding.Context):
    """The photometry library's copy of a problem (celeste_phot_ctx_t), built from a marshalled celeste_problem_t."""
    _name, _load = "phot", staticmethod(load_library)

    def __init__(self, problem: "cabi.Problem", device: int = 0):
        super().__init__(problem, device)
        self._counts = None
        self._bands = np.array([im.b - 1 for im in problem.images], dtype=np.int32)

    def light_curves(self, vp, targets: Sequence[int], tol_sigma: float = 1e-9, max_iters: int = 50,
                     lds_max_pixels: int = 0) -> LightCurves:
        """celeste_phot_light_curves at the table vp [S, 44] for `targets` (repeats allowed).  A target whose parameters or
        model electrons are not sound gets a non-zero status and BAD_MODEL entries; nothing is raised for it.
        lds_max_pixels > 0 lowers the size up to which a patch is solved from LDS (the results do not depend on it)."""
        vp = np.ascontiguousarray(np.asarray(vp, dtype=np.float64).reshape(self.S, P))
        tg = np.ascontiguousarray(np.asarray(targets, dtype=np.int64).reshape(-1))
        if tg.size and (tg.min() < 0 or tg.max() >= self.S):
            raise ValueError("target out of range")
        tg = tg.astype(np.int32)
        T = tg.size
        if self._counts is None:
            self._counts = entry_counts(self.problem)
        want = np.concatenate([[0], np.cumsum(self._counts[tg])]).astype(np.int64)
        E = int(want[-1])
        off = np.zeros(T + 1, dtype=np.int64)
        image, n_pix, iters, flag = (np.zeros(max(E, 1), dtype=np.int32) for _ in range(4))
        alpha, sigma, chi2 = (np.zeros(max(E, 1)) for _ in range(3))
        n_epochs = np.zeros((T, BANDS), dtype=np.int32)
        summary = np.zeros((T, BANDS, NSUMMARY))
        status = np.zeros(T, dtype=np.int32)
        pr = ParamsT(float(tol_sigma), int(max_iters), int(lds_max_pixels))
        rc = self.lib.celeste_phot_light_curves(self.handle, _ptr(vp, _dp), T, _ptr(tg, _ip), C.byref(pr), _ptr(off, _lp),
                                                _ptr(image, _ip), _ptr(alpha, _dp), _ptr(sigma, _dp), _ptr(chi2, _dp),
                                                _ptr(n_pix, _ip), _ptr(iters, _ip), _ptr(flag, _ip), _ptr(n_epochs, _ip),
                                                _ptr(summary, _dp), _ptr(status, _ip))
        if rc not in (cabi.ERR_NONFINITE_INPUT, cabi.ERR_NONFINITE_RESULT):
            _check(self.lib, rc)
        assert np.array_equal(off, want), "the library's entry offsets differ from the patch table's"
        image = image[:E]
        return LightCurves(off, image, self._bands[image], alpha[:E], sigma[:E], chi2[:E], n_pix[:E], iters[:E], flag[:E],
                           n_epochs, summary, status, expected_band_flux(vp[tg]))

    def last_ms(self):
        """device ms of the last call: (per-visit tables, pixel pass, solve pass, band summaries)"""
        ms = (C.c_float * 4)()
        _check(self.lib, self.lib.celeste_phot_last_ms(self.handle, ms))
        return tuple(float(x) for x in ms)
