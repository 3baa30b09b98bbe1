"""Per-source goodness of fit on the device: does the model a parameter table describes resemble the pixels?

  reference                                                  here
  ---------------------------------------------------------  ------------------------------------------------
  bin/write_celeste_expectation.jl (look at the residuals)   FitContext.stats: per target and band chi-square, residual
  elbo_likelihood's pixel visits with active_sources = [s]       flux, purity, flux misfit, largest pixel deviation; the
      (elbo_objective.jl:437-469)                                expected electrons of every patch on request (stamps)

One pass over the target's pixel visits in HIP (csrc/fit/celeste_fit.hip, libceleste_fit.so): the pixels, the densities and
the neighbour rule of the ELBO.  include/celeste_fit.h states every expression.  fp64 only, one device; the context uploads
its own copy of the image planes, as the MCMC and blend contexts do.
"""
import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import _binding, cabi
from .cabi import P

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "fit", "libceleste_fit.so")
ABI_VERSION = 100          # CELESTE_FIT_ABI_VERSION of include/celeste_fit.h
BANDS = 5
NSTATS = 7
CHI2, RESID, OWN, SELF, WRES, WINFO, MAX_Z = range(NSTATS)
EXPORTED_SYMBOLS = ["celeste_fit_version", "celeste_fit_strerror", "celeste_fit_ctx_create", "celeste_fit_ctx_destroy",
                    "celeste_fit_stats", "celeste_fit_last_ms"]

_dp, _ip, _lp = cabi.c_double_p, cabi.c_int32_p, cabi.c_int64_p
_ptr = _binding.ptr
_check = _binding.checker("fit")


def _declare(lib):
    vp = C.c_void_p
    lib.celeste_fit_strerror.restype = C.c_char_p
    lib.celeste_fit_strerror.argtypes = [C.c_int]
    lib.celeste_fit_ctx_create.argtypes = [C.POINTER(cabi.ProblemT), C.c_int, C.POINTER(C.c_void_p)]
    lib.celeste_fit_ctx_destroy.argtypes = [vp]
    lib.celeste_fit_ctx_destroy.restype = None
    lib.celeste_fit_stats.argtypes = [vp, _dp, C.c_int32, _ip, _lp, _dp, _ip, _lp, _dp]
    lib.celeste_fit_last_ms.argtypes = [vp, C.POINTER(C.c_float)]


def load_library(path: Optional[str] = None) -> C.CDLL:
    """libceleste_fit.so; CELESTE_MI355X_FIT_LIB overrides its path (_binding.open_library)"""
    return _binding.open_library("fit", LIB_PATH, "CELESTE_MI355X_FIT_LIB", ABI_VERSION, "celeste_fit_version", _declare, path)


def _ratio(num, den):
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    out = np.full(np.broadcast(num, den).shape, np.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out


@dataclass
class FitStats:
    """The statistics of one or more targets (include/celeste_fit.h).  n_pix [..., 5] int64 and stats [..., 5, 7] per band
    (index = band - 1); status [...] int32 (0 = OK; otherwise the statistics are NaN).  stamps (when asked for): one
    (image, H2 x W2 array of expected electrons, NaN where the pixel is not visited) pair per patch of each target."""
    n_pix: np.ndarray
    stats: np.ndarray
    status: np.ndarray
    stamps: Optional[list] = None

    def __getitem__(self, k) -> "FitStats":
        """the statistics of the k-th target of the call (an index, a slice or a list of indices)"""
        if self.stamps is None:
            stamps = None
        elif isinstance(k, (int, np.integer, slice)):
            stamps = self.stamps[k]
        else:
            stamps = [self.stamps[int(i)] for i in k]
        return FitStats(self.n_pix[k], self.stats[k], self.status[k], stamps)

    def reduced_chi2(self):
        """(per band [..., 5], all bands together [...]): chi2 / n_pix, NaN where no pixel was visited"""
        chi2 = self.stats[..., CHI2]
        return _ratio(chi2, self.n_pix), _ratio(chi2.sum(axis=-1), self.n_pix.sum(axis=-1))

    def flux_z(self):
        """wres / sqrt(winfo) per band: the standardised flux misfit (negative: the model is too bright)"""
        return _ratio(self.stats[..., WRES], np.sqrt(self.stats[..., WINFO]))

    def flux_correction(self):
        """wres / winfo per band: the fractional flux correction of one Newton step on a scale factor of the source's light"""
        return _ratio(self.stats[..., WRES], self.stats[..., WINFO])

    def purity(self):
        """self / own per band: the share of the source's profile-weighted light that is its own (1: isolated)"""
        return _ratio(self.stats[..., SELF], self.stats[..., OWN])

    def max_z(self):
        """the largest |r| / sqrt(lam) over all bands"""
        return self.stats[..., MAX_Z].max(axis=-1)


def patch_shapes(problem: "cabi.Problem") -> List[list]:
    """per source, the (image, H2, W2) of its non-empty patches in image order: what sizes the stamps of a call"""
    arr = np.frombuffer(problem.c_patches, dtype=cabi.PATCH_DTYPE)
    S, N = problem.n_sources, problem.n_images
    out = [[] for _ in range(S)]
    if problem.sparse:
        src, img = problem.patch_source, problem.patch_image
    else:
        src, img = np.repeat(np.arange(S), N), np.tile(np.arange(N), S)
    for e in np.flatnonzero((arr["H2"][:len(src)] > 0) & (arr["W2"][:len(src)] > 0)):
        out[int(src[e])].append((int(img[e]), int(arr["H2"][e]), int(arr["W2"][e])))
    return out


class FitContext(_binding.Context):
    """The fit library's copy of a problem (celeste_fit_ctx_t), built from a marshalled celeste_problem_t."""
    _name, _load = "fit", staticmethod(load_library)

    def __init__(self, problem: "cabi.Problem", device: int = 0):
        super().__init__(problem, device)
        self._shapes = None

    def stats(self, vp, targets: Sequence[int], stamps: bool = False) -> FitStats:
        """celeste_fit_stats at the table vp [S, 44] for `targets` (repeats allowed).  A target whose parameters or expected
        electrons are not finite gets a non-zero status and NaN statistics; nothing is raised for it."""
        vp = np.ascontiguousarray(np.asarray(vp, dtype=np.float64).reshape(self.S, P))
        tg = np.ascontiguousarray(np.asarray(targets, dtype=np.int64).reshape(-1))
        if tg.size and (tg.min() < 0 or tg.max() >= self.S):
            raise ValueError("target out of range")
        tg = tg.astype(np.int32)
        T = tg.size
        n_pix = np.zeros((T, BANDS), dtype=np.int64)
        st = np.zeros((T, BANDS, NSTATS))
        status = np.zeros(T, dtype=np.int32)
        off = buf = None
        if stamps:
            if self._shapes is None:
                self._shapes = patch_shapes(self.problem)
            sizes = [h2 * w2 for t in tg for _, h2, w2 in self._shapes[int(t)]]
            off = np.zeros(len(sizes) + 1, dtype=np.int64)
            buf = np.zeros(max(int(sum(sizes)), 1))
        rc = self.lib.celeste_fit_stats(self.handle, _ptr(vp, _dp), T, _ptr(tg, _ip), _ptr(n_pix, _lp), _ptr(st, _dp),
                                        _ptr(status, _ip), _ptr(off, _lp), _ptr(buf, _dp))
        if rc not in (cabi.ERR_NONFINITE_INPUT, cabi.ERR_NONFINITE_RESULT):
            _check(self.lib, rc)
        out = None
        if stamps:
            assert np.array_equal(off, np.concatenate([[0], np.cumsum(sizes)])), "the library's stamp offsets differ from the patch table's"
            out, e = [], 0
            for t in tg:
                row = []
                for n, h2, w2 in self._shapes[int(t)]:
                    row.append((n, buf[off[e]:off[e + 1]].reshape(w2, h2).T.copy()))
                    e += 1
                out.append(row)
        return FitStats(n_pix, st, status, out)

    def last_ms(self):
        """device ms of the last stats call: (per-visit tables, pixel kernel, per-target sums)"""
        ms = (C.c_float * 3)()
        _check(self.lib, self.lib.celeste_fit_last_ms(self.handle, ms))
        return float(ms[0]), float(ms[1]), float(ms[2])
