"""Position and shape standard errors on the device: how well do the pixels pin down where a source is and what shape it has?

  reference                                                  here
  ---------------------------------------------------------  ------------------------------------------------
  a catalog row carries variational errors of the fluxes      InfoContext.bounds: per target and type the Fisher
      and colours only; pos, gal_frac_dev, gal_axis_ratio,        information of (pos | pos, gal_frac_dev, gal_axis_ratio,
      gal_angle, gal_radius_px are point estimates                gal_angle, gal_radius_px) over the pixels the ELBO visits,
      (AccuracyBenchmark.jl:344-372)                              the band fluxes marginalised, and its Cramer-Rao covariance

One pass over the target's pixel visits in HIP (csrc/info/celeste_info.hip, libceleste_info.so): the pixels, the densities
and the neighbour rule of the ELBO, first derivatives only.  include/celeste_info.h states every expression.  fp64 only, one
device; the context uploads its own copy of the image planes, as the fit and phot contexts do.
"""
import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _binding, cabi
from .cabi import P

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "info", "libceleste_info.so")
ABI_VERSION = 100          # CELESTE_INFO_ABI_VERSION of include/celeste_info.h
BANDS = 5
G = (2, 6)                 # geometry parameters of a star, of a galaxy
NSUM = (6, 28)             # doubles of a (target, band) row of sums: upper triangle of A, c, d
NCOV = (3, 21)             # doubles of a packed covariance
PIVOT_MIN = 1e-8
NO_PIXELS, UNCONSTRAINED, NOT_POSITIVE, ILL_CONDITIONED = 1, 2, 4, 8
STAR, GALAXY = 0, 1
POS1, POS2, FRAC_DEV, AXIS_RATIO, ANGLE, RADIUS = range(6)      # the order of the galaxy's parameters (a star: the first two)
EXPORTED_SYMBOLS = ["celeste_info_version", "celeste_info_strerror", "celeste_info_ctx_create", "celeste_info_ctx_destroy",
                    "celeste_info_bounds", "celeste_info_solve", "celeste_info_last_ms"]

_dp, _ip, _lp = cabi.c_double_p, cabi.c_int32_p, cabi.c_int64_p
_ptr = _binding.ptr
_check = _binding.checker("info")


def _declare(lib):
    vp = C.c_void_p
    lib.celeste_info_strerror.restype = C.c_char_p
    lib.celeste_info_strerror.argtypes = [C.c_int]
    lib.celeste_info_ctx_create.argtypes = [C.POINTER(cabi.ProblemT), C.c_int, C.POINTER(C.c_void_p)]
    lib.celeste_info_ctx_destroy.argtypes = [vp]
    lib.celeste_info_ctx_destroy.restype = None
    lib.celeste_info_bounds.argtypes = [vp, _dp, C.c_int32, _ip, _lp, _dp, _dp, _dp, _dp, _ip, _ip]
    lib.celeste_info_solve.argtypes = [vp, C.c_int32, _dp, _dp, _dp, _dp, _ip]
    lib.celeste_info_last_ms.argtypes = [vp, C.POINTER(C.c_float)]


def load_library(path: Optional[str] = None) -> C.CDLL:
    """libceleste_info.so; CELESTE_MI355X_INFO_LIB overrides its path (_binding.open_library)"""
    return _binding.open_library("info", LIB_PATH, "CELESTE_MI355X_INFO_LIB", ABI_VERSION, "celeste_info_version", _declare, path)


def unpack(tri: np.ndarray, g: int) -> np.ndarray:
    """packed upper triangles [..., g (g + 1) / 2], row-major -> full symmetric matrices [..., g, g]"""
    tri = np.asarray(tri, dtype=np.float64)
    out = np.zeros(tri.shape[:-1] + (g, g))
    iu = np.triu_indices(g)
    out[..., iu[0], iu[1]] = tri
    out[..., iu[1], iu[0]] = tri
    return out


@dataclass
class InfoBounds:
    """The Fisher sums and Cramer-Rao covariances of one or more targets (include/celeste_info.h).  n_pix [..., 5] int64;
    sums_star [..., 5, 6] and sums_gal [..., 5, 28] per band (index = band - 1); cov_star [..., 3] and cov_gal [..., 21] the
    packed upper triangles; flag [..., 2] int32 (bit set per type: NO_PIXELS, UNCONSTRAINED, NOT_POSITIVE,
    ILL_CONDITIONED); status [...] int32 (0 = OK; otherwise sums and covariances are NaN)."""
    n_pix: np.ndarray
    sums_star: np.ndarray
    sums_gal: np.ndarray
    cov_star: np.ndarray
    cov_gal: np.ndarray
    flag: np.ndarray
    status: np.ndarray

    def __getitem__(self, k) -> "InfoBounds":
        """the numbers of the k-th target of the call (an index, a slice or a list of indices)"""
        return InfoBounds(self.n_pix[k], self.sums_star[k], self.sums_gal[k], self.cov_star[k], self.cov_gal[k], self.flag[k],
                          self.status[k])

    def cov(self, type: int) -> np.ndarray:
        """the full symmetric covariance [..., G, G] of a type's block (0 star: G = 2, 1 galaxy: G = 6)"""
        return unpack(self.cov_star if type == STAR else self.cov_gal, G[type])

    def pos_stderr(self, type: int) -> np.ndarray:
        """[..., 2]: the standard errors of (pos1, pos2) in the units of pos"""
        c = self.cov(type)
        with np.errstate(invalid="ignore"):
            return np.sqrt(np.stack([c[..., 0, 0], c[..., 1, 1]], axis=-1))

    def pos_corr(self, type: int) -> np.ndarray:
        """[...]: the correlation of pos1 and pos2 (NaN where a variance is not finite and positive)"""
        c = self.cov(type)
        den = c[..., 0, 0] * c[..., 1, 1]
        out = np.full(den.shape, np.nan)
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(den) & (den > 0)
            np.divide(c[..., 0, 1], np.sqrt(np.where(ok, den, 1.0)), out=out, where=ok)
        return out

    def shape_stderr(self) -> np.ndarray:
        """[..., 4]: the standard errors of (gal_frac_dev, gal_axis_ratio, gal_angle, gal_radius_px) in the galaxy block, in
        the units of the 44-vector"""
        c = self.cov(GALAXY)
        with np.errstate(invalid="ignore"):
            return np.sqrt(np.stack([c[..., k, k] for k in (FRAC_DEV, AXIS_RATIO, ANGLE, RADIUS)], axis=-1))

    def chosen(self, vp) -> np.ndarray:
        """[...]: the block the catalog row's type rule picks for each target from its row of vp [..., 44] (the rows of the
        call's targets, in their order): is_star > 0.5 -> 0 (star), else 1 (galaxy)"""
        from .params import ids
        vp = np.asarray(vp, dtype=np.float64)
        return np.where(vp[..., ids.is_star[0]] > 0.5, STAR, GALAXY)


class InfoContext(_binding.Context):
    """The info library's copy of a problem (celeste_info_ctx_t), built from a marshalled celeste_problem_t."""
    _name, _load = "info", staticmethod(load_library)

    def bounds(self, vp, targets: Sequence[int]) -> InfoBounds:
        """celeste_info_bounds at the table vp [S, 44] for `targets` (repeats allowed).  A target whose parameters or expected
        electrons are not finite gets a non-zero status and NaNs; nothing is raised for it."""
        vp = np.ascontiguousarray(np.asarray(vp, dtype=np.float64).reshape(self.S, P))
        tg = np.ascontiguousarray(np.asarray(targets, dtype=np.int64).reshape(-1))
        if tg.size and (tg.min() < 0 or tg.max() >= self.S):
            raise ValueError("target out of range")
        tg = tg.astype(np.int32)
        T = tg.size
        out = InfoBounds(np.zeros((T, BANDS), dtype=np.int64), np.zeros((T, BANDS, NSUM[0])), np.zeros((T, BANDS, NSUM[1])),
                         np.zeros((T, NCOV[0])), np.zeros((T, NCOV[1])), np.zeros((T, 2), dtype=np.int32),
                         np.zeros(T, dtype=np.int32))
        rc = self.lib.celeste_info_bounds(self.handle, _ptr(vp, _dp), T, _ptr(tg, _ip), _ptr(out.n_pix, _lp),
                                          _ptr(out.sums_star, _dp), _ptr(out.sums_gal, _dp), _ptr(out.cov_star, _dp),
                                          _ptr(out.cov_gal, _dp), _ptr(out.flag, _ip), _ptr(out.status, _ip))
        if rc not in (cabi.ERR_NONFINITE_INPUT, cabi.ERR_NONFINITE_RESULT):
            _check(self.lib, rc)
        return out

    def solve(self, sums_star, sums_gal):
        """celeste_info_solve: the covariance step alone on sums_star [n, 5, 6] and sums_gal [n, 5, 28] ->
        (cov_star [n, 3], cov_gal [n, 21], flag [n, 2])"""
        s0 = np.ascontiguousarray(np.asarray(sums_star, dtype=np.float64).reshape(-1, BANDS, NSUM[0]))
        s1 = np.ascontiguousarray(np.asarray(sums_gal, dtype=np.float64).reshape(-1, BANDS, NSUM[1]))
        if len(s0) != len(s1):
            raise ValueError("sums_star and sums_gal hold different numbers of rows")
        n = len(s0)
        c0, c1, fl = np.zeros((n, NCOV[0])), np.zeros((n, NCOV[1])), np.zeros((n, 2), dtype=np.int32)
        _check(self.lib, self.lib.celeste_info_solve(self.handle, n, _ptr(s0, _dp), _ptr(s1, _dp), _ptr(c0, _dp), _ptr(c1, _dp),
                                                     _ptr(fl, _ip)))
        return c0, c1, fl

    def last_ms(self):
        """device ms of the last bounds call: (per-visit tables, pixel kernel, per-target sums, solve)"""
        ms = (C.c_float * 4)()
        _check(self.lib, self.lib.celeste_info_last_ms(self.handle, ms))
        return tuple(float(x) for x in ms)
