"""Per-exposure astrometry on the device: did a source move between the exposures?

  the catalog reduces every exposure to one position         AstromContext.offsets: per target and image the maximum-likelihood
  (the variational parameters of a source)                       offset (rows, columns, in pixels of that image) and scale of the
                                                                 source's own light in that image, with its covariance, chi-square
                                                                 and a flag; per target the weighted mean offset and a linear
                                                                 motion over the exposures, in the units of the position

Three kernels in HIP (csrc/astrom/celeste_astrom.hip, libceleste_astrom.so): the neighbour rule of the ELBO once per pixel,
then every Fisher-scoring pass of an entry inside one kernel, which evaluates both densities with their gradients at the shifted
pixel, then the summaries.  include/celeste_astrom.h states every expression.  fp64 only, one device.
"""
import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _binding, cabi
from .cabi import P
from .phot import entry_counts

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "astrom", "libceleste_astrom.so")
ABI_VERSION = 100          # CELESTE_ASTROM_ABI_VERSION of include/celeste_astrom.h
NSUMMARY = 22
OK, NO_LIGHT, TOO_FAINT, OUT_OF_RANGE, STALLED, NOT_CONVERGED, BAD_MODEL = range(7)
FLAG_NAMES = ("OK", "NO_LIGHT", "TOO_FAINT", "OUT_OF_RANGE", "STALLED", "NOT_CONVERGED", "BAD_MODEL")
NO_EPOCHS, NO_MOTION = 1, 2
MEAN, MEAN_COV, CHI2_CONST, MOTION, MOTION_COV, CHI2_LIN, T_REF = 0, 2, 5, 6, 10, 20, 21
MAX_STEP_PX, LS_MIN_DEC, MAX_HALVINGS = 0.5, 1e-3, 8
EXPORTED_SYMBOLS = ["celeste_astrom_version", "celeste_astrom_strerror", "celeste_astrom_ctx_create", "celeste_astrom_ctx_destroy",
                    "celeste_astrom_offsets", "celeste_astrom_last_ms"]

_dp, _ip, _lp = cabi.c_double_p, cabi.c_int32_p, cabi.c_int64_p
_ptr = _binding.ptr
_check = _binding.checker("astrom")


class ParamsT(C.Structure):
    """celeste_astrom_params_t"""
    _fields_ = [("tol_sigma", C.c_double), ("max_sigma_px", C.c_double), ("max_shift_px", C.c_double), ("max_iters", C.c_int32),
                ("pad", C.c_int32)]


def _declare(lib):
    vp = C.c_void_p
    lib.celeste_astrom_strerror.restype = C.c_char_p
    lib.celeste_astrom_strerror.argtypes = [C.c_int]
    lib.celeste_astrom_ctx_create.argtypes = [C.POINTER(cabi.ProblemT), C.c_int, C.POINTER(C.c_void_p)]
    lib.celeste_astrom_ctx_destroy.argtypes = [vp]
    lib.celeste_astrom_ctx_destroy.restype = None
    lib.celeste_astrom_offsets.argtypes = [vp, _dp, C.c_int32, _ip, C.POINTER(ParamsT), _dp, _lp, _ip, _dp, _dp, _dp, _dp, _dp, _dp,
                                           _ip, _ip, _ip, _ip, _ip, _dp, _ip]
    lib.celeste_astrom_last_ms.argtypes = [vp, C.POINTER(C.c_float)]


def load_library(path: Optional[str] = None) -> C.CDLL:
    """libceleste_astrom.so; CELESTE_MI355X_ASTROM_LIB overrides its path (_binding.open_library)"""
    return _binding.open_library("astrom", LIB_PATH, "CELESTE_MI355X_ASTROM_LIB", ABI_VERSION, "celeste_astrom_version", _declare,
                                 path)


def full3(packed) -> np.ndarray:
    """[..., 6] packed (00, 01, 02, 11, 12, 22) -> [..., 3, 3] symmetric"""
    packed = np.asarray(packed)
    out = np.empty(packed.shape[:-1] + (3, 3))
    for q, (k, l) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        out[..., k, l] = out[..., l, k] = packed[..., q]
    return out


@dataclass
class Astrometry:
    """The offsets of one or more targets (include/celeste_astrom.h).  Per entry = (target, image with a non-empty patch), in
    (target, image) order: image, delta [E, 2] (rows, columns, pixels of the image), alpha, fisher [E, 6], cov [E, 6] (the
    packed 3 x 3 of (d1, d2, alpha)), chi2, loglik, n_pix, iters (passes), flag; jac [E, 2, 2] = d(pixel) / d(pos) of the entry's
    patch; offsets [T + 1]: the entries of the k-th target are offsets[k]:offsets[k + 1].  Per target: n_epochs [T],
    summary_flag [T], summary [T, 22], status [T] int32 (the fit library's rule)."""
    offsets: np.ndarray
    image: np.ndarray
    delta: np.ndarray
    alpha: np.ndarray
    fisher: np.ndarray
    cov: np.ndarray
    chi2: np.ndarray
    loglik: np.ndarray
    n_pix: np.ndarray
    iters: np.ndarray
    flag: np.ndarray
    jac: np.ndarray
    n_epochs: np.ndarray
    summary_flag: np.ndarray
    summary: np.ndarray
    status: np.ndarray

    _ENTRY = ("image", "delta", "alpha", "fisher", "cov", "chi2", "loglik", "n_pix", "iters", "flag", "jac")

    def __len__(self):
        return len(self.status)

    def __getitem__(self, k) -> "Astrometry":
        """the offsets of the k-th target of the call (an index, a slice or a list of indices); an index keeps the target axis
        (length 1)"""
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
        return Astrometry(offsets=off, n_epochs=self.n_epochs[ks], summary_flag=self.summary_flag[ks], summary=self.summary[ks],
                          status=self.status[ks], **ent)

    def entry_target(self) -> np.ndarray:
        """per entry, the index of its target in the call"""
        return np.repeat(np.arange(len(self.status)), np.diff(self.offsets))

    def pos_stderr_px(self) -> np.ndarray:
        """[E, 2]: the standard errors of delta, from cov"""
        return np.sqrt(self.cov[:, [0, 3]])

    def sky_offset(self):
        """(Delta [E, 2], its covariance [E, 2, 2]) per entry, in the units of the position: Delta = inv(J) delta, the covariance
        inv(J) cov_dd inv(J)' with alpha marginalised"""
        Ji = np.linalg.inv(self.jac) if len(self.jac) else np.zeros((0, 2, 2))
        D = np.einsum("eij,ej->ei", Ji, self.delta)
        cdd = full3(self.cov)[:, :2, :2]
        return D, np.einsum("eij,ejk,elk->eil", Ji, cdd, Ji)

    @property
    def mean(self):
        """[T, 2]: the weighted mean offset over the OK entries, in the units of the position"""
        return self.summary[:, MEAN:MEAN + 2]

    @property
    def mean_cov(self):
        s = self.summary
        return np.stack([np.stack([s[:, 2], s[:, 3]], -1), np.stack([s[:, 3], s[:, 4]], -1)], -2)

    @property
    def chi2_const(self):
        """[T]: the exposures about their mean offset; 2 (n_epochs - 1) degrees of freedom for a source at rest"""
        return self.summary[:, CHI2_CONST]

    @property
    def motion(self):
        """[T, 2]: mu, units of the position per unit of the epochs (NaN where summary_flag has NO_MOTION)"""
        return self.summary[:, MOTION + 2:MOTION + 4]

    @property
    def offset_at_t_ref(self):
        return self.summary[:, MOTION:MOTION + 2]

    @property
    def motion_cov(self):
        """[T, 4, 4]: the covariance of (Delta_0, mu)"""
        T = len(self.status)
        out = np.empty((T, 4, 4))
        q = MOTION_COV
        for k in range(4):
            for l in range(k, 4):
                out[:, k, l] = out[:, l, k] = self.summary[:, q]
                q += 1
        return out

    @property
    def chi2_lin(self):
        """[T]: the exposures about the linear motion; 2 n_epochs - 4 degrees of freedom"""
        return self.summary[:, CHI2_LIN]

    @property
    def t_ref(self):
        return self.summary[:, T_REF]


class AstromContext(_binding.Context):
    """The astrometry library's copy of a problem (celeste_astrom_ctx_t), built from a marshalled celeste_problem_t."""
    _name, _load = "astrom", staticmethod(load_library)

    def __init__(self, problem: "cabi.Problem", device: int = 0):
        super().__init__(problem, device)
        self._counts = None
        self._jac = None

    def _jacobians(self):
        """per source, the Jacobians [n_entries_of_source, 2, 2] of its non-empty patches in image order"""
        if self._jac is None:
            pr = self.problem
            arr = np.frombuffer(pr.c_patches, dtype=cabi.PATCH_DTYPE)
            S, N = pr.n_sources, pr.n_images
            src = np.asarray(pr.patch_source) if pr.sparse else np.repeat(np.arange(S), N)
            arr = arr[:len(src)]
            ok = (arr["H2"] > 0) & (arr["W2"] > 0)
            J = np.asarray(arr["wcs_jacobian"], dtype=np.float64).reshape(-1, 2, 2).transpose(0, 2, 1)      # column-major in the table
            self._jac = [J[ok & (src == s)] for s in range(S)]
        return self._jac

    def offsets(self, vp, targets: Sequence[int], epochs=None, tol_sigma: float = 1e-6, max_iters: int = 50,
                max_sigma_px: float = 0.2, max_shift_px: float = 2.0) -> Astrometry:
        """celeste_astrom_offsets at the table vp [S, 44] for `targets` (repeats allowed).  epochs: one time per image (None: the
        image index).  A target whose parameters or model electrons are not sound gets a non-zero status and BAD_MODEL entries;
        nothing is raised for it."""
        vp = np.ascontiguousarray(np.asarray(vp, dtype=np.float64).reshape(self.S, P))
        tg = np.ascontiguousarray(np.asarray(targets, dtype=np.int64).reshape(-1))
        if tg.size and (tg.min() < 0 or tg.max() >= self.S):
            raise ValueError("target out of range")
        tg = tg.astype(np.int32)
        T = tg.size
        ep = None
        if epochs is not None:
            ep = np.ascontiguousarray(np.asarray(epochs, dtype=np.float64).reshape(-1))
            if ep.size != self.problem.n_images:
                raise ValueError("epochs needs one time per image")
        if self._counts is None:
            self._counts = entry_counts(self.problem)
        want = np.concatenate([[0], np.cumsum(self._counts[tg])]).astype(np.int64)
        E = int(want[-1])
        n = max(E, 1)
        off = np.zeros(T + 1, dtype=np.int64)
        image, n_pix, iters, flag = (np.zeros(n, dtype=np.int32) for _ in range(4))
        alpha, chi2, loglik = (np.zeros(n) for _ in range(3))
        delta, fisher, cov = np.zeros((n, 2)), np.zeros((n, 6)), np.zeros((n, 6))
        n_epochs, sflag, status = (np.zeros(T, dtype=np.int32) for _ in range(3))
        summary = np.zeros((T, NSUMMARY))
        pr = ParamsT(float(tol_sigma), float(max_sigma_px), float(max_shift_px), int(max_iters), 0)
        rc = self.lib.celeste_astrom_offsets(self.handle, _ptr(vp, _dp), T, _ptr(tg, _ip), C.byref(pr), _ptr(ep, _dp),
                                             _ptr(off, _lp), _ptr(image, _ip), _ptr(delta, _dp), _ptr(alpha, _dp),
                                             _ptr(fisher, _dp), _ptr(cov, _dp), _ptr(chi2, _dp), _ptr(loglik, _dp),
                                             _ptr(n_pix, _ip), _ptr(iters, _ip), _ptr(flag, _ip), _ptr(n_epochs, _ip),
                                             _ptr(sflag, _ip), _ptr(summary, _dp), _ptr(status, _ip))
        if rc not in (cabi.ERR_NONFINITE_INPUT, cabi.ERR_NONFINITE_RESULT):
            _check(self.lib, rc)
        assert np.array_equal(off, want), "the library's entry offsets differ from the patch table's"
        jacs = self._jacobians()
        jac = np.concatenate([jacs[t] for t in tg] + [np.zeros((0, 2, 2))])
        return Astrometry(off, image[:E], delta[:E], alpha[:E], fisher[:E], cov[:E], chi2[:E], loglik[:E], n_pix[:E], iters[:E],
                          flag[:E], jac, n_epochs, sflag, summary, status)

    def last_ms(self):
        """device ms of the last call: (per-visit tables, pixel pass, solve pass, summaries)"""
        ms = (C.c_float * 4)()
        _check(self.lib, self.lib.celeste_astrom_last_ms(self.handle, ms))
        return tuple(float(x) for x in ms)
