"""Joint optimisation of blended sources on the device: maximize! with several active sources.

  reference                                                  here
  ---------------------------------------------------------  ------------------------------------------------
  maximize!(ea, vp, cfg) with Sa > 1                         BlendContext.maximize_blends (one blend per
      (ElboMaximize.jl:38-93, 228-242)                           ElboArgs; many blends per call)
  elbo(ea, vp) with Sa > 1 (elbo_objective.jl:400-492)       BlendContext.eval_blends

The evaluation, the chain rule to free space (cross blocks included) and the trust-region steps run in HIP
(csrc/blend/celeste_blend.hip, libceleste_blend.so).  A blend's free-space Hessian is the exact one; the reference's
propagate_derivatives! scrambles it for Sa > 1.
"""
import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

from . import _binding, cabi
from .cabi import FLAG_GRAD, FLAG_HESS, FLAG_KL, P

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "blend", "libceleste_blend.so")
ABI_VERSION = 100          # CELESTE_BLEND_ABI_VERSION of include/celeste_blend.h
SA_MAX = 4                 # CELESTE_BLEND_SA_MAX: members per blend
NF = 41                    # free parameters per member
EXPORTED_SYMBOLS = ["celeste_blend_version", "celeste_blend_strerror", "celeste_blend_ctx_create", "celeste_blend_ctx_destroy",
                    "celeste_blend_eval", "celeste_blend_maximize", "celeste_blend_tr_solve_batch", "celeste_blend_last_ms"]

_dp, _ip, _lp = cabi.c_double_p, cabi.c_int32_p, cabi.c_int64_p
_ptr = _binding.ptr
_check = _binding.checker("blend")


def _declare(lib):
    vp = C.c_void_p
    lib.celeste_blend_strerror.restype = C.c_char_p
    lib.celeste_blend_strerror.argtypes = [C.c_int]
    lib.celeste_blend_ctx_create.argtypes = [C.POINTER(cabi.ProblemT), C.c_int, C.POINTER(C.c_void_p)]
    lib.celeste_blend_ctx_destroy.argtypes = [vp]
    lib.celeste_blend_ctx_destroy.restype = None
    lib.celeste_blend_eval.argtypes = [vp, _dp, C.c_int32, _lp, _ip, C.c_uint32, _dp, _dp, _dp, _lp, _ip]
    lib.celeste_blend_maximize.argtypes = [vp, _dp, _dp, _dp, C.c_int32, _lp, _ip, C.POINTER(cabi.OptimConfigT), _ip, _ip, _dp,
                                           _ip]
    lib.celeste_blend_last_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.celeste_blend_tr_solve_batch.argtypes = [C.c_int, C.c_int32, _ip, _dp, _dp, _dp, C.c_int32, C.c_int32, _dp, _dp, _ip]


def load_library(path: Optional[str] = None) -> C.CDLL:
    """libceleste_blend.so; CELESTE_MI355X_BLEND_LIB overrides its path (_binding.open_library)"""
    return _binding.open_library("blend", LIB_PATH, "CELESTE_MI355X_BLEND_LIB", ABI_VERSION, "celeste_blend_version", _declare, path)


def blend_arrays(blends: Sequence[Sequence[int]]):
    """(offsets int64[B + 1], sources int32[sum Sa]) of a list of blends"""
    off = np.zeros(len(blends) + 1, dtype=np.int64)
    for b, bl in enumerate(blends):
        off[b + 1] = off[b] + len(bl)
    src = np.ascontiguousarray(np.concatenate([np.asarray(bl, dtype=np.int32).reshape(-1) for bl in blends])
                               if len(blends) else np.zeros(0, np.int32), dtype=np.int32)
    return off, src


def tr_solve_batch(Hs, gs, deltas, secular_iters: int = 0, device: int = 0):
    """celeste_blend_tr_solve_batch: the sub-problem min g'p + p'Hp/2, |p| <= delta, for matrices of any size up to 164.
    Returns (p list, m[n], interior[n])."""
    lib = load_library()
    n = len(Hs)
    dims = np.ascontiguousarray([np.asarray(g).size for g in gs], dtype=np.int32)
    H = np.ascontiguousarray(np.concatenate([np.asarray(h, dtype=np.float64).T.reshape(-1) for h in Hs]))
    g = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for x in gs]))
    dl = np.ascontiguousarray(deltas, dtype=np.float64)
    p = np.zeros(g.size)
    m = np.zeros(n)
    interior = np.zeros(n, dtype=np.int32)
    _check(lib, lib.celeste_blend_tr_solve_batch(int(device), n, _ptr(dims, _ip), _ptr(H, _dp), _ptr(g, _dp), _ptr(dl, _dp), 0,
                                                 int(secular_iters), _ptr(p, _dp), _ptr(m, _dp), _ptr(interior, _ip)))
    out, k = [], 0
    for d in dims:
        out.append(p[k:k + d].copy())
        k += d
    return out, m, interior


class BlendContext(_binding.Context):
    """The blend library's copy of a problem (celeste_blend_ctx_t), built from a marshalled celeste_problem_t."""
    _name, _load = "blend", staticmethod(load_library)

    def eval_blends(self, vp, blends: Sequence[Sequence[int]], flags: int = FLAG_GRAD | FLAG_HESS | FLAG_KL,
                    raise_on_error: bool = True):
        """elbo() with active_sources = each blend.  Returns (v[B], d list of [44, Sa], h list of [44 Sa, 44 Sa],
        counters[B, 2], status[B]); d / h entries are None when not requested.  Column a of d and block a of h belong to
        member a (SensitiveFloats.jl:29-31), as celeste_elbo_eval_multi lays them out."""
        vp = np.ascontiguousarray(np.asarray(vp, dtype=np.float64).reshape(self.S, P))
        off, src = blend_arrays(blends)
        B = len(blends)
        sa = np.diff(off).astype(np.int64)
        want_h = bool(flags & FLAG_HESS)
        want_d = want_h or bool(flags & FLAG_GRAD)
        v = np.zeros(B)
        d = np.zeros(int(sa.sum()) * P) if want_d else None
        h = np.zeros(int((sa * P * sa * P).sum())) if want_h else None
        cnt = np.zeros((B, 2), dtype=np.int64)
        status = np.zeros(B, dtype=np.int32)
        st = self.lib.celeste_blend_eval(self.handle, _ptr(vp, _dp), B, _ptr(off, _lp), _ptr(src, _ip), int(flags), _ptr(v, _dp),
                                         _ptr(d, _dp), _ptr(h, _dp), _ptr(cnt, _lp), _ptr(status, _ip))
        if st in (cabi.ERR_NONFINITE_INPUT, cabi.ERR_NONFINITE_RESULT):
            if raise_on_error:
                raise AssertionError(self.lib.celeste_blend_strerror(st).decode())
        else:
            _check(self.lib, st)
        ds, hs, kd, kh = [], [], 0, 0
        for b in range(B):
            n = int(sa[b])
            ds.append(d[kd:kd + n * P].reshape(n, P).T.copy() if want_d else None)
            hs.append(h[kh:kh + (n * P) ** 2].reshape(n * P, n * P).T.copy() if want_h else None)
            kd += n * P
            kh += (n * P) ** 2
        return v, ds, hs, cnt, status

    def maximize_blends(self, vp, blends: Sequence[Sequence[int]], cfg=None, include_kl: bool = True, vp_neighbors=None,
                        pos_centers=None, raise_on_error: bool = True):
        """maximize! for every blend (one Newton trust-region over the 41 Sa free parameters of its members); every
        non-member frozen at `vp_neighbors` (default: vp).  pos_centers: [sum Sa, 2] centres of the members' position boxes
        in blend order (default: their current positions).  Returns (vp_new[S, 44], iterations[B], f_evals[B], elbo[B],
        status[B]); vp is not modified.  A blend whose ELBO turns non-finite keeps its input rows and gets a non-zero
        status; raise_on_error turns that into the reference's AssertionError."""
        from .elbo import ElboConfig
        cfg = cfg or ElboConfig()
        vp = np.ascontiguousarray(np.asarray(vp, dtype=np.float64).reshape(self.S, P)).copy()
        off, src = blend_arrays(blends)
        B = len(blends)
        its = np.zeros(B, dtype=np.int32)
        evals = np.zeros(B, dtype=np.int32)
        el = np.zeros(B)
        status = np.zeros(B, dtype=np.int32)
        nb = None if vp_neighbors is None else np.ascontiguousarray(np.asarray(vp_neighbors, dtype=np.float64).reshape(self.S, P))
        pc = None if pos_centers is None else np.ascontiguousarray(np.asarray(pos_centers, dtype=np.float64).reshape(src.size, 2))
        ccfg = cfg.to_c(include_kl)
        st = self.lib.celeste_blend_maximize(self.handle, _ptr(vp, _dp), _ptr(nb, _dp), _ptr(pc, _dp), B, _ptr(off, _lp),
                                             _ptr(src, _ip), C.byref(ccfg), _ptr(its, _ip), _ptr(evals, _ip), _ptr(el, _dp),
                                             _ptr(status, _ip))
        if st in (cabi.ERR_NONFINITE_INPUT, cabi.ERR_NONFINITE_RESULT):
            if raise_on_error:
                raise AssertionError(self.lib.celeste_blend_strerror(st).decode())
        else:
            _check(self.lib, st)
        return vp, its, evals, el, status

    def last_ms(self):
        """(evaluation ms, step ms, iterations) of the last maximize_blends call: device time summed over its iterations"""
        ms = (C.c_float * 3)()
        _check(self.lib, self.lib.celeste_blend_last_ms(self.handle, ms))
        return float(ms[0]), float(ms[1]), int(ms[2])
