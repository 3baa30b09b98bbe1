"""A numpy restatement of the Poisson sampler of libceleste_synth.so, written from the protocol text of
include/celeste_synth.h / DESIGN.md section 13 (not from the HIP source), vectorised over pixels.

Random numbers: Philox4x32-10, key = (seed low word, seed high word), counter = (pixel index, stream id, block number,
0x53594E54); a block gives two uniforms, u53(x0, x1) then u53(x2, x3).  lambda < 10: the multiplication method, one uniform
per factor; lambda >= 10: Hoermann's PTRS, one block (u, u') per trial.  A pixel that would need block 64 is NaN and capped.
Every fp64 operation below is a single rounded numpy operation in the order the protocol writes it.
"""
import math

import numpy as np

from mcmc_reference import philox4x32_10, u53   # the scalar forms, for the cross-check in test_synth_host.py

TAG = 0x53594E54
MAX_BLOCKS = 64
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox_blocks(c0, c1, c2, c3, seed):
    """Philox4x32-10 on arrays of counter words (uint64 arithmetic on 32-bit values); returns four uint64 arrays"""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(seed) & MASK, (int(seed) >> 32) & MASK
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)) & np.uint64(MASK), p1 & np.uint64(MASK),
             ((p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)) & np.uint64(MASK), p0 & np.uint64(MASK)]
    return c


def u53_array(a, b):
    return ((((a << np.uint64(32)) | b) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def _lgamma(x):
    return np.fromiter((math.lgamma(v) for v in x), dtype=np.float64, count=len(x))


def sample(lam, seed, stream=0, first_index=0, index=None, details=False):
    """Poisson pixels (float32) of the fp64 array lam (any shape; element i in column-major order is pixel index
    first_index + i unless `index` gives the indices).  details=True: also the number of uniforms every pixel consumed, the
    capped mask and, per pixel, the last trial's (k, lhs, rhs) of the PTRS log test (NaN where it was not reached)."""
    lam = np.asarray(lam, dtype=np.float64)
    flat = lam.reshape(-1, order="F")
    n = flat.size
    idx = (np.arange(n, dtype=np.uint64) + np.uint64(first_index)) if index is None else \
        np.asarray(index, dtype=np.uint64).reshape(-1, order="F")
    out = np.full(n, np.nan, dtype=np.float64)
    used = np.zeros(n, dtype=np.int64)
    capped = np.zeros(n, dtype=bool)
    trial = np.full((n, 3), np.nan)
    finite = np.isfinite(flat)
    out[finite & (flat <= 0.0)] = 0.0
    # ---- lambda < 10: L = exp(-lambda); p = 1; k = 0; loop { p *= u; if (p <= L) return k; ++k }
    act = np.flatnonzero(finite & (flat > 0.0) & (flat < 10.0))
    L = np.exp(-flat[act]); p = np.ones(act.size); k = np.zeros(act.size)
    for blk in range(MAX_BLOCKS):
        if act.size == 0:
            break
        r = philox_blocks(idx[act], stream, blk, TAG, seed)
        alive = np.ones(act.size, dtype=bool)        # still running inside this block
        for u in (u53_array(r[0], r[1]), u53_array(r[2], r[3])):
            p = np.where(alive, p * u, p)
            used[act[alive]] += 1
            done = alive & (p <= L)
            out[act[done]] = k[done]
            alive &= ~done
            k = np.where(alive, k + 1.0, k)
        act, L, p, k = act[alive], L[alive], p[alive], k[alive]
    capped[act] = True
    # ---- lambda >= 10: PTRS
    act = np.flatnonzero(finite & (flat >= 10.0))
    lm = flat[act]
    slam, loglam = np.sqrt(lm), np.log(lm)
    b = 0.931 + 2.53 * slam
    a = -0.059 + 0.02483 * b
    linv = np.log(1.1239 + 1.1328 / (b - 3.4))
    vr = 0.9277 - 3.6224 / (b - 2.0)
    for blk in range(MAX_BLOCKS):
        if act.size == 0:
            break
        r = philox_blocks(idx[act], stream, blk, TAG, seed)
        U = u53_array(r[0], r[1]) - 0.5
        V = u53_array(r[2], r[3])
        used[act] += 2
        us = 0.5 - np.abs(U)
        kk = np.floor((2.0 * a / us + b) * U + lm + 0.43)
        acc = (us >= 0.07) & (V <= vr)
        retry = ~acc & ((kk < 0.0) | ((us < 0.013) & (V > us)))
        test = np.flatnonzero(~acc & ~retry)
        lhs = np.log(V[test]) + linv[test] - np.log(a[test] / (us[test] * us[test]) + b[test])
        rhs = -lm[test] + kk[test] * loglam[test] - _lgamma(kk[test] + 1.0)
        trial[act[test], 0], trial[act[test], 1], trial[act[test], 2] = kk[test], lhs, rhs
        acc[test] = lhs <= rhs
        out[act[acc]] = kk[acc]
        go = ~acc
        act, lm, loglam, b, a, linv, vr = act[go], lm[go], loglam[go], b[go], a[go], linv[go], vr[go]
    capped[act] = True
    pixels = out.astype(np.float32).reshape(lam.shape, order="F")
    if details:
        return pixels, used.reshape(lam.shape, order="F"), capped.reshape(lam.shape, order="F"), trial
    return pixels
