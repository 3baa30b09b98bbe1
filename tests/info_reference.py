"""The Fisher sums and Cramer-Rao covariances of include/celeste_info.h, restated in numpy / torch (fp64) and mpmath -- test
infrastructure.

Written from the header's text, not from the kernel: whole-patch arrays, the densities of tests/torch_value_model.py
(star_density, galaxy_density, brightness) with their derivatives from torch.autograd (forward mode: one tangent per
geometry parameter), never from hand-written derivative code; the neighbours' light B, the visited masks and iota from the
helpers of tests/fit_reference.py.  For every sum it also returns sum |term|, which conditions a comparison of the sums.
solve() is the header's covariance step in mpmath at 50 digits with the same exclusion and flag rules, plus the 2-norm
condition number of the scaled matrix R from numpy.
"""
from dataclasses import dataclass

import mpmath as mp
import numpy as np
import torch

import fit_reference as FR
import torch_value_model as tvm
from celeste_jl_amd import cabi

DT = torch.float64
NB = 5
G = (2, 6)
NSUM = (6, 28)
NCOV = (3, 21)
PIVOT_MIN = 1e-8
NO_PIXELS, UNCONSTRAINED, NOT_POSITIVE, ILL_CONDITIONED = 1, 2, 4, 8


def tri(g):
    """(k, l) of the packed upper triangle of a g x g matrix, row-major"""
    return [(k, l) for k in range(g) for l in range(k, g)]


def density_fn(pas, coefs, i):
    """theta [G_i] (pos1, pos2 | pos1, pos2, gal_frac_dev, gal_axis_ratio, gal_angle, gal_radius_px) -> f_i on the grids of the
    patches `pas` of one source, stacked [P, Hm, Wm]: every patch's grid of 1-based image coordinates starts at its own corner
    and runs to the largest height and width of them all (a caller cuts out [:H2, :W2]); one pass serves all the patches.
    coefs: the spline coefficients of each patch's stamp."""
    P = len(pas)
    Hm = max(p.active_pixel_bitmap.shape[0] for p in pas)
    Wm = max(p.active_pixel_bitmap.shape[1] for p in pas)
    hh = torch.stack([torch.arange(p.bitmap_offset[0] + 1, p.bitmap_offset[0] + Hm + 1, dtype=DT)[:, None].expand(Hm, Wm) for p in pas])
    ww = torch.stack([torch.arange(p.bitmap_offset[1] + 1, p.bitmap_offset[1] + Wm + 1, dtype=DT)[None, :].expand(Hm, Wm) for p in pas])
    J = torch.tensor(np.stack([np.asarray(p.wcs_jacobian, dtype=np.float64) for p in pas]), dtype=DT)
    wc = torch.tensor(np.stack([np.asarray(p.world_center, dtype=np.float64) for p in pas]), dtype=DT)
    pc = torch.tensor(np.stack([np.asarray(p.pixel_center, dtype=np.float64) for p in pas]), dtype=DT)
    K = len(pas[0].psf)
    assert all(len(p.psf) == K for p in pas)
    psf = [tuple(torch.tensor(np.array([float(p.psf[k][c]) for p in pas]), dtype=DT)[:, None, None] for c in range(6)) for k in range(K)]

    def fn(th):
        d0, d1 = th[0] - wc[:, 0], th[1] - wc[:, 1]
        m0 = (J[:, 0, 0] * d0 + J[:, 0, 1] * d1 + pc[:, 0])[:, None, None]     # linear_world_to_pix, per patch
        m1 = (J[:, 1, 0] * d0 + J[:, 1, 1] * d1 + pc[:, 1])[:, None, None]
        if i == 0:
            return torch.stack([tvm.star_density(coefs[q], hh[q] - m0[q] + 26, ww[q] - m1[q] + 26) for q in range(P)])
        return tvm.galaxy_density(psf, (m0, m1), th[2], th[3], th[4], th[5], hh, ww)
    return fn


def value_and_jacobian(fn, theta):
    """fn(theta) [P, Hm, Wm] and d fn / d theta [G, P, Hm, Wm] by forward-mode autograd (all G tangents in one pass)"""
    jac, val = torch.func.jacfwd(lambda th: (lambda out: (out, out))(fn(th)), has_aux=True)(theta)
    return val.detach().numpy(), jac.detach().permute(3, 0, 1, 2).contiguous().numpy()


def pixel_terms(images, patches, neighbors, vp, s, expected=None):
    """per non-empty patch of source s: dict(n, band (0-based), visited [H2, W2], iota [H2, 1], and per type i the lists
    g, lam [H2, W2], D [G_i, H2, W2], a [H2, W2]) -- the header's per-pixel quantities (own light 0 in the last column)"""
    vp = np.asarray(vp, dtype=np.float64)
    vs = torch.tensor(vp[s], dtype=DT)
    finite = bool(np.isfinite(vp[s]).all())
    light = FR._Light(images, patches, vp)
    visits = list(expected if expected is not None else FR.expected_nmgy(images, patches, neighbors, vp, s))
    pas = [patches[s][n] for n, *_ in visits]
    dens = [None, None]
    if finite and pas:
        coefs = [light.coef(p.stamp) for p in pas]
        dens = [value_and_jacobian(density_fn(pas, coefs, i), vs[0:G[i]].clone()) for i in range(2)]
    out = []
    for q, (n, visited, E, m, B) in enumerate(visits):
        img, pa = images[n], pas[q]
        H2, W2 = visited.shape
        h0, w0 = pa.bitmap_offset
        iota = img.nelec_per_nmgy[h0:h0 + H2].astype(np.float64)[:, None]
        eps = img.sky[h0:h0 + H2, w0:w0 + W2].astype(np.float64)
        own = visited & (np.arange(1, W2 + 1)[None, :] < W2)
        b = img.b - 1
        rec = dict(n=n, band=b, visited=visited, iota=iota, g=[], lam=[], D=[], a=[])
        for i in range(2):
            if finite:
                El = float(tvm.brightness(vs, i, b)[0])
                f, df = dens[i][0][q, :H2, :W2], dens[i][1][:, q, :H2, :W2]
            else:
                El, f, df = np.nan, np.full((H2, W2), np.nan), np.full((G[i], H2, W2), np.nan)
            g = np.where(own, El * f, 0.0)
            rec["g"].append(g)
            rec["lam"].append(iota * ((eps + g) + B))
            rec["D"].append(np.where(own[None], iota[None] * El * df, 0.0))
            rec["a"].append(iota * g)
        out.append(rec)
    return out


@dataclass
class InfoReference:
    n_pix: np.ndarray       # [T, 5] int64
    sums: list              # [star [T, 5, 6], galaxy [T, 5, 28]]
    abs_sums: list          # the same shapes: sum |term| of every sum
    status: np.ndarray      # [T] int32
    cov: list               # [star [T, 3], galaxy [T, 21]] (mpmath, rounded to double)
    flag: np.ndarray        # [T, 2] int32
    kappa: np.ndarray       # [T, 2]: the 2-norm condition number of R over the parameters kept (NaN where there is no R)


def info_reference(images, patches, neighbors, vp, targets) -> InfoReference:
    vp = np.asarray(vp, dtype=np.float64)
    T = len(targets)
    n_pix = np.zeros((T, NB), dtype=np.int64)
    sums = [np.zeros((T, NB, NSUM[i])) for i in range(2)]
    abs_sums = [np.zeros((T, NB, NSUM[i])) for i in range(2)]
    status = np.zeros(T, dtype=np.int32)
    for ti, s in enumerate(targets):
        bad = False
        for rec in pixel_terms(images, patches, neighbors, vp, s):
            v, b = rec["visited"], rec["band"]
            n_pix[ti, b] += int(v.sum())
            for i in range(2):
                lam = rec["lam"][i][v]
                if lam.size and not (np.isfinite(lam).all() and (lam > 0).all()):
                    bad = True
                    continue
                vec = [rec["D"][i][k][v] for k in range(G[i])] + [rec["a"][i][v]]
                terms = [vec[k] * vec[l] / lam for k, l in tri(G[i])]
                terms += [vec[k] * vec[G[i]] / lam for k in range(G[i] + 1)]
                for q, t in enumerate(terms):
                    sums[i][ti, b, q] += t.sum()
                    abs_sums[i][ti, b, q] += np.abs(t).sum()
        if not np.isfinite(vp[s]).all():
            status[ti] = cabi.ERR_NONFINITE_INPUT
        elif bad:
            status[ti] = cabi.ERR_NONFINITE_RESULT
        if status[ti]:
            sums[0][ti] = np.nan
            sums[1][ti] = np.nan
    cov = [np.zeros((T, NCOV[i])) for i in range(2)]
    flag = np.zeros((T, 2), dtype=np.int32)
    kappa = np.full((T, 2), np.nan)
    for ti in range(T):
        for i in range(2):
            r = solve(sums[i][ti], G[i])
            cov[i][ti], flag[ti, i], kappa[ti, i] = r.cov, r.flag, r.kappa
    return InfoReference(n_pix, sums, abs_sums, status, cov, flag, kappa)


@dataclass
class Solved:
    cov: np.ndarray         # packed upper triangle of C, rounded to double
    flag: int
    kappa: float            # cond_2(R) over the parameters kept (numpy); NaN where there is no R
    s: list                 # mpmath: s_k = sqrt(S_kk) (1 for a dropped parameter); None where there is no R
    rinv: object            # mpmath matrix: inv(R) over all G parameters (a dropped one: unit row); None where there is no R
    rinv_max: float         # max |inv(R)| over the parameters kept


def solve(rows, g) -> Solved:
    """the header's covariance step on one block's five rows of sums [5, g (g + 1) / 2 + g + 1], in mpmath at 50 digits"""
    mp.mp.dps = 50
    rows = np.asarray(rows, dtype=np.float64)
    na = g * (g + 1) // 2
    nan_cov = np.full(na, np.nan)
    pairs = tri(g)
    d = [mp.mpf(float(rows[b, na + g])) for b in range(NB)]
    if not any(mp.isnan(x) or x != 0 for x in d):
        return Solved(nan_cov, NO_PIXELS, np.nan, None, None, np.nan)
    S = mp.zeros(g, g)
    for b in range(NB):
        for q, (k, l) in enumerate(pairs):
            S[k, l] += mp.mpf(float(rows[b, q]))
    for b in range(NB):
        if d[b] > 0:
            c = [mp.mpf(float(rows[b, na + k])) for k in range(g)]
            for k, l in pairs:
                S[k, l] -= c[k] * c[l] / d[b]
    if any(not mp.isfinite(S[k, l]) for k, l in pairs) or any(S[k, k] < 0 for k in range(g)):
        return Solved(nan_cov, NOT_POSITIVE, np.nan, None, None, np.nan)
    for k, l in pairs:
        S[l, k] = S[k, l]
    act = [S[k, k] > 0 for k in range(g)]
    fl = 0 if all(act) else UNCONSTRAINED
    s = [mp.sqrt(S[k, k]) if act[k] else mp.mpf(1) for k in range(g)]
    R = mp.eye(g)
    for k in range(g):
        for l in range(g):
            if k != l and act[k] and act[l]:
                R[k, l] = S[k, l] / (s[k] * s[l])
    keep = [k for k in range(g) if act[k]]
    kappa = float(np.linalg.cond(np.array([[float(R[k, l]) for l in keep] for k in keep]))) if keep else np.nan
    # Cholesky in index order, without pivoting
    L = mp.zeros(g, g)
    minpiv = mp.inf
    for j in range(g):
        piv = R[j, j] - sum(L[j, k] ** 2 for k in range(j))
        if act[j]:
            if not piv > 0:
                return Solved(nan_cov, fl | NOT_POSITIVE, kappa, None, None, np.nan)
            minpiv = min(minpiv, piv)
        L[j, j] = mp.sqrt(piv)
        for i in range(j + 1, g):
            L[i, j] = (R[i, j] - sum(L[i, k] * L[j, k] for k in range(j))) / L[j, j]
    if minpiv < mp.mpf(PIVOT_MIN):
        fl |= ILL_CONDITIONED
    Li = L ** -1
    Rinv = Li.T * Li
    cov = np.zeros(na)
    for q, (k, l) in enumerate(pairs):
        if act[k] and act[l]:
            cov[q] = float(Rinv[k, l] / (s[k] * s[l]))
        else:
            cov[q] = np.inf if k == l else 0.0
    rmax = max([abs(float(Rinv[k, l])) for k in keep for l in keep], default=np.nan)
    return Solved(cov, fl, kappa, s, Rinv, rmax)


def rows_of(A, c=None, d=1.0, band=0):
    """five rows of sums that hold the symmetric matrix A (with c and d) in one band and zeros in the others"""
    A = np.asarray(A, dtype=np.float64)
    g = len(A)
    rows = np.zeros((NB, g * (g + 1) // 2 + g + 1))
    rows[band] = [A[k, l] for k, l in tri(g)] + list(np.zeros(g) if c is None else c) + [d]
    return rows


def hand_made():
    """{name: (rows, expected flag, expected full covariance or None)}: the hand-made blocks of the host and device tests"""
    rng = np.random.Generator(np.random.PCG64(5))
    X = rng.normal(size=(12, 6))
    M = X.T @ X                                              # positive definite, well conditioned
    Z = M.copy()
    Z[4, :] = 0.0
    Z[:, 4] = 0.0                                            # an exact zero row: parameter 4 is unconstrained
    keep = [0, 1, 2, 3, 5]
    Cz = np.zeros((6, 6))
    Cz[np.ix_(keep, keep)] = np.linalg.inv(M[np.ix_(keep, keep)])
    Cz[4, 4] = np.inf
    r = 1.0 - 1e-9
    return {
        "diagonal": (rows_of(np.diag([1.0, 4.0, 9.0, 16.0, 25.0, 36.0])), 0, np.diag([1.0, 1 / 4, 1 / 9, 1 / 16, 1 / 25, 1 / 36])),
        "zero row": (rows_of(Z), UNCONSTRAINED, Cz),
        "negative diagonal": (rows_of([[1.0, 0.0], [0.0, -1.0]]), NOT_POSITIVE, None),
        "nearly singular": (rows_of([[1.0, r], [r, 1.0]]), ILL_CONDITIONED, np.linalg.inv(np.array([[1.0, r], [r, 1.0]]))),
        # S = A - c c' / d = [[2 - 0.5, 0.5 - 0.25], [., 1 - 0.125]]
        "schur": (rows_of([[2.0, 0.5], [0.5, 1.0]], c=[1.0, 0.5], d=2.0, band=3), 0,
                  np.linalg.inv(np.array([[1.5, 0.25], [0.25, 0.875]]))),
        "no pixels": (np.zeros((NB, 6)), NO_PIXELS, None),
    }


def full_information(recs, i=0):
    """the (G + 5) x (G + 5) Fisher information of (geometry, five band scales) of type i from pixel_terms' records"""
    g = G[i]
    out = np.zeros((g + NB, g + NB))
    for rec in recs:
        v, b = rec["visited"], rec["band"]
        lam = rec["lam"][i][v]
        D = [rec["D"][i][k][v] for k in range(g)]
        a = rec["a"][i][v]
        for k in range(g):
            for l in range(g):
                out[k, l] += (D[k] * D[l] / lam).sum()
            out[k, g + b] += (D[k] * a / lam).sum()
            out[g + b, k] = out[k, g + b]
        out[g + b, g + b] += (a * a / lam).sum()
    return out


def bounds_of(ref: InfoReference):
    """a celeste_jl_amd.info.InfoBounds over the restatement's arrays (for its helpers)"""
    from celeste_jl_amd import info
    return info.InfoBounds(ref.n_pix, ref.sums[0], ref.sums[1], ref.cov[0], ref.cov[1], ref.flag, ref.status)
