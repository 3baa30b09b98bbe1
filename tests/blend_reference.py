"""Host restatement of the blends' joint optimiser (celeste_blend_maximize) -- TEST INFRASTRUCTURE.

Built from the CPU oracle's pieces: oracle.elbo_multi (the multi-active objective), oracle.propagate (each member's
diagonal free-space block: J_a' h_aa J_a plus the second-order transform term, as propagate_derivatives! with Sa = 1),
the to_bound! transform with its Jacobian (restated as test_constraint_roundtrip_and_jacobian does), the cross blocks
J_a' h_ab J_b, oracle.solve_tr at n = 41 Sa, and the accept / reject rules of the oracle's maximize! (Optim.jl's
NewtonTrustRegion: eta = 0.1, rho thresholds 0.25 / 0.75, x_tol / f_tol / g_tol)."""
import math

import numpy as np

from celeste_jl_amd import cabi

P, NF = 44, 41
SIMPLEX = ((26, 26, 2, 0.005), (28, 27, 8, 0.01 / 8), (36, 34, 8, 0.01 / 8))   # (bound0, free0, n, lo)


def boxes(centre, loc_width=1e-4, loc_scale=1.0):
    """elbo_constraints' box of the 26 box-constrained parameters (lo, hi, scale), positions around `centre`"""
    lo = np.array([centre[0] - loc_width, centre[1] - loc_width, 1e-2, 1e-2, -10.0, 0.10] + [-1.0] * 2 + [1e-4] * 2 +
                  [-10.0] * 8 + [1e-4] * 8)
    hi = np.array([centre[0] + loc_width, centre[1] + loc_width, 0.99, 0.99, 10.0, 70.0] + [10.0] * 2 + [0.10] * 2 +
                  [10.0] * 8 + [1.0] * 8)
    sc = np.ones(26)
    sc[:2] = loc_scale
    return lo, hi, sc


def enforce_to_free(vs, lo, hi, sc):
    """enforce! then to_free! (ConstraintTransforms.jl:225-253, 84-126): (enforced bound values, free x)"""
    vs = np.array(vs, dtype=np.float64)
    x = np.zeros(NF)
    for i in range(26):
        b = vs[i]
        if not (lo[i] < b < hi[i]):
            b = max(min(b, np.nextafter(hi[i], -np.inf)), np.nextafter(lo[i], np.inf))
        vs[i] = b
        x[i] = -math.log(1.0 / ((b - lo[i]) / (hi[i] - lo[i])) - 1.0) * sc[i]
    for b0, f0, n, l in SIMPLEX:
        s = 0.0
        for i in range(n):
            b = vs[b0 + i]
            if not (l < b < 1.0):
                b = max(min(b, np.nextafter(1.0, -np.inf)), np.nextafter(l, np.inf))
            vs[b0 + i] = b
            s += b
        if not (abs(s - 1.0) <= 1.4901161193847656e-08 * max(abs(s), 1.0)):
            r = (1 - n * l) / (s - n * l)
            for i in range(n):
                vs[b0 + i] = np.nextafter(l, np.inf) + r * (vs[b0 + i] - l)
        last = math.log((vs[b0 + n - 1] - l) / (1 - n * l))
        for i in range(n - 1):
            x[f0 + i] = math.log((vs[b0 + i] - l) / (1 - n * l)) - last
    return vs, x


def to_bound(x, lo, hi, sc):
    """to_bound! with its Jacobian J [44, 41] (d bound / d free)"""
    vs = np.zeros(P)
    J = np.zeros((P, NF))
    for i in range(26):
        s = 1.0 / (1.0 + math.exp(-x[i] / sc[i]))
        vs[i] = s * (hi[i] - lo[i]) + lo[i]
        J[i, i] = (hi[i] - lo[i]) * s * (1 - s) / sc[i]
    for b0, f0, n, l in SIMPLEX:
        z = x[f0:f0 + n - 1]
        m = z.max()
        e = np.exp(z - m)
        tot = math.exp(-m) + e.sum()
        p = np.append(e / tot, math.exp(-m) / tot)
        vs[b0:b0 + n] = (1 - n * l) * p + l
        for a in range(n):
            for j in range(n - 1):
                J[b0 + a, f0 + j] = (1 - n * l) * p[a] * ((a == j) - p[j])
    return vs, J


def free_derivs(oracle, xs, centres, d, h, loc_width=1e-4, loc_scale=1.0):
    """Free-space gradient and Hessian of the blend's ELBO (not negated) at the members' free points xs [Sa, 41]:
    d [Sa, 44] and h [44 Sa, 44 Sa] are the bound-space derivatives.  Diagonal blocks by oracle.propagate, cross blocks
    J_a' h_ab J_b."""
    sa = len(xs)
    n = NF * sa
    g = np.zeros(n)
    H = np.zeros((n, n))
    Js = []
    for a in range(sa):
        lo, hi, sc = boxes(centres[a], loc_width, loc_scale)
        Js.append(to_bound(xs[a], lo, hi, sc)[1])
        c44 = np.zeros(P)
        c44[:2] = centres[a]
        gf, Hf = oracle.propagate(xs[a], c44, d[a], h[P * a:P * (a + 1), P * a:P * (a + 1)], loc_width, loc_scale)
        g[NF * a:NF * (a + 1)] = gf
        H[NF * a:NF * (a + 1), NF * a:NF * (a + 1)] = Hf
    for a in range(sa):
        for b in range(a + 1, sa):
            X = Js[a].T @ h[P * a:P * (a + 1), P * b:P * (b + 1)] @ Js[b]
            H[NF * a:NF * (a + 1), NF * b:NF * (b + 1)] = X
            H[NF * b:NF * (b + 1), NF * a:NF * (a + 1)] = X.T
    return g, H


def maximize_blend(oracle, problem, vp, blend, max_iters=50, include_kl=True, loc_width=1e-4, loc_scale=1.0, xtol_abs=1e-7,
                   ftol_rel=1e-6, gtol=1e-8, initial_delta=1.0, delta_hat=1e9, vp_neighbors=None, pos_centers=None,
                   trace=None):
    """maximize! for one blend, every other source frozen at vp_neighbors (default vp).
    Returns (vp_new, iterations, f_evals, elbo, status); trace (a list) receives (iteration, f, x) of every accepted point."""
    S = problem.n_sources
    vp = np.array(vp, dtype=np.float64).reshape(S, P)
    table = np.array(vp if vp_neighbors is None else vp_neighbors, dtype=np.float64).reshape(S, P)
    sa = len(blend)
    flags = cabi.FLAG_GRAD | cabi.FLAG_HESS | (cabi.FLAG_KL if include_kl else 0)
    centres, bx, xs = [], [], []
    for k, s in enumerate(blend):
        c = vp[s, :2].copy() if pos_centers is None else np.asarray(pos_centers[k], dtype=np.float64)
        lo, hi, sc = boxes(c, loc_width, loc_scale)
        _, x = enforce_to_free(vp[s], lo, hi, sc)
        centres.append(c)
        bx.append((lo, hi, sc))
        xs.append(x)
    x = np.concatenate(xs)

    def evaluate(xf):
        for k, s in enumerate(blend):
            table[s] = to_bound(xf[NF * k:NF * (k + 1)], *bx[k])[0]
        v, d, h, _, st = oracle.elbo_multi(problem, table, blend, flags)
        if st != 0 or not np.isfinite(v):
            return st or cabi.ERR_NONFINITE_RESULT, None, None, None
        g, H = free_derivs(oracle, xf.reshape(sa, NF), centres, d, h, loc_width, loc_scale)
        return 0, -v, -g, -H

    st, f, g, H = evaluate(x)
    its, evals = 0, 1
    if st == 0 and trace is not None:
        trace.append((0, f, x.copy()))
    delta = initial_delta
    if st == 0 and not np.max(np.abs(g)) <= gtol:
        while its < max_iters:
            its += 1
            s, m, interior = oracle.solve_tr(g, H, delta)
            xt = x + s
            st, ft, gt, Ht = evaluate(xt)
            evals += 1
            if st != 0:
                break
            if abs(m) <= 2.220446049250313e-16:
                rho = 1.0
            elif m > 0:
                rho = 0.25 - 1.0
            else:
                rho = (f - ft) / (0 - m)
            if rho < 0.25:
                delta *= 0.25
            elif rho > 0.75 and not interior:
                delta = min(2 * delta, delta_hat)
            if rho > 0.1:
                dx, gmax, df = np.max(np.abs(xt - x)), np.max(np.abs(gt)), abs(ft - f)
                x, f, g, H = xt, ft, gt, Ht
                if trace is not None:
                    trace.append((its, f, x.copy()))
                if dx <= xtol_abs or df <= ftol_rel * abs(f) or gmax <= gtol:
                    break
    out = np.array(vp)
    if st == 0:
        for k, s in enumerate(blend):
            out[s] = to_bound(x[NF * k:NF * (k + 1)], *bx[k])[0]
    return out, its, evals, (-f if st == 0 else float("nan")), st
