// density_grad.h -- the two densities with their first derivatives, shared by the info and astrom libraries.
//
// Included after engine_context.h (bspline_w, exp_nonpos, Comp, CEL_COEF).  Everything is __device__ __forceinline__: what a
// caller does not use of a result is dropped by the compiler, and no library's export map knows of these functions.
#pragma once

// star_light_density! with its gradient with respect to the spline's index (fsm_util.jl:221-237): star_value's cell, weights
// and order of summation; softpluslikeinv branches exactly at 0, its y < 0 branch by the table-driven exponential
__device__ __forceinline__ void info_star_grad(const double *__restrict__ coef, double xh, double xw, const double *etab,
                                               double &f, double &fh, double &fw) {
    int ix = (int)floor(xh); ix = ix < 1 ? 1 : (ix > 50 ? 50 : ix);
    int iy = (int)floor(xw); iy = iy < 1 ? 1 : (iy > 50 ? 50 : iy);
    const double fx = xh - ix, fy = xw - iy;
    double wx[4], wy[4], dwx[4], dwy[4];
    bspline_w(fx, wx); bspline_w(fy, wy);
    {
        const double ox = 1.0 - fx, oy = 1.0 - fy;
        dwx[0] = -0.5 * ox * ox; dwx[1] = -2.0 * fx + 1.5 * fx * fx; dwx[2] = 2.0 * ox - 1.5 * ox * ox; dwx[3] = 0.5 * fx * fx;
        dwy[0] = -0.5 * oy * oy; dwy[1] = -2.0 * fy + 1.5 * fy * fy; dwy[2] = 2.0 * oy - 1.5 * oy * oy; dwy[3] = 0.5 * fy * fy;
    }
    const double *c0 = coef + (ix - 1) + CEL_COEF * (iy - 1);
    double y = 0, yh = 0, yw = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const double *cb = c0 + CEL_COEF * b;
        const double k0 = cb[0], k1 = cb[1], k2 = cb[2], k3 = cb[3];
        const double r = k0 * wx[0] + k1 * wx[1] + k2 * wx[2] + k3 * wx[3];
        const double rh = k0 * dwx[0] + k1 * dwx[1] + k2 * dwx[2] + k3 * dwx[3];
        y += r * wy[b]; yh += rh * wy[b]; yw += r * dwy[b];
    }
    double gp;
    if (y < 0) { f = 1e-3 * exp_nonpos(y, etab); gp = f; }
    else { f = 1e-3 * (y + 1.0); gp = 1e-3; }
    fh = gp * yh; fw = gp * yw;
}

// The galaxy density sum_c w0_c N_c, N_c = exp(-d' P_c d / 2), d = pixel - m_pos - xi_c, and its first derivatives: with
// u = P d,  d/dm_pos = sum w0 N u,  d/d gal_frac_dev = sum wd N,  and, the normalisation of w0 included, the closed form
// dN/dSigma = N (P d d' P - P) / 2 chained to XiXi by nuBar:  d/dXi11 = sum w0 nu N (u1^2 - p11) / 2,  d/dXi12 = sum w0 nu N
// (u1 u2 - p12) (both off-diagonal entries),  d/dXi22 = sum w0 nu N (u2^2 - p22) / 2.  Scalars only: nothing is indexed.
struct InfoGal { double v, m1, m2, dev, x11, x12, x22; };
__device__ __forceinline__ InfoGal info_galaxy_grad(const Comp *tc, int NC, double dx, double dy, const double *etab) {
    double v = 0, g1 = 0, g2 = 0, gd = 0, h11 = 0, h12 = 0, h22 = 0;
    const int n_dev = 8 * (NC / 14);
    for (int c0 = 0; c0 < NC; c0 += (c0 < n_dev ? 8 : 6)) {
        const int len = c0 < n_dev ? 8 : 6;
        const double d1 = dx - tc[c0].xi1, d2 = dy - tc[c0].xi2;
        for (int c = c0; c < c0 + len; ++c) {
            const Comp k = tc[c];
            const double u1 = __builtin_fma(k.p11, d1, k.p12 * d2), u2 = __builtin_fma(k.p12, d1, k.p22 * d2);
            const double e = exp_nonpos(-0.5 * __builtin_fma(d1, u1, d2 * u2), etab);
            const double t = k.w0 * e, tn = t * k.nu;
            v += t;
            g1 = __builtin_fma(t, u1, g1); g2 = __builtin_fma(t, u2, g2);
            gd = __builtin_fma(k.wd, e, gd);
            h11 = __builtin_fma(tn, __builtin_fma(u1, u1, -k.p11), h11);
            h12 = __builtin_fma(tn, __builtin_fma(u1, u2, -k.p12), h12);
            h22 = __builtin_fma(tn, __builtin_fma(u2, u2, -k.p22), h22);
        }
    }
    InfoGal o;
    o.v = v; o.m1 = g1; o.m2 = g2; o.dev = gd; o.x11 = 0.5 * h11; o.x12 = h12; o.x22 = 0.5 * h22;
    return o;
}
