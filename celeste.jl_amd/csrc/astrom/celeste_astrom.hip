// celeste_astrom.hip -- libceleste_astrom.so: per-exposure astrometry (include/celeste_astrom.h).
//
// The engine's context code (engine_context.h) and its kernels' header are compiled into this library, unchanged, as into the fit, phot
// and info libraries; the context, the work list and the pixel walk (the neighbours' light B of every pixel) are
// engine_client.h's, the densities' gradients density_grad.h's (shared with the info library).  This file adds three kernels.
// One call:
//   prep_kernel           (the engine's) SrcImg and Comp of every visit of the context at the call's table
//   astrom_pixel_kernel   one wavefront per work item; the neighbours' light once per pixel; a lane writes b = iota (eps + B)
//                         (0 when the pixel is not visited), x, and e = iota where the own light counts (else 0) to the
//                         entry's planes in device memory (CSR by entry, 24 B per pixel); per tile the visited count and a
//                         bad bit
//   astrom_solve_kernel   one workgroup of four wavefronts per entry runs every pass of that entry: the entry's Comp records
//                         and the exponential's table are staged once; wavefront w takes tiles w, w + 4, ... (a tile = 64
//                         consecutive patch pixels), evaluates both densities with their gradients at the shifted pixel and
//                         sums the tile's 11 terms in a fixed butterfly; lane 0 leaves them in LDS, and after a barrier EVERY
//                         thread adds the tiles in ascending order -- all threads hold the same sums, so the iteration's
//                         control flow is uniform without a broadcast.  Tiles are taken in rounds of AST_PT, the rounds
//                         alternating between two buffers (one barrier per round); the planes are read from device memory on
//                         every pass
//   astrom_summary_kernel one lane per target: its OK entries added in image order; mean, linear motion, status
// No floating-point atomics; every rounded operation of the sums is spelled out (no contraction).
#include "../engine_context.h"
#include "../engine_client.h"
#include "../density_grad.h"
#include "../../../include/celeste_astrom.h"

// Mutation testing (tests/test_astrom_mutants.py builds this library with -DCELESTE_ASTROM_MUTANT=k and checks that a
// selection of tests/test_gpu_astrom.py notices).  A mutant changes arithmetic only; never an index, a bound, a size, a
// launch, a barrier or a loop count.  0 = the product;
//   1 = the star's index is shifted by +delta instead of -delta
//   2 = alpha is missing from D_0 and D_1
//   3 = W_n is formed with J' in place of J
//   4 = e = iota also in the patch's last column: the column is given light
//   5 = above ls_min_dec a trial is rejected when the likelihood ROSE
// Never defined in the shipped build.
#ifndef CELESTE_ASTROM_MUTANT
#define CELESTE_ASTROM_MUTANT 0
#endif

#define AST_THREADS 256
#define AST_WAVES (AST_THREADS / 64)
#define AST_PT 32                      // tiles of a round: 2 buffers x 32 tiles x (11 sums x 8 B + 4 B) = 5.75 KiB of LDS
#define AST_NS 11                      // l, U (3), F (6), chi2
#define AST_NSUM CELESTE_ASTROM_NSUMMARY

struct AstromEntry {
    int64_t px_off;                    // first pixel in the planes
    int32_t npx, tile0;                // pixels of the patch; first tile
    int32_t n, ti;                     // image; index of the target in the call
    int32_t sn, H2;                    // visit (table entry of the patch); rows of the patch
    int32_t off_h, off_w;              // the patch's corner in the image, 0-based
    double J[4];                       // d(m1, m2) / d(pos), column-major (the patch's)
};

struct AstromTileInfo { int32_t n_pix, bad; };   // visited pixels; b unsound at one of them

// ---- pixel pass ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
astrom_pixel_kernel(const VisitItem *__restrict__ items, const DevImage *__restrict__ images, const DevPatch *__restrict__ patches,
                    const double *__restrict__ coefs, const uint8_t *__restrict__ bitmaps, const SrcImg *__restrict__ srcimg,
                    const Comp *__restrict__ comps, const int64_t *__restrict__ nbr_off, const int32_t *__restrict__ nbr_idx,
                    const int32_t *__restrict__ vis_off, const int32_t *__restrict__ vis_img, const int32_t *__restrict__ vis_src,
                    int dense, int N, int NC, int chunk_px, double *__restrict__ sb, double *__restrict__ sx,
                    double *__restrict__ se, AstromTileInfo *__restrict__ info) {
    const VisitItem it = items[blockIdx.x];
    const int lane = threadIdx.x;
    visit_pixel_walk(it, images, patches, coefs, bitmaps, srcimg, comps, nbr_off, nbr_idx, vis_off, vis_img, vis_src, dense, N, NC,
                     chunk_px, [&](const DevImage &, const VisitPixel &px, const VisitOwn &ow) {
        const int tile = px.tile, idx = px.idx;
        const bool inp = px.inp, valid = px.valid;
#if CELESTE_ASTROM_MUTANT == 4
        const bool own = valid;
#else
        const bool own = ow.own;
#endif
        const float xf = px.xf, skyf = px.skyf;
        const double iota = px.iota, B = px.B;
        const double b = __dmul_rn(iota, (double)skyf + B);
        const bool bad = valid && !(isfinite(b) && b > 0.0);
        if (inp) {                                            // idx < npx: inside the entry's planes
            const int64_t o = it.px_off + idx;
            sb[o] = valid ? b : 0.0;
            sx[o] = valid ? (double)xf : 0.0;
            se[o] = own ? iota : 0.0;
        }
        const int n_valid = __popcll(__ballot(valid));
        const int any_bad = __any(bad);
        if (lane == 0) {
            AstromTileInfo ti;
            ti.n_pix = n_valid; ti.bad = any_bad;
            info[tile] = ti;
        }
    });
}

// ---- solve pass ------------------------------------------------------------------------------------------------------------
struct AstromSums {
    double s[AST_NS];                  // l, U0, U1, U2, F00, F01, F02, F11, F12, F22, chi2
    int unsound, light;                // a visited pixel without a finite lam > 0; a visited pixel with a > 0
};

// what the solve kernel keeps of an entry for its passes
struct AstromGeom {
    const double *pb, *px, *pe;
    const double *coef;
    double m1, m2, c0, c1;
    int npx, n_tiles, H2, off_h, off_w, NC;
    float rH2;
};

// One pass over the entry's pixels at theta = (d1, d2, alpha).  part, flg: the two round buffers; round: the running round
// count of the workgroup (selects the buffer).
__device__ __forceinline__ void astrom_pass(const AstromGeom &G, const Comp *tc, const double *etab, double d1, double d2,
                                            double alpha, double (*part)[AST_PT][AST_NS], int (*flg)[AST_PT], int &round,
                                            AstromSums &S) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < AST_NS; ++k) S.s[k] = 0.0;
    S.unsound = 0; S.light = 0;
    for (int t0 = 0; t0 < G.n_tiles; t0 += AST_PT, ++round) {
        double (*buf)[AST_NS] = part[round & 1];
        int *fb = flg[round & 1];
        const int nt = min(G.n_tiles - t0, AST_PT);
        for (int t = wave; t < nt; t += AST_WAVES) {
            const int p = (t0 + t) * 64 + lane;
            double b = 0.0, x = 0.0, e = 0.0;
            if (p < G.npx) { b = G.pb[p]; x = G.px[p]; e = G.pe[p]; }
            double u[AST_NS];
#pragma unroll
            for (int k = 0; k < AST_NS; ++k) u[k] = 0.0;
            bool bad = false, lit = false;
            if (b > 0.0) {                                    // a visited pixel
                double a = 0.0, g0 = 0.0, g1 = 0.0;
                if (e > 0.0) {                                // the own light counts
                    int w2, h2;
                    divmod_small(p, G.H2, G.rH2, w2, h2);
                    const double hh = (double)(G.off_h + h2 + 1), ww = (double)(G.off_w + w2 + 1);
                    const double dx = __dsub_rn(__dsub_rn(hh, G.m1), d1), dy = __dsub_rn(__dsub_rn(ww, G.m2), d2);
                    double f0, f0h, f0w;
#if CELESTE_ASTROM_MUTANT == 1
                    info_star_grad(G.coef, __dadd_rn(__dadd_rn(__dsub_rn(hh, G.m1), d1), 26.0),
                                   __dadd_rn(__dadd_rn(__dsub_rn(ww, G.m2), d2), 26.0), etab, f0, f0h, f0w);
#else
                    info_star_grad(G.coef, __dadd_rn(dx, 26.0), __dadd_rn(dy, 26.0), etab, f0, f0h, f0w);
#endif
                    const InfoGal g = info_galaxy_grad(tc, G.NC, dx, dy, etab);
                    // d/d delta: the spline's index falls with delta, the galaxy's d/d m_pos is d/d delta
                    const double m = __dadd_rn(__dmul_rn(G.c0, f0), __dmul_rn(G.c1, g.v));
                    const double mh = __dsub_rn(__dmul_rn(G.c1, g.m1), __dmul_rn(G.c0, f0h));
                    const double mw = __dsub_rn(__dmul_rn(G.c1, g.m2), __dmul_rn(G.c0, f0w));
                    a = __dmul_rn(e, m); g0 = __dmul_rn(e, mh); g1 = __dmul_rn(e, mw);
                }
                lit = a > 0.0;
                const double lam = __dadd_rn(b, __dmul_rn(alpha, a));
                if (isfinite(lam) && lam > 0.0) {
                    const double q = 1.0 / lam;
#if CELESTE_ASTROM_MUTANT == 2
                    const double D0 = g0, D1 = g1, D2 = a;
#else
                    const double D0 = __dmul_rn(alpha, g0), D1 = __dmul_rn(alpha, g1), D2 = a;
#endif
                    const double r = __dsub_rn(__dmul_rn(x, q), 1.0);
                    const double dl = __dsub_rn(x, lam);
                    u[0] = __dsub_rn(__dmul_rn(x, log_pos(lam)), lam);
                    u[1] = __dmul_rn(D0, r); u[2] = __dmul_rn(D1, r); u[3] = __dmul_rn(D2, r);
                    u[4] = __dmul_rn(__dmul_rn(D0, D0), q); u[5] = __dmul_rn(__dmul_rn(D0, D1), q);
                    u[6] = __dmul_rn(__dmul_rn(D0, D2), q); u[7] = __dmul_rn(__dmul_rn(D1, D1), q);
                    u[8] = __dmul_rn(__dmul_rn(D1, D2), q); u[9] = __dmul_rn(__dmul_rn(D2, D2), q);
                    u[10] = __dmul_rn(__dmul_rn(dl, dl), q);
                } else {
                    bad = true;
                }
            }
#pragma unroll
            for (int k = 0; k < AST_NS; ++k) u[k] = wave_sum(u[k]);
            const int fl = (__any(bad) ? 1 : 0) | (__any(lit) ? 2 : 0);
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < AST_NS; ++k) buf[t][k] = u[k];
                fb[t] = fl;
            }
        }
        __syncthreads();
        for (int t = 0; t < nt; ++t) {                        // every thread: the tiles in ascending order
#pragma unroll
            for (int k = 0; k < AST_NS; ++k) S.s[k] = __dadd_rn(S.s[k], buf[t][k]);
            const int fl = fb[t];
            S.unsound |= fl & 1; S.light |= fl >> 1;
        }
    }
}

// The step of a pass (the header): the unit-diagonal scaling of F, its Cholesky factor in index order, p = inv(F) U,
// dec = sqrt(U' inv(F) U) and inv(F).  ok: every pivot is finite and > 0.
struct AstromStep { double p[3], dec, cov[6]; bool ok; };
__device__ __forceinline__ void astrom_step(const double *s, AstromStep &o) {
    const double U0 = s[1], U1 = s[2], U2 = s[3];
    const double F00 = s[4], F01 = s[5], F02 = s[6], F11 = s[7], F12 = s[8], F22 = s[9];
    bool ok = F00 > 0.0 && F11 > 0.0 && F22 > 0.0 && isfinite(F00) && isfinite(F11) && isfinite(F22);
    const double s0 = sqrt(F00), s1 = sqrt(F11), s2 = sqrt(F22);
    const double L10 = F01 / (s0 * s1), L20 = F02 / (s0 * s2), r12 = F12 / (s1 * s2);
    const double piv1 = 1.0 - L10 * L10;
    ok = ok && piv1 > 0.0;
    const double L11 = sqrt(piv1);
    const double L21 = (r12 - L20 * L10) / L11;
    const double piv2 = 1.0 - L20 * L20 - L21 * L21;
    ok = ok && piv2 > 0.0 && isfinite(piv2);
    const double L22 = sqrt(piv2);
    const double z0 = U0 / s0, z1 = (U1 / s1 - L10 * z0) / L11, z2 = (U2 / s2 - L20 * z0 - L21 * z1) / L22;
    o.dec = sqrt(z0 * z0 + z1 * z1 + z2 * z2);
    const double y2 = z2 / L22, y1 = (z1 - L21 * y2) / L11, y0 = z0 - L10 * y1 - L20 * y2;
    o.p[0] = y0 / s0; o.p[1] = y1 / s1; o.p[2] = y2 / s2;
    const double A11 = 1.0 / L11, A22 = 1.0 / L22;                 // inv(L): unit first diagonal entry
    const double A10 = -L10 * A11, A21 = -L21 * A11 * A22, A20 = -(L20 + L21 * A10) * A22;
    o.cov[0] = (1.0 + A10 * A10 + A20 * A20) / (s0 * s0);
    o.cov[1] = (A10 * A11 + A20 * A21) / (s0 * s1);
    o.cov[2] = (A20 * A22) / (s0 * s2);
    o.cov[3] = (A11 * A11 + A21 * A21) / (s1 * s1);
    o.cov[4] = (A21 * A22) / (s1 * s2);
    o.cov[5] = (A22 * A22) / (s2 * s2);
    o.ok = ok;
}

__global__ void __launch_bounds__(AST_THREADS)
astrom_solve_kernel(const AstromEntry *__restrict__ entries, const AstromTileInfo *__restrict__ info,
                    const int32_t *__restrict__ targets, const double *__restrict__ vp, const DevPatch *__restrict__ patches,
                    const double *__restrict__ coefs, const SrcImg *__restrict__ srcimg, const Comp *__restrict__ comps, int NC,
                    const double *__restrict__ sb, const double *__restrict__ sx, const double *__restrict__ se,
                    double tol_sigma, double max_sigma_px, double max_shift_px, int max_iters, int32_t *__restrict__ o_image,
                    double *__restrict__ o_delta, double *__restrict__ o_alpha, double *__restrict__ o_fisher,
                    double *__restrict__ o_cov, double *__restrict__ o_chi2, double *__restrict__ o_loglik,
                    int32_t *__restrict__ o_npix, int32_t *__restrict__ o_iters, int32_t *__restrict__ o_flag) {
    __shared__ double etab[64];
    __shared__ Comp tc[14 * CEL_MAXK];
    __shared__ double part[2][AST_PT][AST_NS];
    __shared__ int flg[2][AST_PT];
    __shared__ int cnt[2];
    const int e = blockIdx.x;
    const AstromEntry E = entries[e];
    const int tid = threadIdx.x;
    const int npx = E.npx, n_tiles = (npx + 63) >> 6;
    if (tid < 2) cnt[tid] = 0;
    exp_table_init(etab);                                     // (a barrier)
    {
        const double *s = reinterpret_cast<const double *>(comps + (size_t)E.sn * NC);
        double *d = reinterpret_cast<double *>(tc);
        for (int i = tid; i < NC * 8; i += AST_THREADS) d[i] = s[i];
    }
    const double *vs = vp + (size_t)targets[E.ti] * CEL_P;
    const int nonfinite = __syncthreads_or(row_nonfinite(vs, tid));
    {
        int np = 0, bd = 0;
        for (int t = tid; t < n_tiles; t += AST_THREADS) { const AstromTileInfo ti = info[E.tile0 + t]; np += ti.n_pix; bd |= ti.bad; }
        if (np) atomicAdd(&cnt[0], np);                       // (integers: the order does not matter)
        if (bd) atomicOr(&cnt[1], 1);
    }
    __syncthreads();
    const int n_pix = cnt[0], bad = cnt[1];
    const double nan = (double)NAN;
    int flag = CELESTE_ASTROM_BAD_MODEL, iters = 0;
    double th0 = nan, th1 = nan, th2 = nan;
    AstromSums cur;
    AstromStep st;
#pragma unroll
    for (int k = 0; k < AST_NS; ++k) cur.s[k] = nan;
#pragma unroll
    for (int k = 0; k < 6; ++k) st.cov[k] = nan;
    if (!nonfinite && !bad) {
        AstromGeom G;
        const SrcImg si = srcimg[E.sn];
        G.pb = sb + E.px_off; G.px = sx + E.px_off; G.pe = se + E.px_off;
        G.coef = coefs + (size_t)patches[E.sn].stamp * (CEL_COEF * CEL_COEF);
        G.m1 = si.m1; G.m2 = si.m2; G.c0 = si.c0; G.c1 = si.c1;
        G.npx = npx; G.n_tiles = n_tiles; G.H2 = E.H2; G.off_h = E.off_h; G.off_w = E.off_w; G.NC = NC;
        G.rH2 = 1.0f / (float)E.H2;
        int round = 0;
        astrom_pass(G, tc, etab, 0.0, 0.0, 1.0, part, flg, round, cur);
        iters = 1;
        if (cur.unsound) {
#pragma unroll
            for (int k = 0; k < AST_NS; ++k) cur.s[k] = nan;
        } else if (!cur.light) {
            flag = CELESTE_ASTROM_NO_LIGHT;
#pragma unroll
            for (int k = 1; k < 10; ++k) cur.s[k] = nan;
        } else {
            astrom_step(cur.s, st);
            if (!st.ok) {
                flag = CELESTE_ASTROM_TOO_FAINT;
#pragma unroll
                for (int k = 0; k < 6; ++k) st.cov[k] = nan;
            } else if (sqrt(fmax(st.cov[0], st.cov[3])) > max_sigma_px) {
                flag = CELESTE_ASTROM_TOO_FAINT;
            } else {
                th0 = 0.0; th1 = 0.0; th2 = 1.0;
                while (true) {
                    if (st.dec <= tol_sigma) { flag = CELESTE_ASTROM_OK; break; }
                    if (iters >= max_iters) { flag = CELESTE_ASTROM_NOT_CONVERGED; break; }
                    const double big = fmax(fabs(st.p[0]), fabs(st.p[1]));
                    const double sc = big > CELESTE_ASTROM_MAX_STEP_PX ? CELESTE_ASTROM_MAX_STEP_PX / big : 1.0;
                    const double p0 = __dmul_rn(st.p[0], sc), p1 = __dmul_rn(st.p[1], sc), p2 = __dmul_rn(st.p[2], sc);
                    double t = 1.0, n0, n1, n2;
                    int halvings = 0, end = -1;
                    AstromSums trial;
                    while (true) {
                        n0 = __dadd_rn(th0, __dmul_rn(t, p0)); n1 = __dadd_rn(th1, __dmul_rn(t, p1)); n2 = __dadd_rn(th2, __dmul_rn(t, p2));
                        astrom_pass(G, tc, etab, n0, n1, n2, part, flg, round, trial);
                        ++iters;
#if CELESTE_ASTROM_MUTANT == 5
                        const bool fell = trial.s[0] > cur.s[0];
#else
                        const bool fell = trial.s[0] < cur.s[0];
#endif
                        const bool reject = trial.unsound || (st.dec > CELESTE_ASTROM_LS_MIN_DEC && fell);
                        if (!reject) break;
                        if (halvings == CELESTE_ASTROM_MAX_HALVINGS) { end = CELESTE_ASTROM_STALLED; break; }
                        if (iters >= max_iters) { end = CELESTE_ASTROM_NOT_CONVERGED; break; }
                        ++halvings;
                        t = __dmul_rn(t, 0.5);
                    }
                    if (end >= 0) { flag = end; break; }
                    th0 = n0; th1 = n1; th2 = n2;
                    cur = trial;
                    astrom_step(cur.s, st);
                    if (!st.ok) {
                        flag = CELESTE_ASTROM_STALLED;
#pragma unroll
                        for (int k = 0; k < 6; ++k) st.cov[k] = nan;
                        break;
                    }
                    if (fabs(th0) > max_shift_px || fabs(th1) > max_shift_px) { flag = CELESTE_ASTROM_OUT_OF_RANGE; break; }
                }
            }
        }
    }
    if (tid == 0) {
        o_image[e] = E.n;
        o_delta[2 * (size_t)e] = th0; o_delta[2 * (size_t)e + 1] = th1;
        o_alpha[e] = th2;
#pragma unroll
        for (int k = 0; k < 6; ++k) { o_fisher[6 * (size_t)e + k] = cur.s[4 + k]; o_cov[6 * (size_t)e + k] = st.cov[k]; }
        o_chi2[e] = cur.s[10];
        o_loglik[e] = cur.s[0];
        o_npix[e] = n_pix;
        o_iters[e] = iters;
        o_flag[e] = flag;
    }
}

// ---- target summaries ------------------------------------------------------------------------------------------------------
// Cholesky of the packed upper triangle A (row-major) of an N x N matrix in index order, in place of nothing: L (full), then
// inv(A) packed and x = inv(A) r.  false: a pivot is not finite and > 0.  Every index is a constant after unrolling.
template <int N>
__device__ __forceinline__ bool astrom_spd_solve(const double *A, const double *r, double *x, double *inv) {
    auto tri = [](int k, int l) { return k * N - (k * (k - 1)) / 2 + (l - k); };
    double L[N][N], Li[N][N];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double piv = A[tri(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) piv -= L[j][k] * L[j][k];
        ok = ok && piv > 0.0 && isfinite(piv);
        L[j][j] = sqrt(piv);
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double v = A[tri(j, i)];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
        Li[j][j] = 1.0 / L[j][j];
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double v = 0.0;
#pragma unroll
            for (int k = j; k < i; ++k) v -= L[i][k] * Li[k][j];
            Li[i][j] = v / L[i][i];
        }
    }
#pragma unroll
    for (int k = 0; k < N; ++k)
#pragma unroll
        for (int l = k; l < N; ++l) {
            double v = 0.0;
#pragma unroll
            for (int i = l; i < N; ++i) v += Li[i][k] * Li[i][l];
            inv[tri(k, l)] = v;
        }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double v = 0.0;
#pragma unroll
        for (int l = 0; l < N; ++l) v += inv[k <= l ? tri(k, l) : tri(l, k)] * r[l];
        x[k] = v;
    }
    return ok;
}

// Delta_n and W_n (packed 00, 01, 11) of an entry, the header's expressions
__device__ __forceinline__ void astrom_entry_weight(const AstromEntry &E, const double *dl, const double *F, double &D0, double &D1,
                                                    double &W00, double &W01, double &W11) {
    const double J11 = E.J[0], J21 = E.J[1], J12 = E.J[2], J22 = E.J[3];
    const double det = J11 * J22 - J12 * J21;
    D0 = (J22 * dl[0] - J12 * dl[1]) / det;
    D1 = (J11 * dl[1] - J21 * dl[0]) / det;
    const double S00 = F[0] - F[2] * F[2] / F[5], S01 = F[1] - F[2] * F[4] / F[5], S11 = F[3] - F[4] * F[4] / F[5];
#if CELESTE_ASTROM_MUTANT == 3
    const double a = J11, b = J21, c = J12, d = J22;          // J' for J
#else
    const double a = J11, b = J12, c = J21, d = J22;          // J = [a b; c d]
#endif
    // W = J' S J
    const double T00 = S00 * a + S01 * c, T01 = S00 * b + S01 * d, T10 = S01 * a + S11 * c, T11 = S01 * b + S11 * d;
    W00 = a * T00 + c * T10;
    W01 = a * T01 + c * T11;
    W11 = b * T01 + d * T11;
}

__global__ void __launch_bounds__(64)
astrom_summary_kernel(int n_targets, const int64_t *__restrict__ eoff, const int32_t *__restrict__ targets,
                      const double *__restrict__ vp, const AstromEntry *__restrict__ entries, const double *__restrict__ epochs,
                      const int32_t *__restrict__ flag, const double *__restrict__ delta, const double *__restrict__ fisher,
                      int32_t *__restrict__ n_epochs, int32_t *__restrict__ sflag, double *__restrict__ summary,
                      int32_t *__restrict__ status) {
    const int ti = blockIdx.x * 64 + threadIdx.x;
    if (ti >= n_targets) return;
    const int64_t e0 = eoff[ti], e1 = eoff[ti + 1];
    const double *vs = vp + (size_t)targets[ti] * CEL_P;
    bool nonfinite = false, bad = false;
    for (int k = 0; k < CEL_P; ++k) nonfinite |= !isfinite(vs[k]);
    int n = 0, distinct = 0;
    double tsum = 0.0, tfirst = 0.0;
    double SW[3] = {0.0, 0.0, 0.0}, SWD[2] = {0.0, 0.0};
    for (int64_t e = e0; e < e1; ++e) {
        bad |= flag[e] == CELESTE_ASTROM_BAD_MODEL;
        if (flag[e] != CELESTE_ASTROM_OK) continue;
        const AstromEntry E = entries[e];
        double D0, D1, W00, W01, W11;
        astrom_entry_weight(E, delta + 2 * e, fisher + 6 * e, D0, D1, W00, W01, W11);
        const double t = epochs[E.n];
        if (n == 0) tfirst = t; else distinct |= t != tfirst;
        ++n;
        tsum += t;
        SW[0] += W00; SW[1] += W01; SW[2] += W11;
        SWD[0] += W00 * D0 + W01 * D1; SWD[1] += W01 * D0 + W11 * D1;
    }
    const double nan = (double)NAN;
    double out[AST_NSUM];
#pragma unroll
    for (int k = 0; k < AST_NSUM; ++k) out[k] = nan;
    int fl = 0;
    double mean[2], mcov[3];
    if (n == 0 || !astrom_spd_solve<2>(SW, SWD, mean, mcov)) {
        fl = CELESTE_ASTROM_NO_EPOCHS | CELESTE_ASTROM_NO_MOTION;
    } else {
        const double tref = tsum / (double)n;
        double N4[10], r4[4];
#pragma unroll
        for (int k = 0; k < 10; ++k) N4[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) r4[k] = 0.0;
        double c2 = 0.0;
        for (int64_t e = e0; e < e1; ++e) {
            if (flag[e] != CELESTE_ASTROM_OK) continue;
            const AstromEntry E = entries[e];
            double D0, D1, W00, W01, W11;
            astrom_entry_weight(E, delta + 2 * e, fisher + 6 * e, D0, D1, W00, W01, W11);
            const double r0 = D0 - mean[0], r1 = D1 - mean[1];
            c2 += r0 * (W00 * r0 + W01 * r1) + r1 * (W01 * r0 + W11 * r1);
            const double tau = epochs[E.n] - tref, tt = tau * tau;
            const double g0 = W00 * D0 + W01 * D1, g1 = W01 * D0 + W11 * D1;
            // packed 4 x 4: (00 01 02 03 | 11 12 13 | 22 23 | 33) over (Delta_0 (2), mu (2))
            N4[0] += W00; N4[1] += W01; N4[2] += tau * W00; N4[3] += tau * W01;
            N4[4] += W11; N4[5] += tau * W01; N4[6] += tau * W11;
            N4[7] += tt * W00; N4[8] += tt * W01;
            N4[9] += tt * W11;
            r4[0] += g0; r4[1] += g1; r4[2] += tau * g0; r4[3] += tau * g1;
        }
        out[CELESTE_ASTROM_MEAN] = mean[0]; out[CELESTE_ASTROM_MEAN + 1] = mean[1];
#pragma unroll
        for (int k = 0; k < 3; ++k) out[CELESTE_ASTROM_MEAN_COV + k] = mcov[k];
        out[CELESTE_ASTROM_CHI2_CONST] = c2;
        out[CELESTE_ASTROM_T_REF] = tref;
        double beta[4], bcov[10];
        if (!distinct || !astrom_spd_solve<4>(N4, r4, beta, bcov)) {
            fl = CELESTE_ASTROM_NO_MOTION;
        } else {
            double cl = 0.0;
            for (int64_t e = e0; e < e1; ++e) {
                if (flag[e] != CELESTE_ASTROM_OK) continue;
                const AstromEntry E = entries[e];
                double D0, D1, W00, W01, W11;
                astrom_entry_weight(E, delta + 2 * e, fisher + 6 * e, D0, D1, W00, W01, W11);
                const double tau = epochs[E.n] - tref;
                const double r0 = D0 - beta[0] - beta[2] * tau, r1 = D1 - beta[1] - beta[3] * tau;
                cl += r0 * (W00 * r0 + W01 * r1) + r1 * (W01 * r0 + W11 * r1);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) out[CELESTE_ASTROM_MOTION + k] = beta[k];
#pragma unroll
            for (int k = 0; k < 10; ++k) out[CELESTE_ASTROM_MOTION_COV + k] = bcov[k];
            out[CELESTE_ASTROM_CHI2_LIN] = cl;
        }
    }
    n_epochs[ti] = n;
    sflag[ti] = fl;
#pragma unroll
    for (int k = 0; k < AST_NSUM; ++k) summary[(size_t)ti * AST_NSUM + k] = out[k];
    status[ti] = nonfinite ? CELESTE_ERR_NONFINITE_INPUT : (bad ? CELESTE_ERR_NONFINITE_RESULT : CELESTE_OK);
}

// ---- host side ----------------------------------------------------------------------------------------------------------
enum { AB_VP, AB_ITEMS, AB_ENTRIES, AB_INFO, AB_SB, AB_SX, AB_SE, AB_TARGETS, AB_EOFF, AB_EPOCHS, AB_IMAGE, AB_DELTA, AB_ALPHA,
       AB_FISHER, AB_COV, AB_CHI2, AB_LOGLIK, AB_NPIX, AB_ITERS, AB_FLAG, AB_NEPOCHS, AB_SFLAG, AB_SUMMARY, AB_STATUS, AB_COUNT };

struct celeste_astrom_ctx : ClientCtx<AB_COUNT, 5, 4> {
    // host staging of one call: kept here so that it outlives the asynchronous copies
    std::vector<VisitItem> items;
    std::vector<AstromEntry> entries;
    std::vector<int64_t> eoff;
    std::vector<double> epochs;
};

extern "C" int celeste_astrom_version(void) { return CELESTE_ASTROM_ABI_VERSION; }

extern "C" const char *celeste_astrom_strerror(int status) { return celeste_strerror(status); }

extern "C" int celeste_astrom_ctx_create(const celeste_problem_t *problem, int device, celeste_astrom_ctx_t **out) try {
    return client_create(problem, device, out);
} ABI_CATCH

extern "C" void celeste_astrom_ctx_destroy(celeste_astrom_ctx_t *f) { client_destroy(f); }

extern "C" int celeste_astrom_offsets(celeste_astrom_ctx_t *f, const double *vp, int32_t n_targets, const int32_t *targets,
                                      const celeste_astrom_params_t *params, const double *epochs, int64_t *entry_offsets,
                                      int32_t *image, double *delta, double *alpha, double *fisher, double *cov, double *chi2,
                                      double *loglik, int32_t *n_pix, int32_t *iters, int32_t *flag, int32_t *n_epochs,
                                      int32_t *summary_flag, double *summary, int32_t *status) try {
    if (!f || !f->c || !vp || n_targets < 0) return CELESTE_ERR_INVALID_ARG;
    if (n_targets > 0 && (!targets || !entry_offsets || !image || !delta || !alpha || !fisher || !cov || !chi2 || !loglik ||
                          !n_pix || !iters || !flag || !n_epochs || !summary_flag || !summary || !status))
        return CELESTE_ERR_INVALID_ARG;
    celeste_astrom_params_t pr;
    pr.tol_sigma = 1e-6; pr.max_sigma_px = 0.2; pr.max_shift_px = 2.0; pr.max_iters = 50; pr.pad = 0;
    if (params) pr = *params;
    auto pos = [](double v) { return v > 0.0 && std::isfinite(v); };
    if (!pos(pr.tol_sigma) || !pos(pr.max_sigma_px) || !pos(pr.max_shift_px) || pr.max_iters < 1) return CELESTE_ERR_INVALID_ARG;
    celeste_ctx_t *c = f->c;
    if (epochs)
        for (int n = 0; n < c->N; ++n) if (!std::isfinite(epochs[n])) return CELESTE_ERR_INVALID_ARG;
    if (!client_targets_ok(c, n_targets, targets)) return CELESTE_ERR_INVALID_ARG;
    if (n_targets == 0) return CELESTE_OK;
    // the work list, and the entries in (target, image) order: eoff[ti] .. eoff[ti + 1] are target ti's
    std::vector<VisitItem> &items = f->items;
    std::vector<AstromEntry> &entries = f->entries;
    std::vector<int64_t> &eoff = f->eoff;
    entries.clear();
    eoff.assign((size_t)n_targets + 1, 0);
    int64_t n_tiles = 0, poff = 0;
    if (!client_walk(c, n_targets, targets, items, n_tiles, poff, [&](int ti, int v, int npx, int64_t tile0, int64_t, int64_t px_off) {
            if (entries.size() >= 0x7fffff00ull) return false;
            const DevPatch &P = c->h_patches[v];
            AstromEntry E;
            E.px_off = px_off; E.npx = npx; E.tile0 = (int32_t)tile0; E.n = c->h_vis_img[v]; E.ti = ti; E.sn = v; E.H2 = P.H2;
            E.off_h = P.off_h; E.off_w = P.off_w;
            for (int k = 0; k < 4; ++k) E.J[k] = P.J[k];
            entries.push_back(E);
            ++eoff[ti + 1];
            return true;
        })) return CELESTE_ERR_INVALID_ARG;
    for (int ti = 0; ti < n_targets; ++ti) eoff[ti + 1] += eoff[ti];
    f->epochs.resize((size_t)c->N);
    for (int n = 0; n < c->N; ++n) f->epochs[n] = epochs ? epochs[n] : (double)n;
    const size_t nt = (size_t)n_targets, ni = items.size(), ne = entries.size(), nim = (size_t)c->N;
    for (int ti = 0; ti <= n_targets; ++ti) entry_offsets[ti] = eoff[ti];
    HIP_TRY(hipSetDevice(c->device));
    double *d_vp = nullptr, *d_sb = nullptr, *d_sx = nullptr, *d_se = nullptr, *d_epochs = nullptr, *d_delta = nullptr,
           *d_alpha = nullptr, *d_fisher = nullptr, *d_cov = nullptr, *d_chi2 = nullptr, *d_loglik = nullptr, *d_summary = nullptr;
    VisitItem *d_items = nullptr;
    AstromEntry *d_entries = nullptr;
    AstromTileInfo *d_info = nullptr;
    int64_t *d_eoff = nullptr;
    int32_t *d_targets = nullptr, *d_image = nullptr, *d_npix = nullptr, *d_iters = nullptr, *d_flag = nullptr,
            *d_nepochs = nullptr, *d_sflag = nullptr, *d_status = nullptr;
    const size_t npl = (size_t)poff * sizeof(double);
    if (client_get(f, AB_VP, (size_t)c->S * CEL_P * sizeof(double), &d_vp) != hipSuccess ||
        client_get(f, AB_ITEMS, ni * sizeof(VisitItem), &d_items) != hipSuccess ||
        client_get(f, AB_ENTRIES, ne * sizeof(AstromEntry), &d_entries) != hipSuccess ||
        client_get(f, AB_INFO, (size_t)n_tiles * sizeof(AstromTileInfo), &d_info) != hipSuccess ||
        client_get(f, AB_SB, npl, &d_sb) != hipSuccess || client_get(f, AB_SX, npl, &d_sx) != hipSuccess ||
        client_get(f, AB_SE, npl, &d_se) != hipSuccess ||
        client_get(f, AB_TARGETS, nt * sizeof(int32_t), &d_targets) != hipSuccess ||
        client_get(f, AB_EOFF, (nt + 1) * sizeof(int64_t), &d_eoff) != hipSuccess ||
        client_get(f, AB_EPOCHS, nim * sizeof(double), &d_epochs) != hipSuccess ||
        client_get(f, AB_IMAGE, ne * sizeof(int32_t), &d_image) != hipSuccess ||
        client_get(f, AB_DELTA, ne * 2 * sizeof(double), &d_delta) != hipSuccess ||
        client_get(f, AB_ALPHA, ne * sizeof(double), &d_alpha) != hipSuccess ||
        client_get(f, AB_FISHER, ne * 6 * sizeof(double), &d_fisher) != hipSuccess ||
        client_get(f, AB_COV, ne * 6 * sizeof(double), &d_cov) != hipSuccess ||
        client_get(f, AB_CHI2, ne * sizeof(double), &d_chi2) != hipSuccess ||
        client_get(f, AB_LOGLIK, ne * sizeof(double), &d_loglik) != hipSuccess ||
        client_get(f, AB_NPIX, ne * sizeof(int32_t), &d_npix) != hipSuccess ||
        client_get(f, AB_ITERS, ne * sizeof(int32_t), &d_iters) != hipSuccess ||
        client_get(f, AB_FLAG, ne * sizeof(int32_t), &d_flag) != hipSuccess ||
        client_get(f, AB_NEPOCHS, nt * sizeof(int32_t), &d_nepochs) != hipSuccess ||
        client_get(f, AB_SFLAG, nt * sizeof(int32_t), &d_sflag) != hipSuccess ||
        client_get(f, AB_SUMMARY, nt * AST_NSUM * sizeof(double), &d_summary) != hipSuccess ||
        client_get(f, AB_STATUS, nt * sizeof(int32_t), &d_status) != hipSuccess)
        return CELESTE_ERR_HIP;
    hipStream_t st = c->stream;
    HIP_TRY(hipMemcpyAsync(d_vp, vp, (size_t)c->S * CEL_P * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_targets, targets, nt * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_eoff, eoff.data(), (nt + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_epochs, f->epochs.data(), nim * sizeof(double), hipMemcpyHostToDevice, st));
    if (ni > 0) HIP_TRY(hipMemcpyAsync(d_items, items.data(), ni * sizeof(VisitItem), hipMemcpyHostToDevice, st));
    if (ne > 0) HIP_TRY(hipMemcpyAsync(d_entries, entries.data(), ne * sizeof(AstromEntry), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(f->ev[0], st));
    client_launch_prep(c, d_vp, st);
    HIP_TRY(hipEventRecord(f->ev[1], st));
    if (ni > 0)
        hipLaunchKernelGGL(astrom_pixel_kernel, dim3((unsigned)ni), dim3(64), 0, st, d_items, c->d_images, c->d_patches, c->d_coefs,
                           c->d_bitmaps, c->d_srcimg, c->d_comps, c->d_nbr_off, c->d_nbr_idx, c->d_vis_off, c->d_vis_img,
                           c->d_vis_src, (int)c->dense, c->N, c->NC, c->chunk_px, d_sb, d_sx, d_se, d_info);
    HIP_TRY(hipEventRecord(f->ev[2], st));
    if (ne > 0)
        hipLaunchKernelGGL(astrom_solve_kernel, dim3((unsigned)ne), dim3(AST_THREADS), 0, st, d_entries, d_info, d_targets, d_vp,
                           c->d_patches, c->d_coefs, c->d_srcimg, c->d_comps, c->NC, d_sb, d_sx, d_se, pr.tol_sigma,
                           pr.max_sigma_px, pr.max_shift_px, (int)pr.max_iters, d_image, d_delta, d_alpha, d_fisher, d_cov, d_chi2,
                           d_loglik, d_npix, d_iters, d_flag);
    HIP_TRY(hipEventRecord(f->ev[3], st));
    hipLaunchKernelGGL(astrom_summary_kernel, dim3((unsigned)((nt + 63) / 64)), dim3(64), 0, st, n_targets, d_eoff, d_targets, d_vp,
                       d_entries, d_epochs, d_flag, d_delta, d_fisher, d_nepochs, d_sflag, d_summary, d_status);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(f->ev[4], st));
    if (ne > 0) {
        HIP_TRY(hipMemcpyAsync(image, d_image, ne * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(delta, d_delta, ne * 2 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(alpha, d_alpha, ne * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(fisher, d_fisher, ne * 6 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(cov, d_cov, ne * 6 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(chi2, d_chi2, ne * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(loglik, d_loglik, ne * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(n_pix, d_npix, ne * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(iters, d_iters, ne * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(flag, d_flag, ne * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(n_epochs, d_nepochs, nt * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(summary_flag, d_sflag, nt * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(summary, d_summary, nt * AST_NSUM * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(status, d_status, nt * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    client_stage_ms(f);
    return client_first_status(status, n_targets);
} ABI_CATCH

extern "C" int celeste_astrom_last_ms(celeste_astrom_ctx_t *f, float ms[4]) { return client_last_ms(f, ms); }
