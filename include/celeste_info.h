/* celeste_info.h -- C ABI of libceleste_info.so: position and shape standard errors from the pixels' Fisher information
 * on an AMD Instinct MI355X (gfx950).
 *
 * Given a parameter table, the library says for every target how well the pixels pin down where it is and what shape it
 * has: the Fisher information of the geometry of the source under the Poisson model of the pixels, summed over the pixels
 * celeste_fit.h visits under the same neighbour rule, the five band fluxes marginalised, and from it the Cramer-Rao
 * covariance.  Nothing is optimised and nothing is modified.  Two blocks per target, one per type i in {0 star, 1 galaxy}.
 *
 * Geometry parameters, in bound space and in the units of the 44-vector:
 *   star    G = 2   (pos1, pos2)
 *   galaxy  G = 6   (pos1, pos2, gal_frac_dev, gal_axis_ratio, gal_angle, gal_radius_px)
 * pos is in world coordinates; its derivative goes through the patch's wcs_jacobian, as the ELBO's does.
 *
 * Visited pixels of target s: those of celeste_fit.h, the last column of a patch included.
 *
 * At a visited pixel (h, w) of image n (band b), everything in double; x, iota, eps and B exactly as celeste_fit.h
 * defines them (B: the neighbours' full mixture light under the ELBO's neighbour rule):
 *   E_l   = E[l_b | a = i], computed from the target's row (source_brightness.jl:46-50) -- not c_i / a_i, because a_i may
 *           be 0 in a caller's table
 *   f_i   = the type's density as the ELBO evaluates it: f_0 = softpluslikeinv of the star spline, f_1 the mixture of the
 *           28 (14 psf_K) PSF (x) prototype components
 *   g_i   = E_l f_i; 0 in the last column of s's own patch
 *   lam_i = iota * ((eps + g_i) + B)        electrons expected had the source been of type i
 *   D_k   = iota * E_l * d f_i / d theta_k  for k < G: the exact derivative of the piecewise-cubic spline (the cell is the
 *           one the value uses; the y < 0 branch of softpluslikeinv kept) and of the mixture; 0 in the last column
 *   a     = iota * g_i                      the derivative with respect to a log-scale of the source's light in band b; it
 *                                           stands in for the band's flux, which is marginalised
 *
 * Sums per (target, type, band), the images of one band adding into that band (a band without a visited pixel: zeros):
 *   A[k][l] = sum D_k D_l / lam_i  (k <= l)      c[k] = sum D_k a / lam_i      d = sum a^2 / lam_i
 * packed as the upper triangle of A row-major (A[0][0], A[0][1], ..., A[G-1][G-1]), then c, then d: CELESTE_INFO_NSUM_STAR
 * = 6 doubles for a star, CELESTE_INFO_NSUM_GAL = 28 for a galaxy.  n_pix is celeste_fit.h's count of visited pixels.
 *
 * Covariance per (target, type), from the five rows of sums (celeste_info_solve does this step alone):
 *   1. S = sum_b A_b - sum_{b: d_b > 0} c_b c_b' / d_b, bands in ascending order in both sums: the Schur complement of the
 *      five band scales
 *   2. s_k = sqrt(S_kk), R = S / (s s')
 *   3. Cholesky R = L L' in index order, without pivoting
 *   4. C = diag(1 / s) inv(R) diag(1 / s), packed as the upper triangle row-major: CELESTE_INFO_NCOV_STAR = 3 or
 *      CELESTE_INFO_NCOV_GAL = 21 doubles.  sqrt(C_kk) is the Cramer-Rao standard error of parameter k.
 *
 * Flags, an int32 bit set per (target, type); the rules are applied in this order:
 *   NO_PIXELS        d_b = 0 in every band: no visited pixel with g_i != 0.  C is NaN; no other bit is set.
 *   NOT_POSITIVE     an entry of S is not finite or an S_kk < 0 (no other bit is set then), or a pivot l_kk^2 of step 3 is
 *                    not > 0 (the factorisation stops there).  C is NaN.
 *   UNCONSTRAINED    some S_kk == 0 exactly.  By positive semi-definiteness its row is zero, so dropping it is exact: its
 *                    variance is +inf, its covariances are 0, and the rest is solved without it.  gal_axis_ratio == 1
 *                    makes gal_angle such a parameter, exactly.
 *   ILL_CONDITIONED  the smallest pivot l_kk^2 of the unit-diagonal R (over the parameters kept) is below 1e-8: a
 *                    parameter is determined by the others to one part in 1e8.  C is still written.  Not looked at when a
 *                    pivot is not positive.
 *
 * Status of a target, as in celeste_fit.h: CELESTE_ERR_NONFINITE_INPUT when one of its own 44 parameters is not finite;
 * otherwise CELESTE_ERR_NONFINITE_RESULT when a lam_i is not finite or not positive at one of its visited pixels;
 * otherwise CELESTE_OK.  A target with a non-OK status gets NaN in all its sums (its n_pix is still the count of visited
 * pixels); step 1 then finds S not finite: both its flags are NOT_POSITIVE and its covariances NaN.  The other targets of
 * the call are not affected.
 *
 * Order of summation: celeste_fit.h's.  A tile of 64 consecutive pixels of a patch is summed by a fixed butterfly over the
 * wavefront, a pixel that is not visited entering as 0; a target's tiles are then added one after another in ascending
 * (image, tile) order into the band of their image.  No floating-point atomic is used.  A target's numbers therefore depend
 * on its own inputs only -- not on the other targets of the call, their order, repeats of a target, CELESTE_CHUNK_PX or how
 * the work is cut into launches -- and repeat bit for bit.
 *
 * Status codes and celeste_problem_t are those of celeste_mi355x.h.  fp64 only; one device (no device group).  The
 * context uploads its own copy of the image planes, as the fit and phot libraries do.  Thread safety: one call at a time
 * per context.  Without a HIP device celeste_info_ctx_create returns CELESTE_ERR_NO_DEVICE -- there is no CPU path. */
#ifndef CELESTE_INFO_H
#define CELESTE_INFO_H

#include <stdint.h>
#include "celeste_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CELESTE_INFO_ABI_VERSION 100
#define CELESTE_INFO_BANDS 5
#define CELESTE_INFO_G_STAR 2
#define CELESTE_INFO_G_GAL 6
#define CELESTE_INFO_NSUM_STAR 6
#define CELESTE_INFO_NSUM_GAL 28
#define CELESTE_INFO_NCOV_STAR 3
#define CELESTE_INFO_NCOV_GAL 21
#define CELESTE_INFO_PIVOT_MIN 1e-8
enum { CELESTE_INFO_NO_PIXELS = 1, CELESTE_INFO_UNCONSTRAINED = 2, CELESTE_INFO_NOT_POSITIVE = 4,
       CELESTE_INFO_ILL_CONDITIONED = 8 };

typedef struct celeste_info_ctx celeste_info_ctx_t;

int celeste_info_version(void);
const char *celeste_info_strerror(int status);
int celeste_info_ctx_create(const celeste_problem_t *problem, int device, celeste_info_ctx_t **out);
void celeste_info_ctx_destroy(celeste_info_ctx_t *ctx);

/* The sums, covariances and flags of n_targets targets at the parameter table vp (n_sources x 44).  Host pointers.
 *   n_pix     int64  [n_targets][5]
 *   sums_star double [n_targets][5][6]      sums_gal double [n_targets][5][28]
 *   cov_star  double [n_targets][3]         cov_gal  double [n_targets][21]
 *   flag      int32  [n_targets][2]         status   int32  [n_targets]
 * Refused with CELESTE_ERR_INVALID_ARG before the first HIP call, nothing written: a NULL ctx, vp or (n_targets > 0)
 * targets or output, n_targets < 0, a target outside [0, n_sources).  n_targets = 0 returns CELESTE_OK and touches nothing.
 * Returns the first non-OK status of a target; every output is valid then. */
int celeste_info_bounds(celeste_info_ctx_t *ctx, const double *vp, int32_t n_targets, const int32_t *targets, int64_t *n_pix,
                        double *sums_star, double *sums_gal, double *cov_star, double *cov_gal, int32_t *flag,
                        int32_t *status);

/* The covariance step alone, on caller-supplied sums: n rows of sums_star [n][5][6] and sums_gal [n][5][28] give cov_star
 * [n][3], cov_gal [n][21] and flag [n][2].  A NULL pointer or n < 0 is refused as above; n = 0 returns CELESTE_OK. */
int celeste_info_solve(celeste_info_ctx_t *ctx, int32_t n, const double *sums_star, const double *sums_gal, double *cov_star,
                       double *cov_gal, int32_t *flag);

/* Device time (HIP events) of the last celeste_info_bounds: ms[0] the per-visit tables (prep_kernel over every visit of
 * the context), ms[1] the pixel kernel, ms[2] the kernel that adds a target's tiles, ms[3] the solve kernel. */
int celeste_info_last_ms(celeste_info_ctx_t *ctx, float ms[4]);

#ifdef __cplusplus
}
#endif
#endif /* CELESTE_INFO_H */
