/* celeste_astrom.h -- C ABI of libceleste_astrom.so: per-exposure astrometry on an AMD Instinct MI355X (gfx950).
 *
 * Given a parameter table, the library says for every target where it was in each single image: the Poisson
 * maximum-likelihood offset delta = (d1, d2) of the source's own light in that image, in pixels of that image (rows,
 * columns), together with its scale alpha, everything else (its shape, the sky, its neighbours) held fixed at the table;
 * and per target the weighted mean offset and a linear motion over the exposures.  Nothing in the table is modified.
 *
 * Entries are those of celeste_phot.h: for every target s of the call and every image n in which s has a non-empty patch
 * there is one entry (s, n), in (target, image) order, a repeated target once per repeat.
 *
 * Visited pixels, x, iota, eps and B are exactly those of celeste_fit.h and celeste_phot.h: every pixel of s's patch in
 * image n (the last column included) whose bitmap entry is set and whose value is not NaN; B is E_G.v summed over the
 * neighbours of s in the order of the problem's neighbour list (a neighbour counts where the pixel lies inside its patch,
 * not in that patch's last column, with its bitmap entry set), evaluated at the table: it does not move with delta.
 *
 * Model of an entry, per visited pixel (h, w) (1-based image coordinates), everything in double:
 *   m(delta) = c0 f0(h - m1 - d1 + 26, w - m2 - d2 + 26) + c1 f1(h - m1 - d1, w - m2 - d2)     0 in the patch's last column
 *   a = iota m(delta)        b = iota (eps + B)        lam = b + alpha a        theta = (d1, d2, alpha)
 * with (m1, m2) the table's position in the image, c_i = a_i E[l_b | i], f0 the star density and f1 the galaxy density.
 *   f0   the cubic B-spline of the PSF stamp at the given index: the cell is floor(index) clamped to [1, 50] in each
 *        axis (star_value's rule), so a shifted index beyond the stamp extrapolates the edge cell's polynomial;
 *        softpluslikeinv on top: y < 0 ? 1e-3 exp(y) : 1e-3 (y + 1), the branch exactly at 0
 *   f1   sum_c w0_c exp(-d' P_c d / 2) over the staged component records, d = pixel - (m + delta) - xi_c
 * and their first derivatives with respect to delta (no second derivative of any density is formed):
 *   D = (alpha da/dd1, alpha da/dd2, a)
 * One PASS at theta yields, over the visited pixels of the entry,
 *   l    = sum x log lam - lam
 *   U_k  = sum D_k (x / lam - 1)                       k = 0, 1, 2
 *   F_kl = sum D_k D_l / lam                           k <= l: (00, 01, 02, 11, 12, 22), the packing of fisher and cov
 *   chi2 = sum (x - lam)^2 / lam
 * and whether the pass is SOUND: every visited pixel has a finite lam > 0 (a pixel that is not adds 0 to every sum).
 *
 * The step of a pass.  s_k = sqrt(F_kk), R_kl = F_kl / (s_k s_l) with a unit diagonal, R = L L' by Cholesky in index
 * order; a pivot that is not > 0 (or not finite) means the pass has NO STEP.  z = inv(L) (U / s), p = inv(F) U =
 * inv(L') z / s, dec = sqrt(z' z) = sqrt(U' inv(F) U): the length of the scoring step in standard errors.
 * inv(F)_kl = (inv(L)' inv(L))_kl / (s_k s_l).
 *
 * Iteration: Fisher scoring from theta_0 = (0, 0, 1).
 *   1. One pass at theta_0 (iters = 1).  Not sound: BAD_MODEL.  No visited pixel with a > 0: NO_LIGHT.  No step, or
 *      sqrt(max(inv(F)_00, inv(F)_11)) > max_sigma_px: TOO_FAINT -- the gate; F does not depend on x, so neither does it.
 *   2. At the current theta with its pass: dec <= tol_sigma: OK, stop (no further step is taken; this pass's F, chi2, l
 *      are the entry's).  Else iters = max_iters: NOT_CONVERGED, stop.
 *   3. p is multiplied as a whole by min(1, max_step_px / max(|p_0|, |p_1|)), max_step_px = 0.5.  t = 1.
 *   4. One pass at the trial theta + t p (iters + 1).  The trial is REJECTED when its pass is not sound, or when
 *      dec > ls_min_dec = 1e-3 and l(trial) < l(theta).  (Below ls_min_dec the expected gain dec^2 / 2 <= 5e-7 is within
 *      the rounding of l's sum, so the step is taken without the likelihood test.)  Rejected after max_halvings = 8
 *      halvings already: STALLED, stop at theta.  Rejected with iters = max_iters: NOT_CONVERGED, stop at theta.
 *      Rejected otherwise: t = t / 2, again 4.
 *   5. Accepted: theta = trial, its pass the current one.  No step there: STALLED, stop.  |d1| or |d2| > max_shift_px:
 *      OUT_OF_RANGE, stop.  Else 2.
 * A patch whose pixels are all zero under the source drives alpha towards the edge of its domain, where trials stop
 * being sound or stop gaining: such an entry ends STALLED, NOT_CONVERGED or OUT_OF_RANGE, never OK.
 *
 * Per entry: image, delta[2], alpha, fisher[6] (F), cov[6] (inv(F)), chi2, loglik (l), n_pix (visited pixels, under every
 * flag), iters (passes made) and a flag:
 *   CELESTE_ASTROM_OK             converged: everything is of the last pass
 *   CELESTE_ASTROM_NO_LIGHT       delta, alpha, fisher, cov NaN; chi2 and loglik of the pass at theta_0 (lam = b); iters 1
 *   CELESTE_ASTROM_TOO_FAINT      delta, alpha NaN; fisher, chi2, loglik of the pass at theta_0, cov = inv(F) there (NaN
 *                                 when that pass has no step); iters 1
 *   CELESTE_ASTROM_OUT_OF_RANGE   everything is of the accepted iterate that left the range
 *   CELESTE_ASTROM_STALLED        everything is of the last accepted iterate (cov NaN when its pass has no step)
 *   CELESTE_ASTROM_NOT_CONVERGED  everything is of the last accepted iterate
 *   CELESTE_ASTROM_BAD_MODEL      a visited pixel has a b that is not finite and > 0 (iters 0), or the pass at theta_0 is
 *                                 not sound (iters 1): delta, alpha, fisher, cov, chi2, loglik NaN
 *
 * Status of a target (the rule of celeste_fit.h): CELESTE_ERR_NONFINITE_INPUT when one of its own 44 parameters is not
 * finite -- every entry of the target is then BAD_MODEL with iters 0; otherwise CELESTE_ERR_NONFINITE_RESULT when one of
 * its entries is BAD_MODEL (a neighbour's parameters can do that); otherwise CELESTE_OK.  Other targets are untouched.
 *
 * Per target, over its entries flagged OK, of all bands, in ascending image order; t_n = epochs[n], or n when epochs is
 * NULL; J_n = d(m1, m2) / d(pos), the patch's WCS Jacobian:
 *   Delta_n = inv(J_n) delta_n                                            the offset in the units of pos
 *   W_n     = J_n' (F_dd - F_da F_ad / F_aa) J_n                          alpha marginalised; no inverse is taken
 *   n_epochs                      their number
 *   constant    mean = inv(sum W) sum W Delta; mean_cov = inv(sum W), packed (00, 01, 11), by the 2 x 2 Cholesky
 *               chi2_const = sum (Delta - mean)' W (Delta - mean)         2 (n_epochs - 1) degrees of freedom
 *   linear      Delta(t) = Delta_0 + mu (t - t_ref), t_ref = (sum t_n) / n_epochs; beta = (Delta_0, mu), tau = t - t_ref
 *               N = sum [W, tau W; tau W, tau^2 W],  r = sum [W Delta; tau W Delta],  N = L L' by Cholesky in index order,
 *               motion = inv(N) r, motion_cov = inv(N) packed row-major upper triangle (10)
 *               chi2_lin = sum (Delta - Delta_0 - mu tau)' W (Delta - Delta_0 - mu tau)     2 n_epochs - 4 degrees of freedom
 *   flag        CELESTE_ASTROM_NO_EPOCHS: n_epochs = 0, or sum W has a pivot that is not > 0: all of the summary NaN
 *               CELESTE_ASTROM_NO_MOTION: fewer than two distinct t_n, or N has a pivot that is not > 0: motion,
 *               motion_cov, chi2_lin NaN
 * summary [22] = mean (2), mean_cov (3), chi2_const, motion (4), motion_cov (10), chi2_lin, t_ref.
 *
 * Order of summation: the pixels of a patch are taken in tiles of 64 consecutive pixels (column-major, as the patch is
 * stored); a tile is summed by a fixed butterfly over the wavefront, a pixel that is not visited entering as 0; the
 * tiles are then added one after another in ascending order.  Every rounded operation from the densities' values and
 * gradients to the sums is a single IEEE operation in the order written below (no contraction):
 *   a = e m, g_k = e dm/dd_k (e = iota where the own light counts, else 0), lam = b + alpha a, q = 1 / lam,
 *   D_k = alpha g_k (k < 2), D_2 = a, r = x q - 1, l: x log(lam) - lam, U_k: D_k r, F_kl: (D_k D_l) q,
 *   chi2: ((x - lam) (x - lam)) q.
 * The summaries add the entries one after another in image order.  No floating-point atomic is used.  An entry's numbers
 * therefore depend on its own inputs only -- not on the other targets of the call, their order, repeats of a target or
 * CELESTE_CHUNK_PX -- and repeat bit for bit.
 *
 * Status codes and celeste_problem_t are those of celeste_mi355x.h.  fp64 only; one device (no device group).  The
 * context uploads its own copy of the image planes, as the fit library does.  Thread safety: one call at a time per
 * context.  Without a HIP device celeste_astrom_ctx_create returns CELESTE_ERR_NO_DEVICE -- there is no CPU path. */
#ifndef CELESTE_ASTROM_H
#define CELESTE_ASTROM_H

#include <stdint.h>
#include "celeste_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CELESTE_ASTROM_ABI_VERSION 100
#define CELESTE_ASTROM_NSUMMARY 22
#define CELESTE_ASTROM_MAX_STEP_PX 0.5
#define CELESTE_ASTROM_LS_MIN_DEC 1e-3
#define CELESTE_ASTROM_MAX_HALVINGS 8
enum { CELESTE_ASTROM_OK = 0, CELESTE_ASTROM_NO_LIGHT = 1, CELESTE_ASTROM_TOO_FAINT = 2, CELESTE_ASTROM_OUT_OF_RANGE = 3,
       CELESTE_ASTROM_STALLED = 4, CELESTE_ASTROM_NOT_CONVERGED = 5, CELESTE_ASTROM_BAD_MODEL = 6 };
enum { CELESTE_ASTROM_NO_EPOCHS = 1, CELESTE_ASTROM_NO_MOTION = 2 };
enum { CELESTE_ASTROM_MEAN = 0, CELESTE_ASTROM_MEAN_COV = 2, CELESTE_ASTROM_CHI2_CONST = 5, CELESTE_ASTROM_MOTION = 6,
       CELESTE_ASTROM_MOTION_COV = 10, CELESTE_ASTROM_CHI2_LIN = 20, CELESTE_ASTROM_T_REF = 21 };

typedef struct celeste_astrom_ctx celeste_astrom_ctx_t;

typedef struct celeste_astrom_params {
    double tol_sigma;        /* stop at the first pass with dec <= tol_sigma: default 1e-6; finite and > 0 */
    double max_sigma_px;     /* the gate: default 0.2; finite and > 0 */
    double max_shift_px;     /* default 2.0; finite and > 0 */
    int32_t max_iters;       /* passes per entry: default 50; >= 1 */
    int32_t pad;
} celeste_astrom_params_t;

int celeste_astrom_version(void);
const char *celeste_astrom_strerror(int status);
int celeste_astrom_ctx_create(const celeste_problem_t *problem, int device, celeste_astrom_ctx_t **out);
void celeste_astrom_ctx_destroy(celeste_astrom_ctx_t *ctx);

/* The offsets of n_targets targets at the parameter table vp (n_sources x 44).  Host pointers.  params: NULL means the
 * defaults.  epochs: double [n_images] or NULL (the image index).
 *   entry_offsets  int64 [n_targets + 1]  (output) CSR by target, as in celeste_phot.h
 *   image, n_pix, iters, flag  int32 [n_entries]     delta  double [n_entries][2]     alpha, chi2, loglik  double [n_entries]
 *   fisher, cov  double [n_entries][6]
 *   n_epochs, summary_flag  int32 [n_targets]     summary  double [n_targets][22]     status  int32 [n_targets]
 * Refused with CELESTE_ERR_INVALID_ARG before the first HIP call, nothing written: a NULL ctx or vp, n_targets < 0, with
 * n_targets > 0 a NULL targets or output pointer, a target outside [0, n_sources), params with a tol_sigma, max_sigma_px
 * or max_shift_px that is not finite and positive or max_iters < 1, epochs with an entry that is not finite.
 * n_targets = 0 returns CELESTE_OK and touches nothing.  Returns the first non-OK status of a target; every output is
 * valid then. */
int celeste_astrom_offsets(celeste_astrom_ctx_t *ctx, const double *vp, int32_t n_targets, const int32_t *targets,
                           const celeste_astrom_params_t *params, const double *epochs, int64_t *entry_offsets,
                           int32_t *image, double *delta, double *alpha, double *fisher, double *cov, double *chi2,
                           double *loglik, int32_t *n_pix, int32_t *iters, int32_t *flag, int32_t *n_epochs,
                           int32_t *summary_flag, double *summary, int32_t *status);

/* Device time (HIP events) of the last celeste_astrom_offsets: ms[0] the per-visit tables (prep_kernel over every visit
 * of the context), ms[1] the pixel pass, ms[2] the solve pass, ms[3] the summaries. */
int celeste_astrom_last_ms(celeste_astrom_ctx_t *ctx, float ms[4]);

#ifdef __cplusplus
}
#endif
#endif /* CELESTE_ASTROM_H */
