/* celeste_phot.h -- C ABI of libceleste_phot.so: per-exposure forced photometry on an AMD Instinct MI355X (gfx950).
 *
 * Given a parameter table, the library says for every target how bright it was in each single image: the Poisson
 * maximum-likelihood scale of the source's own light in that image, everything else (its position and shape, the sky,
 * its neighbours) held fixed at the table.  A light curve per source, with the image index as its x-axis: the library
 * knows no observation times, callers map the index to a time.  Nothing in the table is optimised or modified.
 *
 * Entries.  For every target s of the call and every image n in which s has a non-empty patch there is one entry (s, n),
 * in (target, image) order -- target k of the call before target k + 1, a repeated target once per repeat.
 *
 * Visited pixels, x, iota, eps, m and B are exactly those of celeste_fit.h: every pixel of s's patch in image n (the last
 * column included) whose bitmap entry is set and whose value is not NaN; m = E_G_s.v of s itself (0 in the last column of
 * its patch), B the same quantity summed over the neighbours of s in the order of the problem's neighbour list (a
 * neighbour counts where the pixel lies inside its patch, not in that patch's last column, with its bitmap entry set).
 *
 * Per visited pixel, everything in double:
 *   a = iota * m                 electrons of the source at unit scale
 *   b = iota * (eps + B)         electrons of sky and neighbours
 *   lam(alpha) = b + alpha * a
 * The estimate alpha_hat of an entry is the root of
 *   g(alpha) = sum a * (x / lam(alpha) - 1)            on  alpha > alpha_min = max over {a > 0} of (-b / a)
 * and with it
 *   I(alpha) = sum a^2 / lam(alpha)                    sigma = 1 / sqrt(I(alpha_hat))
 *   chi2     = sum (x - lam(alpha_hat))^2 / lam(alpha_hat)
 * (sums over the visited pixels of the entry).  alpha_hat may be negative: forced photometry of a faint source must be
 * unbiased.  With x >= 0, g is decreasing and convex on the domain, so Newton's iteration
 *   alpha_{k+1} = alpha_k + g(alpha_k) / D(alpha_k),   D(alpha) = sum x a^2 / lam(alpha)^2 = -g'(alpha)
 * started at alpha_0 = 1 approaches the root monotonically from the left after its first step.  A step that would reach or
 * cross alpha_min goes half of the way from alpha_k to alpha_min instead.  The iteration stops when the Newton step
 * satisfies |step| <= tol_sigma / sqrt(I(alpha_k)) (the step is still taken), or after max_iters steps.  I and chi2 are
 * then evaluated once more at the final alpha.
 *
 * Per entry: image (index), alpha, sigma, chi2, n_pix (visited pixels), iters (Newton steps taken) and a flag:
 *   CELESTE_PHOT_OK             converged
 *   CELESTE_PHOT_NO_LIGHT       no visited pixel has a > 0 (a patch that is only its last column, say): alpha and sigma
 *                               are NaN, chi2 is evaluated at lam = b, n_pix is still counted
 *   CELESTE_PHOT_AT_BOUND       the visited pixels with a > 0 hold no electrons at all (x <= 0 at each), so the likelihood
 *                               rises to the edge of the domain: alpha = alpha_min exactly, sigma and chi2 NaN
 *   CELESTE_PHOT_NOT_CONVERGED  max_iters reached (or a step was not finite): alpha is the last iterate, sigma and chi2 are
 *                               evaluated there
 *   CELESTE_PHOT_BAD_MODEL      a visited pixel has a non-finite a or b, or a < 0, or b <= 0: alpha, sigma, chi2 are NaN
 * n_pix is the count of visited pixels under every flag.
 *
 * Status of a target (the rule of celeste_fit.h): CELESTE_ERR_NONFINITE_INPUT when one of its own 44 parameters is not
 * finite -- every entry of the target is then BAD_MODEL with NaN results; otherwise CELESTE_ERR_NONFINITE_RESULT when one
 * of its entries is BAD_MODEL (a neighbour's parameters can do that); otherwise CELESTE_OK.  Other targets are untouched.
 *
 * Per target and band, over the band's entries flagged OK in ascending image order, w = 1 / sigma^2:
 *   n_epochs                     their number
 *   [0] wmean        (sum w alpha) / (sum w)           NaN when n_epochs = 0 (all three)
 *   [1] wmean_sigma  1 / sqrt(sum w)
 *   [2] chi2_var     sum w (alpha - wmean)^2           n_epochs - 1 degrees of freedom for a source of constant light
 * A target with a non-OK status still gets the summaries of its OK entries.
 *
 * Order of summation: the pixels of a patch are taken in tiles of 64 consecutive pixels (column-major, as the patch is
 * stored); a tile is summed by a fixed butterfly over the wavefront, a pixel that is not visited entering as 0; the tiles
 * are then added one after another in ascending order.  The order is the same whether the entry's pixels are held in LDS
 * or streamed from device memory on every iteration.  No floating-point atomic is used.  An entry's numbers therefore
 * depend on its own inputs only -- not on the other targets of the call, their order, repeats of a target,
 * CELESTE_CHUNK_PX, or which of the two paths ran -- and repeat bit for bit.
 *
 * Status codes and celeste_problem_t are those of celeste_mi355x.h.  fp64 only; one device (no device group).  The
 * context uploads its own copy of the image planes, as the fit library does.  Thread safety: one call at a time per
 * context.  Without a HIP device celeste_phot_ctx_create returns CELESTE_ERR_NO_DEVICE -- there is no CPU path. */
#ifndef CELESTE_PHOT_H
#define CELESTE_PHOT_H

#include <stdint.h>
#include "celeste_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CELESTE_PHOT_ABI_VERSION 100
#define CELESTE_PHOT_BANDS 5
#define CELESTE_PHOT_NSUMMARY 3
#define CELESTE_PHOT_LDS_PIXELS 6400   /* the largest patch whose a, b, x (24 B per pixel) are held in LDS */
enum { CELESTE_PHOT_OK = 0, CELESTE_PHOT_NO_LIGHT = 1, CELESTE_PHOT_AT_BOUND = 2, CELESTE_PHOT_NOT_CONVERGED = 3,
       CELESTE_PHOT_BAD_MODEL = 4 };
enum { CELESTE_PHOT_WMEAN = 0, CELESTE_PHOT_WMEAN_SIGMA = 1, CELESTE_PHOT_CHI2_VAR = 2 };

typedef struct celeste_phot_ctx celeste_phot_ctx_t;

typedef struct celeste_phot_params {
    double tol_sigma;        /* stop when |step| <= tol_sigma / sqrt(I): default 1e-9; finite and > 0 */
    int32_t max_iters;       /* default 50; >= 1 */
    int32_t lds_max_pixels;  /* 0: patches of up to CELESTE_PHOT_LDS_PIXELS pixels are solved from LDS; > 0 lowers that
                                limit (larger patches are streamed): the results do not depend on it */
} celeste_phot_params_t;

int celeste_phot_version(void);
const char *celeste_phot_strerror(int status);
int celeste_phot_ctx_create(const celeste_problem_t *problem, int device, celeste_phot_ctx_t **out);
void celeste_phot_ctx_destroy(celeste_phot_ctx_t *ctx);

/* The light curves of n_targets targets at the parameter table vp (n_sources x 44).  Host pointers.  params: NULL means the
 * defaults.
 *   entry_offsets  int64 [n_targets + 1]  (output) CSR by target: the entries of target k of the call are
 *                  entry_offsets[k] .. entry_offsets[k + 1] - 1; the caller counts the entries from the patch table to size
 *   image, n_pix, iters, flag  int32 [n_entries]        alpha, sigma, chi2  double [n_entries]
 *   n_epochs  int32 [n_targets][5]      summary  double [n_targets][5][3]      status  int32 [n_targets]
 * Refused with CELESTE_ERR_INVALID_ARG before the first HIP call, nothing written: a NULL ctx or vp, n_targets < 0, with
 * n_targets > 0 a NULL targets or output pointer, a target outside [0, n_sources), params with a tol_sigma that is not
 * finite and positive, max_iters < 1 or lds_max_pixels < 0.  n_targets = 0 returns CELESTE_OK and touches nothing.
 * Returns the first non-OK status of a target; every output is valid then. */
int celeste_phot_light_curves(celeste_phot_ctx_t *ctx, const double *vp, int32_t n_targets, const int32_t *targets,
                              const celeste_phot_params_t *params, int64_t *entry_offsets, int32_t *image, double *alpha,
                              double *sigma, double *chi2, int32_t *n_pix, int32_t *iters, int32_t *flag, int32_t *n_epochs,
                              double *summary, int32_t *status);

/* Device time (HIP events) of the last celeste_phot_light_curves: ms[0] the per-visit tables (prep_kernel over every visit
 * of the context), ms[1] the pixel pass, ms[2] the solve pass (both paths), ms[3] the band summaries. */
int celeste_phot_last_ms(celeste_phot_ctx_t *ctx, float ms[4]);

#ifdef __cplusplus
}
#endif
#endif /* CELESTE_PHOT_H */
