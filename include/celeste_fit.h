/* celeste_fit.h -- C ABI of libceleste_fit.so: per-source goodness of fit on an AMD Instinct MI355X (gfx950).
 *
 * Given a parameter table, the library says for every target how well the model those parameters describe resembles the
 * pixels: one pass over the pixels elbo_likelihood visits with active_sources = [s] (elbo_objective.jl:437-469), with the
 * densities, the per-visit tables and the neighbour rule of the ELBO itself.  Nothing is optimised and nothing is modified.
 *
 * Visited pixels of target s: every pixel of s's patch in every image where it has one (the last column included) whose
 * bitmap entry is set (default bitmap: the pixel is not NaN) and whose value is not NaN.
 *
 * At a visited pixel (h, w) of image n (band b), everything in double:
 *   x    = pixels[h, w], iota = nelec_per_nmgy[h], eps = sky[h, w]                (float32 inputs, widened)
 *   m    = E_G_s.v = c0 f0 + c1 f1 of s itself, in nanomaggies (c_i = a_i E[l_i] of band b, f0 the star density, f1 the
 *          galaxy density: elbo_objective.jl:62-65); 0 in the last column of s's patch, where add_pixel_term!'s test
 *          1 <= w2 < W2 excludes it
 *   B    = the same quantity summed over the neighbours of s, in the order of the problem's neighbour list, starting from
 *          0; a neighbour counts at the pixel when the pixel lies inside ITS patch in image n, not in that patch's last
 *          column, and that patch's bitmap entry is set (elbo_objective.jl:349)
 *   lam  = iota * ((eps + m) + B)       electrons the model expects
 *   r    = x - lam
 *
 * Per target and band (the images of one band are summed into that band; a band without a visited pixel gives n_pix = 0
 * and zeros), n_pix = the number of visited pixels and seven statistics:
 *   [0] chi2   sum r^2 / lam                       Pearson's chi-square
 *   [1] resid  sum r                               electrons the model leaves over
 *   [2] own    sum iota m                          the source's model electrons in its patch
 *   [3] self   sum (iota m) * (m / (m + B))        (a term is 0 where m = 0) self / own is the share of the source's
 *                                                  profile-weighted light that is its own: exactly 1 without neighbours
 *   [4] wres   sum (iota m) r / lam                d log-likelihood / d (a scale factor on the source's light)
 *   [5] winfo  sum (iota m)^2 / lam                its Fisher information: wres / sqrt(winfo) is the standardised flux
 *                                                  misfit, wres / winfo the fractional flux correction of one Newton step
 *   [6] max_z  max |r| / sqrt(lam)
 *
 * Status of a target: CELESTE_ERR_NONFINITE_INPUT when one of its own 44 parameters is not finite; otherwise
 * CELESTE_ERR_NONFINITE_RESULT when lam is not finite or not positive at one of its visited pixels (a neighbour's
 * parameters can do that); otherwise CELESTE_OK.  A target with a non-OK status gets NaN in all its 35 statistics (its
 * n_pix is still the count of visited pixels); the other targets of the call are not affected.
 *
 * Order of summation: the visited pixels of a patch are taken in tiles of 64 consecutive pixels (column-major, as the
 * patch is stored); a tile is summed by a fixed butterfly over the wavefront, a pixel that is not visited entering as 0;
 * a target's tiles are then added one after another in ascending (image, tile) order into the band of their image.  No
 * floating-point atomic is used.  A target's numbers therefore depend on its own inputs only -- not on the other targets
 * of the call, their order, repeats of a target (allowed: the call only reads), CELESTE_CHUNK_PX or how the work is cut
 * into launches -- and repeat bit for bit.
 *
 * Status codes and celeste_problem_t are those of celeste_mi355x.h.  fp64 only; one device (no device group).  The
 * context uploads its own copy of the image planes, as the MCMC and blend libraries do.  Thread safety: one call at a
 * time per context.  Without a HIP device celeste_fit_ctx_create returns CELESTE_ERR_NO_DEVICE -- there is no CPU path. */
#ifndef CELESTE_FIT_H
#define CELESTE_FIT_H

#include <stdint.h>
#include "celeste_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CELESTE_FIT_ABI_VERSION 100
#define CELESTE_FIT_BANDS 5
#define CELESTE_FIT_NSTATS 7
enum { CELESTE_FIT_CHI2 = 0, CELESTE_FIT_RESID = 1, CELESTE_FIT_OWN = 2, CELESTE_FIT_SELF = 3, CELESTE_FIT_WRES = 4,
       CELESTE_FIT_WINFO = 5, CELESTE_FIT_MAX_Z = 6 };

typedef struct celeste_fit_ctx celeste_fit_ctx_t;

int celeste_fit_version(void);
const char *celeste_fit_strerror(int status);
int celeste_fit_ctx_create(const celeste_problem_t *problem, int device, celeste_fit_ctx_t **out);
void celeste_fit_ctx_destroy(celeste_fit_ctx_t *ctx);

/* The statistics of n_targets targets at the parameter table vp (n_sources x 44).  Host pointers.
 *   n_pix   int64  [n_targets][5]      stats  double [n_targets][5][7]      status  int32 [n_targets]
 * Stamps (optional): one entry per (target, image) pair with a non-empty patch, in (target, image) order -- target k of
 * the call before target k + 1, a repeated target once per repeat.  stamp_offsets (output, int64, one more than the number
 * of entries: the caller counts them from the patch table) receives the CSR offsets, entry e occupying
 * stamps[stamp_offsets[e] .. stamp_offsets[e + 1]): the H2 x W2 values of lam, column-major as the patch, NaN where the
 * pixel is not visited.  stamp_offsets may be given without stamps (the offsets alone are written); stamps without
 * stamp_offsets is refused.  Both NULL: no stamps.
 * Refused with CELESTE_ERR_INVALID_ARG before the first HIP call, nothing written: a NULL ctx, vp or (n_targets > 0)
 * targets / n_pix / stats / status, n_targets < 0, a target outside [0, n_sources), stamps without stamp_offsets.
 * n_targets = 0 returns CELESTE_OK and touches nothing.  Returns the first non-OK status of a target; every output is
 * valid then. */
int celeste_fit_stats(celeste_fit_ctx_t *ctx, const double *vp, int32_t n_targets, const int32_t *targets, int64_t *n_pix,
                      double *stats, int32_t *status, int64_t *stamp_offsets, double *stamps);

/* Device time (HIP events) of the last celeste_fit_stats: ms[0] the per-visit tables (prep_kernel over every visit of the
 * context), ms[1] the pixel kernel, ms[2] the kernel that adds a target's tiles. */
int celeste_fit_last_ms(celeste_fit_ctx_t *ctx, float ms[3]);

#ifdef __cplusplus
}
#endif
#endif /* CELESTE_FIT_H */
