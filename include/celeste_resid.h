/* celeste_resid.h -- C ABI of libceleste_resid.so: whole-frame residuals and the search for sources a catalog missed, on an
 * AMD Instinct MI355X (gfx950).
 *
 * Given a parameter table, the library renders the model of whole frames, filters the residuals with the PSF and lists the
 * significant peaks of the filtered map: the middle of "subtract the model, look at what is left, add it, fit again".
 * Nothing is optimised and nothing is modified.  The reference has no such step; tests/resid_reference.py restates this
 * header in numpy.
 *
 * Planes are the engine's: pixel (h, w), 0-based, of an H x W image is at index h + H w; that index is the pixel's raster
 * index.  Everything below is double; float32 inputs are widened.
 *
 * Frame model.  For image n and pixel p = (h, w):
 *   m(p)   = sum over the sources s, in ascending s, starting from 0, of c0 f0 + c1 f1 (E_G_s.v in nanomaggies: the per-visit
 *            tables SrcImg / Comp of the engine's prep_kernel at the call's table, f0 = star_value, f1 = galaxy_value).
 *            Source s contributes at p under the rule of the engine's expected image (celeste_render_expected): s has a
 *            patch in n, p is inside it and not in its last column, and the patch's bitmap entry is set -- or, when the
 *            patch has no bitmap, pixels[p] is not NaN.
 *   lam(p) = iota[h] * (eps(p) + m(p))          electrons the model expects; the product is rounded once
 * lam is defined at every pixel of the frame, masked (NaN) pixels included.  It is a gather: a workgroup owns a tile of
 * 32 x 8 pixels and walks the sources whose patch rectangle (without its last column) meets the tile, listed by the host in
 * ascending source order; no atomic is involved, so lam repeats bit for bit.
 *
 * Matched filter.  phi(dh, dw) = sum_k alpha_k N((dh, dw); xi_k, T_k) from the image's own Gaussian mixture (opts.psf: with a
 * spatially variable PSF this is the mixture fitted at the image centre, not the local one -- a deviation from what a
 * per-pixel PSF would give), evaluated at the integer offsets |dh|, |dw| <= R = opts.radius and not renormalised.  A tap
 * q = p + d is good when it is inside the frame, pixels[q] is not NaN and lam(q) > 0.  With r = x - lam:
 *   N(p)   = sum over good taps of phi(d) * (iota(q) r(q) / lam(q))
 *   D(p)   = sum over good taps of phi(d)^2 * (iota(q)^2 / lam(q))
 *   cov(p) = (sum of phi(d) over good taps) / (sum of phi(d) over all taps)          exactly 1 when every tap is good
 *   z(p)   = N / sqrt(D)     f(p) = N / D  (nanomaggies)     both NaN where cov < opts.min_coverage or D == 0
 * Taps are added in a fixed order: dw ascending outside, dh ascending inside.  Why this statistic: add a point source of
 * flux f at p to the model, lam' = lam + iota f phi(. - p); the inverse-variance weighted least-squares f (weights 1 / lam)
 * is sum (iota phi) r / lam / sum (iota phi)^2 / lam = N / D, its variance is 1 / D, and z is its standard score.
 *
 * Frame summary (celeste_resid_frame_t) per image of the call: n_px = pixels that are not NaN; n_bad = pixels (masked ones
 * included) where lam is not finite or <= 0; chi2 = sum r^2 / lam over the pixels that are not NaN; z_max, z_min over
 * the finite z (NaN when there is none).  status: CELESTE_ERR_NONFINITE_INPUT when a source with a patch in the image has a
 * non-finite parameter, otherwise CELESTE_ERR_NONFINITE_RESULT when n_bad > 0, otherwise CELESTE_OK.  A frame that is not
 * OK gets NaN for chi2, z_max, z_min and in its N, D, z and coverage maps, and no candidates; the other frames of the
 * call are not affected.  Sums are taken in two stages in a fixed order (a tile by a fixed tree, then a frame's tiles).
 *
 * Peaks.  p is a candidate when z(p) >= opts.threshold and, for each of its 8 neighbours q inside the frame whose z is not
 * NaN: z(p) > z(q) if q has the lower raster index, z(p) >= z(q) otherwise -- a plateau yields its lowest raster index.
 * Sub-pixel offset per axis, from the two neighbours z_minus, z_plus on that axis and z_0 = z(p):
 *   delta = 0.5 (z_minus - z_plus) / (z_minus - 2 z_0 + z_plus), clamped to [-0.5, 0.5];
 *   0 when a neighbour is outside the frame or NaN, or the denominator is >= 0.
 * Candidates come in (image as listed in the call, raster index) order.  With more than max_candidates the first
 * max_candidates in that order are written, n_found is the true count and the status is CELESTE_RESID_TRUNCATED.
 *
 * The stack (celeste_resid_stack): the maps of the last search added across its images on a sky grid, to find the sources
 * that stay below the threshold in every single image.  For a point source N and D are the sufficient statistics
 * (Var N = D, f = N / D, z = N / sqrt(D)), and they add across independent images at one sky position.
 *   WCS (celeste_resid_wcs_t), of an image or of the grid; world and pixel coordinates are pairs, pixels 1-based (h, w):
 *     AFFINE  pix = J (world - world0) + pix0, m = J11, J21, J12, J22 as celeste_patch_t.wcs_jacobian:
 *             pc1 = (J11 d1 + J12 d2) + pix01, pc2 = (J21 d1 + J22 d2) + pix02 with d = world - world0;
 *             world = (I (pix - pix0)) + world0 likewise, I = J^-1 by the adjugate (four quotients by the determinant, host).
 *     TAN     world0 = crval, pix0 = crpix, m = cd (CD1_1, CD1_2, CD2_1, CD2_2): world_to_pix and pix_to_world are exactly
 *             the expressions celeste_prep.h states for its tangent-plane images -- both arguments of the projection written
 *             without their cancellation, cd^-1 by the adjugate, sin0 and cos0 of crval2 from the host's libm, NaN behind
 *             the plane (not n > 0).  sin, cos, atan2 and hypot are the device's.  No product is contracted into an FMA.
 *   Grid (celeste_resid_grid_t) = {H, W, wcs}: cell (h, w), 0-based, is the grid's 1-based pixel (h + 1, w + 1); the planes
 *     of a channel are H x W, index h + H w.
 *   Channel k has weights s_k[0 .. 4], one per band (an SED: the relative flux assumed in each band), finite, not negative, at
 *     least one above zero.  For cell c, over the images i of the last search in the call's order whose frame status is OK
 *     and whose s = s_k[band_i - 1] is above zero:
 *       world = grid.pix_to_world(c);  (p1, p2) = world_to_pix_i(world), the image is skipped when either is not finite;
 *       qh = rint(p1) - 1, qw = rint(p2) - 1, skipped when outside the frame (tested in double before the conversion);
 *       skipped when z_i(q) is NaN (coverage below the search's min_coverage, or D = 0);
 *       N_k += s * N_i(q);  D_k += (s * s) * D_i(q);  cnt_k += 1     each product rounded once, then added; no FMA.
 *     z = N / sqrt(D) and f = N / D where cnt >= opts.min_images and D > 0, otherwise both NaN.
 *   The sample is the nearest pixel, not an interpolation: Var N = D stays exact, the result repeats bit for bit, and it is
 *   the rule resid.missed_sources samples by.  (The price is the signal a mis-registration of up to half a pixel loses.)
 *   Candidates: the peak rule and the sub-pixel rule above on each channel's z plane, in (channel, raster index) order, cut
 *     at max_candidates with the true count and CELESTE_RESID_TRUNCATED.  world = grid.pix_to_world(h + 1 + dh, w + 1 + dw),
 *     computed on the device.  Channel summary (celeste_resid_stack_frame_t): the number of cells that have a z, z_max, z_min
 *     (NaN when there is none).
 *   Culling (no effect on any number): a workgroup owns 32 x 8 cells; when the grid and the image are of one kind, the four
 *     corner cells of the tile all project in front of the image's plane and their bounding box, widened by one pixel, misses
 *     [1, H] x [1, W], the workgroup skips the image (a map between two tangent planes or two affine planes takes lines to
 *     lines, so the tile stays inside the box of its corners).  CELESTE_STACK_NO_CULL=1 in the environment, read per call,
 *     turns it off.
 *
 * Nothing depends on which other images are in the call, on CELESTE_CHUNK_PX or on how the work is cut into launches; no
 * floating-point atomic is used; every number repeats bit for bit.
 *
 * Status codes and celeste_problem_t are those of celeste_mi355x.h.  fp64 only; one device (no device group).  The context
 * uploads its own copy of the image planes, as the fit library does.  Thread safety: one call at a time per context.
 * Without a HIP device celeste_resid_ctx_create and celeste_resid_find_peaks return CELESTE_ERR_NO_DEVICE -- there is no
 * CPU path. */
#ifndef CELESTE_RESID_H
#define CELESTE_RESID_H

#include <stdint.h>
#include "celeste_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CELESTE_RESID_ABI_VERSION 101
#define CELESTE_RESID_MAX_RADIUS 12
#define CELESTE_RESID_TRUNCATED 100     /* more candidates than max_candidates: the list is cut, n_found is the true count */
enum { CELESTE_RESID_LAM = 0, CELESTE_RESID_N = 1, CELESTE_RESID_D = 2, CELESTE_RESID_Z = 3, CELESTE_RESID_COVERAGE = 4 };

typedef struct celeste_resid_ctx celeste_resid_ctx_t;

typedef struct celeste_resid_opts_t {
    double threshold;        /* 5.0 */
    double min_coverage;     /* 0.8 */
    int32_t radius;          /* 8; 1 .. CELESTE_RESID_MAX_RADIUS */
    int32_t psf_K;           /* components of each image's mixture (celeste_resid_search only) */
    const double *psf;       /* n_images of the problem x psf_K x {alpha, xi1, xi2, tau11, tau12, tau22}, as celeste_patch_t.psf */
} celeste_resid_opts_t;

typedef struct celeste_resid_frame_t {
    int32_t image, status;
    int64_t n_px, n_bad;
    double chi2, z_max, z_min;
} celeste_resid_frame_t;

typedef struct celeste_resid_candidate_t {
    int32_t image, h, w, reserved;     /* 0-based pixel */
    double dh, dw;                     /* sub-pixel offsets: the peak is at (h + dh, w + dw) */
    double z, f, D, cov;               /* celeste_resid_find_peaks: f and D are NaN (it is given no N and D) */
} celeste_resid_candidate_t;

int celeste_resid_version(void);
const char *celeste_resid_strerror(int status);
/* threshold 5, min_coverage 0.8, radius 8, no PSF */
void celeste_resid_opts_default(celeste_resid_opts_t *opts);
int celeste_resid_ctx_create(const celeste_problem_t *problem, int device, celeste_resid_ctx_t **out);
void celeste_resid_ctx_destroy(celeste_resid_ctx_t *ctx);

/* The maps, summaries and candidates of n_images images (images NULL: all images of the problem, n_images ignored) at the
 * parameter table vp (n_sources x 44).  Host pointers.  The maps stay in the context's device buffers until the next
 * search.  out_frames: one per image of the call, in the call's order.  out_candidates: room for max_candidates (may be
 * NULL when max_candidates is 0).  *status: the first non-OK status of a frame, otherwise CELESTE_RESID_TRUNCATED when the
 * list was cut, otherwise CELESTE_OK; the call itself returns CELESTE_OK whenever it ran, and every output is valid then.
 * Refused with CELESTE_ERR_INVALID_ARG before the first HIP call, nothing written: a NULL ctx, vp, opts, opts->psf,
 * out_frames, n_found or status; n_images < 0; an image outside [0, n_images of the problem) or listed twice; a radius
 * outside [1, 12]; psf_K outside [1, 16]; max_candidates < 0; max_candidates > 0 without out_candidates. */
int celeste_resid_search(celeste_resid_ctx_t *ctx, const double *vp, int32_t n_images, const int32_t *images,
                         const celeste_resid_opts_t *opts, celeste_resid_frame_t *out_frames,
                         celeste_resid_candidate_t *out_candidates, int64_t max_candidates, int64_t *n_found, int32_t *status);

/* One map (CELESTE_RESID_LAM .. CELESTE_RESID_COVERAGE) of an image of the last search: H x W doubles, index h + H w.
 * CELESTE_ERR_INVALID_ARG: NULL arguments, `which` unknown, no search yet, or the image was not in the last search. */
int celeste_resid_get_map(celeste_resid_ctx_t *ctx, int32_t image, int32_t which, double *out_plane);

/* N, D and coverage of the last search's maps at n pixels (one small kernel; no plane is copied).  A pixel outside its frame
 * gives zeros with cov = 0; a pixel where z is NaN (cov below the search's min_coverage, D == 0, or a frame that is not OK)
 * gives NaN in N and D and the map's cov.  CELESTE_ERR_INVALID_ARG as for celeste_resid_get_map, and for n < 0. */
int celeste_resid_sample(celeste_resid_ctx_t *ctx, int64_t n, const int32_t *image, const int32_t *h, const int32_t *w,
                         double *out_N, double *out_D, double *out_cov);

/* The peak rule on a caller's planes: z and coverage are H x W (index h + H w; coverage may be NULL: cov is NaN then),
 * opts NULL: the defaults (only threshold is read).  Records carry image = 0 and f = D = NaN.  *status is CELESTE_OK or
 * CELESTE_RESID_TRUNCATED.  CELESTE_ERR_INVALID_ARG before the first HIP call: NULL z, n_found or status, H or W < 1,
 * H * W >= 2^31, max < 0, max > 0 without out. */
int celeste_resid_find_peaks(int device, int32_t H, int32_t W, const double *z, const double *coverage,
                             const celeste_resid_opts_t *opts, celeste_resid_candidate_t *out, int64_t max, int64_t *n_found,
                             int32_t *status);

/* Device time (HIP events) of the last celeste_resid_search: ms[0] the per-visit tables (prep_kernel), ms[1] the frame model
 * and its sums, ms[2] the matched filter and the z range, ms[3] the peaks. */
int celeste_resid_last_ms(celeste_resid_ctx_t *ctx, float ms[4]);

/* ---- the stack ---- */
enum { CELESTE_RESID_WCS_AFFINE = 0, CELESTE_RESID_WCS_TAN = 1 };
enum { CELESTE_RESID_STACK_N = 0, CELESTE_RESID_STACK_D = 1, CELESTE_RESID_STACK_Z = 2, CELESTE_RESID_STACK_COUNT = 3 };
#define CELESTE_RESID_STACK_MAX_CHANNELS 8

typedef struct celeste_resid_wcs_t {
    int32_t kind, reserved;
    double world0[2];                  /* AFFINE: world0; TAN: crval = (ra0, dec0), degrees */
    double pix0[2];                    /* AFFINE: pix0; TAN: crpix, the 1-based reference pixel in (h, w) order */
    double m[4];                       /* AFFINE: J11, J21, J12, J22; TAN: cd, degrees per pixel: CD1_1, CD1_2, CD2_1, CD2_2 */
} celeste_resid_wcs_t;

typedef struct celeste_resid_grid_t {
    int32_t H, W;
    celeste_resid_wcs_t wcs;
} celeste_resid_grid_t;

typedef struct celeste_resid_stack_opts_t {
    double threshold;                  /* 5.0 */
    int32_t min_images, reserved;      /* 1 */
} celeste_resid_stack_opts_t;

typedef struct celeste_resid_stack_frame_t {
    int32_t channel, reserved;
    int64_t n_cells;                   /* cells that have a z */
    double z_max, z_min;
} celeste_resid_stack_frame_t;

typedef struct celeste_resid_stack_candidate_t {
    int32_t channel, h, w, n_images;   /* 0-based cell; the images that were added there */
    double dh, dw;
    double z, f, D;
    double world[2];
} celeste_resid_stack_candidate_t;

/* threshold 5, min_images 1 */
void celeste_resid_stack_opts_default(celeste_resid_stack_opts_t *opts);

/* CELESTE_OK when every one of the n records is usable: a known kind, finite fields, |dec0| <= 90 (TAN), a matrix whose
 * determinant is finite and not zero.  CELESTE_ERR_INVALID_ARG otherwise, and for n < 1 or a NULL array.  No handle, no device. */
int celeste_resid_wcs_check(int32_t n, const celeste_resid_wcs_t *wcs);

/* The stack of the last search's maps on `grid`: wcs holds one record per image of the problem (n_images must be the
 * problem's), weights n_channels x 5.  out_frames: one per channel.  out_candidates: room for max_candidates (may be NULL when
 * max_candidates is 0).  *status: CELESTE_RESID_TRUNCATED when the list was cut, otherwise CELESTE_OK.  The planes stay in the
 * context until its next stack; they describe the search they were made from.
 * Refused with CELESTE_ERR_INVALID_ARG before the first HIP call, nothing written: a NULL ctx, grid, wcs, weights, opts,
 * out_frames, n_found or status; no search yet; n_images differing from the problem's; H or W < 1, or H * W >= 2^31;
 * n_channels outside 1 .. 8; a weight that is not finite or is negative, or a channel whose weights are all zero;
 * min_images < 1; a WCS (the grid's or an image's) that celeste_resid_wcs_check refuses; max_candidates < 0;
 * max_candidates > 0 without out_candidates. */
int celeste_resid_stack(celeste_resid_ctx_t *ctx, const celeste_resid_grid_t *grid, int32_t n_images,
                        const celeste_resid_wcs_t *wcs, int32_t n_channels, const double *weights,
                        const celeste_resid_stack_opts_t *opts, celeste_resid_stack_frame_t *out_frames,
                        celeste_resid_stack_candidate_t *out_candidates, int64_t max_candidates, int64_t *n_found,
                        int32_t *status);

/* One plane (CELESTE_RESID_STACK_N .. COUNT) of a channel of the last stack: H x W doubles, index h + H w (the count as
 * doubles).  CELESTE_ERR_INVALID_ARG: NULL arguments, `which` unknown, no stack yet, or no such channel. */
int celeste_resid_stack_get_map(celeste_resid_ctx_t *ctx, int32_t channel, int32_t which, double *out_plane);

/* Device time (HIP events) of the last celeste_resid_stack: ms[0] the gather and the z ranges, ms[1] the peaks and their
 * world positions. */
int celeste_resid_stack_last_ms(celeste_resid_ctx_t *ctx, float ms[2]);

#ifdef __cplusplus
}
#endif
#endif /* CELESTE_RESID_H */
