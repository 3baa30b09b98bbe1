/* celeste_prep.h -- C ABI of libceleste_prep.so: the input preparation of a box on an AMD Instinct MI355X (gfx950).
 *
 * What model.patch_table, PatchTable.neighbors, SDSSPSFMap.__call__ and infer.bad_sky compute on the host, one (source,
 * image) pair at a time, for a whole catalog in a fixed number of launches: the patch geometry of get_sky_patches
 * (imaged_sources.jl:120-223), the neighbour lists of find_neighbors (imaged_sources.jl:232-244), the eigen-PSF stamps of
 * SDSSIO.jl:239-299 and the sky check of ParallelRun.jl:437-460.  An image has the affine WCS pix = J (world - world0) + pix0
 * or, after celeste_prep_images_set_wcs, a tangent-plane (TAN) one (below).
 *
 * All arithmetic is fp64 (the median: Float32, as the pixels are), compiled without contraction: a * b + c is a rounded
 * product and a rounded sum everywhere in this library.  No result uses a floating-point atomic; results repeat bit for
 * bit and do not depend on the launch geometry.
 *
 * Geometry of the pair (source s, image n), one thread per pair:
 *     d = pos - world0;  pc1 = J11 d1 + J12 d2 + pix01;  pc2 = J21 d1 + J22 d2 + pix02       (Image.world_to_pix)
 *     tried: always with CELESTE_PREP_FLAG_DENSE; otherwise when -reach < pc1 < H + 1 + reach and -reach < pc2 < W + 1 + reach,
 *            reach = (radius_override_pix is NaN ? 25 : radius_override_pix) + 1
 *     r = radius_override_pix unless it is NaN; then choose_patch_radius with width_scale 1.2, max_radius 25:
 *         ow = (is_star ? 0 : 1.2 gal_radius_px / 0.67) + psf_width;   f = flux[band - 1];  not f > 0: INVALID_ARG
 *         p90 = C1 / (C2 ow);  pt = p90 if p90 < eps / (20 f), else eps / (20 f)      C1 = exp(-0.5 * 1.64^2), C2 = sqrt(2 pi)
 *         rhs = log(pt) + C3 + log(ow);  rq = sqrt(((-2) (ow ow)) rhs);  r = 25 if 25 < rq, else rq     C3 = 0.5 log(2 pi)
 *         (C1, C2, C3 are evaluated once, by the host's libm, as Python's math module evaluates them; log and sqrt are the
 *         device's: sqrt is correctly rounded, log may differ from libm in the last place.)  A NaN position, radius or
 *         pixel coordinate of a tried pair: INVALID_ARG (the host raises there).
 *     box: rows rint(pc1 - r) .. rint(pc1 + r), columns rint(pc2 - r) .. rint(pc2 + r), rint = ties to even;
 *          clamp_box: first row into 1 .. H + 1, last row into 0 .. H, columns likewise with W.
 *     pixel_center = ((first row + last row) / 2, (first column + last column) / 2)
 *     world_center = J^-1 (pixel_center - pix0) + world0 by LU with partial pivoting (rows swapped when |J21| > |J11|):
 *         l = J21 / J11;  u = J22 - l J12;  y2 = b2 - l b1;  x2 = y2 / u;  x1 = (b1 - J12 x2) / J11.
 *     An entry is kept for every tried pair (DENSE) or for the tried pairs whose clamped box holds a pixel; entries are
 *     ordered by (source, image) -- an exclusive scan over the pairs in that order, no atomics.
 * active_pixels: the pixels of the box that are not NaN, one wavefront per entry (integer counts).
 * Neighbours of s: the sources t != s with a non-empty box that overlaps one of s's non-empty boxes in the same image
 *     (inclusive ranges: first <= other's last and other's first <= last, rows and columns); ascending, each once.
 * Stamps (CELESTE_PREP_FLAG_STAMPS), one workgroup per entry of an image with an eigen-PSF, at (x, y) = pixel_center:
 *     px_0 = 1, px_i = px_(i-1) (0.001 (x - 1));  py_j likewise with y;
 *     w_k = sum over i ascending, inside it j ascending, of cmat[i][j][k] (px_i py_j)
 *     stamps[stamp][p] = sum over k ascending of rrows[p][k] w_k,  p = 0 .. 51 * 51 - 1
 *     -- the column-major raw stamp celeste_problem_t.stamps takes (p = row + 51 column).
 * Sky check of a position, on the first image of band 4 (none: every flag 0, no launch), one workgroup per position:
 *     h = rint(pc1) into 1 .. H, w = rint(pc2) into 1 .. W;  claimed = (double)sky[h, w] * (double)nelec_per_nmgy[h]
 *     the box of radius 50 as above (at most 102 x 102 pixels);  its n pixels that are not NaN;  k = n / 2;
 *     median = the k-th smallest (0-based) for odd n, (the (k-1)-th + the k-th) * 0.5f in Float32 for even n,
 *     by an 8-bit radix select on ordered keys;  flag = n > 0 and claimed + 5 < (double)median.
 *
 * Detections (celeste_prep_detected): the per-image objects of source extraction become joined objects, one catalog entry
 * per object and the patch table of those objects, as detection.jl:61-171 builds them; the order of every list is fixed.
 *     World position of a detection of image n, one thread per detection: J^-1 ((x, y) - pix0) + world0, by the LU above.
 *     Join: the joined list starts empty; the images are taken in turn.  Every detection of an image looks for the nearest
 *         entry of the list as it stood before that image: d = sqrt(dx dx + dy dy), dx and dy the differences of the world
 *         coordinates; the lowest index among equal distances.  d < match_radius: the detection joins that entry (two
 *         detections of one image may join the same entry, none joins an entry of its own image); otherwise it is
 *         appended, in object order.  So image 0's detections open the list in object order.  One match launch per image
 *         (a thread per detection, the list through LDS in tiles of CELESTE_PREP_MATCH_TILE) and one scan-and-append
 *         launch; the length of the list stays on the device between them.  The search is exhaustive.
 *     Detections of an object: in (image, object) order -- a stable radix sort of the detections by joined index.
 *     Catalog entry, one thread per object: per band the detection with the most pixels (strict >: the first wins a tie);
 *         flux[b] = its flux, 0 for a band without a detection; the shape comes from the best detection of the band with
 *         the largest best npix (the first band on a tie): gal_axis_ratio = b / a, gal_angle = theta + x_vs_n_angle[image],
 *         gal_radius_px = sqrt(a b) C4, C4 = sqrt(2 log 2) evaluated once by the host's libm.  (is_star is false and
 *         gal_frac_dev 0.5 for every entry; the star's fluxes are the galaxy's.)
 *     Box of (object, image), one thread per pair: pc of the joined position as above; minbox = rows rint(pc1 - m) ..
 *         rint(pc1 + m), columns likewise with pc2, m = min_radius_pix.  With a detection of the object in that image (the
 *         last one in object order): its xmin .. xmax are read as a 1-based row range, ymin .. ymax as a column range, each
 *         widened on both sides by rint((dilate length) / 2), length = last - first + 1; the box is the smallest that
 *         holds the widened ranges and minbox.  Without one the box is minbox.  Then clamp_box.  An entry for every pair
 *         (DENSE) or for the pairs whose clamped box holds a pixel; from there on as for celeste_prep_patches.
 *
 * Tangent-plane images (celeste_prep_wcs_t.kind = CELESTE_PREP_WCS_TAN; world = (ra, dec) in degrees): wherever the text above
 * says world_to_pix or J^-1 (...) + world0, such an image uses the gnomonic projection of FITS WCS paper II, in fp64:
 *     world_to_pix: da = (ra - crval1) D, dec' = dec D, D = pi / 180;  l = cos dec' sin da;
 *         m = sin((dec - crval2) D) + (2 (cos dec' sin0)) (sh sh), sh = sin(da / 2)     [= sin dec' cos0 - cos dec' sin0 cos da, without
 *         its cancellation near the tangent point];  n = sin dec' sin0 + (cos dec' cos0) cos da     (sin0, cos0 of crval2 D: the host's libm)
 *         x = (l / n) / D', y = (m / n) / D' with 1 / D' = 180 / pi;  pc1 = crpix1 + (I11 x + I12 y);  pc2 = crpix2 + (I21 x + I22 y),
 *         I = cd^-1 by the adjugate (four quotients by the determinant, formed on the host).  Not n > 0 (behind the plane): NaN.
 *     pix_to_world: u = c1 - crpix1, v = c2 - crpix2;  x = (cd11 u + cd12 v) D;  y = (cd21 u + cd22 v) D;
 *         den = cos0 - y sin0;  num = sin0 + y cos0;  hyp = hypot(x, den);  ra = crval1 + atan2(x, den) / D';
 *         dec = crval2 + atan2(y - sin0 ((x x) / (hyp + den)), num sin0 + hyp cos0) / D'     [the first argument is num cos0 - hyp sin0
 *         without cancellation; crpix maps to crval exactly]
 *         -- ra is continuous around crval1, not wrapped into [0, 360).
 *     Jacobian of an entry (pixel_world_jacobian, wcs_utils.jl:36-51, pixel_delt 0.5), at its pixel_center c:
 *         w = pix_to_world(c);  t = the larger of |pix_to_world(c + (0.5, 0.5)) - w| over the two coordinates;
 *         column 1 = (world_to_pix(w + (t, 0)) - c) / t,  column 2 = (world_to_pix(w + (0, t)) - c) / t.
 *     A pair whose pixel coordinates are not finite (behind the plane) gets the empty box 1 .. 0 and is no error; the sky
 *     check of such a position is 0.  sin, cos, atan2, hypot and asin are the device's (they may differ from libm in the last
 *     places; boxes agree with the host's unless pc -/+ r lies that close to a rounding tie).
 *     Join, when any image is TAN: every detection goes to the unit vector (cos dec' cos ra', cos dec' sin ra', sin dec');
 *         d = sqrt((ex ex + ey ey) + ez ez) of the difference e of two unit vectors (the chord) takes the place of the planar
 *         distance, with the same order and tie rules; the nearest entry is joined when 2 (asin(min(d / 2, 1)) / D') < match_radius,
 *         match_radius in degrees (Coordinates.jl:71-86).  Images that are all affine keep the planar distance.
 *     A problem's catalog and images must lie on one RA branch across 0 / 360: world_to_pix accepts any branch, but positions
 *     returned by pix_to_world are on crval1's.
 *
 * Thread safety: calls are serialised inside the library.  Without a HIP device the entry points that compute return
 * CELESTE_PREP_ERR_NO_DEVICE -- there is no CPU path.  Invalid arguments are refused before any HIP call (the flux and NaN
 * checks above are part of the geometry kernel and are reported when it has run). */
#ifndef CELESTE_PREP_H
#define CELESTE_PREP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CELESTE_PREP_ABI_VERSION 100
#define CELESTE_PREP_STAMP 51          /* rnrow = rncol of an eigen-PSF */
#define CELESTE_PREP_MAX_POLY 8        /* ni, nj <= 8 */
#define CELESTE_PREP_MAX_NK 16         /* nk <= 16 */
#define CELESTE_PREP_N_STAGES 5        /* celeste_prep_last_ms */
#define CELESTE_PREP_MATCH_TILE 1024   /* joined positions per LDS tile of the match kernel */
#define CELESTE_PREP_MATCH_BLOCK 256   /* detections per workgroup of the match kernel */
#define CELESTE_PREP_DETECTED_N_STAGES 6   /* celeste_prep_detected_last_ms */

enum {
    CELESTE_PREP_OK = 0,
    CELESTE_PREP_ERR_INVALID_ARG = 1,
    CELESTE_PREP_ERR_NO_DEVICE = 2,
    CELESTE_PREP_ERR_HIP = 3,
    CELESTE_PREP_ERR_ALLOC = 4
};

enum {
    CELESTE_PREP_FLAG_DENSE = 1u,    /* an entry for every (source, image) pair, empty boxes included */
    CELESTE_PREP_FLAG_STAMPS = 2u    /* evaluate the eigen-PSF stamps */
};

typedef struct celeste_prep_image_t {
    int32_t H, W;
    int32_t band;                    /* 1 .. 5 */
    int32_t reserved;
    const float *pixels;             /* pixel (h, w), 1-based, is pixels[(h - 1) stride_h + (w - 1) stride_w] */
    int64_t stride_h, stride_w;      /* in elements: (W, 1), a row-major H x W array, or (1, H), a column-major plane */
    const float *sky;                /* the sky plane, nmgy; read for the first image of band 4 only, may be NULL elsewhere */
    int64_t sky_stride_h, sky_stride_w;
    const float *nelec_per_nmgy;     /* H */
    double wcs_jacobian[4];          /* J11, J21, J12, J22, as celeste_patch_t.wcs_jacobian */
    double wcs_world0[2], wcs_pix0[2];
    double psf_width;                /* get_psf_width(psf, 1.2) */
    double epsilon;                  /* sky[H / 2, W / 2], 1-based */
    int32_t rnrow, rncol;            /* eigen-PSF: both CELESTE_PREP_STAMP; ignored when rrows is NULL */
    int32_t ni, nj, nk;
    int32_t reserved2;
    const double *rrows;             /* (rnrow rncol) x nk, row-major: rrows[p nk + k]; NULL: a constant PSF map */
    const double *cmat;              /* ni x nj x nk, row-major: cmat[(i nj + j) nk + k] */
} celeste_prep_image_t;

enum { CELESTE_PREP_WCS_AFFINE = 0, CELESTE_PREP_WCS_TAN = 1 };

/* the WCS of one image: kind AFFINE keeps celeste_prep_image_t's matrix (the other fields are not read); kind TAN: */
typedef struct celeste_prep_wcs_t {
    int32_t kind;
    int32_t reserved;
    double crval[2];                 /* (ra0, dec0), degrees */
    double crpix[2];                 /* 1-based reference pixel, (h, w) order: FITS axis 1 = h */
    double cd[4];                    /* degrees per pixel, row-major: CD1_1, CD1_2, CD2_1, CD2_2 */
} celeste_prep_wcs_t;

typedef struct celeste_prep_source_t {
    double pos[2];
    int32_t is_star;
    int32_t reserved;
    double flux[5];                  /* the star's fluxes if is_star, else the galaxy's, nmgy */
    double gal_radius_px;
} celeste_prep_source_t;

/* page-locked host arrays owned by the result; E = n_entries, S = n_sources */
typedef struct celeste_prep_table_t {
    int64_t n_entries, n_sources, n_neighbors, n_stamps;
    const int32_t *source, *image;   /* [E], sorted by (source, image) */
    const int64_t *box;              /* [E][4]: first row, last row, first column, last column; 1-based, inclusive, clamped */
    const double *pixel_center;      /* [E][2] */
    const double *world_center;      /* [E][2] */
    const int64_t *active_pixels;    /* [E] */
    const int64_t *nbr_offsets;      /* [S + 1] */
    const int32_t *nbr_index;        /* [n_neighbors]: the neighbours of s are nbr_index[nbr_offsets[s] .. nbr_offsets[s + 1]) */
    const int32_t *stamp;            /* [E]: index into stamps, -1 for an image with a constant map; NULL without FLAG_STAMPS */
    const double *stamps;            /* [n_stamps][51 * 51], column-major raw stamps; NULL without FLAG_STAMPS */
} celeste_prep_table_t;

/* one object of one image, SEP's axes: x runs along axis 0 (rows) */
typedef struct celeste_prep_detection_t {
    int32_t npix;
    int32_t xmin, xmax, ymin, ymax;  /* 0-based, inclusive, as celeste_detect_object_t */
    int32_t reserved;
    double x, y;                     /* 1-based centroid */
    double a, b, theta, flux;
} celeste_prep_detection_t;

/* page-locked host arrays owned by the result; S = n_objects, the sources of the result's table in the same order */
typedef struct celeste_prep_catalog_t {
    int64_t n_objects, n_detections;
    const double *pos;               /* [S][2] */
    const double *flux;              /* [S][5] */
    const double *gal_axis_ratio;    /* [S] */
    const double *gal_angle;         /* [S] */
    const double *gal_radius_px;     /* [S] */
    const int64_t *det_offsets;      /* [S + 1] */
    const int32_t *det_image;        /* [n_detections]: the detections of s are det_offsets[s] .. det_offsets[s + 1], */
    const int32_t *det_object;       /* [n_detections]  image ascending, within an image the object index ascending */
} celeste_prep_catalog_t;

typedef struct celeste_prep_images celeste_prep_images_t;
typedef struct celeste_prep_result celeste_prep_result_t;

int celeste_prep_version(void);
const char *celeste_prep_strerror(int status);

/* Uploads the planes, calibrations and eigen-PSFs of n_images images to `device`; the host arrays are not needed after
 * the call. */
int celeste_prep_images_create(int device, int32_t n_images, const celeste_prep_image_t *images, celeste_prep_images_t **handle);
void celeste_prep_images_destroy(celeste_prep_images_t *handle);

/* The argument checks of celeste_prep_images_set_wcs that need no handle: INVALID_ARG for a null pointer, n_images <= 0, an
 * unknown kind and, for a TAN entry, a non-finite field, a singular cd or |crval[1]| > 90. */
int celeste_prep_wcs_check(int32_t n_images, const celeste_prep_wcs_t *wcs);
/* Gives image n of `handle` the WCS wcs[n] for every later call; n_images must be the handle's count.  Everything is checked
 * before the device is touched.  A TAN image keeps its wcs_jacobian, wcs_world0 and wcs_pix0 unread. */
int celeste_prep_images_set_wcs(celeste_prep_images_t *handle, int32_t n_images, const celeste_prep_wcs_t *wcs);

/* The patch table, neighbour lists and (FLAG_STAMPS) stamps of n_sources sources on the images of `handle`. */
int celeste_prep_patches(celeste_prep_images_t *handle, int64_t n_sources, const celeste_prep_source_t *sources,
                         double radius_override_pix, uint32_t flags, celeste_prep_result_t **result);
int celeste_prep_result_get(const celeste_prep_result_t *result, celeste_prep_table_t *table);
/* the entries' Jacobians d pix / d world, [E][4]: J11, J21, J12, J22 (an affine image's entries carry its matrix); NULL for a
 * result of a handle without a TAN image, whose patches all carry their image's matrix */
int celeste_prep_result_get_jacobians(const celeste_prep_result_t *result, const double **jac /* [E][4]: J11, J21, J12, J22 */);
void celeste_prep_result_destroy(celeste_prep_result_t *result);

/* The argument checks of celeste_prep_detected that need no handle: INVALID_ARG for a null pointer, offsets that do not
 * ascend from 0, npix <= 0, a non-finite x, y, a, b, theta, flux or angle, a <= 0, xmax < xmin, ymax < ymin, a match_radius
 * that is NaN or negative, a min_radius_pix or dilate that is not finite or is negative, an unknown flag. */
int celeste_prep_detected_check(int32_t n_images, const int64_t *det_offsets, const celeste_prep_detection_t *dets,
                                const double *x_vs_n_angle, double match_radius, double min_radius_pix, double dilate,
                                uint32_t flags);

/* The joined objects of the detections dets[det_offsets[n] .. det_offsets[n + 1]) of image n of `handle`, their catalog
 * entries and their patch table (neighbour lists and, with FLAG_STAMPS, stamps included).  detection.jl uses
 * min_radius_pix = 5 and dilate = 0.2.  No detection at all: OK, zero objects, an empty table. */
int celeste_prep_detected(celeste_prep_images_t *handle, const int64_t *det_offsets, const celeste_prep_detection_t *dets,
                          const double *x_vs_n_angle, double match_radius, double min_radius_pix, double dilate,
                          uint32_t flags, celeste_prep_result_t **result);
/* INVALID_ARG for a result that does not come from the call above */
int celeste_prep_result_get_catalog(const celeste_prep_result_t *result, celeste_prep_catalog_t *catalog);

/* flags[i] = the sky check of pos[2 i], pos[2 i + 1], i < n */
int celeste_prep_bad_sky(celeste_prep_images_t *handle, int64_t n, const double *pos, uint8_t *flags);

/* device time of the stages of the last call of this process, in milliseconds: geometry and compaction, active pixels,
 * neighbours, stamps (celeste_prep_patches; the sky check's slot is 0), sky check (celeste_prep_bad_sky; the others 0) */
int celeste_prep_last_ms(float ms[CELESTE_PREP_N_STAGES]);
/* the same for the last call that took detections: world positions, join and sort; catalog entries; then the four table
 * stages as above (0 after any other call) */
int celeste_prep_detected_last_ms(float ms[CELESTE_PREP_DETECTED_N_STAGES]);

#ifdef __cplusplus
}
#endif
#endif /* CELESTE_PREP_H */
