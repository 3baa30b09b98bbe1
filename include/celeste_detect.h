/*
 * celeste_detect.h -- C ABI of the MI355X source-detection library (libceleste_detect.so).
 *
 *   reference                                               this library
 *   ------------------------------------------------------  --------------------------
 *   SEP.Background(calpixels; boxsize=(256,256),            celeste_detect_run
 *       filtersize=(3,3)) + SEP.global_rms +
 *       SEP.extract(calpixels, 1.3; noise=rms)
 *       src/detection.jl:39-59, src/SEP.jl:318-385
 *
 * Axis convention.  An image is H x W, row-major in memory (numpy's layout of model.Image.pixels).  The reference hands
 * Julia's column-major H x W arrays to SEP with SEP's width = H, so SEP's x is the ROW index (axis 0) and SEP's y the
 * column index (axis 1).  Every quantity below follows SEP: x / xmin / xmax / x2 are along axis 0, y / ymin / ymax / y2
 * along axis 1, theta is measured from the axis-0 direction towards axis 1, and the "column-major linear index" of a
 * pixel (i, j) is  i + H*j  (0-based), SEP's raster order.
 *
 * Status codes are those of celeste_mi355x.h.  No C++ exception crosses this ABI.  Without a HIP device every call that
 * computes returns CELESTE_DETECT_ERR_NO_DEVICE: there is no CPU fallback.
 */
#ifndef CELESTE_DETECT_H
#define CELESTE_DETECT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CELESTE_DETECT_ABI_VERSION 100

enum {
    CELESTE_DETECT_OK = 0,
    CELESTE_DETECT_ERR_INVALID_ARG = 1,
    CELESTE_DETECT_ERR_HIP = 4,
    CELESTE_DETECT_ERR_NO_DEVICE = 5,
    CELESTE_DETECT_ERR_ALLOC = 6
};

/* celeste_detect_params_t.flags */
#define CELESTE_DETECT_WANT_MAPS 1   /* fill mask and segmap of every image result */
#define CELESTE_DETECT_TIMING 2      /* fill celeste_detect_result_t.stage_ms (adds a device sync per stage) */

/* one image: pixels and sky are H x W row-major float32 (NaN pixel = masked), nelec_per_nmgy has H entries (per row) */
typedef struct {
    int32_t H, W;
    const float *pixels;
    const float *sky;
    const float *nelec_per_nmgy;
} celeste_detect_image_t;

typedef struct {
    float thresh;            /* relative threshold (1.3): pixel detected when conv > float(thresh * global_rms) */
    int32_t minarea;         /* 5 */
    int32_t deblend_nthresh; /* 32 */
    int32_t flags;           /* CELESTE_DETECT_* */
    double deblend_cont;     /* 0.005 */
    int32_t lds_max_pixels;  /* parents up to this many pixels are deblended in LDS; 0 = the library's limit (640) */
    int32_t reserved;
} celeste_detect_params_t;

typedef struct {
    int32_t npix;
    int32_t xmin, xmax, ymin, ymax;   /* 0-based, inclusive (x = axis 0) */
    int32_t parent;                   /* ordinal of the connected component (before deblending) within the image */
    int32_t reserved;
    int64_t pix_offset;               /* first entry of this object's pixels in celeste_detect_image_result_t.pix */
    double x, y;                      /* 0-based, flux-weighted centroid of the unconvolved calibrated values */
    double x2, y2, xy;                /* flux-weighted second central moments */
    double a, b, theta;               /* SExtractor ellipse (theta in radians, from +x towards +y) */
    double flux;                      /* sum of calibrated values */
    double peak;                      /* largest calibrated value */
} celeste_detect_object_t;

typedef struct {
    int32_t H, W;
    float rms;                        /* global rms of the background mesh (NaN: no good mesh cell, no object) */
    float thresh;                     /* absolute threshold used: float(params.thresh * rms) */
    int32_t n_objects;
    int32_t n_parents;
    int64_t n_pix;                    /* length of pix */
    celeste_detect_object_t *objects; /* in order of their smallest column-major pixel index */
    int64_t *pix;                     /* column-major linear pixel indices, ascending within each object */
    uint8_t *mask;                    /* WANT_MAPS: H x W row-major, 1 where conv > thresh (before minarea) */
    int32_t *segmap;                  /* WANT_MAPS: H x W row-major, object index + 1, 0 = none */
} celeste_detect_image_result_t;

typedef struct {
    int32_t n_images;
    int32_t reserved;
    double stage_ms[6];               /* TIMING: calibrate, mesh, filter+threshold, labelling, deblend, moments */
    celeste_detect_image_result_t *images;
} celeste_detect_result_t;

int celeste_detect_version(void);
const char *celeste_detect_strerror(int status);

/* Detects the objects of n_images images in one set of launches on HIP device `device`.  On success *out holds a
 * result allocated by the library (free it with celeste_detect_result_free).  Results are bit-identical across calls
 * and do not depend on which other images share the call. */
int celeste_detect_run(int32_t device, int32_t n_images, const celeste_detect_image_t *images,
                       const celeste_detect_params_t *params, celeste_detect_result_t **out);

void celeste_detect_result_free(celeste_detect_result_t *result);

#ifdef __cplusplus
}
#endif

#endif /* CELESTE_DETECT_H */
