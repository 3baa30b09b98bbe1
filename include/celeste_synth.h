/* celeste_synth.h -- C ABI of libceleste_synth.so: synthetic survey images on an AMD Instinct MI355X (gfx950).
 *
 * The reference's Synthetic.gen_images! (Synthetic.jl:15-58): the expected electrons of a catalog on a set of images, and
 * Poisson pixels drawn from them.  The host computes the geometry of every (source, image) pair whose clamped radius-25
 * box is not empty (celeste_jl_amd/synth.py): one celeste_synth_entry_t each.  The device renders and samples.
 *
 * Expected electrons of pixel (h, w), 1-based, of an image:
 *     lambda[h, w] = ((double)sky[h, w] + sum_e f_e(h, w) * flux_e) * (double)nelec_per_nmgy[h]
 * over the entries e whose box holds the pixel, in ascending entry order, in fp64.  f is the star's spline density at
 * (h - m1 + 26, w - m2 + 26) on the entry's stamp, or the galaxy's mixture over the image's PSF (star_value /
 * galaxy_value of the inference kernels).  No floating-point atomics: every pixel gathers its own entries.
 *
 * Poisson sampling (fp64, no contraction); the pixel is (float)k:
 *     lambda not finite -> NaN;  lambda <= 0 -> 0;
 *     lambda < 10:  L = exp(-lambda); p = 1; k = 0; loop { p *= u; if (p <= L) return k; ++k; }
 *     lambda >= 10: Hoermann's PTRS (W. Hoermann, "The transformed rejection method for generating Poisson random
 *                   variables", Insurance: Mathematics and Economics 12 (1993) 39-45):
 *         slam = sqrt(lambda); b = 0.931 + 2.53 slam; a = -0.059 + 0.02483 b; inv_alpha = 1.1239 + 1.1328 / (b - 3.4);
 *         vr = 0.9277 - 3.6224 / (b - 2);
 *         per trial: U = u - 0.5; V = u'; us = 0.5 - |U|; k = floor((2 a / us + b) U + lambda + 0.43);
 *                    accept if us >= 0.07 and V <= vr; retry if k < 0 or (us < 0.013 and V > us);
 *                    accept if log V + log inv_alpha - log(a / us^2 + b) <= -lambda + k log lambda - lgamma(k + 1).
 * Random numbers: Philox4x32-10, key = (seed low word, seed high word), counter = (pixel index (h - 1) + H (w - 1), the
 * image's stream id, block number n = 0, 1, ..., CELESTE_SYNTH_PHILOX_TAG).  A block gives two uniforms,
 * u53(x0, x1) then u53(x2, x3), u53(a, b) = (((a << 32 | b) >> 11) + 0.5) 2^-53, consumed in that order: the
 * multiplication method takes them one after the other, a PTRS trial takes one block (u, u').  A pixel that would need
 * block number CELESTE_SYNTH_MAX_BLOCKS gets NaN and is counted in n_capped.  A pixel's value depends on the seed, its
 * image's stream id, its index and its lambda only.
 *
 * Arrays are column-major planes (h fastest), as in celeste_mi355x.h.  Thread safety: calls are serialised inside the
 * library.  Without a HIP device the entry points that compute return CELESTE_SYNTH_ERR_NO_DEVICE -- there is no CPU path.
 * Invalid arguments are refused before any HIP call. */
#ifndef CELESTE_SYNTH_H
#define CELESTE_SYNTH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CELESTE_SYNTH_ABI_VERSION 100
#define CELESTE_SYNTH_PHILOX_TAG 0x53594E54u   /* "SYNT": the last counter word, apart from the MCMC streams' */
#define CELESTE_SYNTH_MAX_BLOCKS 64
#define CELESTE_SYNTH_MAX_K 4

enum {
    CELESTE_SYNTH_OK = 0,
    CELESTE_SYNTH_ERR_INVALID_ARG = 1,
    CELESTE_SYNTH_ERR_NO_DEVICE = 2,
    CELESTE_SYNTH_ERR_HIP = 3,
    CELESTE_SYNTH_ERR_ALLOC = 4
};

enum {
    CELESTE_SYNTH_FLAG_EXPECTATION = 1u   /* pixels = (float)lambda, no sampling */
};

typedef struct celeste_synth_image_t {
    int32_t H, W;
    int32_t psf_K;                 /* 1 .. CELESTE_SYNTH_MAX_K */
    uint32_t stream;               /* the image's Philox stream id */
    const float *sky;              /* H x W, nmgy */
    const float *nelec_per_nmgy;   /* H */
    const double *psf;             /* psf_K x 6: alphaBar, xiBar1, xiBar2, tauBar11, tauBar12, tauBar22 */
    double *lambda_out;            /* H x W expected electrons, or NULL */
    float *pixels_out;             /* H x W pixels, or NULL */
} celeste_synth_image_t;

/* one (source, image) pair; the table is sorted by (image, source), strictly */
typedef struct celeste_synth_entry_t {
    int32_t image, source;
    int32_t h0, h1, w0, w1;        /* the clamped box, 1-based, inclusive, inside the image and not empty */
    int32_t is_star;
    int32_t stamp;                 /* stars: index into the stamp table; galaxies: ignored */
    double m[2];                   /* the source's pixel position in the image */
    double flux;                   /* of the image's band, nmgy */
    double gal_frac_dev, gal_axis_ratio, gal_angle, gal_radius_px;
} celeste_synth_entry_t;

int celeste_synth_version(void);
const char *celeste_synth_strerror(int status);

/* Renders n_entries entries on n_images images and, unless CELESTE_SYNTH_FLAG_EXPECTATION is set, samples them.
 * stamps: n_stamps raw 51 x 51 PSF stamps, column-major; the library conditions and prefilters them on the device.
 * chunk_tiles: the largest number of pixel tiles per launch, 0 = all in one (results do not depend on it).
 * n_capped (may be NULL): the number of pixels that hit CELESTE_SYNTH_MAX_BLOCKS. */
int celeste_synth_generate(int device, int32_t n_images, const celeste_synth_image_t *images, int64_t n_entries,
                           const celeste_synth_entry_t *entries, int32_t n_stamps, const double *stamps, uint64_t seed,
                           uint32_t flags, int32_t chunk_tiles, int64_t *n_capped);

/* Samples pixels[i] ~ Poisson(lambda[i]), i < n, as pixel index first_index + i of stream `stream`. */
int celeste_synth_sample(int device, int64_t n, const double *lambda, uint64_t seed, uint32_t stream, uint32_t first_index,
                         float *pixels, int64_t *n_capped);

/* device time of the last call of this process: stamp prefilter, galaxy tables, pixel kernel(s), in milliseconds
 * (celeste_synth_sample: the third only) */
int celeste_synth_last_ms(float ms[3]);

#ifdef __cplusplus
}
#endif
#endif /* CELESTE_SYNTH_H */
