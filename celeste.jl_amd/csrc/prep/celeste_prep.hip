// libceleste_prep.so -- the input preparation of a box on gfx950 (include/celeste_prep.h states the arithmetic).
//
//   prep_geometry_kernel     one thread per (source, image) pair: radius, box, clamp; which pairs become entries
//   prep_compact_kernel      one thread per pair: the kept pairs, in (source, image) order, at their scanned positions;
//                            centres, the (image, first row) sort key, the eigen-PSF flag
//   prep_jacobian_kernel     one thread per entry, when an image has a tangent-plane WCS: the finite-difference Jacobian at its centre
//   prep_active_kernel       one wavefront per entry: the pixels of its box that are not NaN
//   prep_gather_kernel       boxes and sources in (image, first row) order
//   prep_nbr_kernel          one thread per entry: the entries of its image whose boxes overlap its own (count, then fill)
//   prep_source_ranges_kernel, prep_unique_kernel
//                            per source: where its links start; its sorted links without repeats (count, then fill)
//   prep_stamp_kernel        one workgroup per entry: polynomial weights, then the weighted sum of eigen-images
//   prep_sky_kernel          one workgroup per position: the median of its box by radix select, the flag
// and for detections (prep_detected.h): prep_det_world_kernel, prep_match_kernel, prep_append_kernel,
//   prep_object_ranges_kernel, prep_entry_kernel, prep_detected_geometry_kernel -- then the stages above from the compaction on
// Scans and sorts are hipCUB's (integer keys: a stable radix sort, results do not depend on the launch geometry).
// The file is compiled with -ffp-contract=off.
//
// CELESTE_PREP_MUTANT=k builds the library with one deliberate bug, for tests/test_prep_mutants.py (the product is 0;
// 17 and up are in prep_detected.h):
//   1 = round_even rounds halves away from zero
//   2 = clamped_box: the last column is clamped to W - 1
//   3 = prep_geometry_kernel: the tried test takes pc1 > reach for pc1 > -reach
//   4 = the radius takes max(pdf_90, epsilon / (20 flux))
//   5 = the radius drops the width scale 1.2
//   6 = pix_to_world does not pivot
//   7 = jacobian_at takes the smaller step
//   8 = prep_active_kernel counts NaN
//   9 = prep_nbr_kernel: the overlap test is strict in the rows
//   10 = prep_nbr_kernel: the row window is one short
//   11 = prep_unique_kernel keeps repeats
//   12 = prep_stamp_kernel: tx without the - 1
//   13 = prep_stamp_kernel: i and j swapped in cmat
//   14 = prep_sky_kernel: an even count's median is its upper value
//   15 = prep_sky_kernel: claimed + 5 <= median
//   16 = prep_sky_kernel takes nelec by column
#ifndef CELESTE_PREP_MUTANT
#define CELESTE_PREP_MUTANT 0
#endif
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../../include/celeste_prep.h"

#define PREP_BLOCK 256
#define PREP_NPIX (CELESTE_PREP_STAMP * CELESTE_PREP_STAMP)
#define PREP_SKY_SIDE 102            // a clamped box of radius 50 has at most 102 rows / columns
#define PREP_SKY_RADIUS 50.0

struct PrepImg {
    int32_t H, W, band, has_eig;
    const float *pix; int64_t sh, sw;
    const float *sky; int64_t ksh, ksw;
    const float *nelec;
    double J11, J21, J12, J22, w0[2], p0[2], psf_width, eps;
    int32_t ni, nj, nk, pad;
    const double *rrows, *cmat;
    // celeste_prep_images_set_wcs: kind TAN reads these in place of J, w0, p0 (ci = cd^-1; sin0, cos0 of crval[1]: the host's libm)
    int32_t kind, pad2;
    double crval[2], crpix[2], cd[4], ci[4], sin0, cos0;
};

#define PREP_D2R (M_PI / 180.0)
#define PREP_R2D (180.0 / M_PI)

struct PrepConsts { double c1, c2, c3; };   // exp(-0.5 * 1.64^2), sqrt(2 pi), 0.5 log(2 pi): the host's libm

// rint, kept inside the int32 range (a box that far away clamps to the same empty range)
__device__ __forceinline__ int32_t round_even(double x) {
#if CELESTE_PREP_MUTANT == 1
    double r = round(x);
#else
    double r = rint(x);
#endif
    r = r < -2.0e9 ? -2.0e9 : (r > 2.0e9 ? 2.0e9 : r);
    return (int32_t)r;
}
__device__ __forceinline__ int32_t clampi(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the gnomonic projection (celeste_prep.h); NaN behind the tangent plane
__device__ __forceinline__ void tan_world_to_pix(const PrepImg &im, double ra, double dec, double &pc1, double &pc2) {
    const double da = (ra - im.crval[0]) * PREP_D2R, dr = dec * PREP_D2R;
    double sd, cdec, sa, ca;
    sincos(dr, &sd, &cdec);
    sincos(da, &sa, &ca);
    const double l = cdec * sa;
    // sin dec cos0 - cos dec sin0 cos da as sin(dec - dec0) + 2 cos dec sin0 sin^2(da / 2): no cancellation near the tangent point
    const double sh = sin(0.5 * da);
    const double m = sin((dec - im.crval[1]) * PREP_D2R) + (2.0 * (cdec * im.sin0)) * (sh * sh);
    const double n = sd * im.sin0 + (cdec * im.cos0) * ca;
    if (!(n > 0.0)) { pc1 = NAN; pc2 = NAN; return; }
    const double x = (l / n) * PREP_R2D, y = (m / n) * PREP_R2D;
    pc1 = im.crpix[0] + (im.ci[0] * x + im.ci[1] * y);
    pc2 = im.crpix[1] + (im.ci[2] * x + im.ci[3] * y);
}

__device__ __forceinline__ void tan_pix_to_world(const PrepImg &im, double c1, double c2, double &ra, double &dec) {
    const double u = c1 - im.crpix[0], v = c2 - im.crpix[1];
    const double x = (im.cd[0] * u + im.cd[1] * v) * PREP_D2R, y = (im.cd[2] * u + im.cd[3] * v) * PREP_D2R;
    const double den = im.cos0 - y * im.sin0, num = im.sin0 + y * im.cos0;
    ra = im.crval[0] + atan2(x, den) * PREP_R2D;
    const double hyp = hypot(x, den);
    // num cos0 - hyp sin0 = y - sin0 (hyp - den) = y - sin0 x^2 / (hyp + den), without cancellation
    dec = im.crval[1] + atan2(y - im.sin0 * ((x * x) / (hyp + den)), num * im.sin0 + hyp * im.cos0) * PREP_R2D;
}

__device__ __forceinline__ void world_to_pix(const PrepImg &im, double x, double y, double &pc1, double &pc2) {
    if (im.kind == CELESTE_PREP_WCS_TAN) { tan_world_to_pix(im, x, y, pc1, pc2); return; }
    const double d1 = x - im.w0[0], d2 = y - im.w0[1];
    pc1 = (im.J11 * d1 + im.J12 * d2) + im.p0[0];
    pc2 = (im.J21 * d1 + im.J22 * d2) + im.p0[1];
}

// J x = (c1, c2) - pix0 by LU with partial pivoting; (w1, w2) = x + world0
__device__ __forceinline__ void pix_to_world(const PrepImg &im, double c1, double c2, double &w1, double &w2) {
    if (im.kind == CELESTE_PREP_WCS_TAN) { tan_pix_to_world(im, c1, c2, w1, w2); return; }
    double a11 = im.J11, a12 = im.J12, a21 = im.J21, a22 = im.J22, b1 = c1 - im.p0[0], b2 = c2 - im.p0[1];
#if CELESTE_PREP_MUTANT == 6
    if (false) {
#else
    if (fabs(a21) > fabs(a11)) {
#endif
        double t = a11; a11 = a21; a21 = t;
        t = a12; a12 = a22; a22 = t;
        t = b1; b1 = b2; b2 = t;
    }
    const double l = a21 / a11;
    const double u = a22 - l * a12;
    const double x2 = (b2 - l * b1) / u;
    const double x1 = (b1 - a12 * x2) / a11;
    w1 = x1 + im.w0[0]; w2 = x2 + im.w0[1];
}

// the clamped box of radius r around (pc1, pc2): first row, last row, first column, last column
__device__ __forceinline__ int4 clamped_box(const PrepImg &im, double pc1, double pc2, double r) {
    int4 b;
    b.x = clampi(round_even(pc1 - r), 1, im.H + 1);
    b.y = clampi(round_even(pc1 + r), 0, im.H);
    b.z = clampi(round_even(pc2 - r), 1, im.W + 1);
#if CELESTE_PREP_MUTANT == 2
    b.w = clampi(round_even(pc2 + r), 0, im.W - 1);
#else
    b.w = clampi(round_even(pc2 + r), 0, im.W);
#endif
    return b;
}

__global__ void __launch_bounds__(PREP_BLOCK) prep_geometry_kernel(const PrepImg *imgs, int N, const celeste_prep_source_t *src, int64_t P,
                                                                   double radius_override, double reach, int dense, PrepConsts C,
                                                                   int32_t *keep, int4 *pbox, int32_t *err) {
    const int64_t p = (int64_t)blockIdx.x * PREP_BLOCK + threadIdx.x;
    if (p >= P) return;
    const int64_t s = p / N;
    const PrepImg &im = imgs[p - s * N];
    const celeste_prep_source_t &S = src[s];
    double pc1, pc2;
    world_to_pix(im, S.pos[0], S.pos[1], pc1, pc2);
#if CELESTE_PREP_MUTANT == 3
    const bool tried = dense || (pc1 > reach && pc1 < (double)(im.H + 1) + reach && pc2 > -reach && pc2 < (double)(im.W + 1) + reach);
#else
    const bool tried = dense || (pc1 > -reach && pc1 < (double)(im.H + 1) + reach && pc2 > -reach && pc2 < (double)(im.W + 1) + reach);
#endif
    if (!tried) { keep[p] = 0; pbox[p] = make_int4(1, 0, 1, 0); return; }
    double r = radius_override;
    // (a TAN image: pixel coordinates that are not finite are no error, the pair gets the empty box below)
    const bool off_plane = im.kind == CELESTE_PREP_WCS_TAN && !(fabs(pc1) < INFINITY && fabs(pc2) < INFINITY);
    bool bad = !off_plane && (!(pc1 == pc1) || !(pc2 == pc2));
    if (r != r) {     // choose_patch_radius, width_scale 1.2, max_radius 25
#if CELESTE_PREP_MUTANT == 5
        double ow = S.is_star ? 0.0 : S.gal_radius_px / 0.67;
#else
        double ow = S.is_star ? 0.0 : 1.2 * S.gal_radius_px / 0.67;
#endif
        ow += im.psf_width;
        const double f = S.flux[im.band - 1];
        if (!(f > 0.0)) bad = true;
        const double p90 = C.c1 / (C.c2 * ow);
        const double pe = im.eps / (20.0 * f);
#if CELESTE_PREP_MUTANT == 4
        const double pt = pe > p90 ? pe : p90;
#else
        const double pt = pe < p90 ? pe : p90;                 // min(pdf_90, epsilon / (20 flux))
#endif
        const double rhs = (log(pt) + C.c3) + log(ow);
        const double rq = sqrt((-2.0 * (ow * ow)) * rhs);
        r = 25.0 < rq ? 25.0 : rq;                             // min(radius_req, max_radius)
        if (!(r == r)) bad = true;
    }
    if (bad) { *err = 1; keep[p] = 0; pbox[p] = make_int4(1, 0, 1, 0); return; }
    if (off_plane) { keep[p] = dense ? 1 : 0; pbox[p] = make_int4(1, 0, 1, 0); return; }
    const int4 b = clamped_box(im, pc1, pc2, r);
    pbox[p] = b;
    keep[p] = (dense || (b.y >= b.x && b.w >= b.z)) ? 1 : 0;
}

struct PrepEntries {
    int32_t *source, *image, *sflag;
    int64_t *box;
    double *pc, *wc;
    int4 *ebox;
    unsigned long long *key;
    int32_t *val;
};

__global__ void __launch_bounds__(PREP_BLOCK) prep_compact_kernel(const PrepImg *imgs, int N, int64_t P, const int32_t *keep, const int32_t *off,
                                                                  const int4 *pbox, int want_stamps, PrepEntries E) {
    const int64_t p = (int64_t)blockIdx.x * PREP_BLOCK + threadIdx.x;
    if (p >= P || !keep[p]) return;
    const int64_t s = p / N;
    const int n = (int)(p - s * N);
    const PrepImg &im = imgs[n];
    const int32_t e = off[p];
    const int4 b = pbox[p];
    E.source[e] = (int32_t)s; E.image[e] = n;
    E.box[4 * (int64_t)e + 0] = b.x; E.box[4 * (int64_t)e + 1] = b.y; E.box[4 * (int64_t)e + 2] = b.z; E.box[4 * (int64_t)e + 3] = b.w;
    E.ebox[e] = b;
    const double c1 = (double)(b.x + b.y) / 2.0, c2 = (double)(b.z + b.w) / 2.0;
    E.pc[2 * (int64_t)e] = c1; E.pc[2 * (int64_t)e + 1] = c2;
    pix_to_world(im, c1, c2, E.wc[2 * (int64_t)e], E.wc[2 * (int64_t)e + 1]);
    const bool nonempty = b.y >= b.x && b.w >= b.z;
    E.key[e] = nonempty ? (((unsigned long long)n << 32) | (unsigned long long)(uint32_t)b.x) : ((unsigned long long)N << 32);
    E.val[e] = e;
    E.sflag[e] = (want_stamps && im.has_eig) ? 1 : 0;
}

// pixel_world_jacobian (wcs_utils.jl:36-51) at (c1, c2), which pix_to_world maps to (w1, w2): J11, J21, J12, J22
__device__ __forceinline__ void jacobian_at(const PrepImg &im, double c1, double c2, double w1, double w2, double *J) {
    if (im.kind != CELESTE_PREP_WCS_TAN) { J[0] = im.J11; J[1] = im.J21; J[2] = im.J12; J[3] = im.J22; return; }
    double s1, s2, a1, a2, b1, b2;
    tan_pix_to_world(im, c1 + 0.5, c2 + 0.5, s1, s2);
    const double t1 = fabs(s1 - w1), t2 = fabs(s2 - w2);
#if CELESTE_PREP_MUTANT == 7
    const double t = t1 < t2 ? t1 : t2;
#else
    const double t = t1 > t2 ? t1 : t2;
#endif
    tan_world_to_pix(im, w1 + t, w2, a1, a2);
    tan_world_to_pix(im, w1, w2 + t, b1, b2);
    J[0] = (a1 - c1) / t; J[1] = (a2 - c2) / t; J[2] = (b1 - c1) / t; J[3] = (b2 - c2) / t;
}

// one thread per entry (launched when an image is TAN): the Jacobian at its pixel centre
__global__ void __launch_bounds__(PREP_BLOCK) prep_jacobian_kernel(const PrepImg *imgs, const int32_t *image, const double *pc, const double *wc,
                                                                   int64_t E, double *jac) {
    const int64_t e = (int64_t)blockIdx.x * PREP_BLOCK + threadIdx.x;
    if (e >= E) return;
    double J[4];
    jacobian_at(imgs[image[e]], pc[2 * e], pc[2 * e + 1], wc[2 * e], wc[2 * e + 1], J);
    jac[4 * e] = J[0]; jac[4 * e + 1] = J[1]; jac[4 * e + 2] = J[2]; jac[4 * e + 3] = J[3];
}

// one wavefront per entry; lanes run along the contiguous direction of the plane
__global__ void __launch_bounds__(PREP_BLOCK) prep_active_kernel(const PrepImg *imgs, const int32_t *image, const int4 *ebox, int64_t E,
                                                                 int64_t *active) {
    const int64_t e = (int64_t)blockIdx.x * (PREP_BLOCK / 64) + (threadIdx.x >> 6);
    if (e >= E) return;
    const int lane = threadIdx.x & 63;
    const PrepImg &im = imgs[image[e]];
    const int4 b = ebox[e];
    const int nh = max(b.y - b.x + 1, 0), nw = max(b.w - b.z + 1, 0);
    int cnt = 0;
#if CELESTE_PREP_MUTANT == 8
    const int nan_counts = 1;
#else
    const int nan_counts = 0;
#endif
    if (nh > 0 && nw > 0) {
        const float *base = im.pix + (int64_t)(b.x - 1) * im.sh + (int64_t)(b.z - 1) * im.sw;
        if (im.sw == 1) {
            for (int h = 0; h < nh; ++h)
                for (int w = lane; w < nw; w += 64) { const float v = base[(int64_t)h * im.sh + w]; cnt += (v == v) ? 1 : nan_counts; }
        } else {
            for (int w = 0; w < nw; ++w)
                for (int h = lane; h < nh; h += 64) { const float v = base[(int64_t)h * im.sh + (int64_t)w * im.sw]; cnt += (v == v) ? 1 : nan_counts; }
        }
    }
    for (int d = 32; d > 0; d >>= 1) cnt += __shfl_down(cnt, d, 64);
    if (lane == 0) active[e] = cnt;
}

__global__ void __launch_bounds__(PREP_BLOCK) prep_gather_kernel(const int32_t *val, const int4 *ebox, const int32_t *source, int64_t E,
                                                                 int4 *sbox, int32_t *ssrc) {
    const int64_t i = (int64_t)blockIdx.x * PREP_BLOCK + threadIdx.x;
    if (i >= E) return;
    const int32_t e = val[i];
    sbox[i] = ebox[e]; ssrc[i] = source[e];
}

__device__ __forceinline__ int64_t lower_bound_u64(const unsigned long long *a, int64_t n, unsigned long long x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Sorted position i: the entries of the same image whose first row lies in [first row - max_rows + 1, last row] and whose box
// overlaps.  raw == nullptr: count into cnt[entry]; else write the overlapping entries' sources at roff[entry].
__global__ void __launch_bounds__(PREP_BLOCK) prep_nbr_kernel(const unsigned long long *key, const int32_t *val, const int4 *sbox,
                                                              const int32_t *ssrc, int64_t E, int N, int max_rows, int64_t *cnt,
                                                              const int64_t *roff, int32_t *raw) {
    const int64_t i = (int64_t)blockIdx.x * PREP_BLOCK + threadIdx.x;
    if (i >= E) return;
    const unsigned long long k = key[i];
    const int32_t e = val[i];
    if ((k >> 32) >= (unsigned long long)N) { if (!raw) cnt[e] = 0; return; }
    const int4 b = sbox[i];
    const unsigned long long hi32 = k & 0xffffffff00000000ull;
#if CELESTE_PREP_MUTANT == 10
    const int64_t first = max((int64_t)b.x - max_rows + 2, (int64_t)0);
#else
    const int64_t first = max((int64_t)b.x - max_rows + 1, (int64_t)0);
#endif
    const int64_t lo = lower_bound_u64(key, E, hi32 | (unsigned long long)first);
    const int64_t hi = lower_bound_u64(key, E, hi32 | (unsigned long long)((int64_t)b.y + 1));
    int64_t c = 0;
    const int64_t at = raw ? roff[e] : 0;
    for (int64_t j = lo; j < hi; ++j) {
        if (j == i) continue;
        const int4 o = sbox[j];
#if CELESTE_PREP_MUTANT == 9
        if (o.y > b.x && o.z <= b.w && b.z <= o.w) {
#else
        if (o.y >= b.x && o.z <= b.w && b.z <= o.w) {     // (o.x <= b.y by the range)
#endif
            if (raw) raw[at + c] = ssrc[j];
            ++c;
        }
    }
    if (!raw) cnt[e] = c;
}

// soff[s] = the first raw link of source s (entries are sorted by source), soff[S] = R
__global__ void __launch_bounds__(PREP_BLOCK) prep_source_ranges_kernel(const int32_t *source, const int64_t *roff, int64_t E, int64_t S, int64_t R,
                                                                        int32_t *soff) {
    const int64_t s = (int64_t)blockIdx.x * PREP_BLOCK + threadIdx.x;
    if (s > S) return;
    int64_t lo = 0, hi = E;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)source[mid] < s) lo = mid + 1; else hi = mid;
    }
    soff[s] = (int32_t)(lo < E ? roff[lo] : R);
}

// sorted links of source s without repeats: out == nullptr counts into ucnt[s] (ucnt[S] = 0), else writes them at noff[s]
__global__ void __launch_bounds__(PREP_BLOCK) prep_unique_kernel(const int32_t *sorted, const int32_t *soff, int64_t S, int64_t *ucnt,
                                                                 const int64_t *noff, int32_t *out) {
    const int64_t s = (int64_t)blockIdx.x * PREP_BLOCK + threadIdx.x;
    if (s > S) return;
    if (s == S) { if (!out) ucnt[s] = 0; return; }
    const int32_t a = soff[s], b = soff[s + 1];
    int64_t c = 0;
    const int64_t at = out ? noff[s] : 0;
    for (int32_t i = a; i < b; ++i)
#if CELESTE_PREP_MUTANT == 11
        if (true) {
#else
        if (i == a || sorted[i] != sorted[i - 1]) {
#endif
            if (out) out[at + c] = sorted[i];
            ++c;
        }
    if (!out) ucnt[s] = c;
}

__global__ void __launch_bounds__(PREP_BLOCK) prep_stamp_kernel(const PrepImg *imgs, const int32_t *image, const double *pc, const int32_t *sflag,
                                                                const int32_t *sidx, int32_t *stamp, double *stamps) {
    const int64_t e = blockIdx.x;
    if (!sflag[e]) { if (threadIdx.x == 0) stamp[e] = -1; return; }     // (uniform over the workgroup)
    const PrepImg &im = imgs[image[e]];
    __shared__ double w[CELESTE_PREP_MAX_NK];
    const int nk = im.nk;
    if ((int)threadIdx.x < nk) {
        const int k = threadIdx.x;
#if CELESTE_PREP_MUTANT == 12
        const double tx = 0.001 * pc[2 * e], ty = 0.001 * (pc[2 * e + 1] - 1.0);
#else
        const double tx = 0.001 * (pc[2 * e] - 1.0), ty = 0.001 * (pc[2 * e + 1] - 1.0);
#endif
        double acc = 0.0, px = 1.0;
        for (int i = 0; i < im.ni; ++i) {
            double py = 1.0;
            for (int j = 0; j < im.nj; ++j) {
#if CELESTE_PREP_MUTANT == 13
                acc += im.cmat[((int64_t)j * im.ni + i) * nk + k] * (px * py);
#else
                acc += im.cmat[((int64_t)i * im.nj + j) * nk + k] * (px * py);
#endif
                py *= ty;
            }
            px *= tx;
        }
        w[k] = acc;
    }
    __syncthreads();
    const int32_t si = sidx[e];
    if (threadIdx.x == 0) stamp[e] = si;
    double *out = stamps + (int64_t)si * PREP_NPIX;
    for (int p = threadIdx.x; p < PREP_NPIX; p += PREP_BLOCK) {
        double acc = 0.0;
        for (int k = 0; k < nk; ++k) acc += im.rrows[(int64_t)p * nk + k] * w[k];
        out[p] = acc;
    }
}

__device__ __forceinline__ uint32_t float_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// k-th smallest (0-based) of the values of vals[0 .. tot) that are not NaN: 8-bit radix select on the ordered keys
// (integer histogram in LDS: the counts do not depend on the order of the atomics)
__device__ float sky_select(const float *vals, int tot, int k, uint32_t *hist, uint32_t *word) {
    uint32_t prefix = 0, pmask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[threadIdx.x] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < tot; i += PREP_BLOCK) {
            const float v = vals[i];
            if (!(v == v)) continue;
            const uint32_t key = float_key(v);
            if ((key & pmask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t cum = 0;
            int b = 0;
            for (; b < 255; ++b) {
                if (cum + hist[b] > (uint32_t)k) break;
                cum += hist[b];
            }
            word[0] = (uint32_t)b;
            word[1] = (uint32_t)k - cum;
        }
        __syncthreads();
        prefix |= word[0] << shift;
        pmask |= 255u << shift;
        k = (int)word[1];
        __syncthreads();
    }
    return key_float(prefix);
}

__global__ void __launch_bounds__(PREP_BLOCK) prep_sky_kernel(const PrepImg *imgs, int n_img, const double *pos, uint8_t *flags) {
    __shared__ float vals[PREP_SKY_SIDE * PREP_SKY_SIDE];
    __shared__ uint32_t hist[PREP_BLOCK];
    __shared__ uint32_t word[2];
    __shared__ uint32_t n_valid;
    const PrepImg &im = imgs[n_img];
    const int64_t i = blockIdx.x;
    double pc1, pc2;
    world_to_pix(im, pos[2 * i], pos[2 * i + 1], pc1, pc2);
    if (im.kind == CELESTE_PREP_WCS_TAN && !(fabs(pc1) < INFINITY && fabs(pc2) < INFINITY)) {    // (uniform over the workgroup)
        if (threadIdx.x == 0) flags[i] = 0;
        return;
    }
    const int4 b = clamped_box(im, pc1, pc2, PREP_SKY_RADIUS);
    const int nh = min(max(b.y - b.x + 1, 0), PREP_SKY_SIDE), nw = min(max(b.w - b.z + 1, 0), PREP_SKY_SIDE);
    const int tot = nh * nw;
    if (threadIdx.x == 0) n_valid = 0;
    __syncthreads();
    uint32_t mine = 0;
    if (tot > 0) {
        const float *base = im.pix + (int64_t)(b.x - 1) * im.sh + (int64_t)(b.z - 1) * im.sw;
        const bool rows = im.sw == 1;      // lanes along a row of the box, else along a column
        for (int t = threadIdx.x; t < tot; t += PREP_BLOCK) {
            const int h = rows ? t / nw : t % nh, w = rows ? t % nw : t / nh;
            const float v = base[(int64_t)h * im.sh + (int64_t)w * im.sw];
            vals[t] = v;
            mine += (v == v) ? 1u : 0u;
        }
    }
    if (mine) atomicAdd(&n_valid, mine);
    __syncthreads();
    const int n = (int)n_valid;
    if (n == 0) { if (threadIdx.x == 0) flags[i] = 0; return; }     // (uniform over the workgroup)
    const int k = n / 2;
    float med = sky_select(vals, tot, k, hist, word);
    if ((n & 1) == 0) {
        const float lo = sky_select(vals, tot, k - 1, hist, word);
#if CELESTE_PREP_MUTANT == 14
        med = lo < med ? med : lo;
#else
        med = (lo + med) * 0.5f;
#endif
    }
    if (threadIdx.x == 0) {
        const int h = clampi(round_even(pc1), 1, im.H), w = clampi(round_even(pc2), 1, im.W);
#if CELESTE_PREP_MUTANT == 16
        const double claimed = (double)im.sky[(int64_t)(h - 1) * im.ksh + (int64_t)(w - 1) * im.ksw] * (double)im.nelec[min(w, im.H) - 1];
#else
        const double claimed = (double)im.sky[(int64_t)(h - 1) * im.ksh + (int64_t)(w - 1) * im.ksw] * (double)im.nelec[h - 1];
#endif
#if CELESTE_PREP_MUTANT == 15
        flags[i] = (claimed + 5.0 <= (double)med) ? 1 : 0;
#else
        flags[i] = (claimed + 5.0 < (double)med) ? 1 : 0;
#endif
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
#define PREP_HIP(expr) do { if ((expr) != hipSuccess) { (void)hipGetLastError(); return CELESTE_PREP_ERR_HIP; } } while (0)

static std::mutex g_mu;                 // one call at a time
static float g_last_ms[CELESTE_PREP_N_STAGES] = {0, 0, 0, 0, 0};
static float g_det_ms[CELESTE_PREP_DETECTED_N_STAGES] = {0, 0, 0, 0, 0, 0};   // of the last call, when it was celeste_prep_detected

// One stream per device, made on first use and kept for the life of the process (calls are serialised by g_mu): the HIP
// runtime has been seen writing into a stream object after hipStreamDestroy freed it (profiles/r08_stale_stream_write.md),
// so this library destroys none.
static hipStream_t g_streams[64] = {};

// one page-locked block is kept between calls: page-locking costs more than the kernels of a small call
static void *g_spare = nullptr;
static size_t g_spare_bytes = 0;

struct celeste_prep_images {
    int device = 0;
    int32_t n_images = 0;
    int sky_image = -1;                 // the first image of band 4
    int any_eig = 0;
    int any_tan = 0;                    // celeste_prep_images_set_wcs gave an image the kind TAN
    std::vector<PrepImg> host;          // (device pointers inside)
    PrepImg *d_imgs = nullptr;
    std::vector<void *> bufs;
};

struct celeste_prep_result {
    void *block = nullptr;              // page-locked
    size_t bytes = 0;
    celeste_prep_table_t table;
    const double *jac = nullptr;        // [E][4] inside block; null when no image of the handle is TAN
    bool has_catalog = false;
    celeste_prep_catalog_t catalog;
};

static int prep_stream(int device, hipStream_t *out) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { (void)hipGetLastError(); return CELESTE_PREP_ERR_NO_DEVICE; }
    if (device >= count) return CELESTE_PREP_ERR_INVALID_ARG;
    PREP_HIP(hipSetDevice(device));
    if (!g_streams[device]) PREP_HIP(hipStreamCreateWithFlags(&g_streams[device], hipStreamNonBlocking));
    *out = g_streams[device];
    return CELESTE_PREP_OK;
}

// the device buffers and the events of one call
struct PrepCall {
    std::vector<void *> bufs;
    hipStream_t stream = nullptr;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t dev[3] = {nullptr, nullptr, nullptr};     // celeste_prep_detected's own stages
    ~PrepCall() {
        if (stream) (void)hipStreamSynchronize(stream);
        for (auto e : ev) if (e) (void)hipEventDestroy(e);
        for (auto e : dev) if (e) (void)hipEventDestroy(e);
        for (void *p : bufs) (void)hipFree(p);
    }
    int open(int device) {
        int st = prep_stream(device, &stream);
        if (st) { stream = nullptr; return st; }
        for (auto &e : ev) PREP_HIP(hipEventCreate(&e));
        return CELESTE_PREP_OK;
    }
    int open_detected(int device) {
        int st = open(device);
        if (st) return st;
        for (auto &e : dev) PREP_HIP(hipEventCreate(&e));
        return CELESTE_PREP_OK;
    }
    template <class T> int alloc(T **dst, size_t n) {
        void *p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); return CELESTE_PREP_ERR_ALLOC; }
        bufs.push_back(p);
        *dst = (T *)p;
        return CELESTE_PREP_OK;
    }
};

static unsigned blocks_for(int64_t n) { return (unsigned)std::max<int64_t>((n + PREP_BLOCK - 1) / PREP_BLOCK, 1); }

static int bits_for(uint64_t max_value) {
    int b = 1;
    while (b < 64 && (max_value >> b)) ++b;
    return b;
}

extern "C" int celeste_prep_version(void) { return CELESTE_PREP_ABI_VERSION; }

extern "C" const char *celeste_prep_strerror(int status) {
    switch (status) {
        case CELESTE_PREP_OK: return "ok";
        case CELESTE_PREP_ERR_INVALID_ARG: return "invalid argument";
        case CELESTE_PREP_ERR_NO_DEVICE: return "no HIP device (there is no CPU fallback)";
        case CELESTE_PREP_ERR_HIP: return "HIP runtime error";
        case CELESTE_PREP_ERR_ALLOC: return "allocation failed";
        default: return "unknown status";
    }
}

extern "C" int celeste_prep_last_ms(float ms[CELESTE_PREP_N_STAGES]) {
    if (!ms) return CELESTE_PREP_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_mu);
    for (int i = 0; i < CELESTE_PREP_N_STAGES; ++i) ms[i] = g_last_ms[i];
    return CELESTE_PREP_OK;
}

static bool plane_strides_ok(int64_t sh, int64_t sw, int32_t H, int32_t W) {
    return (sw == 1 && sh == W) || (sh == 1 && sw == H);
}

static void images_free(celeste_prep_images *h) {
    for (void *p : h->bufs) (void)hipFree(p);
    delete h;
}

template <class T> static int images_up(celeste_prep_images *h, hipStream_t stream, const T **dst, const T *src, size_t n) {
    void *p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); return CELESTE_PREP_ERR_ALLOC; }
    h->bufs.push_back(p);
    PREP_HIP(hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyHostToDevice, stream));
    *dst = (const T *)p;
    return CELESTE_PREP_OK;
}

extern "C" int celeste_prep_images_create(int device, int32_t n_images, const celeste_prep_image_t *images, celeste_prep_images_t **handle) {
    // ---- arguments: everything is checked before the first HIP call
    if (!handle) return CELESTE_PREP_ERR_INVALID_ARG;
    *handle = nullptr;
    if (device < 0 || device >= 64 || n_images <= 0 || !images) return CELESTE_PREP_ERR_INVALID_ARG;
    for (int n = 0; n < n_images; ++n) {
        const celeste_prep_image_t &im = images[n];
        if (im.H <= 0 || im.W <= 0 || (int64_t)im.H * im.W > 0x7fffffff || im.band < 1 || im.band > 5 || !im.pixels || !im.nelec_per_nmgy ||
            !plane_strides_ok(im.stride_h, im.stride_w, im.H, im.W))
            return CELESTE_PREP_ERR_INVALID_ARG;
        if (im.sky && !plane_strides_ok(im.sky_stride_h, im.sky_stride_w, im.H, im.W)) return CELESTE_PREP_ERR_INVALID_ARG;
        for (int k = 0; k < 4; ++k) if (!std::isfinite(im.wcs_jacobian[k])) return CELESTE_PREP_ERR_INVALID_ARG;
        for (int k = 0; k < 2; ++k) if (!std::isfinite(im.wcs_world0[k]) || !std::isfinite(im.wcs_pix0[k])) return CELESTE_PREP_ERR_INVALID_ARG;
        if (im.wcs_jacobian[0] * im.wcs_jacobian[3] - im.wcs_jacobian[1] * im.wcs_jacobian[2] == 0.0) return CELESTE_PREP_ERR_INVALID_ARG;
        if (im.rrows) {
            if (im.rnrow != CELESTE_PREP_STAMP || im.rncol != CELESTE_PREP_STAMP || !im.cmat || im.ni < 1 || im.ni > CELESTE_PREP_MAX_POLY ||
                im.nj < 1 || im.nj > CELESTE_PREP_MAX_POLY || im.nk < 1 || im.nk > CELESTE_PREP_MAX_NK)
                return CELESTE_PREP_ERR_INVALID_ARG;
        }
    }
    bool band4_seen = false;
    for (int n = 0; n < n_images && !band4_seen; ++n)
        if (images[n].band == 4) { band4_seen = true; if (!images[n].sky) return CELESTE_PREP_ERR_INVALID_ARG; }

    // ---- the device
    std::lock_guard<std::mutex> lk(g_mu);
    hipStream_t stream;
    int st = prep_stream(device, &stream);
    if (st) return st;
    celeste_prep_images *h = new celeste_prep_images;
    h->device = device; h->n_images = n_images;
    h->host.resize((size_t)n_images);
    for (int n = 0; n < n_images; ++n) {
        const celeste_prep_image_t &im = images[n];
        PrepImg &D = h->host[(size_t)n];
        memset(&D, 0, sizeof D);
        const size_t np = (size_t)im.H * im.W;
        D.H = im.H; D.W = im.W; D.band = im.band; D.sh = im.stride_h; D.sw = im.stride_w;
        D.J11 = im.wcs_jacobian[0]; D.J21 = im.wcs_jacobian[1]; D.J12 = im.wcs_jacobian[2]; D.J22 = im.wcs_jacobian[3];
        for (int k = 0; k < 2; ++k) { D.w0[k] = im.wcs_world0[k]; D.p0[k] = im.wcs_pix0[k]; }
        D.psf_width = im.psf_width; D.eps = im.epsilon;
        if ((st = images_up(h, stream, &D.pix, im.pixels, np)) || (st = images_up(h, stream, &D.nelec, im.nelec_per_nmgy, (size_t)im.H))) break;
        if (im.band == 4 && h->sky_image < 0) {
            h->sky_image = n;
            D.ksh = im.sky_stride_h; D.ksw = im.sky_stride_w;
            if ((st = images_up(h, stream, &D.sky, im.sky, np))) break;
        }
        if (im.rrows) {
            D.has_eig = 1; D.ni = im.ni; D.nj = im.nj; D.nk = im.nk;
            h->any_eig = 1;
            if ((st = images_up(h, stream, &D.rrows, im.rrows, (size_t)PREP_NPIX * im.nk)) ||
                (st = images_up(h, stream, &D.cmat, im.cmat, (size_t)im.ni * im.nj * im.nk)))
                break;
        }
    }
    if (!st) {
        const PrepImg *d = nullptr;
        st = images_up(h, stream, &d, h->host.data(), h->host.size());
        h->d_imgs = const_cast<PrepImg *>(d);
    }
    if (!st && hipStreamSynchronize(stream) != hipSuccess) { (void)hipGetLastError(); st = CELESTE_PREP_ERR_HIP; }
    if (st) {
        (void)hipStreamSynchronize(stream);
        images_free(h);
        return st;
    }
    *handle = h;
    return CELESTE_PREP_OK;
}

extern "C" void celeste_prep_images_destroy(celeste_prep_images_t *handle) {
    if (!handle) return;
    std::lock_guard<std::mutex> lk(g_mu);
    if (hipSetDevice(handle->device) == hipSuccess && g_streams[handle->device]) (void)hipStreamSynchronize(g_streams[handle->device]);
    images_free(handle);
}

extern "C" int celeste_prep_wcs_check(int32_t n_images, const celeste_prep_wcs_t *wcs) {
    if (n_images <= 0 || !wcs) return CELESTE_PREP_ERR_INVALID_ARG;
    for (int n = 0; n < n_images; ++n) {
        const celeste_prep_wcs_t &w = wcs[n];
        if (w.kind == CELESTE_PREP_WCS_AFFINE) continue;
        if (w.kind != CELESTE_PREP_WCS_TAN) return CELESTE_PREP_ERR_INVALID_ARG;
        for (int k = 0; k < 2; ++k) if (!std::isfinite(w.crval[k]) || !std::isfinite(w.crpix[k])) return CELESTE_PREP_ERR_INVALID_ARG;
        for (int k = 0; k < 4; ++k) if (!std::isfinite(w.cd[k])) return CELESTE_PREP_ERR_INVALID_ARG;
        const double det = w.cd[0] * w.cd[3] - w.cd[1] * w.cd[2];
        if (det == 0.0 || !std::isfinite(det) || std::fabs(w.crval[1]) > 90.0) return CELESTE_PREP_ERR_INVALID_ARG;
    }
    return CELESTE_PREP_OK;
}

extern "C" int celeste_prep_images_set_wcs(celeste_prep_images_t *handle, int32_t n_images, const celeste_prep_wcs_t *wcs) {
    if (!handle) return CELESTE_PREP_ERR_INVALID_ARG;
    int st = celeste_prep_wcs_check(n_images, wcs);
    if (st) return st;
    if (n_images != handle->n_images) return CELESTE_PREP_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_mu);
    hipStream_t stream;
    if ((st = prep_stream(handle->device, &stream))) return st;
    int any_tan = 0;
    for (int n = 0; n < n_images; ++n) {
        const celeste_prep_wcs_t &w = wcs[n];
        PrepImg &D = handle->host[(size_t)n];
        D.kind = w.kind;
        if (w.kind != CELESTE_PREP_WCS_TAN) continue;
        any_tan = 1;
        const double det = w.cd[0] * w.cd[3] - w.cd[1] * w.cd[2];
        for (int k = 0; k < 2; ++k) { D.crval[k] = w.crval[k]; D.crpix[k] = w.crpix[k]; }
        for (int k = 0; k < 4; ++k) D.cd[k] = w.cd[k];
        D.ci[0] = w.cd[3] / det; D.ci[1] = -w.cd[1] / det; D.ci[2] = -w.cd[2] / det; D.ci[3] = w.cd[0] / det;
        const double d0 = w.crval[1] * PREP_D2R;
        D.sin0 = std::sin(d0); D.cos0 = std::cos(d0);
    }
    PREP_HIP(hipStreamSynchronize(stream));       // no call of this handle is in flight
    PREP_HIP(hipMemcpyAsync(handle->d_imgs, handle->host.data(), handle->host.size() * sizeof(PrepImg), hipMemcpyHostToDevice, stream));
    PREP_HIP(hipStreamSynchronize(stream));
    handle->any_tan = any_tan;
    return CELESTE_PREP_OK;
}

// a page-locked block of `bytes` (from the spare one when it is large enough)
static void *pinned_take(size_t bytes, size_t *got) {
    if (g_spare && g_spare_bytes >= bytes) {
        void *p = g_spare;
        *got = g_spare_bytes;
        g_spare = nullptr; g_spare_bytes = 0;
        return p;
    }
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    *got = bytes;
    return p;
}

static void pinned_give(void *p, size_t bytes) {
    if (!p) return;
    if (bytes > g_spare_bytes && bytes <= ((size_t)1 << 30)) {
        if (g_spare) (void)hipHostFree(g_spare);
        g_spare = p; g_spare_bytes = bytes;
    } else {
        (void)hipHostFree(p);
    }
}

extern "C" int celeste_prep_result_get(const celeste_prep_result_t *result, celeste_prep_table_t *table) {
    if (!result || !table) return CELESTE_PREP_ERR_INVALID_ARG;
    *table = result->table;
    return CELESTE_PREP_OK;
}

extern "C" int celeste_prep_result_get_jacobians(const celeste_prep_result_t *result, const double **jac) {
    if (!result || !jac) return CELESTE_PREP_ERR_INVALID_ARG;
    *jac = result->jac;
    return CELESTE_PREP_OK;
}

extern "C" void celeste_prep_result_destroy(celeste_prep_result_t *result) {
    if (!result) return;
    std::lock_guard<std::mutex> lk(g_mu);
    pinned_give(result->block, result->bytes);
    delete result;
}

static size_t carve(size_t *at, size_t bytes) {
    const size_t o = *at;
    *at = (o + bytes + 255) / 256 * 256;
    return o;
}

// what a geometry kernel leaves for the P pairs; err[0]: an invalid pair was met, err[1]: the largest number of rows of a box
struct PrepPairs {
    int32_t *keep = nullptr, *off = nullptr, *err = nullptr;
    int4 *pbox = nullptr;
    int alloc(PrepCall &call, int64_t P) {
        int st;
        if ((st = call.alloc(&keep, (size_t)P)) || (st = call.alloc(&off, (size_t)P)) || (st = call.alloc(&pbox, (size_t)P)) ||
            (st = call.alloc(&err, 2)))
            return st;
        return CELESTE_PREP_OK;
    }
};

struct PrepExtra { const void *dptr; size_t bytes; size_t at; const char *host; };

static int prep_table_stages(celeste_prep_images_t *handle, PrepCall &call, int64_t S, int64_t P, const PrepPairs &G, int max_rows,
                             bool want_stamps, PrepExtra *extra, int n_extra, celeste_prep_result_t **result);

extern "C" int celeste_prep_patches(celeste_prep_images_t *handle, int64_t n_sources, const celeste_prep_source_t *sources,
                                    double radius_override_pix, uint32_t flags, celeste_prep_result_t **result) {
    // ---- arguments
    if (!result) return CELESTE_PREP_ERR_INVALID_ARG;
    *result = nullptr;
    if (!handle || n_sources < 0 || (n_sources && !sources) || (flags & ~(uint32_t)(CELESTE_PREP_FLAG_DENSE | CELESTE_PREP_FLAG_STAMPS)))
        return CELESTE_PREP_ERR_INVALID_ARG;
    const bool has_override = !std::isnan(radius_override_pix);
    if (has_override && !(radius_override_pix >= 0.0 && radius_override_pix <= 1.0e6)) return CELESTE_PREP_ERR_INVALID_ARG;
    const int N = handle->n_images;
    const int64_t S = n_sources, P = S * N;
    if (P > 0x7fffffff) return CELESTE_PREP_ERR_INVALID_ARG;
    for (int64_t s = 0; s < S; ++s)
        if (!std::isfinite(sources[s].pos[0]) || !std::isfinite(sources[s].pos[1])) return CELESTE_PREP_ERR_INVALID_ARG;
    const bool dense = flags & CELESTE_PREP_FLAG_DENSE, want_stamps = (flags & CELESTE_PREP_FLAG_STAMPS) != 0;
    const double radius = has_override ? radius_override_pix : 25.0;
    const double reach = radius + 1.0;
    const int max_rows = (int)std::floor(2.0 * radius) + 3;     // rint(pc + r) - rint(pc - r) + 1 <= 2 r + 2
    PrepConsts C;
    C.c1 = std::exp(-0.5 * std::pow(1.64, 2.0)); C.c2 = std::sqrt(2.0 * M_PI); C.c3 = 0.5 * std::log(2.0 * M_PI);

    std::lock_guard<std::mutex> lk(g_mu);
    PrepCall call;
    int st = call.open(handle->device);
    if (st) return st;
    hipStream_t q = call.stream;
    for (float &m : g_last_ms) m = 0.0f;
    for (float &m : g_det_ms) m = 0.0f;

    // ---- geometry
    PrepPairs G;
    celeste_prep_source_t *d_src;
    if ((st = call.alloc(&d_src, (size_t)S)) || (st = G.alloc(call, P))) return st;
    PREP_HIP(hipEventRecord(call.ev[0], q));
    if (P > 0) {
        PREP_HIP(hipMemcpyAsync(d_src, sources, (size_t)S * sizeof(celeste_prep_source_t), hipMemcpyHostToDevice, q));
        PREP_HIP(hipMemsetAsync(G.err, 0, 2 * sizeof(int32_t), q));
        hipLaunchKernelGGL(prep_geometry_kernel, dim3(blocks_for(P)), dim3(PREP_BLOCK), 0, q, handle->d_imgs, N, d_src, P,
                           has_override ? radius_override_pix : (double)NAN, reach, dense ? 1 : 0, C, G.keep, G.pbox, G.err);
        PREP_HIP(hipGetLastError());
    }
    return prep_table_stages(handle, call, S, P, G, max_rows, want_stamps, nullptr, 0, result);
}

// The stages behind the geometry kernel, which has filled G for the P = S N pairs (call.ev[0] lies in front of it): compaction,
// active pixels, neighbours, stamps, and the table in one page-locked block.  max_rows: no box has more rows; < 0: the largest
// number of rows is read from G.err[1].  extra: n_extra device arrays that go into the same block (a catalog's).
static int prep_table_stages(celeste_prep_images_t *handle, PrepCall &call, int64_t S, int64_t P, const PrepPairs &G, int max_rows,
                             bool want_stamps, PrepExtra *extra, int n_extra, celeste_prep_result_t **result) {
    const int N = handle->n_images;
    hipStream_t q = call.stream;
    int st;
    int32_t *d_keep = G.keep, *d_off = G.off, *d_err = G.err; int4 *d_pbox = G.pbox;
    int64_t E = 0;
    if (P > 0) {
        size_t tb = 0;
        PREP_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, d_keep, d_off, (int)P, q));
        char *d_tmp;
        if ((st = call.alloc(&d_tmp, tb))) return st;
        PREP_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp, tb, d_keep, d_off, (int)P, q));
        int32_t last[4] = {0, 0, 0, 0};
        PREP_HIP(hipMemcpyAsync(&last[0], d_off + (P - 1), sizeof(int32_t), hipMemcpyDeviceToHost, q));
        PREP_HIP(hipMemcpyAsync(&last[1], d_keep + (P - 1), sizeof(int32_t), hipMemcpyDeviceToHost, q));
        PREP_HIP(hipMemcpyAsync(&last[2], d_err, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, q));
        PREP_HIP(hipStreamSynchronize(q));
        if (last[2]) return CELESTE_PREP_ERR_INVALID_ARG;       // a tried pair without a positive flux, or a NaN radius
        E = (int64_t)last[0] + last[1];
        if (max_rows < 0) max_rows = std::max(last[3], 1);
    }
    PrepEntries D;
    memset(&D, 0, sizeof D);
    int64_t *d_active = nullptr;
    if ((st = call.alloc(&D.source, (size_t)E)) || (st = call.alloc(&D.image, (size_t)E)) || (st = call.alloc(&D.sflag, (size_t)E)) ||
        (st = call.alloc(&D.box, (size_t)E * 4)) || (st = call.alloc(&D.pc, (size_t)E * 2)) || (st = call.alloc(&D.wc, (size_t)E * 2)) ||
        (st = call.alloc(&D.ebox, (size_t)E)) || (st = call.alloc(&D.key, (size_t)E)) || (st = call.alloc(&D.val, (size_t)E)) ||
        (st = call.alloc(&d_active, (size_t)E)))
        return st;
    if (E > 0) {
        hipLaunchKernelGGL(prep_compact_kernel, dim3(blocks_for(P)), dim3(PREP_BLOCK), 0, q, handle->d_imgs, N, P, d_keep, d_off, d_pbox,
                           want_stamps ? 1 : 0, D);
        PREP_HIP(hipGetLastError());
    }
    double *d_jac = nullptr;
    if (handle->any_tan) {
        if ((st = call.alloc(&d_jac, (size_t)E * 4))) return st;
        if (E > 0) {
            hipLaunchKernelGGL(prep_jacobian_kernel, dim3(blocks_for(E)), dim3(PREP_BLOCK), 0, q, handle->d_imgs, D.image, D.pc, D.wc, E, d_jac);
            PREP_HIP(hipGetLastError());
        }
    }
    PREP_HIP(hipEventRecord(call.ev[1], q));

    // ---- active pixels
    if (E > 0) {
        hipLaunchKernelGGL(prep_active_kernel, dim3((unsigned)((E + 3) / 4)), dim3(PREP_BLOCK), 0, q, handle->d_imgs, D.image, D.ebox, E, d_active);
        PREP_HIP(hipGetLastError());
    }
    PREP_HIP(hipEventRecord(call.ev[2], q));

    // ---- neighbours: entries by (image, first row); count, scan; [the host sizes the link list]; fill, sort per source, unique
    unsigned long long *d_key2; int32_t *d_val2, *d_ssrc, *d_sidx; int4 *d_sbox; int64_t *d_cnt, *d_roff;
    if ((st = call.alloc(&d_key2, (size_t)E)) || (st = call.alloc(&d_val2, (size_t)E)) || (st = call.alloc(&d_ssrc, (size_t)E)) ||
        (st = call.alloc(&d_sbox, (size_t)E)) || (st = call.alloc(&d_cnt, (size_t)E)) || (st = call.alloc(&d_roff, (size_t)E)) ||
        (st = call.alloc(&d_sidx, (size_t)E)))
        return st;
    int64_t R = 0, n_stamps = 0;
    if (E > 0) {
        const int end_bit = 32 + bits_for((uint64_t)N);
        size_t tb = 0, tb2 = 0, tb3 = 0;
        PREP_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, D.key, d_key2, D.val, d_val2, (int)E, 0, end_bit, q));
        PREP_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb2, d_cnt, d_roff, (int)E, q));
        PREP_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb3, D.sflag, d_sidx, (int)E, q));
        char *d_tmp;
        if ((st = call.alloc(&d_tmp, std::max(tb, std::max(tb2, tb3))))) return st;
        PREP_HIP(hipcub::DeviceRadixSort::SortPairs(d_tmp, tb, D.key, d_key2, D.val, d_val2, (int)E, 0, end_bit, q));
        hipLaunchKernelGGL(prep_gather_kernel, dim3(blocks_for(E)), dim3(PREP_BLOCK), 0, q, d_val2, D.ebox, D.source, E, d_sbox, d_ssrc);
        PREP_HIP(hipGetLastError());
        hipLaunchKernelGGL(prep_nbr_kernel, dim3(blocks_for(E)), dim3(PREP_BLOCK), 0, q, d_key2, d_val2, d_sbox, d_ssrc, E, N, max_rows, d_cnt,
                           (const int64_t *)nullptr, (int32_t *)nullptr);
        PREP_HIP(hipGetLastError());
        PREP_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp, tb2, d_cnt, d_roff, (int)E, q));
        PREP_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp, tb3, D.sflag, d_sidx, (int)E, q));
        int64_t lastr[2] = {0, 0};
        int32_t lasts[2] = {0, 0};
        PREP_HIP(hipMemcpyAsync(&lastr[0], d_roff + (E - 1), sizeof(int64_t), hipMemcpyDeviceToHost, q));
        PREP_HIP(hipMemcpyAsync(&lastr[1], d_cnt + (E - 1), sizeof(int64_t), hipMemcpyDeviceToHost, q));
        PREP_HIP(hipMemcpyAsync(&lasts[0], d_sidx + (E - 1), sizeof(int32_t), hipMemcpyDeviceToHost, q));
        PREP_HIP(hipMemcpyAsync(&lasts[1], D.sflag + (E - 1), sizeof(int32_t), hipMemcpyDeviceToHost, q));
        PREP_HIP(hipStreamSynchronize(q));
        R = lastr[0] + lastr[1];
        n_stamps = (int64_t)lasts[0] + lasts[1];
        if (R > 0x7fffffff) return CELESTE_PREP_ERR_ALLOC;
    }
    int32_t *d_raw, *d_raw2, *d_soff, *d_nbr; int64_t *d_ucnt, *d_noff;
    if ((st = call.alloc(&d_raw, (size_t)R)) || (st = call.alloc(&d_raw2, (size_t)R)) || (st = call.alloc(&d_soff, (size_t)S + 1)) ||
        (st = call.alloc(&d_nbr, (size_t)R)) || (st = call.alloc(&d_ucnt, (size_t)S + 1)) || (st = call.alloc(&d_noff, (size_t)S + 1)))
        return st;
    {
        if (R > 0) {
            hipLaunchKernelGGL(prep_nbr_kernel, dim3(blocks_for(E)), dim3(PREP_BLOCK), 0, q, d_key2, d_val2, d_sbox, d_ssrc, E, N, max_rows, d_cnt,
                               (const int64_t *)d_roff, d_raw);
            PREP_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(prep_source_ranges_kernel, dim3(blocks_for(S + 1)), dim3(PREP_BLOCK), 0, q, D.source, d_roff, E, S, R, d_soff);
        PREP_HIP(hipGetLastError());
        size_t tb = 0, tb2 = 0;
        const int sbits = bits_for((uint64_t)std::max<int64_t>(S, 1));
        if (R > 0) PREP_HIP(hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, tb, d_raw, d_raw2, (int)R, (int)S, d_soff, d_soff + 1, 0, sbits, q));
        PREP_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb2, d_ucnt, d_noff, (int)(S + 1), q));
        char *d_tmp;
        if ((st = call.alloc(&d_tmp, std::max(tb, tb2)))) return st;
        if (R > 0) PREP_HIP(hipcub::DeviceSegmentedRadixSort::SortKeys(d_tmp, tb, d_raw, d_raw2, (int)R, (int)S, d_soff, d_soff + 1, 0, sbits, q));
        hipLaunchKernelGGL(prep_unique_kernel, dim3(blocks_for(S + 1)), dim3(PREP_BLOCK), 0, q, d_raw2, d_soff, S, d_ucnt,
                           (const int64_t *)nullptr, (int32_t *)nullptr);
        PREP_HIP(hipGetLastError());
        PREP_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp, tb2, d_ucnt, d_noff, (int)(S + 1), q));
        if (R > 0) {
            hipLaunchKernelGGL(prep_unique_kernel, dim3(blocks_for(S + 1)), dim3(PREP_BLOCK), 0, q, d_raw2, d_soff, S, d_ucnt,
                               (const int64_t *)d_noff, d_nbr);
            PREP_HIP(hipGetLastError());
        }
    }
    PREP_HIP(hipEventRecord(call.ev[3], q));

    // ---- stamps
    int32_t *d_stamp = nullptr; double *d_stamps = nullptr;
    if (want_stamps) {
        if ((st = call.alloc(&d_stamp, (size_t)E)) || (st = call.alloc(&d_stamps, (size_t)n_stamps * PREP_NPIX))) return st;
        if (E > 0) {
            hipLaunchKernelGGL(prep_stamp_kernel, dim3((unsigned)E), dim3(PREP_BLOCK), 0, q, handle->d_imgs, D.image, D.pc, D.sflag, d_sidx,
                               d_stamp, d_stamps);
            PREP_HIP(hipGetLastError());
        }
    }
    PREP_HIP(hipEventRecord(call.ev[4], q));

    // ---- the table, in one page-locked block
    size_t at = 0;
    const size_t o_source = carve(&at, (size_t)E * 4), o_image = carve(&at, (size_t)E * 4), o_box = carve(&at, (size_t)E * 32),
                 o_pc = carve(&at, (size_t)E * 16), o_wc = carve(&at, (size_t)E * 16), o_active = carve(&at, (size_t)E * 8),
                 o_noff = carve(&at, (size_t)(S + 1) * 8), o_nbr = carve(&at, (size_t)R * 4),
                 o_stamp = carve(&at, want_stamps ? (size_t)E * 4 : 0),
                 o_stamps = carve(&at, want_stamps ? (size_t)n_stamps * PREP_NPIX * 8 : 0),
                 o_jac = carve(&at, d_jac ? (size_t)E * 32 : 0);
    for (int i = 0; i < n_extra; ++i) extra[i].at = carve(&at, extra[i].bytes);
    size_t got = 0;
    char *blk = (char *)pinned_take(std::max<size_t>(at, 256), &got);
    if (!blk) return CELESTE_PREP_ERR_ALLOC;
    celeste_prep_result *res = new celeste_prep_result;
    res->block = blk; res->bytes = got;
    int hst = 0;
#define PREP_DOWN(off, dptr, bytes) do { if (!hst && (bytes) > 0 && hipMemcpyAsync(blk + (off), (dptr), (bytes), hipMemcpyDeviceToHost, q) != hipSuccess) hst = 1; } while (0)
    PREP_DOWN(o_source, D.source, (size_t)E * 4); PREP_DOWN(o_image, D.image, (size_t)E * 4); PREP_DOWN(o_box, D.box, (size_t)E * 32);
    PREP_DOWN(o_pc, D.pc, (size_t)E * 16); PREP_DOWN(o_wc, D.wc, (size_t)E * 16); PREP_DOWN(o_active, d_active, (size_t)E * 8);
    PREP_DOWN(o_noff, d_noff, (size_t)(S + 1) * 8); PREP_DOWN(o_nbr, d_nbr, (size_t)R * 4);
    if (want_stamps) { PREP_DOWN(o_stamp, d_stamp, (size_t)E * 4); PREP_DOWN(o_stamps, d_stamps, (size_t)n_stamps * PREP_NPIX * 8); }
    if (d_jac) PREP_DOWN(o_jac, d_jac, (size_t)E * 32);
    for (int i = 0; i < n_extra; ++i) { PREP_DOWN(extra[i].at, extra[i].dptr, extra[i].bytes); extra[i].host = blk + extra[i].at; }
#undef PREP_DOWN
    if (!hst && hipStreamSynchronize(q) != hipSuccess) hst = 1;
    if (hst) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(q);
        pinned_give(blk, got);
        delete res;
        return CELESTE_PREP_ERR_HIP;
    }
    celeste_prep_table_t &T = res->table;
    memset(&T, 0, sizeof T);
    T.n_entries = E; T.n_sources = S; T.n_stamps = want_stamps ? n_stamps : 0;
    T.source = (const int32_t *)(blk + o_source); T.image = (const int32_t *)(blk + o_image); T.box = (const int64_t *)(blk + o_box);
    T.pixel_center = (const double *)(blk + o_pc); T.world_center = (const double *)(blk + o_wc);
    T.active_pixels = (const int64_t *)(blk + o_active);
    T.nbr_offsets = (const int64_t *)(blk + o_noff); T.nbr_index = (const int32_t *)(blk + o_nbr);
    T.n_neighbors = T.nbr_offsets[S];
    if (want_stamps) { T.stamp = (const int32_t *)(blk + o_stamp); T.stamps = (const double *)(blk + o_stamps); }
    if (d_jac) res->jac = (const double *)(blk + o_jac);
    for (int i = 0; i < 4; ++i) (void)hipEventElapsedTime(&g_last_ms[i], call.ev[i], call.ev[i + 1]);
    *result = res;
    return CELESTE_PREP_OK;
}

extern "C" int celeste_prep_bad_sky(celeste_prep_images_t *handle, int64_t n, const double *pos, uint8_t *flags) {
    if (!handle || n < 0 || (n && (!pos || !flags)) || n > 0x7fffffff) return CELESTE_PREP_ERR_INVALID_ARG;
    for (int64_t i = 0; i < 2 * n; ++i) if (!std::isfinite(pos[i])) return CELESTE_PREP_ERR_INVALID_ARG;
    if (n == 0) return CELESTE_PREP_OK;
    if (handle->sky_image < 0) {            // no image of band 4: nothing to check, no launch
        memset(flags, 0, (size_t)n);
        return CELESTE_PREP_OK;
    }
    std::lock_guard<std::mutex> lk(g_mu);
    PrepCall call;
    int st = call.open(handle->device);
    if (st) return st;
    hipStream_t q = call.stream;
    for (float &m : g_last_ms) m = 0.0f;
    for (float &m : g_det_ms) m = 0.0f;
    double *d_pos; uint8_t *d_flags;
    if ((st = call.alloc(&d_pos, (size_t)n * 2)) || (st = call.alloc(&d_flags, (size_t)n))) return st;
    PREP_HIP(hipMemcpyAsync(d_pos, pos, (size_t)n * 2 * sizeof(double), hipMemcpyHostToDevice, q));
    PREP_HIP(hipEventRecord(call.ev[0], q));
    hipLaunchKernelGGL(prep_sky_kernel, dim3((unsigned)n), dim3(PREP_BLOCK), 0, q, handle->d_imgs, handle->sky_image, d_pos, d_flags);
    PREP_HIP(hipGetLastError());
    PREP_HIP(hipEventRecord(call.ev[1], q));
    PREP_HIP(hipMemcpyAsync(flags, d_flags, (size_t)n, hipMemcpyDeviceToHost, q));
    PREP_HIP(hipStreamSynchronize(q));
    (void)hipEventElapsedTime(&g_last_ms[4], call.ev[0], call.ev[1]);
    return CELESTE_PREP_OK;
}

#include "prep_detected.h"
