// libceleste_detect.so: source detection on the device (include/celeste_detect.h, DESIGN.md section "Detection").
//
// All images of a call are concatenated: image n owns global pixel indices [pix_off[n], pix_off[n+1]) in SEP's raster
// order (column-major, index i + H*j), mesh cells [cell_off[n], cell_off[n+1]).  Launches (each covers every image):
//   calibrate_kernel   cal = pixels / nelec[row] - sky (float32, no contraction), transposed to the raster order
//   mesh_kernel        one workgroup per 256 x 256 cell: kappa-sigma clipping around the median (radix select)
//   mesh_final_kernel  one thread per image: bad cells, 3x3 median filter, global rms, threshold
//   filter_kernel      3x3 [1 2 1; 2 4 2; 1 2 1]/16 in fp64, fixed tap order; mask = conv > thresh
//   union / flatten    8-connected union-find, root = smallest raster index (atomicMin), component sizes
//   select + sort      kept pixels (component >= minarea) grouped by component, ascending inside it (hipCUB)
//   deblend_kernel     one workgroup per component (LDS, or a global scratch for large ones): multi-threshold split
//   scatter / moments  pixel lists per object, then fp64 moments per object with a fixed-order tree reduction
// The host reads the counts between stages (kept pixels, components, children), so no buffer can overflow.
//
// CELESTE_DETECT_MUTANT=k builds the library with one deliberate bug, for tests/test_detect_mutants.py (the product is 0):
//   1 = calibrate_kernel takes nelec by column
//   2 = mesh_kernel: an even count's median is its upper value
//   3 = mesh_kernel: the good-cell rule is strict
//   4 = mesh_kernel: sigma divides by n - 1
//   5 = mesh_final_kernel: a tie goes to the last cell
//   6 = mesh_final_kernel: the threshold uses 1.3, not params.thresh
//   7 = filter_kernel admits a NaN centre to the mask
//   8 = filter_kernel: conv >= thresh
//   9 = union_kernel drops the anti-diagonal neighbour
//   10 = keep_kernel: size > minarea
//   11 = the host's O.parent is the batch-wide parent index
//   12 = deblend_kernel: a piece of any size may split its leaf
//   13 = deblend_kernel: the level exponent is one level ahead
//   14 = deblend_kernel: equal amplitudes go to the higher core
//   15 = deblend_kernel: children stay in core order
//   16 = moments_kernel: the 1/12 rule is unconditional
//   17 = moments_kernel: segmap carries the batch-wide object index
#ifndef CELESTE_DETECT_MUTANT
#define CELESTE_DETECT_MUTANT 0
#endif
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <stdexcept>
#include <vector>

#include "../../../include/celeste_detect.h"

namespace {

constexpr int MESH = 256;
constexpr int BLOCK = 256;
constexpr int LDS_MAX_DEFAULT = 512;   // 124 B per pixel: 63.5 KB of LDS
constexpr uint32_t NONE = 0xFFFFFFFFu;

struct HipError : std::runtime_error {
    explicit HipError(hipError_t e) : std::runtime_error(hipGetErrorString(e)) {}
};
#define HIPCHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) throw HipError(e_); } while (0)

struct ImgDesc {          // device copy of one image's geometry
    int32_t H, W;
    int64_t pix_off;      // global pixel offset
    int64_t row_off;      // offset into the concatenated nelec_per_nmgy
    int32_t cell_off, nx, ny, pad;
};

__device__ int find_image(const ImgDesc *d, int n, int64_t g) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if (d[mid].pix_off <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---- calibrate ----------------------------------------------------------------------------------------------------
__global__ void calibrate_kernel(const ImgDesc *imgs, int n_img, int64_t total, const float *pix_rm, const float *sky_rm,
                                 const float *nelec, float *cal) {
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const ImgDesc d = imgs[find_image(imgs, n_img, g)];
    int64_t cm = g - d.pix_off;
    int i = (int)(cm % d.H), j = (int)(cm / d.H);
    int64_t rm = d.pix_off + (int64_t)i * d.W + j;
#if CELESTE_DETECT_MUTANT == 1
    cal[g] = __fsub_rn(__fdiv_rn(pix_rm[rm], nelec[d.row_off + j % d.H]), sky_rm[rm]);
#else
    cal[g] = __fsub_rn(__fdiv_rn(pix_rm[rm], nelec[d.row_off + i]), sky_rm[rm]);
#endif
}

// ---- background mesh ----------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t float_key(float v) {
    uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

struct Cell {
    const float *cal;
    int64_t base;   // global index of the cell's first pixel
    int H, ci, cj;  // image height (raster stride), cell extent along i and j
};

__device__ __forceinline__ bool in_set(float v, double lo, double hi) {
    return v == v && (double)v >= lo && (double)v <= hi;
}

// block-wide fp64 sum in a fixed order (thread partials in index order, then a fixed tree)
__device__ double block_sum(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
        __syncthreads();
    }
    double r = red[0];
    __syncthreads();
    return r;
}

// k-th smallest (0-based) value of the set, by an 8-bit radix select on the ordered float keys
__device__ float cell_select(const Cell &c, double lo, double hi, int64_t k, uint32_t *hist, uint32_t *shared_word) {
    uint32_t prefix = 0, pmask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[threadIdx.x] = 0;
        __syncthreads();
        if ((int)threadIdx.x < c.ci)
            for (int j = 0; j < c.cj; ++j) {
                float v = c.cal[c.base + threadIdx.x + (int64_t)c.H * j];
                if (!in_set(v, lo, hi)) continue;
                uint32_t key = float_key(v);
                if ((key & pmask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
            }
        __syncthreads();
        if (threadIdx.x == 0) {
            int64_t cum = 0;
            int b = 0;
            for (; b < 255; ++b) {
                if (cum + hist[b] > k) break;
                cum += hist[b];
            }
            k -= cum;
            shared_word[0] = (uint32_t)b;
            shared_word[1] = (uint32_t)k;
        }
        __syncthreads();
        prefix |= shared_word[0] << shift;
        pmask |= 255u << shift;
        k = shared_word[1];
        __syncthreads();
    }
    return key_float(prefix);
}

__device__ int64_t cell_count(const Cell &c, double lo, double hi, double *red) {
    double n = 0;
    if ((int)threadIdx.x < c.ci)
        for (int j = 0; j < c.cj; ++j) n += in_set(c.cal[c.base + threadIdx.x + (int64_t)c.H * j], lo, hi) ? 1.0 : 0.0;
    return (int64_t)block_sum(n, red);
}

__device__ double cell_sigma(const Cell &c, double lo, double hi, int64_t n, double *red) {
    double s = 0;
    if ((int)threadIdx.x < c.ci)
        for (int j = 0; j < c.cj; ++j) {
            float v = c.cal[c.base + threadIdx.x + (int64_t)c.H * j];
            if (in_set(v, lo, hi)) s += (double)v;
        }
    double mean = block_sum(s, red) / (double)n;
    double q = 0;
    if ((int)threadIdx.x < c.ci)
        for (int j = 0; j < c.cj; ++j) {
            float v = c.cal[c.base + threadIdx.x + (int64_t)c.H * j];
            if (in_set(v, lo, hi)) { double d = (double)v - mean; q += d * d; }
        }
#if CELESTE_DETECT_MUTANT == 4
    return sqrt(block_sum(q, red) / (double)(n - 1));
#else
    return sqrt(block_sum(q, red) / (double)n);
#endif
}

// one workgroup per mesh cell: rms of the cell after iterative 3-sigma clipping around the median; good = at least
// half of the cell's pixels are valid
__global__ __launch_bounds__(BLOCK) void mesh_kernel(const ImgDesc *imgs, int n_img, int n_cells, const float *cal,
                                                     double *cell_rms, int32_t *cell_good) {
    __shared__ double red[BLOCK];
    __shared__ uint32_t hist[BLOCK];
    __shared__ uint32_t word[2];
    int cell = blockIdx.x;
    int n = 0;
    while (n + 1 < n_img && imgs[n + 1].cell_off <= cell) ++n;
    const ImgDesc d = imgs[n];
    int local = cell - d.cell_off, cx = local % d.nx, cy = local / d.nx;
    Cell c;
    c.cal = cal; c.H = d.H;
    c.ci = min(MESH, d.H - cx * MESH);
    c.cj = min(MESH, d.W - cy * MESH);
    c.base = d.pix_off + (int64_t)cx * MESH + (int64_t)d.H * cy * MESH;
    double lo = -INFINITY, hi = INFINITY;
    int64_t cnt = cell_count(c, lo, hi, red);
#if CELESTE_DETECT_MUTANT == 3
    bool good = 2 * cnt > (int64_t)c.ci * c.cj && cnt > 0;
#else
    bool good = 2 * cnt >= (int64_t)c.ci * c.cj && cnt > 0;
#endif
    double sigma = NAN;
    if (good) {
        for (int it = 0; it < 100; ++it) {
            double med;
            if (cnt & 1) {
                med = (double)cell_select(c, lo, hi, cnt / 2, hist, word);
            } else {
                double a = (double)cell_select(c, lo, hi, cnt / 2 - 1, hist, word);
                double b = (double)cell_select(c, lo, hi, cnt / 2, hist, word);
#if CELESTE_DETECT_MUTANT == 2
                med = b;
#else
                med = (a + b) * 0.5;
#endif
            }
            sigma = cell_sigma(c, lo, hi, cnt, red);
            double nlo = fmax(lo, med - 3.0 * sigma), nhi = fmin(hi, med + 3.0 * sigma);
            int64_t ncnt = cell_count(c, nlo, nhi, red);
            if (ncnt == cnt) break;
            lo = nlo; hi = nhi; cnt = ncnt;
            if (it == 99) sigma = cell_sigma(c, lo, hi, cnt, red);
        }
    }
    if (threadIdx.x == 0) {
        cell_rms[cell] = sigma;
        cell_good[cell] = good ? 1 : 0;
    }
}

__device__ void sort_small(double *v, int n) {
    for (int a = 1; a < n; ++a) {
        double x = v[a];
        int b = a - 1;
        while (b >= 0 && v[b] > x) { v[b + 1] = v[b]; --b; }
        v[b + 1] = x;
    }
}

__device__ double median_sorted(const double *v, int n) {
    return (n & 1) ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) * 0.5;
}

// one thread per image: bad cells take the nearest good cell's value (ties: lowest cell index), 3x3 median filter
// (threshold 0: every cell is replaced), global rms = median of the filtered mesh, rounded to float32
__global__ void mesh_final_kernel(const ImgDesc *imgs, int n_img, const double *cell_rms, const int32_t *cell_good,
                                  double *scratch, float thresh, float *rms_out, float *thr_out) {
    int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_img) return;
    const ImgDesc d = imgs[n];
    int nc = d.nx * d.ny;
    const double *rms = cell_rms + d.cell_off;
    const int32_t *good = cell_good + d.cell_off;
    double *fixed = scratch + 2 * (int64_t)d.cell_off;
    double *filt = fixed + nc;
    int ngood = 0;
    for (int c = 0; c < nc; ++c) ngood += good[c];
    if (ngood == 0) {
        rms_out[n] = NAN;
        thr_out[n] = NAN;
        return;
    }
    for (int c = 0; c < nc; ++c) {
        if (good[c]) { fixed[c] = rms[c]; continue; }
        int cx = c % d.nx, cy = c / d.nx;
        int best = -1;
        long bestd = 0;
        for (int e = 0; e < nc; ++e) {
            if (!good[e]) continue;
            long dx = e % d.nx - cx, dy = e / d.nx - cy, dd = dx * dx + dy * dy;
#if CELESTE_DETECT_MUTANT == 5
            if (best < 0 || dd <= bestd) { best = e; bestd = dd; }
#else
            if (best < 0 || dd < bestd) { best = e; bestd = dd; }
#endif
        }
        fixed[c] = rms[best];
    }
    for (int c = 0; c < nc; ++c) {
        int cx = c % d.nx, cy = c / d.nx, m = 0;
        double win[9];
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                int x = cx + dx, y = cy + dy;
                if (x >= 0 && x < d.nx && y >= 0 && y < d.ny) win[m++] = fixed[x + d.nx * y];
            }
        sort_small(win, m);
        filt[c] = median_sorted(win, m);
    }
    sort_small(filt, nc);
    float r = (float)median_sorted(filt, nc);
    rms_out[n] = r;
#if CELESTE_DETECT_MUTANT == 6
    thr_out[n] = __fmul_rn(1.3f, r);
#else
    thr_out[n] = __fmul_rn(thresh, r);
#endif
}

// ---- filter, threshold, labelling ---------------------------------------------------------------------------------
__global__ void filter_kernel(const ImgDesc *imgs, int n_img, int64_t total, const float *cal, const float *thr,
                              double *conv, uint32_t *par, uint8_t *mask_rm) {
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    int n = find_image(imgs, n_img, g);
    const ImgDesc d = imgs[n];
    int64_t cm = g - d.pix_off;
    int i = (int)(cm % d.H), j = (int)(cm / d.H);
    double acc = 0.0;
    for (int dj = -1; dj <= 1; ++dj)          // taps [1 2 1; 2 4 2; 1 2 1] / 16, fixed order (j outer, i inner)
        for (int di = -1; di <= 1; ++di) {
            int ii = i + di, jj = j + dj;
            if (ii < 0 || ii >= d.H || jj < 0 || jj >= d.W) continue;
            float v = cal[d.pix_off + ii + (int64_t)d.H * jj];
            if (v != v) continue;
            double wt = (double)((di == 0 ? 2 : 1) * (dj == 0 ? 2 : 1)) / 16.0;
            acc = __dadd_rn(acc, __dmul_rn(wt, (double)v));
        }
    float c0 = cal[g];
#if CELESTE_DETECT_MUTANT == 7
    bool m = acc > (double)thr[n];
#elif CELESTE_DETECT_MUTANT == 8
    bool m = c0 == c0 && acc >= (double)thr[n];
#else
    bool m = c0 == c0 && acc > (double)thr[n];
#endif
    conv[g] = acc;
    par[g] = m ? (uint32_t)g : NONE;
    if (mask_rm) mask_rm[d.pix_off + (int64_t)i * d.W + j] = m ? 1 : 0;
}

__device__ __forceinline__ uint32_t uf_find(const uint32_t *par, uint32_t p) {
    uint32_t q = __hip_atomic_load(&par[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (q != p) {
        p = q;
        q = __hip_atomic_load(&par[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return p;
}

__device__ void uf_union(uint32_t *par, uint32_t a, uint32_t b) {
    for (;;) {
        a = uf_find(par, a);
        b = uf_find(par, b);
        if (a == b) return;
        if (a > b) { uint32_t t = a; a = b; b = t; }
        uint32_t old = atomicMin(&par[b], a);
        if (old == b) return;
        b = old;
    }
}

__global__ void union_kernel(const ImgDesc *imgs, int n_img, int64_t total, uint32_t *par) {
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    if (par[g] == NONE) return;
    const ImgDesc d = imgs[find_image(imgs, n_img, g)];
    int64_t cm = g - d.pix_off;
    int i = (int)(cm % d.H), j = (int)(cm / d.H);
    const int di[4] = {-1, -1, 0, 1}, dj[4] = {0, -1, -1, -1};
    for (int t = 0; t < 4; ++t) {
        int ii = i + di[t], jj = j + dj[t];
#if CELESTE_DETECT_MUTANT == 9
        if (t == 3) continue;
#endif
        if (ii < 0 || ii >= d.H || jj < 0) continue;
        uint32_t q = (uint32_t)(d.pix_off + ii + (int64_t)d.H * jj);
        if (__hip_atomic_load(&par[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != NONE) uf_union(par, (uint32_t)g, q);
    }
}

__global__ void flatten_kernel(int64_t total, uint32_t *par, uint32_t *size) {
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    if (par[g] == NONE) return;
    uint32_t r = uf_find(par, (uint32_t)g);
    par[g] = r;   // an ancestor: concurrent finds stay valid
    atomicAdd(&size[r], 1u);
}

__global__ void keep_kernel(int64_t total, const uint32_t *par, const uint32_t *size, int minarea, uint8_t *keep) {
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    uint32_t p = par[g];
#if CELESTE_DETECT_MUTANT == 10
    keep[g] = (p != NONE && size[p] > (uint32_t)minarea) ? 1 : 0;
#else
    keep[g] = (p != NONE && size[p] >= (uint32_t)minarea) ? 1 : 0;
#endif
}

__global__ void root_kernel(int64_t n, const uint32_t *pix, const uint32_t *par, uint32_t *root) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    root[k] = par[pix[k]];
}

// ---- deblending ---------------------------------------------------------------------------------------------------
struct Parent {
    int64_t start;   // first entry in the sorted pixel list
    int32_t npix, img;
};

struct DebWork {     // per-pixel (k < n) and per-leaf arrays of one parent, in LDS or in the global scratch
    uint32_t *g;
    double *c;
    int32_t *leaf, *lab, *nbr, *cnt, *newid, *lsig;   // nbr: 8 per pixel; lsig: 2n + 2 (leaf ids)
    double *acc;
    double *lstat;                                     // 6 per final leaf
};

__device__ int bsearch_u32(const uint32_t *a, int n, uint32_t v) {
    int lo = 0, hi = n - 1;
    while (lo <= hi) {
        int mid = (lo + hi) >> 1;
        uint32_t x = a[mid];
        if (x == v) return mid;
        if (x < v) lo = mid + 1; else hi = mid - 1;
    }
    return -1;
}

struct LeafGauss { double xm, ym, cxx, cyy, cxy, peak; };

__device__ void ellipse_coeffs(double x2, double y2, double xy, double *cxx, double *cyy, double *cxy) {
    double det = x2 * y2 - xy * xy;
    if (det < 1.0 / 144.0) { x2 += 1.0 / 12.0; y2 += 1.0 / 12.0; det = x2 * y2 - xy * xy; }
    *cxx = y2 / det;
    *cyy = x2 / det;
    *cxy = -2.0 * xy / det;
}

// one workgroup per parent.  rank[start + k] = child index of pixel k (children ordered by smallest raster index),
// nchild[p] = number of children, child_npix[start + r] = pixels of child r
__global__ __launch_bounds__(BLOCK) void deblend_kernel(
        const ImgDesc *imgs, const Parent *parents, const int32_t *plist, int n_list, const uint32_t *spix,
        const double *conv, const float *thr_img, int nthresh, double cont, int minarea, int use_lds, int lds_max,
        char *gscratch, int64_t per_pixel_bytes, int32_t *rank, int32_t *nchild, int32_t *child_npix) {
    extern __shared__ __align__(16) char lds[];
    __shared__ int s_nleaves, s_changed, s_split, s_nfinal;
    __shared__ double s_F, s_peak;
    if ((int)blockIdx.x >= n_list) return;
    const int p = plist[blockIdx.x];
    const Parent P = parents[p];
    const ImgDesc d = imgs[P.img];
    const int n = P.npix;
    const int T = blockDim.x, tid = threadIdx.x;
    char *base = use_lds ? lds : gscratch + P.start * per_pixel_bytes;
    const int cap = use_lds ? lds_max : n;
    DebWork w;
    w.c = (double *)base;
    w.acc = w.c + cap;
    w.lstat = w.acc + cap;                                   // 6 * (cap + 1) doubles
    w.g = (uint32_t *)(w.lstat + 6 * (cap + 1));
    w.leaf = (int32_t *)(w.g + cap);
    w.lab = w.leaf + cap;
    w.cnt = w.lab + cap;
    w.newid = w.cnt + cap;
    w.nbr = w.newid + cap;
    w.lsig = w.nbr + 8 * cap;                                // 2 * cap + 2
    const float thr = thr_img[P.img];

    for (int k = tid; k < n; k += T) {
        uint32_t g = spix[P.start + k];
        w.g[k] = g;
        w.c[k] = conv[g];
        w.leaf[k] = 0;
    }
    __syncthreads();
    for (int k = tid; k < n; k += T) {
        int64_t cm = (int64_t)w.g[k] - d.pix_off;
        int i = (int)(cm % d.H), j = (int)(cm / d.H), t = 0;
        for (int dj = -1; dj <= 1; ++dj)
            for (int di = -1; di <= 1; ++di) {
                if (di == 0 && dj == 0) continue;
                int ii = i + di, jj = j + dj;
                int q = -1;
                if (ii >= 0 && ii < d.H && jj >= 0 && jj < d.W)
                    q = bsearch_u32(w.g, n, (uint32_t)(d.pix_off + ii + (int64_t)d.H * jj));
                w.nbr[8 * k + t++] = q;
            }
    }
    if (tid == 0) {
        double F = 0, pk = -INFINITY;
        for (int k = 0; k < n; ++k) { F += w.c[k]; pk = fmax(pk, w.c[k]); }
        s_F = F; s_peak = pk; s_nleaves = 1;
    }
    __syncthreads();
    const double F = s_F, peak = s_peak;
    for (int lev = 1; lev < nthresh && n >= 2 * minarea; ++lev) {
#if CELESTE_DETECT_MUTANT == 13
        const double t = (double)thr * pow(peak / (double)thr, (double)(lev + 1) / (double)nthresh);
#else
        const double t = (double)thr * pow(peak / (double)thr, (double)lev / (double)nthresh);
#endif
        for (int k = tid; k < n; k += T) w.lab[k] = (w.leaf[k] >= 0 && w.c[k] > t) ? k : -1;
        __syncthreads();
        // pieces: min-label propagation with pointer jumping inside each leaf
        for (;;) {
            if (tid == 0) s_changed = 0;
            __syncthreads();
            for (int k = tid; k < n; k += T) {
                int m = w.lab[k];
                if (m < 0) continue;
                const int L = w.leaf[k];
                int m0 = m;
                for (int e = 0; e < 8; ++e) {
                    int q = w.nbr[8 * k + e];
                    if (q >= 0 && w.leaf[q] == L) { int lq = w.lab[q]; if (lq >= 0 && lq < m) m = lq; }
                }
                m = min(m, w.lab[m]);
                if (m < m0) { atomicMin(&w.lab[k], m); s_changed = 1; }
            }
            __syncthreads();
            if (!s_changed) break;
            __syncthreads();
        }
        // piece flux and size, significance, splits: serial in raster order (fixed summation order)
        if (tid == 0) {
            for (int k = 0; k < n; ++k) if (w.lab[k] == k) { w.acc[k] = 0; w.cnt[k] = 0; }
            for (int k = 0; k < n; ++k) { int r = w.lab[k]; if (r >= 0) { w.acc[r] += w.c[k]; w.cnt[r] += 1; } }
            const int nl = s_nleaves;
            for (int L = 0; L < nl; ++L) w.lsig[L] = 0;
#if CELESTE_DETECT_MUTANT == 12
            const int piece_area = 1;
#else
            const int piece_area = minarea;
#endif
            for (int k = 0; k < n; ++k)
                if (w.lab[k] == k && w.acc[k] >= cont * F && w.cnt[k] >= piece_area) w.lsig[w.leaf[k]] += 1;
            int next = nl, split = 0;
            for (int k = 0; k < n; ++k) {
                w.newid[k] = -1;
                if (w.lab[k] == k && w.lsig[w.leaf[k]] >= 2 && w.acc[k] >= cont * F && w.cnt[k] >= piece_area) {
                    w.newid[k] = next++;
                    split = 1;
                }
            }
            s_nleaves = next;
            s_split = split;
        }
        __syncthreads();
        if (s_split) {
            for (int k = tid; k < n; k += T) {
                const int L = w.leaf[k];
                if (L < 0 || w.lsig[L] < 2) continue;
                const int r = w.lab[k];
                w.leaf[k] = (r >= 0 && w.newid[r] >= 0) ? w.newid[r] : -1;
            }
        }
        __syncthreads();
    }
    // final leaves in the order of their cores' smallest raster index
    if (tid == 0) {
        const int nl = s_nleaves;
        for (int L = 0; L < nl; ++L) w.lsig[L] = -1;
        int K = 0;
        for (int k = 0; k < n; ++k) { int L = w.leaf[k]; if (L >= 0 && w.lsig[L] < 0) w.lsig[L] = K++; }
        s_nfinal = K;
    }
    __syncthreads();
    const int K = s_nfinal;
    if (K <= 1) {
        for (int k = tid; k < n; k += T) rank[P.start + k] = 0;
        if (tid == 0) { nchild[p] = 1; child_npix[P.start] = n; }
        return;
    }
    for (int k = tid; k < n; k += T) w.lab[k] = w.leaf[k] >= 0 ? w.lsig[w.leaf[k]] : -1;   // core index or -1
    __syncthreads();
    // core moments (convolved values), one thread per core, serial in raster order
    for (int L = tid; L < K; L += T) {
        double f = 0, fx = 0, fy = 0, pk = -INFINITY;
        for (int k = 0; k < n; ++k) {
            if (w.lab[k] != L) continue;
            int64_t cm = (int64_t)w.g[k] - d.pix_off;
            double x = (double)(cm % d.H), y = (double)(cm / d.H), v = w.c[k];
            f += v; fx += v * x; fy += v * y; pk = fmax(pk, v);
        }
        const double xm = fx / f, ym = fy / f;
        double x2 = 0, y2 = 0, xy = 0;
        for (int k = 0; k < n; ++k) {
            if (w.lab[k] != L) continue;
            int64_t cm = (int64_t)w.g[k] - d.pix_off;
            double dx = (double)(cm % d.H) - xm, dy = (double)(cm / d.H) - ym, v = w.c[k];
            x2 += v * dx * dx; y2 += v * dy * dy; xy += v * dx * dy;
        }
        double cxx, cyy, cxy;
        ellipse_coeffs(x2 / f, y2 / f, xy / f, &cxx, &cyy, &cxy);
        double *s = w.lstat + 6 * L;
        s[0] = xm; s[1] = ym; s[2] = cxx; s[3] = cyy; s[4] = cxy; s[5] = pk;
    }
    __syncthreads();
    // pixels outside every core: the core of the largest Gaussian amplitude (ties: lower core index)
    for (int k = tid; k < n; k += T) {
        if (w.lab[k] >= 0) { w.cnt[k] = w.lab[k]; continue; }
        int64_t cm = (int64_t)w.g[k] - d.pix_off;
        double x = (double)(cm % d.H), y = (double)(cm / d.H);
        int best = 0;
        double bamp = -1.0;
        for (int L = 0; L < K; ++L) {
            const double *s = w.lstat + 6 * L;
            double dx = x - s[0], dy = y - s[1];
            double amp = s[5] * exp(-0.5 * (s[2] * dx * dx + s[3] * dy * dy + s[4] * dx * dy));
#if CELESTE_DETECT_MUTANT == 14
            if (amp >= bamp) { bamp = amp; best = L; }
#else
            if (amp > bamp) { bamp = amp; best = L; }
#endif
        }
        w.cnt[k] = best;
    }
    __syncthreads();
    // children ordered by their smallest raster index (pixels are in raster order)
    if (tid == 0) {
        for (int L = 0; L < K; ++L) w.newid[L] = -1;
        int r = 0;
#if CELESTE_DETECT_MUTANT == 15
        for (int L = 0; L < K; ++L) w.newid[L] = r++;
#else
        for (int k = 0; k < n; ++k) if (w.newid[w.cnt[k]] < 0) w.newid[w.cnt[k]] = r++;
#endif
        for (int q = 0; q < K; ++q) child_npix[P.start + q] = 0;
        for (int k = 0; k < n; ++k) child_npix[P.start + w.newid[w.cnt[k]]] += 1;
        nchild[p] = K;
    }
    __syncthreads();
    for (int k = tid; k < n; k += T) rank[P.start + k] = w.newid[w.cnt[k]];
}

// ---- objects ------------------------------------------------------------------------------------------------------
struct ObjDesc {
    int64_t pix_start;   // into the object pixel list
    int32_t npix, img;
};

// one workgroup per parent: each child's pixels in raster order
__global__ void scatter_kernel(const Parent *parents, const int32_t *nchild, const int64_t *obj_base, const ObjDesc *objs,
                               const uint32_t *spix, const int32_t *rank, uint32_t *opix) {
    const Parent P = parents[blockIdx.x];
    const int K = nchild[blockIdx.x];
    const int64_t ob = obj_base[blockIdx.x];
    if (K == 1) {
        const int64_t o = objs[ob].pix_start;
        for (int k = threadIdx.x; k < P.npix; k += blockDim.x) opix[o + k] = spix[P.start + k];
        return;
    }
    for (int r = threadIdx.x; r < K; r += blockDim.x) {
        int64_t o = objs[ob + r].pix_start;
        for (int k = 0; k < P.npix; ++k)
            if (rank[P.start + k] == r) opix[o++] = spix[P.start + k];
    }
}

struct ObjOut {
    int32_t xmin, xmax, ymin, ymax;
    double x, y, x2, y2, xy, a, b, theta, flux, peak;
};

__device__ int block_min_i(int v, int *ired) {
    ired[threadIdx.x] = v;
    __syncthreads();
    for (int s = BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) ired[threadIdx.x] = min(ired[threadIdx.x], ired[threadIdx.x + s]);
        __syncthreads();
    }
    int r = ired[0];
    __syncthreads();
    return r;
}

// one workgroup per object: fp64 moments of the calibrated values, fixed-order reductions
__global__ __launch_bounds__(BLOCK) void moments_kernel(const ImgDesc *imgs, const ObjDesc *objs, const uint32_t *opix,
                                                        const float *cal, ObjOut *out, int32_t *segmap_rm,
                                                        const int32_t *obj_local) {
    __shared__ double red[BLOCK];
    __shared__ int ired[BLOCK];
    const ObjDesc o = objs[blockIdx.x];
    const ImgDesc d = imgs[o.img];
    double f = 0, fx = 0, fy = 0;
    int xmin = INT32_MAX, ymin = INT32_MAX, nxmax = INT32_MAX, nymax = INT32_MAX;
    for (int k = threadIdx.x; k < o.npix; k += BLOCK) {
        uint32_t g = opix[o.pix_start + k];
        int64_t cm = (int64_t)g - d.pix_off;
        int i = (int)(cm % d.H), j = (int)(cm / d.H);
        double v = (double)cal[g];
        f += v; fx += v * i; fy += v * j;
        xmin = min(xmin, i); ymin = min(ymin, j); nxmax = min(nxmax, -i); nymax = min(nymax, -j);
#if CELESTE_DETECT_MUTANT == 17
        if (segmap_rm) segmap_rm[d.pix_off + (int64_t)i * d.W + j] = (int32_t)blockIdx.x + 1;
#else
        if (segmap_rm) segmap_rm[d.pix_off + (int64_t)i * d.W + j] = obj_local[blockIdx.x] + 1;
#endif
    }
    f = block_sum(f, red); fx = block_sum(fx, red); fy = block_sum(fy, red);
    xmin = block_min_i(xmin, ired); ymin = block_min_i(ymin, ired);
    nxmax = block_min_i(nxmax, ired); nymax = block_min_i(nymax, ired);
    const double xm = fx / f, ym = fy / f;
    double x2 = 0, y2 = 0, xy = 0, lpk = -INFINITY;
    for (int k = threadIdx.x; k < o.npix; k += BLOCK) {
        uint32_t g = opix[o.pix_start + k];
        int64_t cm = (int64_t)g - d.pix_off;
        double dx = (double)(cm % d.H) - xm, dy = (double)(cm / d.H) - ym, v = (double)cal[g];
        x2 += v * dx * dx; y2 += v * dy * dy; xy += v * dx * dy; lpk = fmax(lpk, v);
    }
    x2 = block_sum(x2, red) / f; y2 = block_sum(y2, red) / f; xy = block_sum(xy, red) / f;
    red[threadIdx.x] = lpk;
    __syncthreads();
    for (int s = BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    const double pk = red[0];
    if (threadIdx.x == 0) {
        ObjOut r;
        r.xmin = xmin; r.xmax = -nxmax; r.ymin = ymin; r.ymax = -nymax;
        r.x = xm; r.y = ym; r.x2 = x2; r.y2 = y2; r.xy = xy; r.flux = f; r.peak = pk;
        double mx2 = x2, my2 = y2;
#if CELESTE_DETECT_MUTANT == 16
        { mx2 += 1.0 / 12.0; my2 += 1.0 / 12.0; }
#else
        if (mx2 * my2 - xy * xy < 1.0 / 144.0) { mx2 += 1.0 / 12.0; my2 += 1.0 / 12.0; }
#endif
        double tmp = mx2 - my2;
        r.theta = fabs(tmp) > 0.0 ? atan2(2.0 * xy, tmp) / 2.0 : M_PI / 4.0;
        tmp = sqrt(0.25 * tmp * tmp + xy * xy);
        double pm = 0.5 * (mx2 + my2);
        r.a = sqrt(pm + tmp);
        r.b = sqrt(fmax(pm - tmp, 0.0));
        out[blockIdx.x] = r;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    template <class T> T *alloc(size_t n) {
        if (p) { (void)hipFree(p); p = nullptr; }
        HIPCHECK(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
        return (T *)p;
    }
    template <class T> T *get() const { return (T *)p; }
};

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

struct Timer {
    bool on;
    hipStream_t s;
    std::vector<hipEvent_t> ev;
    Timer(bool on_, hipStream_t s_) : on(on_), s(s_) {}
    void mark() {
        if (!on) return;
        hipEvent_t e;
        HIPCHECK(hipEventCreate(&e));
        HIPCHECK(hipEventRecord(e, s));
        ev.push_back(e);
    }
    ~Timer() { for (auto e : ev) (void)hipEventDestroy(e); }
};

void free_result(celeste_detect_result_t *r) {
    if (!r) return;
    if (r->images)
        for (int n = 0; n < r->n_images; ++n) {
            std::free(r->images[n].objects);
            std::free(r->images[n].pix);
            std::free(r->images[n].mask);
            std::free(r->images[n].segmap);
        }
    std::free(r->images);
    std::free(r);
}

template <class T> T *host_calloc(size_t n) {
    void *p = std::calloc(std::max<size_t>(n, 1), sizeof(T));
    if (!p) throw std::bad_alloc();
    return (T *)p;
}

int run(int32_t device, int32_t n_img, const celeste_detect_image_t *images, const celeste_detect_params_t *prm,
        celeste_detect_result_t **out) {
    const bool maps = prm->flags & CELESTE_DETECT_WANT_MAPS;
    const int lds_max = prm->lds_max_pixels > 0 ? std::min(prm->lds_max_pixels, LDS_MAX_DEFAULT) : LDS_MAX_DEFAULT;
    HIPCHECK(hipSetDevice(device));
    hipStream_t st;
    HIPCHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    struct StreamGuard { hipStream_t s; ~StreamGuard() { (void)hipStreamDestroy(s); } } sg{st};
    Timer tm(prm->flags & CELESTE_DETECT_TIMING, st);

    // geometry
    std::vector<ImgDesc> desc(n_img);
    int64_t total = 0, rows = 0;
    int cells = 0;
    for (int n = 0; n < n_img; ++n) {
        ImgDesc &d = desc[n];
        d.H = images[n].H; d.W = images[n].W; d.pix_off = total; d.row_off = rows; d.cell_off = cells;
        d.nx = (d.H + MESH - 1) / MESH; d.ny = (d.W + MESH - 1) / MESH; d.pad = 0;
        total += (int64_t)d.H * d.W; rows += d.H; cells += d.nx * d.ny;
    }
    if (total > (int64_t)INT32_MAX) return CELESTE_DETECT_ERR_INVALID_ARG;   // hipCUB item counts are int

    DevBuf b_desc, b_pix, b_sky, b_nelec, b_cal, b_crms, b_cgood, b_cscr, b_rms, b_thr, b_conv, b_par, b_size, b_mask;
    ImgDesc *d_desc = b_desc.alloc<ImgDesc>(n_img);
    float *d_pix = b_pix.alloc<float>(total), *d_sky = b_sky.alloc<float>(total), *d_nelec = b_nelec.alloc<float>(rows);
    HIPCHECK(hipMemcpyAsync(d_desc, desc.data(), sizeof(ImgDesc) * n_img, hipMemcpyHostToDevice, st));
    for (int n = 0; n < n_img; ++n) {
        size_t np = (size_t)desc[n].H * desc[n].W;
        HIPCHECK(hipMemcpyAsync(d_pix + desc[n].pix_off, images[n].pixels, np * 4, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(d_sky + desc[n].pix_off, images[n].sky, np * 4, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(d_nelec + desc[n].row_off, images[n].nelec_per_nmgy, (size_t)desc[n].H * 4,
                                hipMemcpyHostToDevice, st));
    }
    float *d_cal = b_cal.alloc<float>(total);
    tm.mark();
    calibrate_kernel<<<blocks_for(total), BLOCK, 0, st>>>(d_desc, n_img, total, d_pix, d_sky, d_nelec, d_cal);
    HIPCHECK(hipGetLastError());
    tm.mark();
    double *d_crms = b_crms.alloc<double>(cells);
    int32_t *d_cgood = b_cgood.alloc<int32_t>(cells);
    double *d_cscr = b_cscr.alloc<double>(2 * (size_t)cells);
    float *d_rms = b_rms.alloc<float>(n_img), *d_thr = b_thr.alloc<float>(n_img);
    mesh_kernel<<<cells, BLOCK, 0, st>>>(d_desc, n_img, cells, d_cal, d_crms, d_cgood);
    HIPCHECK(hipGetLastError());
    mesh_final_kernel<<<(n_img + 63) / 64, 64, 0, st>>>(d_desc, n_img, d_crms, d_cgood, d_cscr, prm->thresh, d_rms, d_thr);
    HIPCHECK(hipGetLastError());
    tm.mark();
    double *d_conv = b_conv.alloc<double>(total);
    uint32_t *d_par = b_par.alloc<uint32_t>(total);
    uint8_t *d_mask = maps ? b_mask.alloc<uint8_t>(total) : nullptr;
    filter_kernel<<<blocks_for(total), BLOCK, 0, st>>>(d_desc, n_img, total, d_cal, d_thr, d_conv, d_par, d_mask);
    HIPCHECK(hipGetLastError());
    tm.mark();
    uint32_t *d_size = b_size.alloc<uint32_t>(total);
    HIPCHECK(hipMemsetAsync(d_size, 0, total * 4, st));
    union_kernel<<<blocks_for(total), BLOCK, 0, st>>>(d_desc, n_img, total, d_par);
    flatten_kernel<<<blocks_for(total), BLOCK, 0, st>>>(total, d_par, d_size);
    DevBuf b_keep, b_sel, b_nsel, b_tmp;
    uint8_t *d_keep = b_keep.alloc<uint8_t>(total);
    keep_kernel<<<blocks_for(total), BLOCK, 0, st>>>(total, d_par, d_size, prm->minarea, d_keep);
    HIPCHECK(hipGetLastError());
    uint32_t *d_sel = b_sel.alloc<uint32_t>(total);
    int64_t *d_nsel = b_nsel.alloc<int64_t>(1);
    hipcub::CountingInputIterator<uint32_t> count_it(0);
    size_t tmp_bytes = 0;
    HIPCHECK(hipcub::DeviceSelect::Flagged(nullptr, tmp_bytes, count_it, d_keep, d_sel, d_nsel, (int)total, st));
    void *d_tmp = b_tmp.alloc<char>(tmp_bytes);
    HIPCHECK(hipcub::DeviceSelect::Flagged(d_tmp, tmp_bytes, count_it, d_keep, d_sel, d_nsel, (int)total, st));
    int64_t n_kept = 0;
    HIPCHECK(hipMemcpyAsync(&n_kept, d_nsel, 8, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));

    // kept pixels grouped by component (stable: ascending raster index inside a component)
    DevBuf b_root, b_root2, b_spix, b_uniq, b_cnts, b_nruns;
    uint32_t *d_root = b_root.alloc<uint32_t>(n_kept), *d_root2 = b_root2.alloc<uint32_t>(n_kept);
    uint32_t *d_spix = b_spix.alloc<uint32_t>(n_kept);
    uint32_t *d_uniq = b_uniq.alloc<uint32_t>(n_kept);
    int32_t *d_cnts = b_cnts.alloc<int32_t>(n_kept);
    int32_t *d_nruns = b_nruns.alloc<int32_t>(1);
    std::vector<Parent> parents;
    std::vector<uint32_t> uniq;
    if (n_kept > 0) {
        root_kernel<<<blocks_for(n_kept), BLOCK, 0, st>>>(n_kept, d_sel, d_par, d_root);
        HIPCHECK(hipGetLastError());
        int bits = 1;
        while (bits < 32 && ((int64_t)1 << bits) < total) ++bits;
        size_t sb = 0;
        HIPCHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, sb, d_root, d_root2, d_sel, d_spix, (int)n_kept, 0, bits, st));
        DevBuf b_tmp2;
        void *d_tmp2 = b_tmp2.alloc<char>(sb);
        HIPCHECK(hipcub::DeviceRadixSort::SortPairs(d_tmp2, sb, d_root, d_root2, d_sel, d_spix, (int)n_kept, 0, bits, st));
        size_t rb = 0;
        HIPCHECK(hipcub::DeviceRunLengthEncode::Encode(nullptr, rb, d_root2, d_uniq, d_cnts, d_nruns, (int)n_kept, st));
        DevBuf b_tmp3;
        void *d_tmp3 = b_tmp3.alloc<char>(rb);
        HIPCHECK(hipcub::DeviceRunLengthEncode::Encode(d_tmp3, rb, d_root2, d_uniq, d_cnts, d_nruns, (int)n_kept, st));
        int32_t nruns = 0;
        HIPCHECK(hipMemcpyAsync(&nruns, d_nruns, 4, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipStreamSynchronize(st));
        std::vector<int32_t> cnts(nruns);
        uniq.resize(nruns);
        HIPCHECK(hipMemcpyAsync(cnts.data(), d_cnts, 4 * (size_t)nruns, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipMemcpyAsync(uniq.data(), d_uniq, 4 * (size_t)nruns, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipStreamSynchronize(st));
        parents.resize(nruns);
        int64_t s = 0;
        int img = 0;
        for (int r = 0; r < nruns; ++r) {
            while (img + 1 < n_img && desc[img + 1].pix_off <= (int64_t)uniq[r]) ++img;
            parents[r] = Parent{s, cnts[r], img};
            s += cnts[r];
        }
    }
    tm.mark();

    // deblending
    const int n_par = (int)parents.size();
    DevBuf b_parents, b_rank, b_nchild, b_cnpix, b_lds_list, b_glob_list, b_gscr;
    Parent *d_parents = b_parents.alloc<Parent>(n_par);
    int32_t *d_rank = b_rank.alloc<int32_t>(n_kept), *d_nchild = b_nchild.alloc<int32_t>(n_par);
    int32_t *d_cnpix = b_cnpix.alloc<int32_t>(n_kept);
    // bytes per pixel of DebWork: c, acc (8 + 8), lstat (6 x 8), g, leaf, lab, cnt, newid (5 x 4), nbr (32), lsig (8)
    const int64_t per_px = 16 + 48 + 20 + 32 + 8;
    const int64_t fixed_extra = 48 + 8;   // lstat's and lsig's extra entries
    const int64_t glob_stride = 184;      // >= per_px + fixed_extra, a multiple of 8 (a parent's slice starts 8-aligned)
    std::vector<int32_t> small_list, big_list;
    int64_t big_pixels = 0;
    for (int p = 0; p < n_par; ++p) {
        if (parents[p].npix <= lds_max) small_list.push_back(p);
        else { big_list.push_back(p); big_pixels += parents[p].npix; }
    }
    if (n_par > 0) {
        HIPCHECK(hipMemcpyAsync(d_parents, parents.data(), sizeof(Parent) * n_par, hipMemcpyHostToDevice, st));
        int32_t *d_small = b_lds_list.alloc<int32_t>(small_list.size());
        int32_t *d_big = b_glob_list.alloc<int32_t>(big_list.size());
        if (!small_list.empty()) {
            HIPCHECK(hipMemcpyAsync(d_small, small_list.data(), 4 * small_list.size(), hipMemcpyHostToDevice, st));
            size_t lds_bytes = (size_t)(per_px * lds_max + fixed_extra);
            deblend_kernel<<<(unsigned)small_list.size(), BLOCK, lds_bytes, st>>>(
                d_desc, d_parents, d_small, (int)small_list.size(), d_spix, d_conv, d_thr, prm->deblend_nthresh,
                prm->deblend_cont, prm->minarea, 1, lds_max, nullptr, 0, d_rank, d_nchild, d_cnpix);
            HIPCHECK(hipGetLastError());
        }
        if (!big_list.empty()) {
            HIPCHECK(hipMemcpyAsync(d_big, big_list.data(), 4 * big_list.size(), hipMemcpyHostToDevice, st));
            // each large parent works in its own slice of the scratch, [start, start + npix) * glob_stride bytes
            char *d_g = b_gscr.alloc<char>((size_t)glob_stride * n_kept + 64);
            deblend_kernel<<<(unsigned)big_list.size(), BLOCK, 0, st>>>(
                d_desc, d_parents, d_big, (int)big_list.size(), d_spix, d_conv, d_thr, prm->deblend_nthresh,
                prm->deblend_cont, prm->minarea, 0, 0, d_g, glob_stride, d_rank, d_nchild, d_cnpix);
            HIPCHECK(hipGetLastError());
        }
    }
    std::vector<int32_t> nchild(n_par), cnpix(n_kept);
    if (n_par > 0) {
        HIPCHECK(hipMemcpyAsync(nchild.data(), d_nchild, 4 * (size_t)n_par, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipMemcpyAsync(cnpix.data(), d_cnpix, 4 * (size_t)n_kept, hipMemcpyDeviceToHost, st));
    }
    HIPCHECK(hipStreamSynchronize(st));
    tm.mark();

    // objects: parents in raster order of their smallest pixel, children after their parent's position
    std::vector<ObjDesc> objs;
    std::vector<int64_t> obj_base(n_par);
    std::vector<int32_t> obj_local, obj_parent;
    std::vector<int32_t> n_obj_img(n_img, 0), n_par_img(n_img, 0), par_local(n_par);
    int64_t opos = 0;
    for (int p = 0; p < n_par; ++p) {
        const int img = parents[p].img;
        par_local[p] = n_par_img[img]++;
        obj_base[p] = (int64_t)objs.size();
        for (int r = 0; r < nchild[p]; ++r) {
            const int32_t np = cnpix[parents[p].start + r];
            objs.push_back(ObjDesc{opos, np, img});
            obj_local.push_back(n_obj_img[img]++);
#if CELESTE_DETECT_MUTANT == 11
            obj_parent.push_back(p);
#else
            obj_parent.push_back(par_local[p]);
#endif
            opos += np;
        }
    }
    const int n_obj = (int)objs.size();
    DevBuf b_objs, b_obase, b_opix, b_oout, b_seg, b_olocal;
    ObjDesc *d_objs = b_objs.alloc<ObjDesc>(n_obj);
    int64_t *d_obase = b_obase.alloc<int64_t>(n_par);
    uint32_t *d_opix = b_opix.alloc<uint32_t>(n_kept);
    ObjOut *d_oout = b_oout.alloc<ObjOut>(n_obj);
    int32_t *d_olocal = b_olocal.alloc<int32_t>(n_obj);
    int32_t *d_seg = maps ? b_seg.alloc<int32_t>(total) : nullptr;
    if (maps) HIPCHECK(hipMemsetAsync(d_seg, 0, total * 4, st));
    if (n_obj > 0) {
        HIPCHECK(hipMemcpyAsync(d_objs, objs.data(), sizeof(ObjDesc) * n_obj, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(d_obase, obj_base.data(), 8 * (size_t)n_par, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(d_olocal, obj_local.data(), 4 * (size_t)n_obj, hipMemcpyHostToDevice, st));
        scatter_kernel<<<n_par, BLOCK, 0, st>>>(d_parents, d_nchild, d_obase, d_objs, d_spix, d_rank, d_opix);
        HIPCHECK(hipGetLastError());
        moments_kernel<<<n_obj, BLOCK, 0, st>>>(d_desc, d_objs, d_opix, d_cal, d_oout, d_seg, d_olocal);
        HIPCHECK(hipGetLastError());
    }
    tm.mark();
    std::vector<ObjOut> oout(n_obj);
    std::vector<uint32_t> opix(n_kept);
    std::vector<float> rms(n_img), thr(n_img);
    if (n_obj > 0) {
        HIPCHECK(hipMemcpyAsync(oout.data(), d_oout, sizeof(ObjOut) * n_obj, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipMemcpyAsync(opix.data(), d_opix, 4 * (size_t)n_kept, hipMemcpyDeviceToHost, st));
    }
    HIPCHECK(hipMemcpyAsync(rms.data(), d_rms, 4 * (size_t)n_img, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(thr.data(), d_thr, 4 * (size_t)n_img, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));

    celeste_detect_result_t *res = host_calloc<celeste_detect_result_t>(1);
    struct ResGuard { celeste_detect_result_t *r; ~ResGuard() { free_result(r); } } rg{res};
    res->n_images = n_img;
    res->images = host_calloc<celeste_detect_image_result_t>(n_img);
    for (int n = 0; n < n_img; ++n) {
        celeste_detect_image_result_t &R = res->images[n];
        R.H = desc[n].H; R.W = desc[n].W; R.rms = rms[n]; R.thresh = thr[n];
        R.n_objects = n_obj_img[n]; R.n_parents = n_par_img[n];
        R.objects = host_calloc<celeste_detect_object_t>(R.n_objects);
        int64_t np = 0;
        for (int o = 0; o < n_obj; ++o) if (objs[o].img == n) np += objs[o].npix;
        R.n_pix = np;
        R.pix = host_calloc<int64_t>(np);
        if (maps) {
            size_t sz = (size_t)R.H * R.W;
            R.mask = host_calloc<uint8_t>(sz);
            R.segmap = host_calloc<int32_t>(sz);
            HIPCHECK(hipMemcpy(R.mask, d_mask + desc[n].pix_off, sz, hipMemcpyDeviceToHost));
            HIPCHECK(hipMemcpy(R.segmap, d_seg + desc[n].pix_off, sz * 4, hipMemcpyDeviceToHost));
        }
    }
    std::vector<int64_t> fill(n_img, 0);
    for (int o = 0; o < n_obj; ++o) {
        const int n = objs[o].img;
        celeste_detect_image_result_t &R = res->images[n];
        celeste_detect_object_t &O = R.objects[obj_local[o]];
        const ObjOut &s = oout[o];
        O.npix = objs[o].npix; O.xmin = s.xmin; O.xmax = s.xmax; O.ymin = s.ymin; O.ymax = s.ymax;
        O.parent = obj_parent[o]; O.reserved = 0; O.pix_offset = fill[n];
        O.x = s.x; O.y = s.y; O.x2 = s.x2; O.y2 = s.y2; O.xy = s.xy; O.a = s.a; O.b = s.b; O.theta = s.theta;
        O.flux = s.flux; O.peak = s.peak;
        for (int k = 0; k < objs[o].npix; ++k) R.pix[fill[n] + k] = (int64_t)opix[objs[o].pix_start + k] - desc[n].pix_off;
        fill[n] += objs[o].npix;
    }
    if (tm.on && tm.ev.size() == 7)
        for (int s = 0; s < 6; ++s) {
            float ms = 0;
            HIPCHECK(hipEventElapsedTime(&ms, tm.ev[s], tm.ev[s + 1]));
            res->stage_ms[s] = ms;
        }
    rg.r = nullptr;
    *out = res;
    return CELESTE_DETECT_OK;
}

}  // namespace

extern "C" {

int celeste_detect_version(void) { return CELESTE_DETECT_ABI_VERSION; }

const char *celeste_detect_strerror(int status) {
    switch (status) {
        case CELESTE_DETECT_OK: return "ok";
        case CELESTE_DETECT_ERR_INVALID_ARG: return "invalid argument";
        case CELESTE_DETECT_ERR_HIP: return "HIP runtime error";
        case CELESTE_DETECT_ERR_NO_DEVICE: return "no HIP device (detection has no CPU fallback)";
        case CELESTE_DETECT_ERR_ALLOC: return "host allocation failed";
        default: return "unknown status";
    }
}

int celeste_detect_run(int32_t device, int32_t n_images, const celeste_detect_image_t *images,
                       const celeste_detect_params_t *params, celeste_detect_result_t **out) {
    try {
        if (!out || !params || n_images < 0 || (n_images > 0 && !images)) return CELESTE_DETECT_ERR_INVALID_ARG;
        *out = nullptr;
        if (params->minarea < 1 || params->deblend_nthresh < 1 || !(params->deblend_cont >= 0) ||
            !(params->thresh > 0))
            return CELESTE_DETECT_ERR_INVALID_ARG;
        for (int n = 0; n < n_images; ++n)
            if (images[n].H < 1 || images[n].W < 1 || !images[n].pixels || !images[n].sky || !images[n].nelec_per_nmgy)
                return CELESTE_DETECT_ERR_INVALID_ARG;
        int count = 0;
        hipError_t e = hipGetDeviceCount(&count);
        if (e != hipSuccess || count <= 0) return CELESTE_DETECT_ERR_NO_DEVICE;
        if (device < 0 || device >= count) return CELESTE_DETECT_ERR_INVALID_ARG;
        if (n_images == 0) {
            celeste_detect_result_t *r = host_calloc<celeste_detect_result_t>(1);
            *out = r;
            return CELESTE_DETECT_OK;
        }
        return run(device, n_images, images, params, out);
    } catch (const std::bad_alloc &) {
        return CELESTE_DETECT_ERR_ALLOC;
    } catch (...) {
        return CELESTE_DETECT_ERR_HIP;
    }
}

void celeste_detect_result_free(celeste_detect_result_t *result) { free_result(result); }

}  // extern "C"
