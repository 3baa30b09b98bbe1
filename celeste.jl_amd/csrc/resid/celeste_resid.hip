// celeste_resid.hip -- libceleste_resid.so: whole-frame residuals and their peaks (include/celeste_resid.h).
//
// The engine's context code (engine_context.h) and its kernels' header are compiled into this library, unchanged: the patch table, the
// per-visit tables of prep_kernel, the spline coefficients and the bitmaps are the engine's, and the two densities are its
// star_value and galaxy_value.  The context, its growable buffers and the stage times are engine_client.h's.  One search:
//   prep_kernel            (the engine's) SrcImg and Comp of every visit of the context at the call's table
//   resid_model_kernel     a workgroup of 256 owns a tile of 32 x 8 pixels and walks the visits the host listed for it
//                          (ascending source), each staged in LDS once; writes lam and the tile's sums
//   resid_frame_kernel     one workgroup per image adds its tiles in a fixed order: n_px, n_bad, chi2, status
//   resid_filter_kernel    a workgroup owns 32 x 16 outputs; a = iota r / lam and b = iota^2 / lam with their halo of R
//                          pixels and the taps sit in LDS; writes N, D, coverage, z and the tile's z range
//   resid_zrange_kernel    one workgroup per image: z_max, z_min
//   peaks_count / peaks_scan / peaks_write   the peak rule per pixel, counts per 256 raster indices, an exclusive scan of
//                          the counts by one workgroup, and the records in (image, raster index) order
// The stack of a search's maps across images (celeste_resid_stack) is resid_stack.h: its kernels, its mutant switches.
// No floating-point atomic anywhere; a pixel's numbers depend on its own image only.
//
// LDS of the filter: (32 + 24) x (16 + 24) doubles twice and 25 x 25 taps = 40.8 KB at the largest radius, so three
// workgroups share a CU's 160 KB; a lane reads two LDS doubles and one tap per (tap, output) for three fp64 FMAs.
#include "../engine_context.h"
#include "../engine_client.h"
#include "../../../include/celeste_resid.h"

// Mutation testing (tests/test_resid_mutants.py builds this library with -DCELESTE_RESID_MUTANT=k and checks that
// tests/test_gpu_resid.py notices).  A mutant changes arithmetic or an index inside the same array; never a size, a launch, a
// barrier or anything that could leave an array.  0 = the product;
//   1 = a source's light also in its patch's last column (b < W2; its bitmap index a + H2 b stays <= H2 W2 - 1)
//   2 = the bitmap is ignored in the frame model
//   3 = phi transposed: tap (dh, dw) read at (dw, dh) (the tap table is square)
//   4 = iota taken by column in the filter, clamped to its H entries (iota[min(w, H - 1)])
//   5 = the tie rule uses >= on both sides
// Never defined in the shipped build.
#ifndef CELESTE_RESID_MUTANT
#define CELESTE_RESID_MUTANT 0
#endif

#define RS_TH 32                         // rows of a tile (h runs fastest in a plane)
#define RS_MW 8                          // columns of a model tile: 256 pixels, one per lane
#define RS_FW 16                         // columns of a filter tile: two outputs per lane
#define RS_R CELESTE_RESID_MAX_RADIUS
#define RS_LH (RS_TH + 2 * RS_R)         // the filter's LDS tile at the largest radius
#define RS_LW (RS_FW + 2 * RS_R)
#define RS_PB 256                        // raster indices per workgroup of the peak kernels

struct ResidTile { int32_t h0, w0, v0, v1; };               // origin; its visits are tile_vis[v0 .. v1)
struct ResidTileRec { double chi2; int32_t n_px, n_bad; };
// an image of the call: its planes start at `off`; mt0 / ft0 / pb0: its first model tile, filter tile and peak block in the
// call; tile_base: its first tile in the context's tile table; tap_off: its taps
struct ResidImg {
    int32_t img, H, W, input_bad;
    int64_t off;
    int32_t mt0, ft0, pb0, tile_base;
    int32_t tap_off, pad;
};

// the image whose range [starts[k], starts[k + 1]) holds block b
__device__ __forceinline__ int resid_slot(const int32_t *__restrict__ starts, int n, int b) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (starts[mid] <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// a fixed tree over the workgroup's 4 wavefronts: butterfly inside a wavefront, then the four partial sums in order
__device__ __forceinline__ double block_sum_256(double x, double *sh) {
    x = wave_sum(x);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ void __launch_bounds__(256)
resid_model_kernel(const ResidImg *__restrict__ cimg, const int32_t *__restrict__ mt_start, int n_img,
                   const ResidTile *__restrict__ tiles, const int32_t *__restrict__ tile_vis,
                   const DevImage *__restrict__ images, const DevPatch *__restrict__ patches, const double *__restrict__ coefs,
                   const uint8_t *__restrict__ bitmaps, const SrcImg *__restrict__ srcimg, const Comp *__restrict__ comps,
                   int NC, double *__restrict__ lam_plane, ResidTileRec *__restrict__ rec) {
    __shared__ double etab[64];
    __shared__ Comp tc[14 * CEL_MAXK];
    __shared__ double sh[4];
    const int t = threadIdx.x;
    const int k = resid_slot(mt_start, n_img, blockIdx.x);
    const ResidImg ci = cimg[k];
    const ResidTile tl = tiles[ci.tile_base + ((int)blockIdx.x - ci.mt0)];
    const DevImage &img = images[ci.img];
    const int H = ci.H, W = ci.W;
    const int h = tl.h0 + (t & (RS_TH - 1)), w = tl.w0 + (t >> 5);
    const bool inb = h < H && w < W;
    const size_t gi = inb ? (size_t)h + (size_t)H * w : 0;
    const float xf = img.pixels[gi], skyf = img.sky[gi];
    const double iota = (double)img.iota[inb ? h : 0];
    exp_table_init(etab);
    const double hh = (double)(h + 1), ww = (double)(w + 1);
    double m = 0.0;
    for (int e = tl.v0; e < tl.v1; ++e) {                      // (uniform over the workgroup)
        const int sn = tile_vis[e];
        const DevPatch &P = patches[sn];
        const int a = h - P.off_h, b = w - P.off_w;            // 0-based in the patch
#if CELESTE_RESID_MUTANT == 1
        bool in = inb & (a >= 0) & (a < P.H2) & (b >= 0) & (b < P.W2);
#else
        bool in = inb & (a >= 0) & (a < P.H2) & (b >= 0) & (b < P.W2 - 1);
#endif
#if CELESTE_RESID_MUTANT == 2
        if (in) in = !isnan(xf) || P.bitmap_off >= 0;
#else
        if (in) in = P.bitmap_off >= 0 ? bitmaps[P.bitmap_off + a + (int64_t)P.H2 * b] != 0 : !isnan(xf);
#endif
        __syncthreads();
        {
            const double *s = reinterpret_cast<const double *>(comps + (size_t)sn * NC);
            double *d = reinterpret_cast<double *>(tc);
            for (int i = t; i < NC * 8; i += 256) d[i] = s[i];
        }
        __syncthreads();
        if (in) {
            const SrcImg si = srcimg[sn];
            // (a non-finite row leaves a non-finite position: the frame is flagged, the densities are not asked)
            m += isfinite(si.m1 + si.m2) ? visit_light(si, tc, NC, coefs + (size_t)P.stamp * (CEL_COEF * CEL_COEF), etab, hh, ww)
                                         : (double)NAN;
        }
    }
    const double lam = __dmul_rn(iota, (double)skyf + m);
    if (inb) lam_plane[ci.off + (int64_t)gi] = lam;
    const bool bad = inb && !(lam > 0.0 && isfinite(lam));
    const bool cnt = inb && !isnan(xf);
    double c2 = 0.0;
    if (cnt && !bad) { const double r = __dsub_rn((double)xf, lam); c2 = __dmul_rn(r, r) / lam; }
    c2 = block_sum_256(c2, sh);
    const int n_px = __syncthreads_count(cnt), n_bad = __syncthreads_count(bad);
    if (t == 0) { ResidTileRec r; r.chi2 = c2; r.n_px = n_px; r.n_bad = n_bad; rec[blockIdx.x] = r; }
}

// one workgroup per image of the call: lane t adds the tiles t, t + 256, ... one after another, then the fixed tree
__global__ void __launch_bounds__(256)
resid_frame_kernel(const ResidImg *__restrict__ cimg, const int32_t *__restrict__ mt_start, const ResidTileRec *__restrict__ rec,
                   celeste_resid_frame_t *__restrict__ frames) {
    __shared__ double sh[4];
    __shared__ long long shn[2][4];
    const int k = blockIdx.x, t = threadIdx.x;
    const ResidImg ci = cimg[k];
    double c2 = 0.0;
    long long n_px = 0, n_bad = 0;
    for (int i = mt_start[k] + t; i < mt_start[k + 1]; i += 256) { c2 += rec[i].chi2; n_px += rec[i].n_px; n_bad += rec[i].n_bad; }
    c2 = block_sum_256(c2, sh);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { n_px += __shfl_xor(n_px, o, 64); n_bad += __shfl_xor(n_bad, o, 64); }
    if ((t & 63) == 0) { shn[0][t >> 6] = n_px; shn[1][t >> 6] = n_bad; }
    __syncthreads();
    if (t == 0) {
        celeste_resid_frame_t f;
        f.image = ci.img;
        f.n_px = shn[0][0] + shn[0][1] + shn[0][2] + shn[0][3];
        f.n_bad = shn[1][0] + shn[1][1] + shn[1][2] + shn[1][3];
        f.status = ci.input_bad ? CELESTE_ERR_NONFINITE_INPUT : (f.n_bad > 0 ? CELESTE_ERR_NONFINITE_RESULT : CELESTE_OK);
        f.chi2 = f.status != CELESTE_OK ? (double)NAN : c2;
        f.z_max = f.z_min = (double)NAN;
        frames[k] = f;
    }
}

__global__ void __launch_bounds__(256)
resid_filter_kernel(const ResidImg *__restrict__ cimg, const int32_t *__restrict__ ft_start, int n_img,
                    const DevImage *__restrict__ images, const celeste_resid_frame_t *__restrict__ frames,
                    const double *__restrict__ taps, int R, double min_cov, const double *__restrict__ lam_plane,
                    double *__restrict__ n_plane, double *__restrict__ d_plane, double *__restrict__ z_plane,
                    double *__restrict__ c_plane, double2 *__restrict__ zrec) {
    __shared__ double A[RS_LH * RS_LW];
    __shared__ double B[RS_LH * RS_LW];                       // -1: not a good tap
    __shared__ double phi[(2 * RS_R + 1) * (2 * RS_R + 1)];
    __shared__ double shz[2][4];
    const int t = threadIdx.x;
    const int k = resid_slot(ft_start, n_img, blockIdx.x);
    const ResidImg ci = cimg[k];
    const DevImage &img = images[ci.img];
    const int H = ci.H, W = ci.W;
    const int tiles_h = (H + RS_TH - 1) / RS_TH;
    const int tb = (int)blockIdx.x - ci.ft0;
    const int tw_i = tb / tiles_h, th_i = tb - tw_i * tiles_h;
    const int h0 = th_i * RS_TH, w0 = tw_i * RS_FW;
    const int T = 2 * R + 1, LH = RS_TH + 2 * R, LW = RS_FW + 2 * R;
    const bool frame_ok = frames[k].status == CELESTE_OK;
    for (int i = t; i < T * T; i += 256) phi[i] = taps[ci.tap_off + i];
    for (int i = t; i < LH * LW; i += 256) {
        const int lw = i / LH, lh = i - lw * LH;
        const int gh = h0 - R + lh, gw = w0 - R + lw;
        double a = 0.0, b = -1.0;
        if (gh >= 0 && gh < H && gw >= 0 && gw < W) {
            const size_t gi = (size_t)gh + (size_t)H * gw;
            const double x = (double)img.pixels[gi], lam = lam_plane[ci.off + (int64_t)gi];
#if CELESTE_RESID_MUTANT == 4
            const double iota = (double)img.iota[min(gw, H - 1)];
#else
            const double iota = (double)img.iota[gh];
#endif
            if (!isnan(x) && lam > 0.0) {
                a = __dmul_rn(iota, __dsub_rn(x, lam)) / lam;
                b = __dmul_rn(iota, iota) / lam;
            }
        }
        A[i] = a;
        B[i] = b;
    }
    __syncthreads();
    const int lh = t & (RS_TH - 1), lw = t >> 5;              // outputs (lh, lw) and (lh, lw + 8) of the tile
    double Ns[2] = {0.0, 0.0}, Ds[2] = {0.0, 0.0}, cs[2] = {0.0, 0.0}, tot = 0.0;
    for (int dw = 0; dw < T; ++dw) {
        for (int dh = 0; dh < T; ++dh) {
#if CELESTE_RESID_MUTANT == 3
            const double p = phi[dh * T + dw];
#else
            const double p = phi[dw * T + dh];
#endif
            const double p2 = __dmul_rn(p, p);
            tot += p;
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                const int li = (lh + dh) + LH * (lw + 8 * o + dw);
                const double b = B[li];
                const bool good = b >= 0.0;
                Ns[o] += p * A[li];                          // (a is 0 at a tap that is not good)
                Ds[o] += good ? p2 * b : 0.0;
                cs[o] += good ? p : 0.0;
            }
        }
    }
    double zmax = -INFINITY, zmin = INFINITY;
#pragma unroll
    for (int o = 0; o < 2; ++o) {
        const int h = h0 + lh, w = w0 + lw + 8 * o;
        if (h < H && w < W) {
            const int64_t gi = ci.off + (int64_t)h + (int64_t)H * w;
            const double cov = cs[o] / tot;
            double z = (double)NAN;
            if (frame_ok && !(cov < min_cov) && Ds[o] != 0.0) z = Ns[o] / sqrt(Ds[o]);
            n_plane[gi] = frame_ok ? Ns[o] : (double)NAN;
            d_plane[gi] = frame_ok ? Ds[o] : (double)NAN;
            c_plane[gi] = frame_ok ? cov : (double)NAN;
            z_plane[gi] = z;
            if (isfinite(z)) { zmax = fmax(zmax, z); zmin = fmin(zmin, z); }
        }
    }
    zmax = wave_max(zmax);
    zmin = -wave_max(-zmin);
    if ((t & 63) == 0) { shz[0][t >> 6] = zmax; shz[1][t >> 6] = zmin; }
    __syncthreads();
    if (t == 0)
        zrec[blockIdx.x] = make_double2(fmax(fmax(shz[0][0], shz[0][1]), fmax(shz[0][2], shz[0][3])),
                                        fmin(fmin(shz[1][0], shz[1][1]), fmin(shz[1][2], shz[1][3])));
}

__global__ void __launch_bounds__(256)
resid_zrange_kernel(const int32_t *__restrict__ ft_start, const double2 *__restrict__ zrec, celeste_resid_frame_t *__restrict__ frames) {
    __shared__ double shz[2][4];
    const int k = blockIdx.x, t = threadIdx.x;
    double zmax = -INFINITY, zmin = INFINITY;
    for (int i = ft_start[k] + t; i < ft_start[k + 1]; i += 256) { zmax = fmax(zmax, zrec[i].x); zmin = fmin(zmin, zrec[i].y); }
    zmax = wave_max(zmax);
    zmin = -wave_max(-zmin);
    if ((t & 63) == 0) { shz[0][t >> 6] = zmax; shz[1][t >> 6] = zmin; }
    __syncthreads();
    if (t == 0 && frames[k].status == CELESTE_OK) {
        zmax = fmax(fmax(shz[0][0], shz[0][1]), fmax(shz[0][2], shz[0][3]));
        zmin = fmin(fmin(shz[1][0], shz[1][1]), fmin(shz[1][2], shz[1][3]));
        frames[k].z_max = zmax >= zmin ? zmax : (double)NAN;     // (no finite z: the range is still (-inf, inf) turned round)
        frames[k].z_min = zmax >= zmin ? zmin : (double)NAN;
    }
}

// ---- peaks -----------------------------------------------------------------------------------------------------------------
struct PeakImg { int32_t img, H, W, pad; int64_t off; };

// the peak rule at raster index r of an H x W plane z (r < H W)
__device__ __forceinline__ bool resid_is_peak(const double *__restrict__ z, int H, int W, int r, double thr) {
    const double z0 = z[r];
    if (!(z0 >= thr)) return false;
    const int w = r / H, h = r - w * H;
    bool ok = true;
#pragma unroll
    for (int dw = -1; dw <= 1; ++dw)
#pragma unroll
        for (int dh = -1; dh <= 1; ++dh) {
            if (dh == 0 && dw == 0) continue;
            const int qh = h + dh, qw = w + dw;
            if (qh < 0 || qh >= H || qw < 0 || qw >= W) continue;
            const double zq = z[qh + H * qw];
            if (isnan(zq)) continue;
#if CELESTE_RESID_MUTANT == 5
            ok &= z0 >= zq;
#else
            ok &= (dw < 0 || (dw == 0 && dh < 0)) ? z0 > zq : z0 >= zq;     // (q has the lower raster index)
#endif
        }
    return ok;
}

__device__ __forceinline__ double resid_subpixel(double zm, double z0, double zp, bool have) {
    if (!have || isnan(zm) || isnan(zp)) return 0.0;
    const double den = __dadd_rn(__dsub_rn(zm, __dmul_rn(2.0, z0)), zp);
    if (!(den < 0.0)) return 0.0;
    const double d = __dmul_rn(0.5, __dsub_rn(zm, zp)) / den;
    return fmin(0.5, fmax(-0.5, d));
}

__global__ void __launch_bounds__(RS_PB)
peaks_count_kernel(const PeakImg *__restrict__ pimg, const int32_t *__restrict__ pb_start, int n_img,
                   const double *__restrict__ z_plane, double thr, int32_t *__restrict__ counts) {
    const int k = resid_slot(pb_start, n_img, blockIdx.x);
    const PeakImg pi = pimg[k];
    const int64_t r = (int64_t)((int)blockIdx.x - pb_start[k]) * RS_PB + threadIdx.x;
    const bool pk = r < (int64_t)pi.H * pi.W && resid_is_peak(z_plane + pi.off, pi.H, pi.W, (int)r, thr);
    const int n = __syncthreads_count(pk);
    if (threadIdx.x == 0) counts[blockIdx.x] = n;
}

// exclusive scan of n counts by one workgroup of 1024: a lane adds its run of consecutive counts, the runs' sums are scanned
// in LDS, the lane writes its run's offsets; total[0] = the sum
__global__ void __launch_bounds__(1024)
peaks_scan_kernel(const int32_t *__restrict__ counts, int n, int64_t *__restrict__ offsets, int64_t *__restrict__ total) {
    __shared__ long long sh[1024];
    const int t = threadIdx.x;
    const int per = (n + 1023) / 1024;
    const int i0 = min(n, t * per), i1 = min(n, i0 + per);
    long long s = 0;
    for (int i = i0; i < i1; ++i) s += counts[i];
    sh[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const long long v = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += v;
        __syncthreads();
    }
    long long run = sh[t] - s;
    for (int i = i0; i < i1; ++i) { offsets[i] = run; run += counts[i]; }
    if (t == 1023) total[0] = sh[1023];
}

__global__ void __launch_bounds__(RS_PB)
peaks_write_kernel(const PeakImg *__restrict__ pimg, const int32_t *__restrict__ pb_start, int n_img,
                   const double *__restrict__ z_plane, const double *__restrict__ n_plane, const double *__restrict__ d_plane,
                   const double *__restrict__ c_plane, double thr, const int64_t *__restrict__ offsets, int64_t max_out,
                   celeste_resid_candidate_t *__restrict__ out) {
    __shared__ int shc[RS_PB / 64];
    const int k = resid_slot(pb_start, n_img, blockIdx.x);
    const PeakImg pi = pimg[k];
    const int H = pi.H, W = pi.W, t = threadIdx.x;
    const int64_t r = (int64_t)((int)blockIdx.x - pb_start[k]) * RS_PB + t;
    const double *z = z_plane + pi.off;
    const bool pk = r < (int64_t)H * W && resid_is_peak(z, H, W, (int)r, thr);
    const unsigned long long bal = __ballot(pk);
    if ((t & 63) == 0) shc[t >> 6] = __popcll(bal);
    __syncthreads();
    int rank = __popcll(bal & ((1ull << (t & 63)) - 1ull));
    for (int wv = 0; wv < (t >> 6); ++wv) rank += shc[wv];
    const int64_t pos = offsets[blockIdx.x] + rank;
    if (!pk || pos >= max_out) return;
    const int w = (int)r / H, h = (int)r - w * H;
    const double z0 = z[r];
    celeste_resid_candidate_t c;
    c.image = pi.img; c.h = h; c.w = w; c.reserved = 0;
    const bool hv = h > 0 && h < H - 1, wv2 = w > 0 && w < W - 1;
    c.dh = resid_subpixel(hv ? z[r - 1] : 0.0, z0, hv ? z[r + 1] : 0.0, hv);
    c.dw = resid_subpixel(wv2 ? z[r - H] : 0.0, z0, wv2 ? z[r + H] : 0.0, wv2);
    c.z = z0;
    const double Dv = d_plane ? d_plane[pi.off + r] : (double)NAN;
    c.D = Dv;
    c.f = n_plane ? n_plane[pi.off + r] / Dv : (double)NAN;
    c.cov = c_plane ? c_plane[pi.off + r] : (double)NAN;
    out[pos] = c;
}

// N, D, coverage of the last search's maps at n pixels; slot[image] = the image's place in the last search
__global__ void resid_sample_kernel(int64_t n, const int32_t *__restrict__ image, const int32_t *__restrict__ hs,
                                    const int32_t *__restrict__ ws, const int32_t *__restrict__ slot,
                                    const ResidImg *__restrict__ cimg, const double *__restrict__ n_plane,
                                    const double *__restrict__ d_plane, const double *__restrict__ z_plane,
                                    const double *__restrict__ c_plane, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ResidImg ci = cimg[slot[image[i]]];
    const int h = hs[i], w = ws[i];
    double N = 0.0, D = 0.0, cov = 0.0;
    if (h >= 0 && h < ci.H && w >= 0 && w < ci.W) {
        const int64_t gi = ci.off + (int64_t)h + (int64_t)ci.H * w;
        cov = c_plane[gi];
        const bool masked = isnan(z_plane[gi]);
        N = masked ? (double)NAN : n_plane[gi];
        D = masked ? (double)NAN : d_plane[gi];
    }
    out[i] = N; out[n + i] = D; out[2 * n + i] = cov;
}

#include "resid_stack.h"

// ---- host side ---------------------------------------------------------------------------------------------------------------
enum { RB_VP = 0, RB_TILES, RB_TILE_VIS, RB_LAM, RB_N, RB_D, RB_Z, RB_COV, RB_REC, RB_FRAMES, RB_TAPS, RB_CIMG, RB_STARTS,
       RB_PIMG, RB_COUNTS, RB_OFFSETS, RB_TOTAL, RB_CAND, RB_ZREC, RB_SLOT, RB_SAMPLE_IN, RB_SAMPLE_OUT,
       // the stack's
       RB_SK_IMGS, RB_SK_WTS, RB_SK_N, RB_SK_D, RB_SK_Z, RB_SK_CNT, RB_SK_REC, RB_SK_FRAMES, RB_SK_PIMG, RB_SK_STARTS, RB_SK_COUNTS,
       RB_SK_OFFSETS, RB_SK_TOTAL, RB_SK_PEAKS, RB_SK_CAND, RB_COUNT };

struct celeste_resid_ctx : ClientCtx<RB_COUNT, 5, 4> {
    // the tile table of every image (built once: the patches do not change), and its host mirror's offsets
    bool tiles_built = false;
    std::vector<int32_t> tile_off;         // per image: its first tile (N + 1)
    // the last search
    std::vector<ResidImg> cimg;
    std::vector<int32_t> slot;             // per image of the problem: its place in cimg, -1: not searched
    double min_cov = 0.0;
    bool searched = false;
    // host staging of one call: kept here so that it outlives the asynchronous copies
    std::vector<int32_t> starts;
    std::vector<PeakImg> pimg;
    std::vector<double> taps;
    std::vector<int32_t> sample_in;
    std::vector<double> sample_out;
    // the stack: the frames of the last search that are OK; the last stack's grid and channels; its events and times
    std::vector<char> frame_ok;
    bool stacked = false;
    int32_t sk_H = 0, sk_W = 0, sk_ch = 0;
    std::vector<StackImg> sk_imgs;
    std::vector<double> sk_wts;
    std::vector<PeakImg> sk_pimg;
    std::vector<int32_t> sk_starts;
    hipEvent_t sk_ev[3] = {};
    float sk_ms[2] = {};
};

extern "C" int celeste_resid_version(void) { return CELESTE_RESID_ABI_VERSION; }

extern "C" const char *celeste_resid_strerror(int status) {
    if (status == CELESTE_RESID_TRUNCATED) return "more candidates than max_candidates: the list is truncated";
    return celeste_strerror(status);
}

extern "C" void celeste_resid_opts_default(celeste_resid_opts_t *o) {
    if (!o) return;
    o->threshold = 5.0; o->min_coverage = 0.8; o->radius = 8; o->psf_K = 0; o->psf = nullptr;
}

extern "C" int celeste_resid_ctx_create(const celeste_problem_t *problem, int device, celeste_resid_ctx_t **out) try {
    return client_create(problem, device, out);
} ABI_CATCH

extern "C" void celeste_resid_ctx_destroy(celeste_resid_ctx_t *f) {
    if (f && f->c) {
        (void)hipSetDevice(f->c->device);
        (void)hipStreamSynchronize(f->c->stream);
        for (auto &e : f->sk_ev) if (e) (void)hipEventDestroy(e);
    }
    client_destroy(f);
}

// The tile table: for every image its 32 x 8 tiles in (column of tiles, row of tiles) order, and per tile the visits whose
// patch rectangle without its last column meets it, in ascending visit (hence source) order.  Uploaded once.
static int resid_build_tiles(celeste_resid_ctx_t *f) {
    celeste_ctx_t *c = f->c;
    const int N = c->N;
    f->tile_off.assign((size_t)N + 1, 0);
    std::vector<int> th((size_t)N), tw((size_t)N);
    for (int n = 0; n < N; ++n) {
        const DevImage &im = c->imgs->h_images[n];
        th[n] = (im.H + RS_TH - 1) / RS_TH; tw[n] = (im.W + RS_MW - 1) / RS_MW;
        const int64_t nt = (int64_t)f->tile_off[n] + (int64_t)th[n] * tw[n];
        if (nt > 0x7fffff00ll) return CELESTE_ERR_INVALID_ARG;
        f->tile_off[n + 1] = (int32_t)nt;
    }
    const size_t n_tiles = (size_t)f->tile_off[N];
    std::vector<int64_t> cnt(n_tiles + 1, 0);
    const int64_t V = c->V;
    // the tiles a visit's rectangle meets: rows [a0, a1), columns [b0, b1) of tiles of its image (clipped to the frame)
    auto span = [&](int64_t v, int &n, int &a0, int &a1, int &b0, int &b1) {
        const DevPatch &P = c->h_patches[v];
        if (P.H2 <= 0 || P.W2 <= 1) return false;
        n = c->h_vis_img[v];
        const DevImage &im = c->imgs->h_images[n];
        const int h_lo = std::max(0, P.off_h), h_hi = std::min(im.H, P.off_h + P.H2);
        const int w_lo = std::max(0, P.off_w), w_hi = std::min(im.W, P.off_w + P.W2 - 1);
        if (h_lo >= h_hi || w_lo >= w_hi) return false;
        a0 = h_lo / RS_TH; a1 = (h_hi - 1) / RS_TH + 1; b0 = w_lo / RS_MW; b1 = (w_hi - 1) / RS_MW + 1;
        return true;
    };
    for (int64_t v = 0; v < V; ++v) {
        int n, a0, a1, b0, b1;
        if (!span(v, n, a0, a1, b0, b1)) continue;
        for (int b = b0; b < b1; ++b) for (int a = a0; a < a1; ++a) ++cnt[(size_t)f->tile_off[n] + a + (size_t)th[n] * b + 1];
    }
    for (size_t i = 0; i < n_tiles; ++i) cnt[i + 1] += cnt[i];
    if (cnt[n_tiles] > 0x7fffff00ll) return CELESTE_ERR_INVALID_ARG;
    std::vector<int32_t> vis((size_t)cnt[n_tiles]);
    std::vector<int64_t> fill(cnt.begin(), cnt.end() - 1);
    for (int64_t v = 0; v < V; ++v) {
        int n, a0, a1, b0, b1;
        if (!span(v, n, a0, a1, b0, b1)) continue;
        for (int b = b0; b < b1; ++b) for (int a = a0; a < a1; ++a) vis[(size_t)fill[(size_t)f->tile_off[n] + a + (size_t)th[n] * b]++] = (int32_t)v;
    }
    std::vector<ResidTile> tiles(n_tiles);
    for (int n = 0; n < N; ++n)
        for (int b = 0; b < tw[n]; ++b) for (int a = 0; a < th[n]; ++a) {
            const size_t i = (size_t)f->tile_off[n] + a + (size_t)th[n] * b;
            tiles[i].h0 = a * RS_TH; tiles[i].w0 = b * RS_MW; tiles[i].v0 = (int32_t)cnt[i]; tiles[i].v1 = (int32_t)cnt[i + 1];
        }
    ResidTile *d_tiles = nullptr;
    int32_t *d_vis = nullptr;
    if (client_get(f, RB_TILES, n_tiles * sizeof(ResidTile), &d_tiles) != hipSuccess ||
        client_get(f, RB_TILE_VIS, vis.size() * sizeof(int32_t), &d_vis) != hipSuccess) return CELESTE_ERR_HIP;
    // (synchronous copies: the vectors are locals)
    if (n_tiles) HIP_TRY(hipMemcpy(d_tiles, tiles.data(), n_tiles * sizeof(ResidTile), hipMemcpyHostToDevice));
    if (!vis.empty()) HIP_TRY(hipMemcpy(d_vis, vis.data(), vis.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    f->tiles_built = true;
    return CELESTE_OK;
}

static double resid_phi(const double *psf, int K, double dh, double dw) {
    double s = 0.0;
    for (int k = 0; k < K; ++k) {
        const double *p = psf + 6 * k;
        const double det = p[3] * p[5] - p[4] * p[4];
        const double d0 = dh - p[1], d1 = dw - p[2];
        const double q = (p[5] * d0 * d0 - 2.0 * p[4] * d0 * d1 + p[3] * d1 * d1) / det;
        s += p[0] * std::exp(-0.5 * q) / (2.0 * M_PI * std::sqrt(det));
    }
    return s;
}

// count, scan and write over n_img images described by d_pimg / d_pb (pb_start has n_img + 1 entries, n_blocks the last)
static int resid_run_peaks(hipStream_t st, const PeakImg *d_pimg, const int32_t *d_pb, int n_img, int n_blocks,
                           const double *d_z, const double *d_n, const double *d_d, const double *d_c, double thr,
                           int32_t *d_counts, int64_t *d_offsets, int64_t *d_total, celeste_resid_candidate_t *d_cand, int64_t max_out) {
    if (n_blocks > 0)
        hipLaunchKernelGGL(peaks_count_kernel, dim3((unsigned)n_blocks), dim3(RS_PB), 0, st, d_pimg, d_pb, n_img, d_z, thr, d_counts);
    hipLaunchKernelGGL(peaks_scan_kernel, dim3(1), dim3(1024), 0, st, d_counts, n_blocks, d_offsets, d_total);
    if (n_blocks > 0 && max_out > 0)
        hipLaunchKernelGGL(peaks_write_kernel, dim3((unsigned)n_blocks), dim3(RS_PB), 0, st, d_pimg, d_pb, n_img, d_z, d_n, d_d, d_c,
                           thr, d_offsets, max_out, d_cand);
    HIP_TRY(hipGetLastError());
    return CELESTE_OK;
}

extern "C" int celeste_resid_search(celeste_resid_ctx_t *f, const double *vp, int32_t n_images, const int32_t *images,
                                    const celeste_resid_opts_t *opts, celeste_resid_frame_t *out_frames,
                                    celeste_resid_candidate_t *out_candidates, int64_t max_candidates, int64_t *n_found,
                                    int32_t *status) try {
    if (!f || !f->c || !vp || !opts || !opts->psf || !out_frames || !n_found || !status) return CELESTE_ERR_INVALID_ARG;
    if (opts->radius < 1 || opts->radius > RS_R || opts->psf_K < 1 || opts->psf_K > 16) return CELESTE_ERR_INVALID_ARG;
    if (max_candidates < 0 || (max_candidates > 0 && !out_candidates)) return CELESTE_ERR_INVALID_ARG;
    celeste_ctx_t *c = f->c;
    const int N = c->N;
    if (!images) n_images = N;
    if (n_images < 0) return CELESTE_ERR_INVALID_ARG;
    std::vector<int32_t> slot((size_t)N, -1);
    for (int k = 0; k < n_images; ++k) {
        const int n = images ? images[k] : k;
        if (n < 0 || n >= N || slot[n] >= 0) return CELESTE_ERR_INVALID_ARG;
        slot[n] = k;
    }
    *n_found = 0;
    *status = CELESTE_OK;
    if (n_images == 0) return CELESTE_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (!f->tiles_built) { const int rc = resid_build_tiles(f); if (rc != CELESTE_OK) return rc; }
    // images touched by a source with a non-finite row
    std::vector<char> input_bad((size_t)N, 0);
    for (int s = 0; s < c->S; ++s) {
        bool fin = true;
        for (int j = 0; j < CEL_P; ++j) fin &= std::isfinite(vp[(size_t)s * CEL_P + j]);
        if (fin) continue;
        for (int v = c->h_vis_off[s]; v < c->h_vis_off[s + 1]; ++v)
            if (c->h_patches[v].H2 > 0 && c->h_patches[v].W2 > 0) input_bad[c->h_vis_img[v]] = 1;
    }
    const int R = opts->radius, T = 2 * R + 1, K = opts->psf_K;
    const size_t ni = (size_t)n_images;
    f->searched = false;
    f->stacked = false;
    std::vector<ResidImg> &cimg = f->cimg;
    cimg.assign(ni, ResidImg());
    std::vector<int32_t> &starts = f->starts;                 // [3][ni + 1]: model tiles, filter tiles, peak blocks
    starts.assign(3 * (ni + 1), 0);
    f->pimg.assign(ni, PeakImg());
    f->taps.assign(ni * T * T, 0.0);
    int64_t off = 0, mt = 0, ft = 0, pb = 0;
    for (size_t k = 0; k < ni; ++k) {
        const int n = images ? images[k] : (int)k;
        const DevImage &im = c->imgs->h_images[n];
        ResidImg &ci = cimg[k];
        ci.img = n; ci.H = im.H; ci.W = im.W; ci.input_bad = input_bad[n];
        ci.off = off; ci.mt0 = (int32_t)mt; ci.ft0 = (int32_t)ft; ci.pb0 = (int32_t)pb; ci.tile_base = f->tile_off[n];
        ci.tap_off = (int32_t)(k * T * T); ci.pad = 0;
        const int64_t npx = (int64_t)im.H * im.W;
        if (npx >= 0x7fffff00ll) return CELESTE_ERR_INVALID_ARG;
        starts[k] = (int32_t)mt; starts[(ni + 1) + k] = (int32_t)ft; starts[2 * (ni + 1) + k] = (int32_t)pb;
        f->pimg[k].img = n; f->pimg[k].H = im.H; f->pimg[k].W = im.W; f->pimg[k].pad = 0; f->pimg[k].off = off;
        off += npx;
        mt += f->tile_off[n + 1] - f->tile_off[n];
        ft += (int64_t)((im.H + RS_TH - 1) / RS_TH) * ((im.W + RS_FW - 1) / RS_FW);
        pb += (npx + RS_PB - 1) / RS_PB;
        if (mt > 0x7fffff00ll || pb > 0x7fffff00ll) return CELESTE_ERR_INVALID_ARG;
        double *tp = f->taps.data() + k * T * T;
        const double *psf = opts->psf + (size_t)n * K * 6;
        for (int dw = -R; dw <= R; ++dw) for (int dh = -R; dh <= R; ++dh) tp[(dw + R) * T + (dh + R)] = resid_phi(psf, K, dh, dw);
    }
    starts[ni] = (int32_t)mt; starts[(ni + 1) + ni] = (int32_t)ft; starts[2 * (ni + 1) + ni] = (int32_t)pb;
    const size_t plane = (size_t)off * sizeof(double);
    double *d_vp = nullptr, *d_lam = nullptr, *d_n = nullptr, *d_d = nullptr, *d_z = nullptr, *d_c = nullptr, *d_taps = nullptr;
    ResidTile *d_tiles = nullptr;
    int32_t *d_vis = nullptr, *d_starts = nullptr, *d_counts = nullptr, *d_slot = nullptr;
    ResidTileRec *d_rec = nullptr;
    celeste_resid_frame_t *d_frames = nullptr;
    ResidImg *d_cimg = nullptr;
    PeakImg *d_pimg = nullptr;
    int64_t *d_offsets = nullptr, *d_total = nullptr;
    celeste_resid_candidate_t *d_cand = nullptr;
    double2 *d_zrec = nullptr;
    if (client_get(f, RB_VP, (size_t)c->S * CEL_P * sizeof(double), &d_vp) != hipSuccess ||
        client_get(f, RB_TILES, 0, &d_tiles) != hipSuccess || client_get(f, RB_TILE_VIS, 0, &d_vis) != hipSuccess ||
        client_get(f, RB_LAM, plane, &d_lam) != hipSuccess || client_get(f, RB_N, plane, &d_n) != hipSuccess ||
        client_get(f, RB_D, plane, &d_d) != hipSuccess || client_get(f, RB_Z, plane, &d_z) != hipSuccess ||
        client_get(f, RB_COV, plane, &d_c) != hipSuccess ||
        client_get(f, RB_REC, (size_t)mt * sizeof(ResidTileRec), &d_rec) != hipSuccess ||
        client_get(f, RB_FRAMES, ni * sizeof(celeste_resid_frame_t), &d_frames) != hipSuccess ||
        client_get(f, RB_TAPS, f->taps.size() * sizeof(double), &d_taps) != hipSuccess ||
        client_get(f, RB_CIMG, ni * sizeof(ResidImg), &d_cimg) != hipSuccess ||
        client_get(f, RB_STARTS, starts.size() * sizeof(int32_t), &d_starts) != hipSuccess ||
        client_get(f, RB_PIMG, ni * sizeof(PeakImg), &d_pimg) != hipSuccess ||
        client_get(f, RB_COUNTS, (size_t)pb * sizeof(int32_t), &d_counts) != hipSuccess ||
        client_get(f, RB_OFFSETS, (size_t)pb * sizeof(int64_t), &d_offsets) != hipSuccess ||
        client_get(f, RB_TOTAL, sizeof(int64_t), &d_total) != hipSuccess ||
        client_get(f, RB_CAND, (size_t)max_candidates * sizeof(celeste_resid_candidate_t), &d_cand) != hipSuccess ||
        client_get(f, RB_ZREC, (size_t)ft * sizeof(double2), &d_zrec) != hipSuccess ||
        client_get(f, RB_SLOT, (size_t)N * sizeof(int32_t), &d_slot) != hipSuccess)
        return CELESTE_ERR_HIP;
    f->slot = slot;
    f->min_cov = opts->min_coverage;
    hipStream_t st = c->stream;
    HIP_TRY(hipMemcpyAsync(d_vp, vp, (size_t)c->S * CEL_P * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_cimg, cimg.data(), ni * sizeof(ResidImg), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_pimg, f->pimg.data(), ni * sizeof(PeakImg), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_starts, starts.data(), starts.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_taps, f->taps.data(), f->taps.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_slot, f->slot.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, st));
    const int32_t *d_mt = d_starts, *d_ft = d_starts + (ni + 1), *d_pb = d_starts + 2 * (ni + 1);
    HIP_TRY(hipEventRecord(f->ev[0], st));
    client_launch_prep(c, d_vp, st);
    HIP_TRY(hipEventRecord(f->ev[1], st));
    hipLaunchKernelGGL(resid_model_kernel, dim3((unsigned)mt), dim3(256), 0, st, d_cimg, d_mt, (int)ni, d_tiles, d_vis, c->d_images,
                       c->d_patches, c->d_coefs, c->d_bitmaps, c->d_srcimg, c->d_comps, c->NC, d_lam, d_rec);
    hipLaunchKernelGGL(resid_frame_kernel, dim3((unsigned)ni), dim3(256), 0, st, d_cimg, d_mt, d_rec, d_frames);
    HIP_TRY(hipEventRecord(f->ev[2], st));
    hipLaunchKernelGGL(resid_filter_kernel, dim3((unsigned)ft), dim3(256), 0, st, d_cimg, d_ft, (int)ni, c->d_images, d_frames,
                       d_taps, R, opts->min_coverage, d_lam, d_n, d_d, d_z, d_c, d_zrec);
    hipLaunchKernelGGL(resid_zrange_kernel, dim3((unsigned)ni), dim3(256), 0, st, d_ft, d_zrec, d_frames);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(f->ev[3], st));
    {
        const int rc = resid_run_peaks(st, d_pimg, d_pb, (int)ni, (int)pb, d_z, d_n, d_d, d_c, opts->threshold, d_counts, d_offsets,
                                       d_total, d_cand, max_candidates);
        if (rc != CELESTE_OK) return rc;
    }
    HIP_TRY(hipEventRecord(f->ev[4], st));
    int64_t total = 0;
    HIP_TRY(hipMemcpyAsync(out_frames, d_frames, ni * sizeof(celeste_resid_frame_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&total, d_total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t n_out = std::min(total, max_candidates);
    if (n_out > 0) {
        HIP_TRY(hipMemcpyAsync(out_candidates, d_cand, (size_t)n_out * sizeof(celeste_resid_candidate_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    client_stage_ms(f);
    f->frame_ok.assign(ni, 0);
    for (size_t k = 0; k < ni; ++k) f->frame_ok[k] = out_frames[k].status == CELESTE_OK;
    f->searched = true;
    *n_found = total;
    for (size_t k = 0; k < ni && *status == CELESTE_OK; ++k) *status = out_frames[k].status;
    if (*status == CELESTE_OK && total > max_candidates) *status = CELESTE_RESID_TRUNCATED;
    return CELESTE_OK;
} ABI_CATCH

extern "C" int celeste_resid_get_map(celeste_resid_ctx_t *f, int32_t image, int32_t which, double *out_plane) try {
    if (!f || !f->c || !out_plane || which < CELESTE_RESID_LAM || which > CELESTE_RESID_COVERAGE) return CELESTE_ERR_INVALID_ARG;
    if (!f->searched || image < 0 || image >= f->c->N || f->slot[image] < 0) return CELESTE_ERR_INVALID_ARG;
    static const int buf_of[5] = {RB_LAM, RB_N, RB_D, RB_Z, RB_COV};
    const ResidImg &ci = f->cimg[f->slot[image]];
    HIP_TRY(hipSetDevice(f->c->device));
    const double *src = (const double *)f->buf[buf_of[which]].p + ci.off;
    HIP_TRY(hipMemcpyAsync(out_plane, src, (size_t)ci.H * ci.W * sizeof(double), hipMemcpyDeviceToHost, f->c->stream));
    HIP_TRY(hipStreamSynchronize(f->c->stream));
    return CELESTE_OK;
} ABI_CATCH

extern "C" int celeste_resid_sample(celeste_resid_ctx_t *f, int64_t n, const int32_t *image, const int32_t *h, const int32_t *w,
                                    double *out_N, double *out_D, double *out_cov) try {
    if (!f || !f->c || n < 0 || n > 0x7fffff00ll) return CELESTE_ERR_INVALID_ARG;
    if (n > 0 && (!image || !h || !w || !out_N || !out_D || !out_cov)) return CELESTE_ERR_INVALID_ARG;
    if (!f->searched) return CELESTE_ERR_INVALID_ARG;
    for (int64_t i = 0; i < n; ++i)
        if (image[i] < 0 || image[i] >= f->c->N || f->slot[image[i]] < 0) return CELESTE_ERR_INVALID_ARG;
    if (n == 0) return CELESTE_OK;
    HIP_TRY(hipSetDevice(f->c->device));
    int32_t *d_in = nullptr;
    double *d_out = nullptr;
    if (client_get(f, RB_SAMPLE_IN, (size_t)n * 3 * sizeof(int32_t), &d_in) != hipSuccess ||
        client_get(f, RB_SAMPLE_OUT, (size_t)n * 3 * sizeof(double), &d_out) != hipSuccess) return CELESTE_ERR_HIP;
    f->sample_in.resize((size_t)n * 3);
    std::copy(image, image + n, f->sample_in.begin());
    std::copy(h, h + n, f->sample_in.begin() + n);
    std::copy(w, w + n, f->sample_in.begin() + 2 * n);
    f->sample_out.resize((size_t)n * 3);
    hipStream_t st = f->c->stream;
    HIP_TRY(hipMemcpyAsync(d_in, f->sample_in.data(), (size_t)n * 3 * sizeof(int32_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(resid_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, d_in, d_in + n, d_in + 2 * n,
                       (const int32_t *)f->buf[RB_SLOT].p, (const ResidImg *)f->buf[RB_CIMG].p, (const double *)f->buf[RB_N].p,
                       (const double *)f->buf[RB_D].p, (const double *)f->buf[RB_Z].p, (const double *)f->buf[RB_COV].p, d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(f->sample_out.data(), d_out, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::copy(f->sample_out.begin(), f->sample_out.begin() + n, out_N);
    std::copy(f->sample_out.begin() + n, f->sample_out.begin() + 2 * n, out_D);
    std::copy(f->sample_out.begin() + 2 * n, f->sample_out.end(), out_cov);
    return CELESTE_OK;
} ABI_CATCH

// The peak rule on a caller's planes.  No context: the buffers live for the call (this entry point is off every hot path).
extern "C" int celeste_resid_find_peaks(int device, int32_t H, int32_t W, const double *z, const double *coverage,
                                        const celeste_resid_opts_t *opts, celeste_resid_candidate_t *out, int64_t max,
                                        int64_t *n_found, int32_t *status) try {
    if (!z || !n_found || !status || H < 1 || W < 1 || (int64_t)H * W >= 0x7fffff00ll) return CELESTE_ERR_INVALID_ARG;
    if (max < 0 || (max > 0 && !out)) return CELESTE_ERR_INVALID_ARG;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return CELESTE_ERR_NO_DEVICE;
    if (device < 0 || device >= n_dev) return CELESTE_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(device));
    const double thr = opts ? opts->threshold : 5.0;
    const int64_t npx = (int64_t)H * W;
    const int nb = (int)((npx + RS_PB - 1) / RS_PB);
    struct Bufs {
        void *p[7] = {};
        ~Bufs() { for (void *q : p) if (q) (void)hipFree(q); }
    } b;
    const size_t sizes[7] = {(size_t)npx * sizeof(double), coverage ? (size_t)npx * sizeof(double) : 0, sizeof(PeakImg), 2 * sizeof(int32_t),
                             (size_t)nb * sizeof(int32_t), ((size_t)nb + 1) * sizeof(int64_t),
                             (size_t)max * sizeof(celeste_resid_candidate_t)};
    for (int i = 0; i < 7; ++i)
        if (sizes[i] && hipMalloc(&b.p[i], sizes[i]) != hipSuccess) return CELESTE_ERR_ALLOC;
    PeakImg pi; pi.img = 0; pi.H = H; pi.W = W; pi.pad = 0; pi.off = 0;
    const int32_t pbs[2] = {0, nb};
    HIP_TRY(hipMemcpy(b.p[0], z, sizes[0], hipMemcpyHostToDevice));
    if (coverage) HIP_TRY(hipMemcpy(b.p[1], coverage, sizes[1], hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b.p[2], &pi, sizeof pi, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b.p[3], pbs, sizeof pbs, hipMemcpyHostToDevice));
    int64_t *d_offsets = (int64_t *)b.p[5];
    const int rc = resid_run_peaks((hipStream_t) nullptr, (const PeakImg *)b.p[2], (const int32_t *)b.p[3], 1, nb,
                                   (const double *)b.p[0], nullptr, nullptr, (const double *)b.p[1], thr, (int32_t *)b.p[4], d_offsets,
                                   d_offsets + nb, (celeste_resid_candidate_t *)b.p[6], max);
    if (rc != CELESTE_OK) return rc;
    int64_t total = 0;
    HIP_TRY(hipMemcpy(&total, d_offsets + nb, sizeof(int64_t), hipMemcpyDeviceToHost));   // (waits for the null stream)
    const int64_t n_out = std::min(total, max);
    if (n_out > 0) HIP_TRY(hipMemcpy(out, b.p[6], (size_t)n_out * sizeof(celeste_resid_candidate_t), hipMemcpyDeviceToHost));
    *n_found = total;
    *status = total > max ? CELESTE_RESID_TRUNCATED : CELESTE_OK;
    return CELESTE_OK;
} ABI_CATCH

extern "C" int celeste_resid_last_ms(celeste_resid_ctx_t *f, float ms[4]) { return client_last_ms(f, ms); }

// ---- the stack -------------------------------------------------------------------------------------------------------------------
extern "C" void celeste_resid_stack_opts_default(celeste_resid_stack_opts_t *o) {
    if (!o) return;
    o->threshold = 5.0; o->min_images = 1; o->reserved = 0;
}

extern "C" int celeste_resid_wcs_check(int32_t n, const celeste_resid_wcs_t *wcs) {
    if (n < 1 || !wcs) return CELESTE_ERR_INVALID_ARG;
    for (int i = 0; i < n; ++i) if (!stack_wcs_ok(wcs[i])) return CELESTE_ERR_INVALID_ARG;
    return CELESTE_OK;
}

template <int NCH>
static void stack_launch(hipStream_t st, unsigned n_tiles, const StackGrid &g, const StackImg *d_imgs, int n_img, const double *d_wts,
                         int n_ch, int min_images, int cull, const double *d_n, const double *d_d, const double *d_z, double *oN,
                         double *oD, double *oZ, int32_t *oC, StackTileRec *rec) {
    hipLaunchKernelGGL(resid_stack_kernel<NCH>, dim3(n_tiles), dim3(256), 0, st, g, d_imgs, n_img, d_wts, n_ch, min_images, cull, d_n,
                       d_d, d_z, oN, oD, oZ, oC, rec);
}

extern "C" int celeste_resid_stack(celeste_resid_ctx_t *f, const celeste_resid_grid_t *grid, int32_t n_images,
                                   const celeste_resid_wcs_t *wcs, int32_t n_channels, const double *weights,
                                   const celeste_resid_stack_opts_t *opts, celeste_resid_stack_frame_t *out_frames,
                                   celeste_resid_stack_candidate_t *out_candidates, int64_t max_candidates, int64_t *n_found,
                                   int32_t *status) try {
    if (!f || !f->c || !grid || !wcs || !weights || !opts || !out_frames || !n_found || !status) return CELESTE_ERR_INVALID_ARG;
    if (!f->searched || n_images != f->c->N) return CELESTE_ERR_INVALID_ARG;
    if (grid->H < 1 || grid->W < 1 || (int64_t)grid->H * grid->W >= (1ll << 31)) return CELESTE_ERR_INVALID_ARG;
    if (n_channels < 1 || n_channels > SK_MAXCH || opts->min_images < 1) return CELESTE_ERR_INVALID_ARG;
    if (max_candidates < 0 || (max_candidates > 0 && !out_candidates)) return CELESTE_ERR_INVALID_ARG;
    for (int k = 0; k < n_channels; ++k) {
        bool any = false;
        for (int b = 0; b < 5; ++b) {
            const double s = weights[k * 5 + b];
            if (!std::isfinite(s) || s < 0.0) return CELESTE_ERR_INVALID_ARG;
            any |= s > 0.0;
        }
        if (!any) return CELESTE_ERR_INVALID_ARG;
    }
    if (!stack_wcs_ok(grid->wcs) || celeste_resid_wcs_check(n_images, wcs) != CELESTE_OK) return CELESTE_ERR_INVALID_ARG;
    celeste_ctx_t *c = f->c;
    const char *nc = std::getenv("CELESTE_STACK_NO_CULL");
    const int cull = !(nc && nc[0] == '1');
    // the images that can add something: OK in the last search, a weight above zero in some channel; in the search's order
    std::vector<StackImg> &imgs = f->sk_imgs;
    imgs.clear();
    for (size_t k = 0; k < f->cimg.size(); ++k) {
        const ResidImg &ci = f->cimg[k];
        const int band = c->imgs->h_images[ci.img].band;
        if (band < 1 || band > 5) return CELESTE_ERR_INVALID_ARG;
        bool used = false;
        for (int ch = 0; ch < n_channels; ++ch) used |= weights[ch * 5 + band - 1] > 0.0;
        if (!f->frame_ok[k] || !used) continue;
        const StackWcs w = stack_wcs_dev(wcs[ci.img]);
        StackImg im;
        im.kind = w.kind; im.band = band; im.H = ci.H; im.W = ci.W; im.off = ci.off;
        for (int j = 0; j < 4; ++j) im.fwd[j] = w.fwd[j];
        for (int j = 0; j < 2; ++j) { im.w0[j] = w.w0[j]; im.p0[j] = w.p0[j]; }
        im.sin0 = w.sin0; im.cos0 = w.cos0;
        imgs.push_back(im);
    }
    StackGrid g;
    g.H = grid->H; g.W = grid->W; g.wcs = stack_wcs_dev(grid->wcs);
    const int H = g.H, W = g.W, nch = n_channels;
    const int64_t HW = (int64_t)H * W;
    const int64_t n_tiles = (int64_t)((H + SK_TH - 1) / SK_TH) * ((W + SK_TW - 1) / SK_TW);
    const int64_t pb1 = (HW + RS_PB - 1) / RS_PB, pb = pb1 * nch;
    f->sk_wts.assign(weights, weights + (size_t)nch * 5);
    f->sk_pimg.assign((size_t)nch, PeakImg());
    f->sk_starts.assign((size_t)nch + 1, 0);
    for (int k = 0; k < nch; ++k) {
        PeakImg &pi = f->sk_pimg[k];
        pi.img = k; pi.H = H; pi.W = W; pi.pad = 0; pi.off = (int64_t)k * HW;
        f->sk_starts[k + 1] = (int32_t)(pb1 * (k + 1));
    }
    *n_found = 0;
    *status = CELESTE_OK;
    HIP_TRY(hipSetDevice(c->device));
    for (auto &e : f->sk_ev) if (!e) HIP_TRY(hipEventCreate(&e));
    f->stacked = false;
    StackImg *d_imgs = nullptr;
    double *d_wts = nullptr, *oN = nullptr, *oD = nullptr, *oZ = nullptr;
    int32_t *oC = nullptr, *d_starts = nullptr, *d_counts = nullptr;
    StackTileRec *d_rec = nullptr;
    celeste_resid_stack_frame_t *d_frames = nullptr;
    PeakImg *d_pimg = nullptr;
    int64_t *d_offsets = nullptr, *d_total = nullptr;
    celeste_resid_candidate_t *d_peaks = nullptr;
    celeste_resid_stack_candidate_t *d_cand = nullptr;
    const size_t planes = (size_t)nch * (size_t)HW;
    if (client_get(f, RB_SK_IMGS, imgs.size() * sizeof(StackImg), &d_imgs) != hipSuccess ||
        client_get(f, RB_SK_WTS, (size_t)nch * 5 * sizeof(double), &d_wts) != hipSuccess ||
        client_get(f, RB_SK_N, planes * sizeof(double), &oN) != hipSuccess ||
        client_get(f, RB_SK_D, planes * sizeof(double), &oD) != hipSuccess ||
        client_get(f, RB_SK_Z, planes * sizeof(double), &oZ) != hipSuccess ||
        client_get(f, RB_SK_CNT, planes * sizeof(int32_t), &oC) != hipSuccess ||
        client_get(f, RB_SK_REC, (size_t)nch * (size_t)n_tiles * sizeof(StackTileRec), &d_rec) != hipSuccess ||
        client_get(f, RB_SK_FRAMES, (size_t)nch * sizeof(celeste_resid_stack_frame_t), &d_frames) != hipSuccess ||
        client_get(f, RB_SK_PIMG, (size_t)nch * sizeof(PeakImg), &d_pimg) != hipSuccess ||
        client_get(f, RB_SK_STARTS, ((size_t)nch + 1) * sizeof(int32_t), &d_starts) != hipSuccess ||
        client_get(f, RB_SK_COUNTS, (size_t)pb * sizeof(int32_t), &d_counts) != hipSuccess ||
        client_get(f, RB_SK_OFFSETS, (size_t)pb * sizeof(int64_t), &d_offsets) != hipSuccess ||
        client_get(f, RB_SK_TOTAL, sizeof(int64_t), &d_total) != hipSuccess ||
        client_get(f, RB_SK_PEAKS, (size_t)max_candidates * sizeof(celeste_resid_candidate_t), &d_peaks) != hipSuccess ||
        client_get(f, RB_SK_CAND, (size_t)max_candidates * sizeof(celeste_resid_stack_candidate_t), &d_cand) != hipSuccess)
        return CELESTE_ERR_HIP;
    hipStream_t st = c->stream;
    if (!imgs.empty()) HIP_TRY(hipMemcpyAsync(d_imgs, imgs.data(), imgs.size() * sizeof(StackImg), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_wts, f->sk_wts.data(), (size_t)nch * 5 * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_pimg, f->sk_pimg.data(), (size_t)nch * sizeof(PeakImg), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_starts, f->sk_starts.data(), ((size_t)nch + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
    const double *d_n = (const double *)f->buf[RB_N].p, *d_d = (const double *)f->buf[RB_D].p, *d_z = (const double *)f->buf[RB_Z].p;
    HIP_TRY(hipEventRecord(f->sk_ev[0], st));
    {
        const unsigned nt = (unsigned)n_tiles;
        const int ni = (int)imgs.size(), mi = opts->min_images;
        if (nch <= 1) stack_launch<1>(st, nt, g, d_imgs, ni, d_wts, nch, mi, cull, d_n, d_d, d_z, oN, oD, oZ, oC, d_rec);
        else if (nch <= 2) stack_launch<2>(st, nt, g, d_imgs, ni, d_wts, nch, mi, cull, d_n, d_d, d_z, oN, oD, oZ, oC, d_rec);
        else if (nch <= 4) stack_launch<4>(st, nt, g, d_imgs, ni, d_wts, nch, mi, cull, d_n, d_d, d_z, oN, oD, oZ, oC, d_rec);
        else stack_launch<8>(st, nt, g, d_imgs, ni, d_wts, nch, mi, cull, d_n, d_d, d_z, oN, oD, oZ, oC, d_rec);
    }
    hipLaunchKernelGGL(stack_zrange_kernel, dim3((unsigned)nch), dim3(256), 0, st, d_rec, (int)n_tiles, d_frames);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(f->sk_ev[1], st));
    {
        const int rc = resid_run_peaks(st, d_pimg, d_starts, nch, (int)pb, oZ, oN, oD, nullptr, opts->threshold, d_counts, d_offsets,
                                       d_total, d_peaks, max_candidates);
        if (rc != CELESTE_OK) return rc;
    }
    int64_t total = 0;
    HIP_TRY(hipMemcpyAsync(out_frames, d_frames, (size_t)nch * sizeof(celeste_resid_stack_frame_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&total, d_total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t n_out = std::min(total, max_candidates);
    if (n_out > 0) {
        hipLaunchKernelGGL(stack_finish_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, n_out, d_peaks, g, oC, d_cand);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(f->sk_ev[2], st));
    if (n_out > 0)
        HIP_TRY(hipMemcpyAsync(out_candidates, d_cand, (size_t)n_out * sizeof(celeste_resid_stack_candidate_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int k = 0; k < 2; ++k)
        if (hipEventElapsedTime(&f->sk_ms[k], f->sk_ev[k], f->sk_ev[k + 1]) != hipSuccess) f->sk_ms[k] = 0;
    f->sk_H = H; f->sk_W = W; f->sk_ch = nch;
    f->stacked = true;
    *n_found = total;
    if (total > max_candidates) *status = CELESTE_RESID_TRUNCATED;
    return CELESTE_OK;
} ABI_CATCH

extern "C" int celeste_resid_stack_get_map(celeste_resid_ctx_t *f, int32_t channel, int32_t which, double *out_plane) try {
    if (!f || !f->c || !out_plane || which < CELESTE_RESID_STACK_N || which > CELESTE_RESID_STACK_COUNT) return CELESTE_ERR_INVALID_ARG;
    if (!f->stacked || channel < 0 || channel >= f->sk_ch) return CELESTE_ERR_INVALID_ARG;
    static const int buf_of[4] = {RB_SK_N, RB_SK_D, RB_SK_Z, RB_SK_CNT};
    const size_t HW = (size_t)f->sk_H * f->sk_W;
    HIP_TRY(hipSetDevice(f->c->device));
    hipStream_t st = f->c->stream;
    if (which == CELESTE_RESID_STACK_COUNT) {
        std::vector<int32_t> cnt(HW);
        HIP_TRY(hipMemcpyAsync(cnt.data(), (const int32_t *)f->buf[RB_SK_CNT].p + (size_t)channel * HW, HW * sizeof(int32_t),
                               hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t i = 0; i < HW; ++i) out_plane[i] = (double)cnt[i];
        return CELESTE_OK;
    }
    HIP_TRY(hipMemcpyAsync(out_plane, (const double *)f->buf[buf_of[which]].p + (size_t)channel * HW, HW * sizeof(double),
                           hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return CELESTE_OK;
} ABI_CATCH

extern "C" int celeste_resid_stack_last_ms(celeste_resid_ctx_t *f, float ms[2]) {
    if (!f || !ms) return CELESTE_ERR_INVALID_ARG;
    ms[0] = f->sk_ms[0]; ms[1] = f->sk_ms[1];
    return CELESTE_OK;
}
