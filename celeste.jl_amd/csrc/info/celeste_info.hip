// celeste_info.hip -- libceleste_info.so: position and shape standard errors from the pixels' Fisher information
// (include/celeste_info.h).
//
// The engine's context code (engine_context.h) and its kernels' header are compiled into this library, unchanged, as into the fit and phot
// libraries; the context, the work list and the pixel walk (the neighbours' light B of every pixel) are engine_client.h's.
// This file adds three kernels.  One call:
//   prep_kernel          (the engine's) SrcImg and Comp of every visit of the context at the call's table
//   info_pixel_kernel    one wavefront per work item; a lane forms the star spline's value and gradient and the galaxy
//                        mixture's value and gradient at its pixel (first derivatives only), from them the 34 products of
//                        the header; the wavefront sums each in a fixed butterfly and lane k writes sum k of the tile's row
//   info_reduce_kernel   one workgroup per target adds its tile rows one after another, in ascending (image, tile) order,
//                        into its band rows (thread = band x sum) and writes its status
//   info_solve_kernel    one thread per (target, type): Schur complement, scaling, Cholesky, inverse and flags
// A tile is 64 consecutive pixels of a patch whatever the chunk size is, so the sums do not depend on it.  No floating-point
// atomics.
#include "../engine_context.h"
#include "../engine_client.h"
#include "../density_grad.h"
#include "../../../include/celeste_info.h"

#define INFO_NB CELESTE_INFO_BANDS
#define INFO_S0 CELESTE_INFO_NSUM_STAR
#define INFO_S1 CELESTE_INFO_NSUM_GAL
#define INFO_REC (INFO_S0 + INFO_S1)   // doubles of a tile row: the star's 6 sums, then the galaxy's 28
#define INFO_NT 192                    // threads of info_reduce_kernel: 5 x 34 sums, 5 pixel counts

struct InfoTileInfo { int32_t n_pix, bad, band, pad; };   // visited pixels; a lam_i non-finite or <= 0 at one of them; band 0..4

// (a work item's tiles number the tile rows)
__global__ void __launch_bounds__(64)
info_pixel_kernel(const VisitItem *__restrict__ items, const double *__restrict__ vp, const DevImage *__restrict__ images,
                  const DevPatch *__restrict__ patches, const double *__restrict__ coefs, const uint8_t *__restrict__ bitmaps,
                  const SrcImg *__restrict__ srcimg, const Comp *__restrict__ comps, const int64_t *__restrict__ nbr_off,
                  const int32_t *__restrict__ nbr_idx, const int32_t *__restrict__ vis_off, const int32_t *__restrict__ vis_img,
                  const int32_t *__restrict__ vis_src, int dense, int N, int NC, int chunk_px, double *__restrict__ rec,
                  InfoTileInfo *__restrict__ info) {
    // per work item, by lanes 0 and 1: E[l_b | a = i] of the target's row; by lane 2: d(Xi11, Xi12, Xi22) / d(axis_ratio,
    // angle, radius) (source_geo_values)
    __shared__ double s_El[2];
    __shared__ SrcGeo s_geo;
    const VisitItem it = items[blockIdx.x];
    const int lane = threadIdx.x;
    {
        const double *vs = vp + (size_t)vis_src[it.sn] * CEL_P;
        if (lane < 2) {
            double El, Ell;
            brightness(vs, lane, images[it.n].band - 1, El, Ell);
            s_El[lane] = El;
        } else if (lane == 2) {
            source_geo_values(vs, &s_geo);
        }
    }
    __syncthreads();
    const DevPatch &P = patches[it.sn];
    const double J11 = P.J[0], J21 = P.J[1], J12 = P.J[2], J22 = P.J[3];      // d(m1, m2) / d(pos1, pos2), column-major
    visit_pixel_walk(it, images, patches, coefs, bitmaps, srcimg, comps, nbr_off, nbr_idx, vis_off, vis_img, vis_src, dense, N, NC,
                     chunk_px, [&](const DevImage &img, const VisitPixel &px, const VisitOwn &ow) {
        const int tile = px.tile;
        const bool valid = px.valid, own = ow.own;
        const double iota = px.iota, B = px.B, eps = (double)px.skyf;
        const double El0 = s_El[0], El1 = s_El[1];
        // the two densities and their gradients with respect to (m1, m2 | frac_dev, Xi11, Xi12, Xi22)
        double f0 = 0, f0h = 0, f0w = 0;
        InfoGal g = {0, 0, 0, 0, 0, 0, 0};
        if (own) {
            info_star_grad(ow.coef, ow.hh + (26.0 - ow.m1), ow.ww + (26.0 - ow.m2), ow.etab, f0, f0h, f0w);
            g = info_galaxy_grad(ow.tc, NC, ow.hh - ow.m1, ow.ww - ow.m2, ow.etab);
        }
        const double g0 = El0 * f0, g1 = El1 * g.v;
        const double lam0 = __dmul_rn(iota, (eps + g0) + B), lam1 = __dmul_rn(iota, (eps + g1) + B);
        const bool bad = valid && !(lam0 > 0.0 && isfinite(lam0) && lam1 > 0.0 && isfinite(lam1));
        const bool use = own && !bad;
        const double rl0 = use ? 1.0 / lam0 : 0.0, rl1 = use ? 1.0 / lam1 : 0.0;
        // D_k = iota E_l df/dtheta_k; the spline's index is h - m + 26, so d/dm = -d/d(index)
        const double e0 = iota * El0, e1 = iota * El1;
        double Ds[3], Dg[7];                                       // (the last entry: a = iota g_i)
        {
            const double sm1 = -f0h, sm2 = -f0w;
            Ds[0] = e0 * (sm1 * J11 + sm2 * J21);
            Ds[1] = e0 * (sm1 * J12 + sm2 * J22);
            Ds[2] = iota * g0;
            const double *j = s_geo.jsh;
            Dg[0] = e1 * (g.m1 * J11 + g.m2 * J21);
            Dg[1] = e1 * (g.m1 * J12 + g.m2 * J22);
            Dg[2] = e1 * g.dev;
            Dg[3] = e1 * (g.x11 * j[0] + g.x12 * j[1] + g.x22 * j[2]);
            Dg[4] = e1 * (g.x11 * j[3] + g.x12 * j[4] + g.x22 * j[5]);
            Dg[5] = e1 * (g.x11 * j[6] + g.x12 * j[7] + g.x22 * j[8]);
            Dg[6] = iota * g1;
        }
        if (!use) {
#pragma unroll
            for (int k = 0; k < 3; ++k) Ds[k] = 0.0;
#pragma unroll
            for (int k = 0; k < 7; ++k) Dg[k] = 0.0;
        }
        // the 34 sums of the tile, in the header's packing: the upper triangle of A row-major, then c, then d
        double mine = 0.0;
        int q = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int l = k; l < 3; ++l) {
                // (k, l) of the 3 x 3 triangle over (D_0, D_1, a): (0,0) (0,1) (1,1) are A, (0,2) (1,2) are c, (2,2) is d
                const int slot = (k < 2 && l < 2) ? (k == 0 ? l : 2) : (l == 2 && k < 2 ? 3 + k : 5);
                const double s = wave_sum(__dmul_rn(__dmul_rn(Ds[k], Ds[l]), rl0));
                mine = lane == slot ? s : mine;
            }
#pragma unroll
        for (int k = 0; k < 6; ++k)
#pragma unroll
            for (int l = k; l < 6; ++l, ++q) {
                const double s = wave_sum(__dmul_rn(__dmul_rn(Dg[k], Dg[l]), rl1));
                mine = lane == INFO_S0 + q ? s : mine;
            }
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const double s = wave_sum(__dmul_rn(__dmul_rn(Dg[k], Dg[6]), rl1));
            mine = lane == INFO_S0 + 21 + k ? s : mine;
        }
        const int n_valid = __popcll(__ballot(valid));
        const int any_bad = __any(bad);
        if (lane < INFO_REC) rec[(size_t)tile * INFO_REC + lane] = mine;
        if (lane == 0) {
            InfoTileInfo ti;
            ti.n_pix = n_valid; ti.bad = any_bad; ti.band = img.band - 1; ti.pad = 0;
            info[tile] = ti;
        }
    });
}

// tgt_rec[ti] = {first tile row, number of tile rows} of target ti of the call
__global__ void __launch_bounds__(INFO_NT)
info_reduce_kernel(const int2 *__restrict__ tgt_rec, const int32_t *__restrict__ targets, const double *__restrict__ vp,
                   const double *__restrict__ rec, const InfoTileInfo *__restrict__ info, double *__restrict__ sums_star,
                   double *__restrict__ sums_gal, int64_t *__restrict__ n_pix, int32_t *__restrict__ status) {
    const int ti = blockIdx.x, t = threadIdx.x;
    // threads 0 .. 169: band b, sum k of the tile row; threads 170 .. 174: the pixel count of band t - 170
    const bool is_sum = t < INFO_NB * INFO_REC, is_cnt = !is_sum && t < INFO_NB * INFO_REC + INFO_NB;
    const int b = is_sum ? t / INFO_REC : t - INFO_NB * INFO_REC, k = is_sum ? t - b * INFO_REC : 0;
    const int2 tr = tgt_rec[ti];
    double acc = 0.0;
    int64_t cnt = 0;
    int bad = 0;
#pragma unroll 4
    for (int r = tr.x; r < tr.x + tr.y; ++r) {
        const InfoTileInfo fi = info[r];
        const double x = rec[(size_t)r * INFO_REC + k];
        bad |= fi.bad;
        const bool mine = fi.band == b;
        acc = mine ? acc + x : acc;
        cnt += mine ? fi.n_pix : 0;
    }
    const double *vs = vp + (size_t)targets[ti] * CEL_P;
    const int nonfinite = __syncthreads_or(row_nonfinite(vs, t));
    const int st = nonfinite ? CELESTE_ERR_NONFINITE_INPUT : (bad ? CELESTE_ERR_NONFINITE_RESULT : CELESTE_OK);
    if (is_sum) {
        const double out = st != CELESTE_OK ? (double)NAN : acc;
        if (k < INFO_S0) sums_star[((size_t)ti * INFO_NB + b) * INFO_S0 + k] = out;
        else sums_gal[((size_t)ti * INFO_NB + b) * INFO_S1 + (k - INFO_S0)] = out;
    } else if (is_cnt) {
        n_pix[(size_t)ti * INFO_NB + b] = cnt;
    }
    if (t == 0) status[ti] = st;
}

// The covariance step of the header for one (target, type): sums [5][G (G + 1) / 2 + G + 1] -> cov [G (G + 1) / 2], flag.
// Every index is a compile-time constant after unrolling.  A dropped parameter stays in the matrix as a unit diagonal with
// zero off-diagonals: its products are exact zeros, so the rest is the smaller problem's arithmetic.
template <int G>
__device__ __forceinline__ void info_solve_block(const double *__restrict__ sums, double *__restrict__ cov, int32_t *__restrict__ flag) {
    constexpr int NA = G * (G + 1) / 2, NS = NA + G + 1;
    auto tri = [](int k, int l) { return k * G - (k * (k - 1)) / 2 + (l - k); };
    double S[NA], T[NA];
#pragma unroll
    for (int q = 0; q < NA; ++q) { S[q] = 0.0; T[q] = 0.0; }
    bool any_d = false;
#pragma unroll
    for (int b = 0; b < INFO_NB; ++b) {
        const double *row = sums + b * NS;
#pragma unroll
        for (int q = 0; q < NA; ++q) S[q] += row[q];
        const double d = row[NA + G];
        any_d |= d != 0.0;
        if (d > 0.0) {
#pragma unroll
            for (int k = 0; k < G; ++k)
#pragma unroll
                for (int l = k; l < G; ++l) T[tri(k, l)] += row[NA + k] * row[NA + l] / d;
        }
    }
    const double nan = (double)NAN;
    if (!any_d) {
#pragma unroll
        for (int q = 0; q < NA; ++q) cov[q] = nan;
        *flag = CELESTE_INFO_NO_PIXELS;
        return;
    }
    bool notpos = false;
#pragma unroll
    for (int q = 0; q < NA; ++q) { S[q] = S[q] - T[q]; notpos |= !isfinite(S[q]); }
#pragma unroll
    for (int k = 0; k < G; ++k) notpos |= S[tri(k, k)] < 0.0;
    if (notpos) {
#pragma unroll
        for (int q = 0; q < NA; ++q) cov[q] = nan;
        *flag = CELESTE_INFO_NOT_POSITIVE;
        return;
    }
    int fl = 0;
    bool act[G];
    double is[G];                                                  // 1 / s_k (1 for a dropped parameter)
#pragma unroll
    for (int k = 0; k < G; ++k) {
        act[k] = S[tri(k, k)] > 0.0;
        if (!act[k]) fl |= CELESTE_INFO_UNCONSTRAINED;
        is[k] = act[k] ? 1.0 / sqrt(S[tri(k, k)]) : 1.0;
    }
    double L[G][G], Li[G][G];
    double minpiv = INFINITY;
    bool stop = false;
#pragma unroll
    for (int j = 0; j < G; ++j) {
        double piv = 1.0;                                          // R_jj: the unit diagonal
#pragma unroll
        for (int k = 0; k < j; ++k) piv -= L[j][k] * L[j][k];
        if (act[j]) { stop |= !(piv > 0.0); minpiv = fmin(minpiv, piv); }
        L[j][j] = sqrt(piv);
#pragma unroll
        for (int i = j + 1; i < G; ++i) {
            double r = (act[i] && act[j]) ? S[tri(j, i)] * is[i] * is[j] : 0.0;
#pragma unroll
            for (int k = 0; k < j; ++k) r -= L[i][k] * L[j][k];
            L[i][j] = r / L[j][j];
        }
    }
    if (stop) {
#pragma unroll
        for (int q = 0; q < NA; ++q) cov[q] = nan;
        *flag = fl | CELESTE_INFO_NOT_POSITIVE;
        return;
    }
    if (minpiv < CELESTE_INFO_PIVOT_MIN) fl |= CELESTE_INFO_ILL_CONDITIONED;
    // inv(L), then inv(R) = inv(L)' inv(L)
#pragma unroll
    for (int j = 0; j < G; ++j) {
        Li[j][j] = 1.0 / L[j][j];
#pragma unroll
        for (int i = j + 1; i < G; ++i) {
            double r = 0.0;
#pragma unroll
            for (int k = j; k < i; ++k) r -= L[i][k] * Li[k][j];
            Li[i][j] = r / L[i][i];
        }
    }
#pragma unroll
    for (int k = 0; k < G; ++k)
#pragma unroll
        for (int l = k; l < G; ++l) {
            double r = 0.0;
#pragma unroll
            for (int i = l; i < G; ++i) r += Li[i][k] * Li[i][l];
            double c = r * is[k] * is[l];
            if (!act[k] || !act[l]) c = (k == l) ? (double)INFINITY : 0.0;
            cov[tri(k, l)] = c;
        }
    *flag = fl;
}

__global__ void __launch_bounds__(64)
info_solve_kernel(int n, const double *__restrict__ sums_star, const double *__restrict__ sums_gal, double *__restrict__ cov_star,
                  double *__restrict__ cov_gal, int32_t *__restrict__ flag) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= 2 * n) return;
    const int ti = t >> 1;
    if ((t & 1) == 0)
        info_solve_block<CELESTE_INFO_G_STAR>(sums_star + (size_t)ti * INFO_NB * INFO_S0, cov_star + (size_t)ti * CELESTE_INFO_NCOV_STAR,
                                              flag + 2 * (size_t)ti);
    else
        info_solve_block<CELESTE_INFO_G_GAL>(sums_gal + (size_t)ti * INFO_NB * INFO_S1, cov_gal + (size_t)ti * CELESTE_INFO_NCOV_GAL,
                                             flag + 2 * (size_t)ti + 1);
}

// ---- host side ----------------------------------------------------------------------------------------------------------
struct celeste_info_ctx : ClientCtx<14, 5, 4> {
    // host staging of one call: kept here so that it outlives the asynchronous copies
    std::vector<VisitItem> items;
    std::vector<int2> tgt_rec;
};

extern "C" int celeste_info_version(void) { return CELESTE_INFO_ABI_VERSION; }

extern "C" const char *celeste_info_strerror(int status) { return celeste_strerror(status); }

extern "C" int celeste_info_ctx_create(const celeste_problem_t *problem, int device, celeste_info_ctx_t **out) try {
    return client_create(problem, device, out);
} ABI_CATCH

extern "C" void celeste_info_ctx_destroy(celeste_info_ctx_t *f) { client_destroy(f); }

extern "C" int celeste_info_bounds(celeste_info_ctx_t *f, const double *vp, int32_t n_targets, const int32_t *targets,
                                   int64_t *n_pix, double *sums_star, double *sums_gal, double *cov_star, double *cov_gal,
                                   int32_t *flag, int32_t *status) try {
    if (!f || !f->c || !vp || n_targets < 0) return CELESTE_ERR_INVALID_ARG;
    if (n_targets > 0 && (!targets || !n_pix || !sums_star || !sums_gal || !cov_star || !cov_gal || !flag || !status))
        return CELESTE_ERR_INVALID_ARG;
    celeste_ctx_t *c = f->c;
    if (!client_targets_ok(c, n_targets, targets)) return CELESTE_ERR_INVALID_ARG;
    if (n_targets == 0) return CELESTE_OK;
    // the work list; a target's tile rows follow each other
    std::vector<VisitItem> &items = f->items;
    std::vector<int2> &tgt_rec = f->tgt_rec;
    tgt_rec.assign((size_t)n_targets, make_int2(0, 0));
    int64_t n_rec = 0, n_px = 0;
    if (!client_walk(c, n_targets, targets, items, n_rec, n_px, [&](int ti, int, int, int64_t tile0, int64_t tile1, int64_t) {
            if (tgt_rec[ti].y == 0) tgt_rec[ti].x = (int)tile0;
            tgt_rec[ti].y = (int)tile1 - tgt_rec[ti].x;
            return true;
        })) return CELESTE_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(c->device));
    const size_t nt = (size_t)n_targets, ni = items.size();
    double *d_vp = nullptr, *d_rec = nullptr, *d_s0 = nullptr, *d_s1 = nullptr, *d_c0 = nullptr, *d_c1 = nullptr;
    VisitItem *d_items = nullptr;
    InfoTileInfo *d_info = nullptr;
    int2 *d_tgt_rec = nullptr;
    int32_t *d_targets = nullptr, *d_status = nullptr, *d_flag = nullptr;
    int64_t *d_npix = nullptr;
    if (client_get(f, 0, (size_t)c->S * CEL_P * sizeof(double), &d_vp) != hipSuccess ||
        client_get(f, 1, ni * sizeof(VisitItem), &d_items) != hipSuccess ||
        client_get(f, 2, (size_t)n_rec * INFO_REC * sizeof(double), &d_rec) != hipSuccess ||
        client_get(f, 3, (size_t)n_rec * sizeof(InfoTileInfo), &d_info) != hipSuccess ||
        client_get(f, 4, nt * sizeof(int2), &d_tgt_rec) != hipSuccess ||
        client_get(f, 5, nt * sizeof(int32_t), &d_targets) != hipSuccess ||
        client_get(f, 6, nt * INFO_NB * INFO_S0 * sizeof(double), &d_s0) != hipSuccess ||
        client_get(f, 7, nt * INFO_NB * INFO_S1 * sizeof(double), &d_s1) != hipSuccess ||
        client_get(f, 8, nt * INFO_NB * sizeof(int64_t), &d_npix) != hipSuccess ||
        client_get(f, 9, nt * sizeof(int32_t), &d_status) != hipSuccess ||
        client_get(f, 10, nt * CELESTE_INFO_NCOV_STAR * sizeof(double), &d_c0) != hipSuccess ||
        client_get(f, 11, nt * CELESTE_INFO_NCOV_GAL * sizeof(double), &d_c1) != hipSuccess ||
        client_get(f, 12, nt * 2 * sizeof(int32_t), &d_flag) != hipSuccess)
        return CELESTE_ERR_HIP;
    hipStream_t st = c->stream;
    HIP_TRY(hipMemcpyAsync(d_vp, vp, (size_t)c->S * CEL_P * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_targets, targets, nt * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_tgt_rec, tgt_rec.data(), nt * sizeof(int2), hipMemcpyHostToDevice, st));
    if (ni > 0) HIP_TRY(hipMemcpyAsync(d_items, items.data(), ni * sizeof(VisitItem), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(f->ev[0], st));
    client_launch_prep(c, d_vp, st);
    HIP_TRY(hipEventRecord(f->ev[1], st));
    if (ni > 0)
        hipLaunchKernelGGL(info_pixel_kernel, dim3((unsigned)ni), dim3(64), 0, st, d_items, d_vp, c->d_images, c->d_patches,
                           c->d_coefs, c->d_bitmaps, c->d_srcimg, c->d_comps, c->d_nbr_off, c->d_nbr_idx, c->d_vis_off,
                           c->d_vis_img, c->d_vis_src, (int)c->dense, c->N, c->NC, c->chunk_px, d_rec, d_info);
    HIP_TRY(hipEventRecord(f->ev[2], st));
    hipLaunchKernelGGL(info_reduce_kernel, dim3((unsigned)nt), dim3(INFO_NT), 0, st, d_tgt_rec, d_targets, d_vp, d_rec, d_info,
                       d_s0, d_s1, d_npix, d_status);
    HIP_TRY(hipEventRecord(f->ev[3], st));
    hipLaunchKernelGGL(info_solve_kernel, dim3((unsigned)((2 * nt + 63) / 64)), dim3(64), 0, st, n_targets, d_s0, d_s1, d_c0, d_c1,
                       d_flag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(f->ev[4], st));
    HIP_TRY(hipMemcpyAsync(sums_star, d_s0, nt * INFO_NB * INFO_S0 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(sums_gal, d_s1, nt * INFO_NB * INFO_S1 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(cov_star, d_c0, nt * CELESTE_INFO_NCOV_STAR * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(cov_gal, d_c1, nt * CELESTE_INFO_NCOV_GAL * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(flag, d_flag, nt * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(n_pix, d_npix, nt * INFO_NB * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(status, d_status, nt * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    client_stage_ms(f);
    return client_first_status(status, n_targets);
} ABI_CATCH

extern "C" int celeste_info_solve(celeste_info_ctx_t *f, int32_t n, const double *sums_star, const double *sums_gal,
                                  double *cov_star, double *cov_gal, int32_t *flag) try {
    if (!f || !f->c || n < 0) return CELESTE_ERR_INVALID_ARG;
    if (n > 0 && (!sums_star || !sums_gal || !cov_star || !cov_gal || !flag)) return CELESTE_ERR_INVALID_ARG;
    if (n == 0) return CELESTE_OK;
    celeste_ctx_t *c = f->c;
    HIP_TRY(hipSetDevice(c->device));
    const size_t nt = (size_t)n;
    double *d_s0 = nullptr, *d_s1 = nullptr, *d_c0 = nullptr, *d_c1 = nullptr;
    int32_t *d_flag = nullptr;
    if (client_get(f, 6, nt * INFO_NB * INFO_S0 * sizeof(double), &d_s0) != hipSuccess ||
        client_get(f, 7, nt * INFO_NB * INFO_S1 * sizeof(double), &d_s1) != hipSuccess ||
        client_get(f, 10, nt * CELESTE_INFO_NCOV_STAR * sizeof(double), &d_c0) != hipSuccess ||
        client_get(f, 11, nt * CELESTE_INFO_NCOV_GAL * sizeof(double), &d_c1) != hipSuccess ||
        client_get(f, 12, nt * 2 * sizeof(int32_t), &d_flag) != hipSuccess)
        return CELESTE_ERR_HIP;
    hipStream_t st = c->stream;
    HIP_TRY(hipMemcpyAsync(d_s0, sums_star, nt * INFO_NB * INFO_S0 * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_s1, sums_gal, nt * INFO_NB * INFO_S1 * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(info_solve_kernel, dim3((unsigned)((2 * nt + 63) / 64)), dim3(64), 0, st, n, d_s0, d_s1, d_c0, d_c1, d_flag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(cov_star, d_c0, nt * CELESTE_INFO_NCOV_STAR * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(cov_gal, d_c1, nt * CELESTE_INFO_NCOV_GAL * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(flag, d_flag, nt * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return CELESTE_OK;
} ABI_CATCH

extern "C" int celeste_info_last_ms(celeste_info_ctx_t *f, float ms[4]) { return client_last_ms(f, ms); }
