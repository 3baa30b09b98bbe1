// celeste_fit.hip -- libceleste_fit.so: per-source goodness of fit (include/celeste_fit.h).
//
// The engine's context and evaluation code (celeste_abi.hip) is compiled into this library, unchanged: the patch table, the
// per-visit tables of prep_kernel, the spline coefficients, the bitmaps and the neighbour lists are the engine's, and the
// two densities are its star_value and galaxy_value.  This file adds a work list and two kernels.  One call:
//   prep_kernel          (the engine's) SrcImg and Comp of every visit of the context at the call's table
//   fit_pixel_kernel     one wavefront per work item = (visit of a target, chunk of CELESTE_CHUNK_PX pixels of its patch): a
//                        lane owns a pixel of a 64-pixel tile; it forms the target's own light m, the neighbours' light B (each
//                        neighbour that covers the pixel evaluated there: per link, not once per neighbour pixel), lam, the
//                        stamp value if asked, and the seven terms; the wavefront sums them in a fixed butterfly and lane 0
//                        writes the tile's record
//   fit_reduce_kernel    one wavefront per target adds its tile records one after another, in ascending (image, tile) order,
//                        into its band rows (lane = band x statistic) and writes its status
// A tile is 64 consecutive pixels of a patch whatever the chunk size is (chunks are multiples of 64 pixels), so the sums do not
// depend on it.  No floating-point atomics.
#include "../celeste_abi.hip"
#include "../../../include/celeste_fit.h"

#define FIT_NB CELESTE_FIT_BANDS
#define FIT_NS CELESTE_FIT_NSTATS
#define FIT_REC 8                      // doubles of a tile record: the seven statistics, one unused

struct FitItem {
    int32_t sn, n;                     // visit (table entry of the target's patch), image
    int32_t p0;                        // first pixel of the chunk
    int32_t rec0;                      // the chunk's first tile record
    int64_t stamp_off;                 // where the visit's stamp starts in the stamp buffer
};

struct FitTileInfo { int32_t n_pix, bad, band, pad; };   // visited pixels; lam non-finite or <= 0 at one of them; band 0..4

// E_G_s.v of one source at the pixel (hh, ww) (1-based image coordinates): value_pixel's expression
__device__ __forceinline__ double fit_light(const SrcImg &si, const Comp *tc, int NC, const double *__restrict__ coef,
                                            const double *etab, double hh, double ww) {
    const double f0 = star_value(coef, hh + (26.0 - si.m1), ww + (26.0 - si.m2));
    const double f1 = galaxy_value(tc, NC, hh - si.m1, ww - si.m2, etab);
    return si.c0 * f0 + si.c1 * f1;
}

__device__ __forceinline__ double fit_wave_max(double x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x = fmax(x, __shfl_xor(x, o, 64));
    return x;
}

__device__ __forceinline__ void fit_stage_comps(Comp *dst, const Comp *__restrict__ src, int NC) {
    const double *s = reinterpret_cast<const double *>(src);
    double *d = reinterpret_cast<double *>(dst);
    for (int i = threadIdx.x; i < NC * 8; i += 64) d[i] = s[i];
}

__global__ void __launch_bounds__(64)
fit_pixel_kernel(const FitItem *__restrict__ items, const DevImage *__restrict__ images, const DevPatch *__restrict__ patches,
                 const double *__restrict__ coefs, const uint8_t *__restrict__ bitmaps, const SrcImg *__restrict__ srcimg,
                 const Comp *__restrict__ comps, const int64_t *__restrict__ nbr_off, const int32_t *__restrict__ nbr_idx,
                 const int32_t *__restrict__ vis_off, const int32_t *__restrict__ vis_img, const int32_t *__restrict__ vis_src,
                 int dense, int N, int NC, int chunk_px, double *__restrict__ rec, FitTileInfo *__restrict__ info,
                 double *__restrict__ stamps) {
    __shared__ double etab[64];
    __shared__ Comp tc[14 * CEL_MAXK];     // the target's components
    __shared__ Comp tq[14 * CEL_MAXK];     // the current neighbour's
    const FitItem it = items[blockIdx.x];
    const int lane = threadIdx.x;
    const int sn = it.sn, n = it.n;
    const int s = vis_src[sn];
    const DevPatch &P = patches[sn];
    const DevImage &img = images[n];
    const int H2 = P.H2, W2 = P.W2, npx = H2 * W2;
    const int p1 = min(npx, it.p0 + chunk_px);
    const float rH2 = 1.0f / (float)H2;
    exp_table_init(etab);
    const SrcImg si = srcimg[sn];
    fit_stage_comps(tc, comps + (size_t)sn * NC, NC);
    __syncthreads();
    const double *__restrict__ coef = coefs + (size_t)P.stamp * (CEL_COEF * CEL_COEF);
    const int64_t nb0 = nbr_off[s], nb1 = nbr_off[s + 1];
    int tile = it.rec0;
    for (int base = it.p0; base < p1; base += 64, ++tile) {
        const int idx = base + lane;
        const bool inp = idx < p1;
        int w2, h2;                                           // 0-based in the patch
        divmod_small(min(idx, npx - 1), H2, rH2, w2, h2);
        const int h0 = P.off_h + h2, w0 = P.off_w + w2;       // 0-based in the image
        const size_t gi = (size_t)h0 + (size_t)img.H * w0;
        const float xf = img.pixels[gi], skyf = img.sky[gi];
        const double iota = (double)img.iota[h0];             // per ROW: nelec_per_nmgy[h] (elbo_objective.jl:374-385)
        bool valid = inp && !isnan(xf);                                                              // :459
        if (valid && P.bitmap_off >= 0) valid = bitmaps[P.bitmap_off + h2 + (int64_t)H2 * w2] != 0;  // :445
        const double hh = (double)(h0 + 1), ww = (double)(w0 + 1);
        double m = 0.0;
        if (valid && w2 < W2 - 1) m = fit_light(si, tc, NC, coef, etab, hh, ww);   // 1 <= w2 < W2, 1-based
        double B = 0.0;
        for (int64_t q = nb0; q < nb1; ++q) {
            const int v2 = table_entry(vis_off, vis_img, dense, N, nbr_idx[q], n);
            if (v2 < 0) continue;
            const DevPatch &Q = patches[v2];
            const int a = h0 - Q.off_h, b = w0 - Q.off_w;     // 0-based in the neighbour's patch
            bool in = valid & (a >= 0) & (a < Q.H2) & (b >= 0) & (b < Q.W2 - 1);   // strict: elbo_objective.jl:349
            if (in && Q.bitmap_off >= 0) in = bitmaps[Q.bitmap_off + a + (int64_t)Q.H2 * b] != 0;
            if (!__any(in)) continue;                         // (the workgroup is one wavefront: uniform)
            __syncthreads();
            fit_stage_comps(tq, comps + (size_t)v2 * NC, NC);
            __syncthreads();
            if (in) B += fit_light(srcimg[v2], tq, NC, coefs + (size_t)Q.stamp * (CEL_COEF * CEL_COEF), etab, hh, ww);
        }
        const double x = (double)xf;
        // (rounded products and differences by name: lam is the value the stamp shows, r the residual against that value)
        const double lam = __dmul_rn(iota, (double)skyf + m + B);
        const bool bad = valid && !(lam > 0.0 && isfinite(lam));
        double t[FIT_NS];
#pragma unroll
        for (int k = 0; k < FIT_NS; ++k) t[k] = 0.0;
        if (valid) {
            const double r = __dsub_rn(x, lam), own = __dmul_rn(iota, m);
            t[CELESTE_FIT_CHI2] = __dmul_rn(r, r) / lam;
            t[CELESTE_FIT_RESID] = r;
            t[CELESTE_FIT_OWN] = own;
            t[CELESTE_FIT_SELF] = m != 0.0 ? __dmul_rn(own, m / (m + B)) : 0.0;   // (m / (m + 0) = 1: self = own to the bit without neighbours)
            t[CELESTE_FIT_WRES] = __dmul_rn(own, r) / lam;
            t[CELESTE_FIT_WINFO] = __dmul_rn(own, own) / lam;
            t[CELESTE_FIT_MAX_Z] = fabs(r) / sqrt(lam);
        }
        if (stamps && inp) stamps[it.stamp_off + idx] = valid ? lam : (double)NAN;
#pragma unroll
        for (int k = 0; k < FIT_NS - 1; ++k) t[k] = wave_sum(t[k]);
        t[CELESTE_FIT_MAX_Z] = fit_wave_max(t[CELESTE_FIT_MAX_Z]);
        const int n_valid = __popcll(__ballot(valid));
        const int any_bad = __any(bad);
        if (lane == 0) {
            double *o = rec + (size_t)tile * FIT_REC;
#pragma unroll
            for (int k = 0; k < FIT_NS; ++k) o[k] = t[k];
            o[FIT_NS] = 0.0;
            FitTileInfo ti;
            ti.n_pix = n_valid; ti.bad = any_bad; ti.band = img.band - 1; ti.pad = 0;
            info[tile] = ti;
        }
    }
}

// tgt_rec[ti] = {first tile record, number of tile records} of target ti of the call
__global__ void __launch_bounds__(64)
fit_reduce_kernel(const int2 *__restrict__ tgt_rec, const int32_t *__restrict__ targets, const double *__restrict__ vp,
                  const double *__restrict__ rec, const FitTileInfo *__restrict__ info, double *__restrict__ stats,
                  int64_t *__restrict__ n_pix, int32_t *__restrict__ status) {
    const int ti = blockIdx.x, lane = threadIdx.x;
    const int b = lane >> 3, k = lane & 7;                    // lanes 0 .. 39: band b, statistic k (k = 7: the pixel count)
    const int2 tr = tgt_rec[ti];
    double acc = 0.0;
    int64_t cnt = 0;
    int bad = 0;
    // (a lane's loads do not depend on the tile's band: the loop is a chain of additions, not of loads)
    const int col = k < FIT_NS ? k : 0;
#pragma unroll 4
    for (int r = tr.x; r < tr.x + tr.y; ++r) {
        const FitTileInfo fi = info[r];
        const double x = rec[(size_t)r * FIT_REC + col];
        bad |= fi.bad;
        const bool mine = fi.band == b;
        if (k < CELESTE_FIT_MAX_Z) acc = mine ? acc + x : acc;
        else if (k == CELESTE_FIT_MAX_Z) acc = mine ? fmax(acc, x) : acc;
        else cnt += mine ? fi.n_pix : 0;
    }
    const double *vs = vp + (size_t)targets[ti] * CEL_P;
    const int nonfinite = __any(lane < CEL_P && !isfinite(vs[lane < CEL_P ? lane : 0]));
    const int st = nonfinite ? CELESTE_ERR_NONFINITE_INPUT : (bad ? CELESTE_ERR_NONFINITE_RESULT : CELESTE_OK);
    if (b < FIT_NB) {
        if (k < FIT_NS) stats[((size_t)ti * FIT_NB + b) * FIT_NS + k] = st != CELESTE_OK ? (double)NAN : acc;
        else n_pix[(size_t)ti * FIT_NB + b] = cnt;
    }
    if (lane == 0) status[ti] = st;
}

// ---- host side ----------------------------------------------------------------------------------------------------------
struct FitBuf { void *p = nullptr; size_t cap = 0; };

struct celeste_fit_ctx {
    celeste_ctx_t *c = nullptr;
    FitBuf buf[10];
    // host staging of one call: kept here so that it outlives the asynchronous copies
    std::vector<FitItem> items;
    std::vector<int2> tgt_rec;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    float last_ms[3] = {0, 0, 0};
};

template <class T>
static hipError_t fit_get(celeste_fit_ctx_t *f, int k, size_t bytes, T **out) {
    FitBuf &s = f->buf[k];
    if (bytes > s.cap) {
        hipError_t e = hipStreamSynchronize(f->c->stream);
        if (e != hipSuccess) return e;
        if (s.p) { (void)hipFree(s.p); s.p = nullptr; s.cap = 0; }
        const size_t cap = std::max<size_t>(bytes, 256);
        e = hipMalloc(&s.p, cap);
        if (e != hipSuccess) return e;
        s.cap = cap;
    }
    *out = (T *)s.p;
    return hipSuccess;
}

extern "C" int celeste_fit_version(void) { return CELESTE_FIT_ABI_VERSION; }

extern "C" const char *celeste_fit_strerror(int status) { return celeste_strerror(status); }

// The context's stream comes from the engine's pool (celeste_ctx_create: stream_acquire) and goes back to it
// (celeste_ctx_destroy: stream_retire); no stream is created or destroyed per call.
extern "C" int celeste_fit_ctx_create(const celeste_problem_t *problem, int device, celeste_fit_ctx_t **out) try {
    if (!out) return CELESTE_ERR_INVALID_ARG;
    *out = nullptr;
    celeste_ctx_t *c = nullptr;
    const int rc = celeste_ctx_create(problem, device, &c);
    if (rc != CELESTE_OK) return rc;
    celeste_fit_ctx_t *f = new celeste_fit_ctx_t();
    f->c = c;
    for (auto &e : f->ev)
        if (hipEventCreate(&e) != hipSuccess) { celeste_fit_ctx_destroy(f); return CELESTE_ERR_HIP; }
    *out = f;
    return CELESTE_OK;
} ABI_CATCH

extern "C" void celeste_fit_ctx_destroy(celeste_fit_ctx_t *f) {
    if (!f) return;
    if (f->c) {
        (void)hipSetDevice(f->c->device);
        (void)hipStreamSynchronize(f->c->stream);
        for (auto &s : f->buf) if (s.p) (void)hipFree(s.p);
        for (auto &e : f->ev) if (e) (void)hipEventDestroy(e);
        celeste_ctx_destroy(f->c);
    }
    delete f;
}

extern "C" int celeste_fit_stats(celeste_fit_ctx_t *f, const double *vp, int32_t n_targets, const int32_t *targets,
                                 int64_t *n_pix, double *stats, int32_t *status, int64_t *stamp_offsets, double *stamps) try {
    if (!f || !f->c || !vp || n_targets < 0 || (stamps && !stamp_offsets)) return CELESTE_ERR_INVALID_ARG;
    if (n_targets > 0 && (!targets || !n_pix || !stats || !status)) return CELESTE_ERR_INVALID_ARG;
    celeste_ctx_t *c = f->c;
    for (int ti = 0; ti < n_targets; ++ti)
        if (targets[ti] < 0 || targets[ti] >= c->S) return CELESTE_ERR_INVALID_ARG;
    if (n_targets == 0) return CELESTE_OK;
    // the work list: (visit of a target, chunk) in (target, image, chunk) order; a chunk's tile records follow each other
    std::vector<FitItem> &items = f->items;
    std::vector<int2> &tgt_rec = f->tgt_rec;
    items.clear();
    tgt_rec.assign((size_t)n_targets, make_int2(0, 0));
    const int chunk = c->chunk_px;       // (a multiple of 64)
    int64_t n_rec = 0, soff = 0, n_ent = 0;
    for (int ti = 0; ti < n_targets; ++ti) {
        const int t = targets[ti];
        const int64_t first = n_rec;
        for (int v = c->h_vis_off[t]; v < c->h_vis_off[t + 1]; ++v) {
            const DevPatch &P = c->h_patches[v];
            const int npx = P.H2 * P.W2;
            if (npx <= 0) continue;      // (every image is listed when the table is dense: an empty patch is no entry)
            for (int p0 = 0; p0 < npx; p0 += chunk) {
                if (n_rec > 0x7fffff00ll || items.size() >= 0x7fffff00ull) return CELESTE_ERR_INVALID_ARG;   // (32-bit record and grid indices)
                FitItem it;
                it.sn = v; it.n = c->h_vis_img[v]; it.p0 = p0; it.rec0 = (int32_t)n_rec; it.stamp_off = soff;
                items.push_back(it);
                n_rec += (std::min(npx, p0 + chunk) - p0 + 63) / 64;
            }
            if (stamp_offsets) stamp_offsets[n_ent] = soff;
            ++n_ent;
            soff += npx;
        }
        tgt_rec[ti] = make_int2((int)first, (int)(n_rec - first));
    }
    if (stamp_offsets) stamp_offsets[n_ent] = soff;
    HIP_TRY(hipSetDevice(c->device));
    const size_t nt = (size_t)n_targets, ni = items.size();
    double *d_vp = nullptr, *d_rec = nullptr, *d_stats = nullptr, *d_stamps = nullptr;
    FitItem *d_items = nullptr;
    FitTileInfo *d_info = nullptr;
    int2 *d_tgt_rec = nullptr;
    int32_t *d_targets = nullptr, *d_status = nullptr;
    int64_t *d_npix = nullptr;
    if (fit_get(f, 0, (size_t)c->S * CEL_P * sizeof(double), &d_vp) != hipSuccess ||
        fit_get(f, 1, ni * sizeof(FitItem), &d_items) != hipSuccess ||
        fit_get(f, 2, (size_t)n_rec * FIT_REC * sizeof(double), &d_rec) != hipSuccess ||
        fit_get(f, 3, (size_t)n_rec * sizeof(FitTileInfo), &d_info) != hipSuccess ||
        fit_get(f, 4, nt * sizeof(int2), &d_tgt_rec) != hipSuccess ||
        fit_get(f, 5, nt * sizeof(int32_t), &d_targets) != hipSuccess ||
        fit_get(f, 6, nt * FIT_NB * FIT_NS * sizeof(double), &d_stats) != hipSuccess ||
        fit_get(f, 7, nt * FIT_NB * sizeof(int64_t), &d_npix) != hipSuccess ||
        fit_get(f, 8, nt * sizeof(int32_t), &d_status) != hipSuccess ||
        (stamps && fit_get(f, 9, (size_t)soff * sizeof(double), &d_stamps) != hipSuccess))
        return CELESTE_ERR_HIP;
    hipStream_t st = c->stream;
    HIP_TRY(hipMemcpyAsync(d_vp, vp, (size_t)c->S * CEL_P * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_targets, targets, nt * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_tgt_rec, tgt_rec.data(), nt * sizeof(int2), hipMemcpyHostToDevice, st));
    if (ni > 0) HIP_TRY(hipMemcpyAsync(d_items, items.data(), ni * sizeof(FitItem), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(f->ev[0], st));
    if (c->V > 0)
        hipLaunchKernelGGL(prep_kernel, dim3((unsigned)c->V), dim3(64), 0, st, d_vp, c->d_images, c->d_patches, c->d_vis_src,
                           c->d_vis_img, c->N, c->K, c->d_srcimg, c->d_comps, nullptr, c->d_vis_off, c->M, (int)c->dense, nullptr,
                           nullptr, 0);
    HIP_TRY(hipEventRecord(f->ev[1], st));
    if (ni > 0)
        hipLaunchKernelGGL(fit_pixel_kernel, dim3((unsigned)ni), dim3(64), 0, st, d_items, c->d_images, c->d_patches, c->d_coefs,
                           c->d_bitmaps, c->d_srcimg, c->d_comps, c->d_nbr_off, c->d_nbr_idx, c->d_vis_off, c->d_vis_img,
                           c->d_vis_src, (int)c->dense, c->N, c->NC, chunk, d_rec, d_info, stamps ? d_stamps : nullptr);
    HIP_TRY(hipEventRecord(f->ev[2], st));
    hipLaunchKernelGGL(fit_reduce_kernel, dim3((unsigned)nt), dim3(64), 0, st, d_tgt_rec, d_targets, d_vp, d_rec, d_info, d_stats,
                       d_npix, d_status);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(f->ev[3], st));
    HIP_TRY(hipMemcpyAsync(stats, d_stats, nt * FIT_NB * FIT_NS * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(n_pix, d_npix, nt * FIT_NB * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(status, d_status, nt * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (stamps && soff > 0) HIP_TRY(hipMemcpyAsync(stamps, d_stamps, (size_t)soff * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int k = 0; k < 3; ++k)
        if (hipEventElapsedTime(&f->last_ms[k], f->ev[k], f->ev[k + 1]) != hipSuccess) f->last_ms[k] = 0;
    for (int ti = 0; ti < n_targets; ++ti) if (status[ti] != CELESTE_OK) return status[ti];
    return CELESTE_OK;
} ABI_CATCH

extern "C" int celeste_fit_last_ms(celeste_fit_ctx_t *f, float ms[3]) {
    if (!f || !ms) return CELESTE_ERR_INVALID_ARG;
    for (int k = 0; k < 3; ++k) ms[k] = f->last_ms[k];
    return CELESTE_OK;
}
