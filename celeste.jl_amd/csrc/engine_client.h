// engine_client.h -- what the libraries that compile the engine's context into themselves (blend, fit, phot, info, resid, astrom) share.
//
// Included right after engine_context.h (blend: after engine_eval.h, which includes it), whose celeste_ctx, HIP_TRY, Comp, SrcImg, DevPatch, table_entry ... it uses; the engine
// does not include it.  Everything here is static or __device__ __forceinline__: no library's export map knows of it.
//   host    a context base (engine context, growable device buffers, stage events, stage times) with its create and destroy,
//           the status fold; for the libraries that walk pixel visits (fit, phot, info): the target check, the prep_kernel
//           launch at the call's table, the stage times, the work item and the walk over (target, non-empty visit, chunk)
//   device  one source's light at a pixel, the staging of its components, the wavefront maximum, the non-finite test of a
//           parameter row, and the pixel walk of a work item with the ELBO's neighbour rule (visit_pixel_walk)
#pragma once
#include <type_traits>

// Mutation testing (tests/test_satellite_mutants.py builds fit and phot with -DCELESTE_CLIENT_MUTANT=k and checks that their
// parity tests notice; its own macro, because both libraries compile the engine, whose CELESTE_MUTANT numbers keep their
// meaning).  All in visit_pixel_walk; a mutant changes arithmetic or an index inside the same array, never a bound, a size, a
// barrier or the control flow around one.  0 = the product;
//   1 = the target's own light also in its patch's last column (w2 < W2)
//   2 = a neighbour's light also in the neighbour's last column (b < Q.W2; its bitmap index a + Q.H2 b stays <= Q.H2 Q.W2 - 1)
//   3 = the neighbour's bitmap is ignored
//   4 = the target's bitmap is read transposed (w2 + W2 h2 <= W2 - 1 + W2 (H2 - 1) = W2 H2 - 1)
//   5 = iota indexed by column, clamped to its H entries (img.iota[min(w0, img.H - 1)])
//   6 = the neighbour's star density uses the target's stamp (P.stamp for Q.stamp: both checked at context creation)
// Never defined in the shipped build.
#ifndef CELESTE_CLIENT_MUTANT
#define CELESTE_CLIENT_MUTANT 0
#endif

// ---- host: the context --------------------------------------------------------------------------------------------------
struct ClientBuf { void *p = nullptr; size_t cap = 0; };

// NEV events bound the stages of a call; last_ms holds NMS figures about the last one
template <int NBUF, int NEV, int NMS>
struct ClientCtx {
    celeste_ctx_t *c = nullptr;
    ClientBuf buf[NBUF];
    hipEvent_t ev[NEV] = {};
    float last_ms[NMS] = {};
};

// Buffer k of the context with room for `bytes` (at least 256 B; a buffer keeps its capacity).  Growing waits for the
// context's stream first: work in flight may still use the old block.
template <class Ctx, class T>
static hipError_t client_get(Ctx *f, int k, size_t bytes, T **out) {
    ClientBuf &s = f->buf[k];
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

template <class Ctx>
static void client_destroy(Ctx *f) {
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

// The context's stream comes from the engine's pool (celeste_ctx_create: stream_acquire) and goes back to it
// (celeste_ctx_destroy: stream_retire); no stream is created or destroyed per call.
template <class Ctx>
static int client_create(const celeste_problem_t *problem, int device, Ctx **out) {
    if (!out) return CELESTE_ERR_INVALID_ARG;
    *out = nullptr;
    celeste_ctx_t *c = nullptr;
    const int rc = celeste_ctx_create(problem, device, &c);
    if (rc != CELESTE_OK) return rc;
    Ctx *f = new Ctx();
    f->c = c;
    for (auto &e : f->ev)
        if (hipEventCreate(&e) != hipSuccess) { client_destroy(f); return CELESTE_ERR_HIP; }
    *out = f;
    return CELESTE_OK;
}

template <class Ctx>
static int client_last_ms(const Ctx *f, float *ms) {
    if (!f || !ms) return CELESTE_ERR_INVALID_ARG;
    for (size_t k = 0; k < sizeof(f->last_ms) / sizeof(float); ++k) ms[k] = f->last_ms[k];
    return CELESTE_OK;
}

// the first non-OK status is the call's return code
static inline int client_first_status(const int32_t *status, int32_t n) {
    for (int i = 0; i < n; ++i) if (status[i] != CELESTE_OK) return status[i];
    return CELESTE_OK;
}

// ---- host: a call over pixel visits (fit, phot, info) ----------------------------------------------------------------------
static inline bool client_targets_ok(const celeste_ctx_t *c, int32_t n_targets, const int32_t *targets) {
    for (int ti = 0; ti < n_targets; ++ti)
        if (targets[ti] < 0 || targets[ti] >= c->S) return false;
    return true;
}

// SrcImg and Comp of every visit of the context at the table d_vp
static inline void client_launch_prep(celeste_ctx_t *c, const double *d_vp, hipStream_t st) {
    if (c->V > 0)
        hipLaunchKernelGGL(prep_kernel, dim3((unsigned)c->V), dim3(64), 0, st, d_vp, c->d_images, c->d_patches, c->d_vis_src,
                           c->d_vis_img, c->N, c->K, c->d_srcimg, c->d_comps, nullptr, c->d_vis_off, c->M, (int)c->dense, nullptr,
                           nullptr, 0);
}

// last_ms[k] = the device time between events k and k + 1 (after the stream has been waited for)
template <class Ctx>
static void client_stage_ms(Ctx *f) {
    for (size_t k = 0; k < sizeof(f->last_ms) / sizeof(float); ++k)
        if (hipEventElapsedTime(&f->last_ms[k], f->ev[k], f->ev[k + 1]) != hipSuccess) f->last_ms[k] = 0;
}

// A work item of the pixel kernels: a chunk of CELESTE_CHUNK_PX pixels of a visit.  Tiles (64 consecutive pixels of a patch)
// and pixels are numbered through the call, in (target, image) order.
struct VisitItem {
    int32_t sn, n;                     // visit (table entry of the target's patch), image
    int32_t p0;                        // first pixel of the chunk
    int32_t tile0;                     // the chunk's first tile
    int64_t px_off;                    // where the visit's pixels start in the call's per-pixel planes
};

// The work list of a call: the chunks of every non-empty visit of every target, in (target, image, chunk) order, appended to
// items; entry(ti, v, npx, tile0, tile1, px_off) is called once per visit (an empty patch is no entry: every image is listed
// when the table is dense) and may refuse.  false: refused, or an index of the call leaves 32 bits.
template <class F>
static bool client_walk(const celeste_ctx_t *c, int32_t n_targets, const int32_t *targets, std::vector<VisitItem> &items,
                        int64_t &n_tiles, int64_t &n_px, F entry) {
    const int chunk = c->chunk_px;       // (a multiple of 64)
    items.clear();
    n_tiles = n_px = 0;
    for (int ti = 0; ti < n_targets; ++ti) {
        const int t = targets[ti];
        for (int v = c->h_vis_off[t]; v < c->h_vis_off[t + 1]; ++v) {
            const DevPatch &P = c->h_patches[v];
            const int npx = P.H2 * P.W2;
            if (npx <= 0) continue;
            const int64_t tile0 = n_tiles;
            for (int p0 = 0; p0 < npx; p0 += chunk) {
                if (n_tiles > 0x7fffff00ll || items.size() >= 0x7fffff00ull) return false;   // (32-bit tile and grid indices)
                VisitItem it;
                it.sn = v; it.n = c->h_vis_img[v]; it.p0 = p0; it.tile0 = (int32_t)n_tiles; it.px_off = n_px;
                items.push_back(it);
                n_tiles += (std::min(npx, p0 + chunk) - p0 + 63) / 64;
            }
            if (!entry(ti, v, npx, tile0, n_tiles, n_px)) return false;
            n_px += npx;
        }
    }
    return true;
}

// ---- device ----------------------------------------------------------------------------------------------------------------
// E_G_s.v of one source at the pixel (hh, ww) (1-based image coordinates): value_pixel's expression
__device__ __forceinline__ double visit_light(const SrcImg &si, const Comp *tc, int NC, const double *__restrict__ coef,
                                              const double *etab, double hh, double ww) {
    const double f0 = star_value(coef, hh + (26.0 - si.m1), ww + (26.0 - si.m2));
    const double f1 = galaxy_value(tc, NC, hh - si.m1, ww - si.m2, etab);
    return si.c0 * f0 + si.c1 * f1;
}

__device__ __forceinline__ void visit_stage_comps(Comp *dst, const Comp *__restrict__ src, int NC) {
    const double *s = reinterpret_cast<const double *>(src);
    double *d = reinterpret_cast<double *>(dst);
    for (int i = threadIdx.x; i < NC * 8; i += 64) d[i] = s[i];
}

__device__ __forceinline__ double wave_max(double x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x = fmax(x, __shfl_xor(x, o, 64));
    return x;
}

// lane's share of "one of the row's 44 parameters is not finite" (to be joined by __any or __syncthreads_or)
__device__ __forceinline__ bool row_nonfinite(const double *vs, int lane) {
    return lane < CEL_P && !isfinite(vs[lane < CEL_P ? lane : 0]);
}

// What the pixel walk hands a lane per tile (line numbers: elbo_objective.jl)
struct VisitPixel {
    int tile, idx;                     // the tile (numbered through the call); the lane's pixel in the patch
    bool inp, valid;                   // the pixel is in the chunk; it is visited too: not NaN (:459) and set in the patch's bitmap (:445)
    float xf, skyf;                    // the pixel and its sky
    double iota;                       // per ROW: nelec_per_nmgy[h] (:374-385)
    double m;                          // the target's own light; 0 in the patch's last column: 1 <= w2 < W2, 1-based
    double B;                          // the neighbours' light
};

// What a tile_fn that takes a third argument gets besides (info: the densities' gradients are its own work): the target's
// staged components and the exponential's table (LDS), its spline coefficients, its pixel-space position, the lane's 1-based
// image coordinates, and whether the target's own light counts at the pixel (visited and not in the patch's last column)
struct VisitOwn {
    const Comp *tc;
    const double *etab;
    const double *coef;
    double m1, m2;
    double hh, ww;
    bool own;
};

// The pixel walk of a work item by its wavefront (a workgroup of 64): for each 64-pixel tile of the chunk a lane owns a pixel and
// calls tile_fn(img, px) -- or tile_fn(img, px, own) where tile_fn takes a VisitOwn -- in uniform control flow, so tile_fn may
// use wavefront operations.  The neighbour rule: B adds each neighbour listed for the target that has an entry for the image,
// whose patch holds the pixel strictly inside (not in its last column, :349) and whose bitmap has it set, evaluated at the
// pixel -- per link, not once per neighbour pixel.  A neighbour no lane of the tile needs is skipped without staging its
// components.
// The tables are the kernel's own __restrict__ parameters, passed on one by one: a struct of them loses the no-alias
// information and with it the scalar loads.  The pixel goes to tile_fn as one struct by reference and tile_fn reads it into
// locals first; with ten arguments by value the compiler folds phot's soundness test another way (two more VGPRs).

template <class F>
__device__ __forceinline__ void visit_pixel_walk(const VisitItem &it, const DevImage *__restrict__ images,
                                                 const DevPatch *__restrict__ patches, const double *__restrict__ coefs,
                                                 const uint8_t *__restrict__ bitmaps, const SrcImg *__restrict__ srcimg,
                                                 const Comp *__restrict__ comps, const int64_t *__restrict__ nbr_off,
                                                 const int32_t *__restrict__ nbr_idx, const int32_t *__restrict__ vis_off,
                                                 const int32_t *__restrict__ vis_img, const int32_t *__restrict__ vis_src,
                                                 int dense, int N, int NC, int chunk_px, F tile_fn) {
    __shared__ double etab[64];
    __shared__ Comp tc[14 * CEL_MAXK];     // the target's components
    __shared__ Comp tq[14 * CEL_MAXK];     // the current neighbour's
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
    visit_stage_comps(tc, comps + (size_t)sn * NC, NC);
    __syncthreads();
    const double *__restrict__ coef = coefs + (size_t)P.stamp * (CEL_COEF * CEL_COEF);
    const int64_t nb0 = nbr_off[s], nb1 = nbr_off[s + 1];
    int tile = it.tile0;
    for (int base = it.p0; base < p1; base += 64, ++tile) {
        const int idx = base + lane;
        const bool inp = idx < p1;
        int w2, h2;                                           // 0-based in the patch
        divmod_small(min(idx, npx - 1), H2, rH2, w2, h2);
        const int h0 = P.off_h + h2, w0 = P.off_w + w2;       // 0-based in the image
        const size_t gi = (size_t)h0 + (size_t)img.H * w0;
        const float xf = img.pixels[gi], skyf = img.sky[gi];
#if CELESTE_CLIENT_MUTANT == 5
        const double iota = (double)img.iota[min(w0, img.H - 1)];
#else
        const double iota = (double)img.iota[h0];
#endif
        bool valid = inp && !isnan(xf);
#if CELESTE_CLIENT_MUTANT == 4
        if (valid && P.bitmap_off >= 0) valid = bitmaps[P.bitmap_off + w2 + (int64_t)W2 * h2] != 0;
#else
        if (valid && P.bitmap_off >= 0) valid = bitmaps[P.bitmap_off + h2 + (int64_t)H2 * w2] != 0;
#endif
        const double hh = (double)(h0 + 1), ww = (double)(w0 + 1);
        double m = 0.0;
#if CELESTE_CLIENT_MUTANT == 1
        const bool own = valid && w2 < W2;
#else
        const bool own = valid && w2 < W2 - 1;
#endif
        if (own) m = visit_light(si, tc, NC, coef, etab, hh, ww);
        double B = 0.0;
        for (int64_t q = nb0; q < nb1; ++q) {
            const int v2 = table_entry(vis_off, vis_img, dense, N, nbr_idx[q], n);
            if (v2 < 0) continue;
            const DevPatch &Q = patches[v2];
            const int a = h0 - Q.off_h, b = w0 - Q.off_w;     // 0-based in the neighbour's patch
#if CELESTE_CLIENT_MUTANT == 2
            bool in = valid & (a >= 0) & (a < Q.H2) & (b >= 0) & (b < Q.W2);
#else
            bool in = valid & (a >= 0) & (a < Q.H2) & (b >= 0) & (b < Q.W2 - 1);
#endif
#if CELESTE_CLIENT_MUTANT == 3
            // (the neighbour's bitmap is not read)
#else
            if (in && Q.bitmap_off >= 0) in = bitmaps[Q.bitmap_off + a + (int64_t)Q.H2 * b] != 0;
#endif
            if (!__any(in)) continue;                         // (the workgroup is one wavefront: uniform)
            __syncthreads();
            visit_stage_comps(tq, comps + (size_t)v2 * NC, NC);
            __syncthreads();
#if CELESTE_CLIENT_MUTANT == 6
            if (in) B += visit_light(srcimg[v2], tq, NC, coefs + (size_t)P.stamp * (CEL_COEF * CEL_COEF), etab, hh, ww);
#else
            if (in) B += visit_light(srcimg[v2], tq, NC, coefs + (size_t)Q.stamp * (CEL_COEF * CEL_COEF), etab, hh, ww);
#endif
        }
        const VisitPixel px = {tile, idx, inp, valid, xf, skyf, iota, m, B};
        if constexpr (std::is_invocable_v<F, const DevImage &, const VisitPixel &, const VisitOwn &>) {
            const VisitOwn ow = {tc, etab, coef, si.m1, si.m2, hh, ww, own};
            tile_fn(img, px, ow);
        } else {
            tile_fn(img, px);
        }
    }
}
