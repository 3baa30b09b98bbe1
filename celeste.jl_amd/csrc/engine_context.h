// engine_context.h -- the engine's context: the host side every library that walks the problem's pixels compiles.
//
// Owns the device copies of the problem (images, patches, spline coefficients, neighbour graph), the stream and
// page-locked pools and the upload arena, and defines celeste_images_create / celeste_ctx_create[_on] / celeste_ctx_destroy.
// engine_eval.h (the evaluation launcher: the engine's celeste_abi.hip and the blend library) includes it under the kernels
// it launches; the fit, phot, info, resid and astrom libraries include it alone, followed by engine_client.h.  Nothing here
// evaluates the ELBO: a context's evaluation and optimiser buffers are plain pointers that only engine_eval.h and
// celeste_abi.hip fill.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "elbo_kernels.h"
#include "host_tables.h"
#include "value_union.h"

#define HIP_TRY(expr)                                                                    \
    do {                                                                                 \
        hipError_t e__ = (expr);                                                         \
        if (e__ != hipSuccess) {                                                         \
            fprintf(stderr, "celeste_mi355x: %s failed: %s (%s:%d)\n", #expr,            \
                    hipGetErrorString(e__), __FILE__, __LINE__);                         \
            return CELESTE_ERR_HIP;                                                      \
        }                                                                                \
    } while (0)

// Every device allocation of the library goes through here.  CELESTE_POISON=1 (testing) fills fresh allocations with 0xFF
// bytes -- NaN as a double or float, -1 as an integer -- so that a kernel that reads what no kernel or copy has written
// shows it in every run instead of in the rare one where recycled memory happens to hold something harmful (the tables of a
// batch are marked with batch stamps, not cleared: DESIGN.md section 3).
static hipError_t celeste_device_malloc(void **p, size_t bytes) {
    hipError_t e = (hipMalloc)(p, bytes);
    static const bool poison = [] { const char *v = getenv("CELESTE_POISON"); return v && atoi(v) != 0; }();
    if (e == hipSuccess && poison) {
        e = hipMemset(*p, 0xFF, bytes);
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    return e;
}
#define hipMalloc(p, bytes) celeste_device_malloc((void **)(p), (bytes))

// ---- streams are recycled, never destroyed ------------------------------------------------------------------------------
// The HIP runtime (ROCm 7.0.2's libamdhip64, the one PyTorch bundles) was caught writing into a stream object AFTER
// hipStreamDestroy had freed it: with the host's cores oversubscribed (eight test processes, each with a 256-thread OpenMP
// checker) one context in ~800 left a stale decrement and a stale 32-bit zero in whatever heap block took the 920 bytes of its
// copy stream next -- a numpy array of the following test (found with tools/heapwho: the block's last owner allocated in
// hipStreamCreateWithFlags under celeste_ctx_create_on and freed in hipStreamDestroy under celeste_ctx_destroy; the streams
// were idle and synchronised, their events destroyed).  A library whose callers create a context per source
// (ParallelRun.jl:468-488) cannot afford a destroy that corrupts the caller's heap, so a context's streams go back to a
// per-device pool (idle, synchronised) and the next context takes them from there; the pool is never torn down.  It also
// keeps the stream -> hardware-queue assignment of a process stable (pick_copy_stream).  An idle stream holds about 1 MB of
// device memory (measured: 200 streams, 216 MB), so the pool keeps at most CELESTE_STREAM_POOL_MAX streams per device (default
// 32: the streams of 16 contexts); beyond that a stream is destroyed as before -- only a process that closes more than
// 16 contexts without opening one in between gets there.
struct StreamPool {
    std::mutex mu;
    std::vector<hipStream_t> idle[16];
};
static StreamPool &stream_pool() { static StreamPool *p = new StreamPool(); return *p; }   // (leaked on purpose: no HIP call at exit)
static hipError_t stream_acquire(int device, hipStream_t *out) {
    *out = nullptr;
    if (device >= 0 && device < 16) {
        StreamPool &sp = stream_pool();
        std::lock_guard<std::mutex> lk(sp.mu);
        if (!sp.idle[device].empty()) { *out = sp.idle[device].back(); sp.idle[device].pop_back(); return hipSuccess; }
    }
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}
static void stream_retire(int device, hipStream_t s) {
    if (!s) return;
    if (hipStreamSynchronize(s) == hipSuccess && device >= 0 && device < 16) {
        static const size_t cap = [] { const char *e = getenv("CELESTE_STREAM_POOL_MAX"); return e ? (size_t)std::max(0, atoi(e)) : (size_t)32; }();
        StreamPool &sp = stream_pool();
        std::lock_guard<std::mutex> lk(sp.mu);
        if (sp.idle[device].size() < cap) { sp.idle[device].push_back(s); return; }
    } else (void)hipGetLastError();
    (void)hipStreamDestroy(s);
}

// ---- page-locked staging blocks are recycled too -------------------------------------------------------------------------
// A context's staging (the block pair of the small host-pointer calls, the parts' blocks of a host-pointer sweep, the
// optimiser's table and state copies) is page-locked memory, and the runtime takes 30 .. 115 us to lock a block and 210 .. 330 us
// to release one: of the 1.1 ms that creating a per-source context, calling it once and destroying it took (process_source's
// pattern, ParallelRun.jl:468-488; tools/gpu_per_source_ctx_time.py under rocprofv3 --hip-trace), two hipHostFree were 483 us and
// two hipHostMalloc 102 -- against 76 us for an evaluation.  Blocks of up to 1 MB go back to a pool of power-of-two size classes
// (CELESTE_PINNED_POOL_KB, default 16384 per process) instead; larger ones and everything beyond the cap are released as before.
struct PinnedPool {
    std::mutex mu;
    std::unordered_map<void *, int> live;       // blocks handed out -> size class
    std::vector<void *> idle[9];                // 4 KB << class, class 0 .. 8 (1 MB)
    size_t idle_bytes = 0;
};
static PinnedPool &pinned_pool() { static PinnedPool *p = new PinnedPool(); return *p; }   // (leaked on purpose)
static size_t pinned_pool_cap() {
    static const size_t cap = [] { const char *v = getenv("CELESTE_PINNED_POOL_KB"); return (size_t)(v ? std::max(0, atoi(v)) : 16384) << 10; }();
    return cap;
}
static hipError_t staging_alloc(void **p, size_t bytes) {
    *p = nullptr;
    int k = -1;
    if (pinned_pool_cap() && bytes <= (1u << 20)) { k = 0; while (((size_t)4096 << k) < bytes) ++k; }
    // (hipHostMallocPortable: a recycled block may serve a context on another device of the process)
    if (k < 0) return hipHostMalloc(p, std::max<size_t>(bytes, 1), hipHostMallocPortable);
    PinnedPool &pp = pinned_pool();
    {
        std::lock_guard<std::mutex> lk(pp.mu);
        if (!pp.idle[k].empty()) { *p = pp.idle[k].back(); pp.idle[k].pop_back(); pp.idle_bytes -= (size_t)4096 << k; pp.live[*p] = k; return hipSuccess; }
    }
    hipError_t e = hipHostMalloc(p, (size_t)4096 << k, hipHostMallocPortable);
    if (e == hipSuccess) { std::lock_guard<std::mutex> lk(pp.mu); pp.live[*p] = k; }
    return e;
}
static void staging_free(void *p) {
    if (!p) return;
    {
        PinnedPool &pp = pinned_pool();
        std::lock_guard<std::mutex> lk(pp.mu);
        auto it = pp.live.find(p);
        if (it != pp.live.end()) {
            const int k = it->second;
            pp.live.erase(it);
            if (pp.idle_bytes + ((size_t)4096 << k) <= pinned_pool_cap()) { pp.idle[k].push_back(p); pp.idle_bytes += (size_t)4096 << k; return; }
        }
    }
    (void)hipHostFree(p);
}


// image planes in HBM, shared by every context created on the handle (reference counted)
struct celeste_images {
    int device = 0;
    int N = 0;
    std::vector<DevImage> h_images;
    std::vector<void *> plane_allocs;
    DevImage *d_images = nullptr;
    std::atomic<int> refs{1};
};

static void images_release(celeste_images *im) {
    if (!im || im->refs.fetch_sub(1) != 1) return;
    (void)hipSetDevice(im->device);
    for (void *p : im->plane_allocs) (void)hipFree(p);
    if (im->d_images) (void)hipFree(im->d_images);
    delete im;
}

struct celeste_ctx {
    int device = 0;
    celeste_images *imgs = nullptr;
    hipStream_t stream = nullptr;        // private non-blocking stream of the host-pointer entry points
    hipStream_t copy_stream = nullptr;   // device-to-host copies of finished parts of a batch
    bool copy_stream_checked = false;    // pick_copy_stream has run (first batch that overlaps copies with kernels)
    int N = 0, S = 0, K = 0, NC = 0, n_stamps = 0;
    int chunk_px = 256, CH = 1;
    int max_npx = 0;
    // host mirrors (for work stats / validation)
    std::vector<DevPatch> h_patches;
    std::vector<int64_t> h_nbr_off;
    std::vector<int32_t> h_nbr_idx;
    // device
    DevImage *d_images = nullptr;        // = imgs->d_images
    DevPatch *d_patches = nullptr;
    double *d_coefs = nullptr;
    float *d_coefs_f = nullptr;          // the spline coefficients rounded to float (single-precision mode)
    uint8_t *d_bitmaps = nullptr;
    int64_t *d_nbr_off = nullptr;
    int32_t *d_nbr_idx = nullptr;
    PriorDev *d_prior = nullptr;
    SrcImg *d_srcimg = nullptr;
    Comp *d_comps = nullptr;
    SrcGeo *d_geo = nullptr;
    int64_t *d_val_off = nullptr;   // per (source, image): offset of the patch in d_val
    double2 *d_val = nullptr;       // pre-rendered (E_G_s.v, var_G_s.v) of neighbour sources, per patch pixel
    int32_t *d_needed = nullptr;    // per source: stamp of the last batch it was a target of
    int32_t stamp = 0;
    // visit lists: the images each source has a non-empty patch in (grids run over these, tables stay S x N)
    std::vector<int32_t> h_vis_off, h_vis_img, h_vis_src;
    int32_t *d_vis_off = nullptr, *d_vis_img = nullptr, *d_vis_src = nullptr;
    int4 *d_value_items = nullptr;  // value_kernel work items: {neighbour's table entry, target's, chunk, target}
    int4 *d_vitems_src = nullptr;   // the same, grouped by target
    int32_t *d_vitem_off = nullptr; // S + 1 offsets into d_vitems_src
    std::vector<int32_t> h_vitem_off;
    std::vector<int32_t> h_vitem_tgt;   // target of every item of d_value_items (prepared target lists pick theirs by it)
    std::vector<ValueUnionLink> h_vitem_link;   // ... and its {neighbour's visit, target's visit} (value_union_build)
    int64_t n_value_items = 0;
    std::vector<struct celeste_targets *> lists;   // prepared target lists still alive (celeste_targets_create)
    int32_t *d_prep_mark = nullptr; // per source: stamp of the last batch that read its per-image tables
    double *d_lg_sum = nullptr;     // per visit: sum of lgamma(pixel + 1) over the patch's visited pixels
    int64_t *d_nv_base = nullptr;   // visit-list mode: per source, start of its rows in d_nbr_vis
    std::vector<int64_t> h_nv_base; // its host mirror (a prepared list describes its work items from it)
    int32_t *d_nbr_vis = nullptr;   // visit-list mode: [visit of s][neighbour of s] -> the neighbour's visit in that image
    int2 *d_items = nullptr;         // [ti * M + j] of the current batch: {visit, image}
    size_t items_cap = 0;
    // work list of pixel_kernel (work_count / work_scan / work_fill kernels), per batch
    std::vector<int32_t> h_src_chunks;   // per source: chunks of all its patches
    std::vector<int64_t> h_top_chunks;   // [k]: chunks of the k sources that have most (bound for k unknown targets)
    int max_src_chunks = 0;
    int32_t *d_work = nullptr, *d_work_blk = nullptr, *d_work_total = nullptr;
    size_t work_cap = 0, work_blk_cap = 0;
    int M = 1;        // largest number of images one source appears in
    bool dense = false;
    int64_t V = 0;    // visits in total
    // split variant: per (source, image) first 64-pixel tile in d_rec, allocated on first use
    std::vector<int64_t> h_tile_off;
    int64_t *d_tile_off = nullptr;
    int64_t n_tiles = 0;
    int sum_tiles = 4, RCH = 1;   // record_sum_kernel: tiles per workgroup, parts per patch
    double *d_rec = nullptr;
    double *d_acc_split = nullptr;
    size_t acc_split_cap = 0;
    // per-batch scratch (grown on demand)
    double *d_acc = nullptr;
    size_t acc_cap = 0;
    int32_t *d_rec_off = nullptr;    // [ti * M + j]: first chunk record of the j-th visit of target ti in d_acc
    size_t rec_off_cap = 0;
    // staging for the host-pointer API: device side, and page-locked host side
    double *d_vp = nullptr;
    int32_t *d_targets = nullptr;
    double *d_v = nullptr, *d_d = nullptr, *d_h = nullptr;
    int64_t *d_cnt = nullptr;
    int32_t *d_status = nullptr;
    size_t stage_cap = 0;
    double *p_vp = nullptr;              // pinned: S x 44
    int32_t *p_targets = nullptr, *p_status = nullptr;
    double *p_v = nullptr, *p_d = nullptr, *p_h = nullptr;
    int64_t *p_cnt = nullptr;
    size_t pin_cap = 0;
    // small host-pointer calls (eval_small): one block up (table + targets), one block down (all outputs)
    double *d_small_in = nullptr, *p_small_in = nullptr, *d_small_out = nullptr, *p_small_out = nullptr;
    static const int MAX_PARTS = 8;
    hipEvent_t part_done[MAX_PARTS] = {}, part_copied[MAX_PARTS] = {};
    // buffers of celeste_maximize_batch, kept between calls (grown on demand)
    struct OptBuffers {
        size_t cap = 0;
        double *d_vp = nullptr, *d_v = nullptr, *d_d = nullptr, *d_h = nullptr, *d_H = nullptr, *d_T = nullptr, *d_S = nullptr, *d_pos = nullptr;
        int32_t *d_targets = nullptr, *d_act[2] = {nullptr, nullptr}, *d_evt[2] = {nullptr, nullptr}, *d_count = nullptr,
                *d_st = nullptr;
        void *d_state = nullptr;
        // page-locked: the parameter table (in / out), the final optimiser states, a ring of live-target counts
        static const int RING = 4;
        double *h_vp = nullptr;
        void *h_state = nullptr;
        int32_t *h_count = nullptr;
        hipEvent_t ev[RING] = {};
    } opt;
    // buffers of the fused optimiser launch, kept between calls (grown on demand)
    struct FusedBuffers {
        size_t cap_t = 0, cap_rec = 0, cap_q = 0, cap_saved = 0;
        bool arrivals_dirty = true;        // the arrival counters may hold anything (fresh allocation, an aborted launch)
        int4 *d_chunk_desc = nullptr;
        int2 *d_tgt_rec = nullptr;
        int32_t *d_q_items = nullptr, *d_q_ctl = nullptr, *d_arrivals = nullptr;
        double *d_saved = nullptr;          // the targets' rows before the optimisation
        int32_t *h_ctl = nullptr;           // page-locked copy of the queue control words of the last launch
        int max_resident = 0;               // workgroups of that launch the device holds at once
        int cus = 0;                        // compute units of the device
    } fused;
    // device scratch of the less travelled entry points (eval_multi, render_expected): grown on demand, kept
    struct Scratch { void *p = nullptr; size_t cap = 0; } scratch[24];   // 13..22: the joint inference
    // timing
    int timing = 0;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int ev_split = 0;
    int ev_valid = 0;
};

// No C++ exception crosses the C ABI (the callers are C, Julia's ccall, ctypes): every entry point that can allocate through
// the standard library is a function-try-block ending in this handler.
#define ABI_CATCH catch (const std::bad_alloc &) { return CELESTE_ERR_ALLOC; } catch (...) { return CELESTE_ERR_HIP; }

extern "C" int celeste_version(void) { return CELESTE_ABI_VERSION; }

extern "C" const char *celeste_strerror(int status) {
    switch (status) {
        case CELESTE_OK: return "ok";
        case CELESTE_ERR_INVALID_ARG: return "invalid argument";
        case CELESTE_ERR_NONFINITE_INPUT: return "vp contains NaNs or Infs";
        case CELESTE_ERR_NONFINITE_RESULT: return "ELBO value, gradient or Hessian contains Inf/NaNs";
        case CELESTE_ERR_HIP: return "HIP runtime error";
        case CELESTE_ERR_NO_DEVICE: return "no HIP device (the engine has no CPU fallback)";
        case CELESTE_ERR_ALLOC: return "allocation failed";
        case CELESTE_ERR_ABORTED: return "device group aborted: a member failed in front of a collective (destroy the group and create it again)";
        default: return "unknown status";
    }
}

// ---- spline prefilter (imaged_sources.jl:97-107; Interpolations BSpline(Cubic(Line())), OnGrid) ----
// 1-D: n samples -> n + 2 coefficients.  The two boundary rows c[0] - 2 c[1] + c[2] = 0 reduce the
// first/last interior equations to c[1] = d[0], c[n] = d[n-1]; the rest is a tridiagonal
// (1, 4, 1) / 6 system solved with the Thomas algorithm.
static void prefilter_line(int n, const double *d, int dstride, double *c, int cstride) {
    std::vector<double> cp(n), dp(n), x(n + 2);
    x[1] = d[0];
    x[n] = d[(size_t)(n - 1) * dstride];
    const int m = n - 2;  // unknowns x[2..n-1]
    if (m > 0) {
        // (x[q-1] + 4 x[q] + x[q+1]) = 6 d[q-1], q = 2..n-1
        for (int q = 0; q < m; ++q) {
            double rhs = 6.0 * d[(size_t)(q + 1) * dstride];
            if (q == 0) rhs -= x[1];
            if (q == m - 1) rhs -= x[n];
            const double lower = (q == 0) ? 0.0 : 1.0;
            const double denom = 4.0 - lower * (q ? cp[q - 1] : 0.0);
            cp[q] = 1.0 / denom;
            dp[q] = (rhs - lower * (q ? dp[q - 1] : 0.0)) / denom;
        }
        x[2 + m - 1] = dp[m - 1];
        for (int q = m - 2; q >= 0; --q) x[2 + q] = dp[q] - cp[q] * x[2 + q + 1];
    }
    x[0] = 2.0 * x[1] - x[2];
    x[n + 1] = 2.0 * x[n] - x[n - 1];
    for (int q = 0; q < n + 2; ++q) c[(size_t)q * cstride] = x[q];
}

extern "C" int celeste_spline_prefilter(const double *stamp51, double *coef53) try {
    if (!stamp51 || !coef53) return CELESTE_ERR_INVALID_ARG;
    const int n = CEL_STAMP, m = CEL_COEF;
    std::vector<double> g((size_t)n * n), tmp((size_t)m * n);
    double sum = 0;
    for (int k = 0; k < n * n; ++k) { g[k] = std::fmax(stamp51[k], 0.0) + 1e-6; sum += g[k]; }
    for (int k = 0; k < n * n; ++k) {
        const double x = g[k] / sum;
        g[k] = (1000 * x > 1) ? 1000 * x - 1 : std::log(1000 * x);  // softpluslike (fsm_util.jl:221)
    }
    for (int w = 0; w < n; ++w) prefilter_line(n, g.data() + (size_t)n * w, 1, tmp.data() + (size_t)m * w, 1);
    for (int h = 0; h < m; ++h) prefilter_line(n, tmp.data() + h, m, coef53 + h, m);
    return CELESTE_OK;
} ABI_CATCH

// The small tables of a context go up through ONE page-locked arena with asynchronous copies on the NULL stream (a synchronous
// hipMemcpy from pageable memory is 14 us, and a per-source context makes thirteen of them: 180 of its 300 us); celeste_ctx_create_on
// opens the arena (ArenaScope), the copies complete at its final wait for the NULL stream.  A table that does not fit (a whole
// field's patch list, 8765 PSF stamps) is copied synchronously as before.
struct UploadArena { char *base = nullptr; size_t cap = 0, used = 0; };
static thread_local UploadArena *tl_arena = nullptr;
struct ArenaScope {
    UploadArena a;
    explicit ArenaScope(size_t cap) {
        if (staging_alloc((void **)&a.base, cap) == hipSuccess) a.cap = cap;
        else { (void)hipGetLastError(); a.base = nullptr; }
        tl_arena = &a;
    }
    ~ArenaScope() {
        tl_arena = nullptr;
        if (a.base) { (void)hipStreamSynchronize(nullptr); staging_free(a.base); }   // (no copy out of the block is in flight when it goes back)
    }
    ArenaScope(const ArenaScope &) = delete;
    ArenaScope &operator=(const ArenaScope &) = delete;
};

template <class T>
static int dev_upload(T **dst, const T *src, size_t n) {
    *dst = nullptr;
    HIP_TRY(hipMalloc((void **)dst, std::max<size_t>(n, 1) * sizeof(T)));   // never a null table, even when empty
    if (src && n > 0) {
        const size_t bytes = n * sizeof(T);
        UploadArena *a = tl_arena;
        if (a && a->base && a->used + bytes <= a->cap) {
            memcpy(a->base + a->used, src, bytes);
            HIP_TRY(hipMemcpyAsync(*dst, a->base + a->used, bytes, hipMemcpyHostToDevice, nullptr));
            a->used += (bytes + 63) & ~(size_t)63;
        } else HIP_TRY(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
    }
    return CELESTE_OK;
}

static int select_device(int device) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) return CELESTE_ERR_NO_DEVICE;
    if (device < 0 || device >= count) return CELESTE_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(device));
    return CELESTE_OK;
}

extern "C" int celeste_images_create(int32_t n_images, const celeste_image_t *images, int device,
                                     celeste_images_t **out) try {
    if (!images || !out || n_images <= 0) return CELESTE_ERR_INVALID_ARG;
    *out = nullptr;
    int st = select_device(device);
    if (st != CELESTE_OK) return st;
    celeste_images *c = new (std::nothrow) celeste_images();
    if (!c) return CELESTE_ERR_ALLOC;
    c->device = device; c->N = n_images;
#define IMG_TRY(expr) do { int s__ = (expr); if (s__ != CELESTE_OK) { images_release(c); return s__; } } while (0)
    c->h_images.resize(c->N);
    for (int n = 0; n < c->N; ++n) {
        const celeste_image_t &im = images[n];
        if (im.H <= 0 || im.W <= 0 || im.band < 1 || im.band > 5 || !im.pixels || !im.sky || !im.nelec_per_nmgy) {
            images_release(c); return CELESTE_ERR_INVALID_ARG;
        }
        DevImage d; d.H = im.H; d.W = im.W; d.band = im.band; d.pad = 0;
        float *dp = nullptr, *ds = nullptr, *di = nullptr;
        IMG_TRY(dev_upload(&dp, im.pixels, (size_t)im.H * im.W)); c->plane_allocs.push_back(dp);
        IMG_TRY(dev_upload(&ds, im.sky, (size_t)im.H * im.W)); c->plane_allocs.push_back(ds);
        IMG_TRY(dev_upload(&di, im.nelec_per_nmgy, (size_t)im.H)); c->plane_allocs.push_back(di);
        d.pixels = dp; d.sky = ds; d.iota = di;
        double *dli = nullptr;
        IMG_TRY(dev_upload<double>(&dli, nullptr, (size_t)im.H)); c->plane_allocs.push_back(dli);
        hipLaunchKernelGGL(iota_kernel, dim3((unsigned)((im.H + 255) / 256)), dim3(256), 0, nullptr, di, im.H, dli);
        d.log_iota = dli;
        c->h_images[n] = d;
    }
    IMG_TRY(dev_upload(&c->d_images, c->h_images.data(), c->h_images.size()));
#undef IMG_TRY
    if (hipDeviceSynchronize() != hipSuccess) { images_release(c); return CELESTE_ERR_HIP; }
    *out = c;
    return CELESTE_OK;
} ABI_CATCH

extern "C" void celeste_images_destroy(celeste_images_t *images) { images_release(images); }

extern "C" int celeste_ctx_create(const celeste_problem_t *pr, int device, celeste_ctx_t **out) try {
    if (!pr || !out) return CELESTE_ERR_INVALID_ARG;
    *out = nullptr;
    if (pr->n_images <= 0 || !pr->images) return CELESTE_ERR_INVALID_ARG;
    celeste_images_t *im = nullptr;
    int st = celeste_images_create(pr->n_images, pr->images, device, &im);
    if (st != CELESTE_OK) return st;
    st = celeste_ctx_create_on(im, pr, out);
    images_release(im);   // the context holds its own reference
    return st;
} ABI_CATCH

extern "C" int celeste_ctx_create_on(celeste_images_t *imgs, const celeste_problem_t *pr, celeste_ctx_t **out) try {
    if (!imgs || !pr || !out) return CELESTE_ERR_INVALID_ARG;
    *out = nullptr;
    if (pr->n_images != imgs->N || pr->n_sources <= 0 || pr->psf_K <= 0 || pr->psf_K > CEL_MAXK ||
        !pr->patches || pr->n_stamps <= 0 || !pr->stamps || 14 * pr->psf_K > 62)
        return CELESTE_ERR_INVALID_ARG;
    const int device = imgs->device;
    int st = select_device(device);
    if (st != CELESTE_OK) return st;

    celeste_ctx *c = new (std::nothrow) celeste_ctx();
    if (!c) return CELESTE_ERR_ALLOC;
    ArenaScope upload_arena(256u << 10);    // (declared after `c`: a failed creation destroys the context first, then the arena waits)
    c->device = device;
    c->imgs = imgs; imgs->refs.fetch_add(1);
    c->d_images = imgs->d_images;
    c->N = pr->n_images; c->S = pr->n_sources; c->K = pr->psf_K; c->NC = 14 * pr->psf_K;
    c->n_stamps = pr->n_stamps;
#define CTX_TRY(expr) do { int s__ = (expr); if (s__ != CELESTE_OK) { celeste_ctx_destroy(c); return s__; } } while (0)
    // (The copy stream carries the device-to-host copies of finished parts while the next part computes on `stream`.  HIP maps
    // streams onto a handful of hardware queues, and which queue a stream gets depends on how many streams the process has
    // created before: one context in four or so sweeps 2000 sources through the host-pointer entry in 2.0 - 2.4 ms instead of
    // 1.35 -- its copies do not overlap its kernels.  Creating the copy stream at high priority only moves the bad draw to other
    // contexts: tools/gpu_group_stream_lottery.py, profiles/r06_stream_lottery.txt.)
    if (stream_acquire(device, &c->stream) != hipSuccess || stream_acquire(device, &c->copy_stream) != hipSuccess) {
        celeste_ctx_destroy(c); return CELESTE_ERR_HIP;
    }

    // patches + explicit bitmaps (dense [s * N + n] table, or the sparse list sorted by (source, image)).
    // Every per-(source, image) table of the context is indexed by VISIT: the v-th non-empty patch in (source, image)
    // order (h_vis_off / h_vis_img / h_vis_src).  When every source appears in (nearly) every image the visit lists
    // simply enumerate all S x N pairs (empty patches included), visit id = s * N + n, and the kernels skip the lists.
    std::vector<uint8_t> pool;
    const bool sparse = pr->n_patch_entries > 0;
    if (sparse && (!pr->patch_source || !pr->patch_image)) { celeste_ctx_destroy(c); return CELESTE_ERR_INVALID_ARG; }
    const size_t n_entries = sparse ? (size_t)pr->n_patch_entries : (size_t)c->S * c->N;
    std::vector<int64_t> ent_key; std::vector<DevPatch> ent;     // the non-empty patches, by key s * N + n
    std::vector<int32_t> n_vis((size_t)c->S, 0);
    int64_t prev = -1;
    for (size_t k = 0; k < n_entries; ++k) {
        size_t q = k;
        if (sparse) {
            const int32_t s = pr->patch_source[k], n = pr->patch_image[k];
            if (s < 0 || s >= c->S || n < 0 || n >= c->N || (int64_t)s * c->N + n <= prev) {
                celeste_ctx_destroy(c); return CELESTE_ERR_INVALID_ARG;
            }
            prev = (int64_t)s * c->N + n;
            q = (size_t)prev;
        }
        const celeste_patch_t &p = pr->patches[k];
        const DevImage &im = imgs->h_images[q % c->N];
        DevPatch d; memset(&d, 0, sizeof d);
        d.off_h = p.off_h; d.off_w = p.off_w; d.H2 = p.H2 < 0 ? 0 : p.H2; d.W2 = p.W2 < 0 ? 0 : p.W2;
        if (d.H2 > 0 && d.W2 > 0 &&
            (p.off_h < 0 || p.off_w < 0 || p.off_h + d.H2 > im.H || p.off_w + d.W2 > im.W)) {
            celeste_ctx_destroy(c); return CELESTE_ERR_INVALID_ARG;
        }
        if (p.stamp < 0 || p.stamp >= pr->n_stamps || !p.psf) { celeste_ctx_destroy(c); return CELESTE_ERR_INVALID_ARG; }
        if (d.H2 * d.W2 <= 0) continue;                          // an empty patch is no visit
        d.stamp = p.stamp;
        d.bitmap_off = -1;
        if (p.bitmap) {
            d.bitmap_off = (int64_t)pool.size();
            pool.insert(pool.end(), p.bitmap, p.bitmap + (size_t)d.H2 * d.W2);
        }
        memcpy(d.J, p.wcs_jacobian, sizeof d.J);
        memcpy(d.wc, p.world_center, sizeof d.wc);
        memcpy(d.pc, p.pixel_center, sizeof d.pc);
        memcpy(d.psf, p.psf, sizeof(double) * 6 * c->K);
        ent_key.push_back((int64_t)q); ent.push_back(d);
        n_vis[q / c->N]++;
        if (d.H2 * d.W2 > c->max_npx) c->max_npx = d.H2 * d.W2;
    }
    for (int s = 0; s < c->S; ++s) c->M = std::max(c->M, n_vis[s]);
    // single-field problems (every source in every image, or nearly: at least 3/4 of the S x N pairs exist): list all
    // N images for every source and let the kernels map (target, j) -> image j directly
    c->dense = (int64_t)ent.size() * 4 >= (int64_t)c->S * c->N * 3 && !getenv("CELESTE_FORCE_VISIT_LISTS");   // (the variable exists for testing)
    if (c->dense) c->M = c->N;
    c->h_vis_off.assign((size_t)c->S + 1, 0);
    if (c->dense) {
        DevPatch empty; memset(&empty, 0, sizeof empty);
        empty.bitmap_off = -1;
        c->h_patches.assign((size_t)c->S * c->N, empty);
        for (size_t k = 0; k < ent.size(); ++k) c->h_patches[(size_t)ent_key[k]] = ent[k];
        for (int s = 0; s < c->S; ++s) {
            for (int n = 0; n < c->N; ++n) { c->h_vis_img.push_back(n); c->h_vis_src.push_back(s); }
            c->h_vis_off[s + 1] = (int32_t)c->h_vis_img.size();
        }
    } else {
        c->h_patches.swap(ent);
        for (size_t k = 0; k < ent_key.size(); ++k) {
            c->h_vis_src.push_back((int32_t)(ent_key[k] / c->N)); c->h_vis_img.push_back((int32_t)(ent_key[k] % c->N));
            c->h_vis_off[(size_t)(ent_key[k] / c->N) + 1] = (int32_t)(k + 1);
        }
        for (int s = 0; s < c->S; ++s) c->h_vis_off[s + 1] = std::max(c->h_vis_off[s + 1], c->h_vis_off[s]);
    }
    c->V = (int64_t)c->h_vis_img.size();
    if (c->V > 0x7fffffffll / std::max(c->NC, 1)) { celeste_ctx_destroy(c); return CELESTE_ERR_INVALID_ARG; }
    if (c->max_npx >= (1 << 22)) { celeste_ctx_destroy(c); return CELESTE_ERR_INVALID_ARG; }   // (divmod_small: pixel indices of a patch in 22 bits)
    CTX_TRY(dev_upload(&c->d_patches, c->h_patches.data(), c->h_patches.size()));
    CTX_TRY(dev_upload(&c->d_bitmaps, pool.data(), pool.size()));

    // conditioned + prefiltered star splines
    {
        // (on the device: spline_prefilter_kernel -- the raw stamps go up, the coefficient tables never exist on the host)
        double *d_stamps = nullptr;
        CTX_TRY(dev_upload(&d_stamps, pr->stamps, (size_t)c->n_stamps * CEL_STAMP * CEL_STAMP));
        int st_c = dev_upload<double>(&c->d_coefs, nullptr, (size_t)c->n_stamps * CEL_COEF * CEL_COEF);
        if (st_c == CELESTE_OK) st_c = dev_upload<float>(&c->d_coefs_f, nullptr, (size_t)c->n_stamps * CEL_COEF * CEL_COEF);
        if (st_c == CELESTE_OK) {
            hipLaunchKernelGGL(spline_prefilter_kernel, dim3((unsigned)c->n_stamps), dim3(64), 0, nullptr, d_stamps, c->d_coefs, c->d_coefs_f);
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) st_c = CELESTE_ERR_HIP;
        }
        (void)hipFree(d_stamps);
        CTX_TRY(st_c);
    }

    // neighbour CSR
    c->h_nbr_off.assign((size_t)c->S + 1, 0);
    if (pr->nbr_offsets) {
        for (int s = 0; s <= c->S; ++s) c->h_nbr_off[s] = pr->nbr_offsets[s];
        const int64_t tot = c->h_nbr_off[c->S];
        if (tot < 0 || (tot > 0 && !pr->nbr_index)) { celeste_ctx_destroy(c); return CELESTE_ERR_INVALID_ARG; }
        c->h_nbr_idx.assign(pr->nbr_index, pr->nbr_index + tot);
        for (int32_t v : c->h_nbr_idx) if (v < 0 || v >= c->S) { celeste_ctx_destroy(c); return CELESTE_ERR_INVALID_ARG; }
    }
    CTX_TRY(dev_upload(&c->d_nbr_off, c->h_nbr_off.data(), c->h_nbr_off.size()));
    CTX_TRY(dev_upload(&c->d_nbr_idx, c->h_nbr_idx.data(), c->h_nbr_idx.size()));

    // prior (+ inverse covariances, parameter independent)
    {
        PriorDev pd;
        pd.p = pr->prior ? *pr->prior : DEFAULT_PRIOR;
        for (int i = 0; i < 2; ++i) for (int d = 0; d < 8; ++d) inv4_logdet(pd.p.color_cov[i][d], pd.inv_cov[i][d], &pd.logdet[i][d]);
        CTX_TRY(dev_upload(&c->d_prior, &pd, 1));
    }
    {
        // the galaxy prototypes and the exponential's table are constants of the library: written once per device and process
        // (two synchronous symbol copies + a launch per context were 35 us of a per-source context's 320)
        static std::mutex consts_mu;
        static bool consts_ready[16] = {};
        std::lock_guard<std::mutex> lk(consts_mu);
        if (device < 0 || device >= 16 || !consts_ready[device]) {
            double eta[16], nu[16];
            galaxy_prototypes(eta, nu);
            if (hipMemcpyToSymbol(HIP_SYMBOL(c_eta), eta, sizeof eta) != hipSuccess ||
                hipMemcpyToSymbol(HIP_SYMBOL(c_nu), nu, sizeof nu) != hipSuccess) {
                celeste_ctx_destroy(c); return CELESTE_ERR_HIP;
            }
            hipLaunchKernelGGL(exp_table_kernel, dim3(1), dim3(64), 0, nullptr);
            if (hipStreamSynchronize(nullptr) != hipSuccess) { celeste_ctx_destroy(c); return CELESTE_ERR_HIP; }
            if (device >= 0 && device < 16) consts_ready[device] = true;
        }
    }
    CTX_TRY(dev_upload<SrcImg>(&c->d_srcimg, nullptr, (size_t)c->V));
    CTX_TRY(dev_upload<Comp>(&c->d_comps, nullptr, (size_t)c->V * c->NC));
    CTX_TRY(dev_upload<SrcGeo>(&c->d_geo, nullptr, (size_t)c->S));
    {
        std::vector<int64_t> voff(c->h_patches.size());
        int64_t tot = 0;
        for (size_t q = 0; q < c->h_patches.size(); ++q) { voff[q] = tot; tot += (int64_t)c->h_patches[q].H2 * c->h_patches[q].W2; }
        CTX_TRY(dev_upload(&c->d_val_off, voff.data(), voff.size()));
        CTX_TRY(dev_upload<double2>(&c->d_val, nullptr, (size_t)tot));
        CTX_TRY(dev_upload<int32_t>(&c->d_needed, nullptr, (size_t)c->S));
        if (hipMemset(c->d_needed, 0, (size_t)c->S * sizeof(int32_t)) != hipSuccess) { celeste_ctx_destroy(c); return CELESTE_ERR_HIP; }
    }

    CTX_TRY(dev_upload(&c->d_vis_off, c->h_vis_off.data(), c->h_vis_off.size()));
    CTX_TRY(dev_upload(&c->d_vis_img, c->h_vis_img.data(), c->h_vis_img.size()));
    CTX_TRY(dev_upload(&c->d_vis_src, c->h_vis_src.data(), c->h_vis_src.size()));
    CTX_TRY(dev_upload<double>(&c->d_lg_sum, nullptr, (size_t)c->V));
    if (c->V > 0)
        hipLaunchKernelGGL(patch_lgamma_kernel, dim3((unsigned)c->V), dim3(256), 0, nullptr, c->d_images, c->d_patches,
                           c->d_vis_img, c->d_bitmaps, c->d_lg_sum);
    const char *env_chunk = getenv("CELESTE_CHUNK_PX");
    if (env_chunk && atoi(env_chunk) >= 64) c->chunk_px = (atoi(env_chunk) + 63) / 64 * 64;
    c->CH = c->max_npx > 0 ? (c->max_npx + c->chunk_px - 1) / c->chunk_px : 1;
    c->h_src_chunks.assign((size_t)c->S, 0);
    for (int s = 0; s < c->S; ++s) {
        for (int v = c->h_vis_off[s]; v < c->h_vis_off[s + 1]; ++v) {
            const DevPatch &q = c->h_patches[v];
            c->h_src_chunks[s] += (q.H2 * q.W2 + c->chunk_px - 1) / c->chunk_px;
        }
        c->max_src_chunks = std::max(c->max_src_chunks, c->h_src_chunks[s]);
    }
    // visit of (source, image), -1: none
    auto hv = [c](int s, int n) -> int64_t {
        if (c->dense) return (int64_t)s * c->N + n;
        const int32_t *b = c->h_vis_img.data() + c->h_vis_off[s], *e = c->h_vis_img.data() + c->h_vis_off[s + 1];
        const int32_t *it = std::lower_bound(b, e, n);
        return it != e && *it == n ? (int64_t)(it - c->h_vis_img.data()) : -1;
    };
    if (!c->dense) {
        // the visits of every source's neighbours, image by image: row j (= visit vis_off[s] + j) of source s holds the
        // visit of each of its K neighbours in that visit's image (-1: the neighbour is not in it), at nv_base[s] + j K
        std::vector<int64_t> base((size_t)c->S + 1, 0);
        for (int s = 0; s < c->S; ++s)
            base[s + 1] = base[s] + (int64_t)(c->h_vis_off[s + 1] - c->h_vis_off[s]) * (c->h_nbr_off[s + 1] - c->h_nbr_off[s]);
        std::vector<int32_t> nv((size_t)base[c->S]);
        for (int s = 0; s < c->S; ++s) {
            const int64_t K = c->h_nbr_off[s + 1] - c->h_nbr_off[s];
            for (int v = c->h_vis_off[s]; v < c->h_vis_off[s + 1]; ++v)
                for (int64_t q = 0; q < K; ++q)
                    nv[base[s] + (int64_t)(v - c->h_vis_off[s]) * K + q] = (int32_t)hv(c->h_nbr_idx[c->h_nbr_off[s] + q], c->h_vis_img[v]);
        }
        CTX_TRY(dev_upload(&c->d_nv_base, base.data(), base.size()));
        CTX_TRY(dev_upload(&c->d_nbr_vis, nv.data(), nv.size()));
        c->h_nv_base.swap(base);
    }
    {
        std::vector<int32_t> sorted(c->h_src_chunks);
        std::sort(sorted.begin(), sorted.end(), [](int32_t a, int32_t b) { return a > b; });
        c->h_top_chunks.assign((size_t)c->S + 1, 0);
        for (int s = 0; s < c->S; ++s) c->h_top_chunks[s + 1] = c->h_top_chunks[s] + sorted[s];
    }
    CTX_TRY(dev_upload<int32_t>(&c->d_work_total, nullptr, 1));
    {
        // work items of value_kernel: (link, image, chunk) with a non-empty overlap rectangle, longest first (by the
        // number of 64-pixel iterations the chunk takes) so that the kernel's tail is made of its shortest workgroups
        if (c->N > 0xffff) { celeste_ctx_destroy(c); return CELESTE_ERR_INVALID_ARG; }
        const int n_cls = c->chunk_px / 64;
        std::vector<std::vector<std::pair<int32_t, int32_t>>> by_len(n_cls);   // [n_cls - iterations]
        for (int s = 0; s < c->S; ++s)
            for (int64_t q = c->h_nbr_off[s]; q < c->h_nbr_off[s + 1]; ++q) {
                const int s2 = c->h_nbr_idx[q];
                for (int va = c->h_vis_off[s]; va < c->h_vis_off[s + 1]; ++va) {
                    const int n = c->h_vis_img[va];
                    const int64_t vb = hv(s2, n);
                    if (vb < 0) continue;
                    const DevPatch &a = c->h_patches[va], &b = c->h_patches[vb];
                    const int rh = std::min(a.off_h + a.H2, b.off_h + b.H2) - std::max(a.off_h, b.off_h);
                    const int rw = std::min(a.off_w + a.W2, b.off_w + b.W2 - 1) - std::max(a.off_w, b.off_w);
                    if (rh <= 0 || rw <= 0) continue;
                    const int npx = rh * rw, nch = (npx + c->chunk_px - 1) / c->chunk_px;
                    for (int ch = 0; ch < nch; ++ch) {
                        const int px = std::min(c->chunk_px, npx - ch * c->chunk_px);
                        by_len[n_cls - (px + 63) / 64].push_back({(int32_t)q, (int32_t)(n | (ch << 16))});
                    }
                }
            }
        std::vector<int32_t> link_src(c->h_nbr_idx.size());
        for (int s = 0; s < c->S; ++s)
            for (int64_t q = c->h_nbr_off[s]; q < c->h_nbr_off[s + 1]; ++q) link_src[q] = s;
        std::vector<int4> desc;
        for (auto &v : by_len)
            for (auto &e : v) {
                const int t = link_src[e.first], s2 = c->h_nbr_idx[e.first], n = e.second & 0xffff, ch = e.second >> 16;
                desc.push_back(make_int4((int)hv(s2, n), (int)hv(t, n), ch, t));
            }
        c->n_value_items = (int64_t)desc.size();
        c->h_vitem_tgt.resize(desc.size());
        c->h_vitem_link.resize(desc.size());
        for (size_t i = 0; i < desc.size(); ++i) { c->h_vitem_tgt[i] = desc[i].w; c->h_vitem_link[i] = {desc[i].x, desc[i].y}; }
        CTX_TRY(dev_upload(&c->d_value_items, desc.data(), desc.size()));
        // the same items grouped by target (joint dataflow launch: an entry renders its own source's neighbours)
        c->h_vitem_off.assign((size_t)c->S + 1, 0);
        for (auto &d : desc) c->h_vitem_off[(size_t)d.w + 1]++;
        for (int s = 0; s < c->S; ++s) c->h_vitem_off[s + 1] += c->h_vitem_off[s];
        {
            std::vector<int4> by_src(desc.size());
            std::vector<int32_t> fill(c->h_vitem_off.begin(), c->h_vitem_off.end() - 1);
            for (auto &d : desc) by_src[(size_t)fill[d.w]++] = d;
            CTX_TRY(dev_upload(&c->d_vitems_src, by_src.data(), by_src.size()));
            CTX_TRY(dev_upload(&c->d_vitem_off, c->h_vitem_off.data(), c->h_vitem_off.size()));
        }
        CTX_TRY(dev_upload<int32_t>(&c->d_prep_mark, nullptr, (size_t)c->S));
        if (hipMemset(c->d_prep_mark, 0, (size_t)c->S * sizeof(int32_t)) != hipSuccess) { celeste_ctx_destroy(c); return CELESTE_ERR_HIP; }
    }
    {
        c->h_tile_off.resize(c->h_patches.size());
        int64_t tot = 0;
        for (size_t q = 0; q < c->h_patches.size(); ++q) {
            c->h_tile_off[q] = tot;
            tot += ((int64_t)c->h_patches[q].H2 * c->h_patches[q].W2 + 63) / 64;
        }
        c->n_tiles = tot;
        if (const char *e = getenv("CELESTE_SUM_TILES")) if (atoi(e) > 0) c->sum_tiles = atoi(e);
        c->RCH = std::max(1, ((c->max_npx + 63) / 64 + c->sum_tiles - 1) / c->sum_tiles);
    }
    // (the timing events and the part events of the host-pointer sweep are created on first use: celeste_ctx_enable_timing,
    // celeste_elbo_eval_batch -- a per-source context that serves a few one-target calls never needs them)
    // the constant tables above were written on the NULL stream; the context's own streams do not wait for it
    if (hipStreamSynchronize(nullptr) != hipSuccess) { celeste_ctx_destroy(c); return CELESTE_ERR_HIP; }
#undef CTX_TRY
    *out = c;
    return CELESTE_OK;
} ABI_CATCH

// a prepared target list (celeste_abi.hip, "prepared target lists", builds and runs them; the context frees the ones left)
struct celeste_targets {
    celeste_ctx_t *ctx = nullptr;
    int32_t n = 0;
    int G = 1;
    int32_t *d_targets = nullptr;       // the list's own copy
    int32_t *d_work = nullptr, *d_work_total = nullptr, *d_rec_off = nullptr;
    int2 *d_items = nullptr;            // sparse contexts only
    int32_t *d_needed = nullptr;        // per source: LIST_STAMP for the targets, else 0
    int32_t *d_visits = nullptr;        // the visits whose tables the list reads: its targets' and their neighbours'
    int32_t *d_vitems = nullptr;        // the items of the context's d_value_items that belong to the list's targets
    // the same pixels, each once (value_union.h): what a sweep renders; d_vitems is the A/B switch's (CELESTE_NO_VALUE_UNION=1)
    int4 *d_uitems = nullptr;           // {neighbour's visit, first, count, trips}, longest first
    int32_t *d_upx = nullptr;           // per wanted pixel: its offset in the neighbour's patch buffer (4 B per pixel)
    int64_t n_visits = 0, n_vitems = 0, n_uitems = 0;
    int64_t n_records = 0;              // chunk records of a sweep (exact)
    int32_t n_work = 0;                 // work items of pixel_kernel (exact: its grid)
    // the same items, each described once (work_sequences.h): one workgroup of pixel_desc_kernel per descriptor;
    // CELESTE_NO_SEQUENCES=1 (the A/B switch) runs pixel_kernel over d_work instead
    WorkSeqDesc *d_desc = nullptr;      // one 64-byte descriptor per item that has pixels, most trips first
    int32_t n_desc = 0;
};
static const int32_t LIST_STAMP = 1;

static void targets_free(celeste_targets *t) {
    if (!t) return;
    void *ptrs[] = {t->d_targets, t->d_work, t->d_work_total, t->d_rec_off, t->d_items, t->d_needed, t->d_visits, t->d_vitems,
                    t->d_uitems, t->d_upx, t->d_desc};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    delete t;
}

extern "C" void celeste_ctx_destroy(celeste_ctx_t *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    for (struct celeste_targets *t : c->lists) targets_free(t);   // (the lists their owners have not destroyed)
    c->lists.clear();
    void *ptrs[] = {c->d_patches, c->d_coefs, c->d_coefs_f, c->d_bitmaps, c->d_nbr_off, c->d_nbr_idx, c->d_prior,
                    c->d_srcimg, c->d_comps, c->d_geo, c->d_val_off, c->d_val, c->d_needed, c->d_vis_off, c->d_vis_img, c->d_vis_src, c->d_value_items, c->d_vitems_src, c->d_vitem_off, c->d_prep_mark, c->d_rec_off, c->d_lg_sum, c->d_nv_base, c->d_nbr_vis, c->d_items, c->d_work, c->d_work_blk, c->d_work_total, c->d_tile_off, c->d_rec, c->d_acc_split, c->d_acc, c->d_vp, c->d_targets, c->d_v, c->d_d, c->d_h,
                    c->d_cnt, c->d_status};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    {
        auto &o = c->opt;
        void *optr[] = {o.d_vp, o.d_v, o.d_d, o.d_h, o.d_H, o.d_T, o.d_S, o.d_pos, o.d_targets, o.d_act[0], o.d_act[1], o.d_evt[0], o.d_evt[1],
                        o.d_count, o.d_st, o.d_state};
        for (void *q : optr) if (q) (void)hipFree(q);
        void *hptr[] = {o.h_vp, o.h_state, o.h_count};
        for (void *q : hptr) if (q) staging_free(q);
        for (int k = 0; k < celeste_ctx::OptBuffers::RING; ++k) if (o.ev[k]) (void)hipEventDestroy(o.ev[k]);
        auto &f = c->fused;
        void *fptr[] = {f.d_chunk_desc, f.d_tgt_rec, f.d_q_items, f.d_q_ctl, f.d_arrivals, f.d_saved};
        for (void *q : fptr) if (q) (void)hipFree(q);
        if (f.h_ctl) staging_free(f.h_ctl);
    }
    for (auto &sc : c->scratch) if (sc.p) (void)hipFree(sc.p);
    for (int i = 0; i < 5; ++i) if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
    for (int i = 0; i < celeste_ctx::MAX_PARTS; ++i) {
        if (c->part_done[i]) (void)hipEventDestroy(c->part_done[i]);
        if (c->part_copied[i]) (void)hipEventDestroy(c->part_copied[i]);
    }
    void *pins[] = {c->p_vp, c->p_targets, c->p_status, c->p_v, c->p_d, c->p_h, c->p_cnt, c->p_small_in, c->p_small_out};
    if (c->d_small_in) (void)hipFree(c->d_small_in);
    if (c->d_small_out) (void)hipFree(c->d_small_out);
    for (void *q : pins) if (q) staging_free(q);
    stream_retire(c->device, c->stream);
    stream_retire(c->device, c->copy_stream);
    images_release(c->imgs);
    delete c;
}
