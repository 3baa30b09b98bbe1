// engine_eval.h -- the engine's evaluation launcher: launch_eval (prep_kernel -> pixel_kernel -> lift_kernel, or
// eval_fused_kernel for small batches, on one HIP stream) over a context (engine_context.h), the cross blocks of several
// active sources (nbr_lists, launch_cross) and optim_config.  Everything here is static host code.  celeste_abi.hip (the
// engine) includes it under the optimiser's kernels; the blend library includes it alone, followed by engine_client.h, and so
// compiles neither the optimiser's step and fused kernels nor the host ABI nor the device groups.
#pragma once
#include "elbo_kernels.h"
#include "eval_fused.h"

// Evaluation batches of up to this many targets run eval_fused_kernel (launch_eval): a batch whose chunk records fit the
// chip in one round of 256-thread workgroups is latency-bound, and four wavefronts per record + the lift in the same
// launch shorten its critical path.  Beyond that the chip is full and pixel_kernel's one wavefront per record (its
// prologue paid once per four iterations, no turn-taking) has 2-3 x the throughput: a rank's N = 8 shard of the bench
// field (250 targets) takes 0.168 ms with pixel_kernel + lift_kernel, 0.287 ms with eval_fused_kernel (measured).
#define EVAL_FUSED_MAX 32

#include "engine_context.h"

// slot `k` of the context's scratch arena, at least `bytes` large (the stream is drained before a buffer moves)
template <class T>
static hipError_t scratch_get(celeste_ctx_t *c, int k, size_t bytes, T **out) {
    auto &s = c->scratch[k];
    if (bytes > s.cap) {
        hipError_t e = s.p ? hipStreamSynchronize(c->stream) : hipSuccess;     // (only a block in use has to be waited for)
        if (e != hipSuccess) return e;
        if (s.p) { (void)hipFree(s.p); s.p = nullptr; s.cap = 0; }
        e = hipMalloc(&s.p, std::max<size_t>(bytes, 256));
        if (e != hipSuccess) return e;
        s.cap = std::max<size_t>(bytes, 256);
    }
    *out = (T *)s.p;
    return hipSuccess;
}

static int launch_eval(celeste_ctx_t *c, const double *d_vp, int32_t n_targets, const int32_t *d_targets,
                       uint32_t flags, double *d_v, double *d_d, double *d_h, int64_t *d_counters, int32_t *d_status,
                       void *stream_, bool render_neighbors, const int32_t *d_active_rank = nullptr,
                       int64_t n_chunks = -1, bool tables_current = false, const int32_t *d_live = nullptr,
                       bool prep_all = false, bool render_only = false, const int32_t *d_h_pos = nullptr);

// the context's tables, as the fused kernels take them
static void fused_args_tables(celeste_ctx_t *c, FusedArgs &A) {
    A.images = c->d_images; A.patches = c->d_patches; A.coefs = c->d_coefs; A.bitmaps = c->d_bitmaps;
    A.nbr_off = c->d_nbr_off; A.nbr_idx = c->d_nbr_idx; A.val_off = c->d_val_off; A.val = c->d_val;
    A.nv_base = c->d_nv_base; A.nbr_vis = c->d_nbr_vis; A.items = c->dense ? nullptr : c->d_items; A.geo = c->d_geo;
    A.prior = c->d_prior; A.vis_off = c->d_vis_off; A.vis_img = c->d_vis_img; A.lg_sum = c->d_lg_sum; A.rec_off = c->d_rec_off;
    A.N = c->N; A.NC = c->NC; A.K = c->K; A.M = c->M; A.CH = c->CH; A.chunk_px = c->chunk_px;
    A.acc = c->d_acc;
    A.st = nullptr; A.Hstate = nullptr; A.Tstate = nullptr; A.Spec = nullptr; A.q_items = nullptr; A.q_ctl = nullptr; A.q_cap = 0; A.timeout_ticks = 0;
    A.j_R = 0; A.j_gshift = 0; A.j_dep = nullptr; A.j_succ_off = nullptr; A.j_succ = nullptr; A.j_vitem_off = nullptr;
    A.j_vitems = nullptr; A.j_render_arr = nullptr; A.j_saved = nullptr; A.j_pos = nullptr; A.j_srcimg = nullptr;
    A.j_comps = nullptr; A.j_geo = nullptr;
}

// per-target / per-record buffers of the fused kernels at capacity >= (n, rec)
static int fused_buffers(celeste_ctx_t *c, size_t n, size_t rec, hipStream_t stream) {
    auto &fb = c->fused;
    if (n > fb.cap_t) {
        if (fb.d_tgt_rec || fb.d_arrivals) HIP_TRY(hipStreamSynchronize(stream));   // (a buffer in use is about to be freed; nothing to wait for the first time)
        void **ps[] = {(void **)&fb.d_tgt_rec, (void **)&fb.d_arrivals};
        for (void **q : ps) if (*q) { (void)hipFree(*q); *q = nullptr; }
        fb.cap_t = 0;
        HIP_TRY(hipMalloc((void **)&fb.d_tgt_rec, n * sizeof(int2)));
        HIP_TRY(hipMalloc((void **)&fb.d_arrivals, n * sizeof(int32_t)));
        fb.cap_t = n;
        fb.arrivals_dirty = true;
    }
    if (rec > fb.cap_rec) {
        if (fb.d_chunk_desc) { HIP_TRY(hipStreamSynchronize(stream)); (void)hipFree(fb.d_chunk_desc); fb.d_chunk_desc = nullptr; }
        fb.cap_rec = 0;
        HIP_TRY(hipMalloc((void **)&fb.d_chunk_desc, std::max<size_t>(rec, 1) * 2 * sizeof(int4)));
        fb.cap_rec = rec;
    }
    return CELESTE_OK;
}

#define VALUE_WIDE_MAX 768     // batches up to this size render the neighbours' light with four wavefronts per item
// small Hessian-mode fp64 batches run eval_fused_kernel instead of pixel_kernel + lift_kernel; `plain`: none of the
// launch's optional arguments (active ranks, live count, Hessian slots, render-only) is in use
static bool want_eval_fused(uint32_t flags, int32_t n_targets, bool plain, const double *d_d, const double *d_h) {
    const bool can = plain && (flags & CELESTE_FLAG_HESS) && !(flags & (CELESTE_FLAG_FP32 | CELESTE_FLAG_SPLIT)) && d_d && d_h;
    bool eval_fused = can && n_targets <= EVAL_FUSED_MAX;
    if (const char *e = getenv("CELESTE_EVAL_FUSED")) {
        if (atoi(e) == 0) eval_fused = false;
        else if (atoi(e) == 1) eval_fused = can;
    }
    return eval_fused;
}
// a workgroup of pixel_kernel handles a group of up to G consecutive chunks of a patch (results do not depend on G, see
// visit_chunks): 4 for large sweeps, 1 for small batches whose critical path is one patch
// (measured, round 5: the 2000-target sweep of the bench field 0.499 ms with 2, 0.503 with 1, 0.502 with 3, 0.512 with 4;
// config 5's 30 000 targets 5.31 ms with 4, 5.45 with 2, 5.30 with 8; a 1000-target shard 0.287 ms with 2, 0.315 with 4)
static int chunk_group(int32_t n_targets) {
    int G = n_targets >= 8192 ? 4 : n_targets >= 768 ? 2 : 1;
    if (const char *e = getenv("CELESTE_CHUNK_GROUP")) if (atoi(e) >= 1 && atoi(e) <= 16) G = atoi(e);
    return G;
}
// render_neighbors = false keeps the neighbours' pre-rendered light of an earlier call (frozen neighbours
// during an optimisation, ParallelRun.jl:474-488)
static int launch_eval(celeste_ctx_t *c, const double *d_vp, int32_t n_targets, const int32_t *d_targets,
                       uint32_t flags, double *d_v, double *d_d, double *d_h, int64_t *d_counters, int32_t *d_status,
                       void *stream_, bool render_neighbors, const int32_t *d_active_rank, int64_t n_chunks,
                       bool tables_current, const int32_t *d_live, bool prep_all, bool render_only, const int32_t *d_h_pos) {
    // d_h_pos (device, optional): target i's Hessian goes to slot d_h_pos[i] of d_h instead of slot i (celeste_group_*: a
    // member's shard written to its places in the caller's array)
    // render_only: the batch's bookkeeping (SrcGeo, visit items, record offsets, marks), the per-image tables of the
    // targets and their neighbours and the neighbours' pre-rendered light -- everything the optimiser needs before its
    // first evaluation -- and no evaluation
    // prep_all: the per-(source, image) tables of EVERY source are filled (the first part of a host batch does it for
    // the parts that follow, which pass tables_current); else only those of the targets and their neighbours
    // d_live (device, optional): the number of leading entries of d_targets that are live; n_targets is then an upper
    // bound known to the host (the optimiser loop runs ahead of the device)
    // tables_current: the per-(source, image) tables were filled from this very vp by an earlier launch of the same
    // call (parts of one host batch): only the neighbours of this part's targets are rendered
    if (!c || !d_vp || !d_targets || !d_v || !d_status || n_targets < 0) return CELESTE_ERR_INVALID_ARG;
    if ((flags & CELESTE_FLAG_HESS) && !d_h) return CELESTE_ERR_INVALID_ARG;
    if ((flags & (CELESTE_FLAG_GRAD | CELESTE_FLAG_HESS)) && !d_d) return CELESTE_ERR_INVALID_ARG;
    if (n_targets == 0) return CELESTE_OK;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    // Pixel chunks of THIS launch.  Single precision: 512 pixels, i.e. four 128-pixel trips of pixel_iter_px2 per record
    // instead of two -- half the records to zero, fold, store and lift (measured on config 5: 5.31 -> 5.20 ms; the fp64 kernel
    // loses 3-5 % with 512, so the context's own chunk stays 256).  Everything that depends on the chunk size is per launch
    // (work list, record offsets, pixel and lift kernels); the host's chunk counts (256-pixel chunks) remain upper bounds.
    const bool big_chunks = (flags & CELESTE_FLAG_FP32) && !(flags & CELESTE_FLAG_SPLIT) && !d_active_rank && c->chunk_px == 256 &&
                            !getenv("CELESTE_FP32_CHUNK_256");
    const int chunk_px = big_chunks ? 512 : c->chunk_px;
    const int CH = big_chunks ? std::max(1, (c->max_npx + chunk_px - 1) / chunk_px) : c->CH;
    // one 68-double record per chunk that exists (rec_off = prefix sum of the visits' chunk counts): exactly n_chunks
    // when the caller knows its targets on the host, else at most n_targets x the chunk count of the richest source
    const size_t rec_cap = n_chunks >= 0 ? (size_t)n_chunks
                                         : std::min((size_t)n_targets * c->max_src_chunks, (size_t)n_targets * c->M * c->CH);
    const size_t need = std::max<size_t>(rec_cap, 1) * ACC_N;
    if ((size_t)n_targets * c->M > c->rec_off_cap) {
        if (c->d_rec_off) { HIP_TRY(hipStreamSynchronize(stream)); HIP_TRY(hipFree(c->d_rec_off)); c->d_rec_off = nullptr; }
        HIP_TRY(hipMalloc((void **)&c->d_rec_off, (size_t)n_targets * c->M * sizeof(int32_t)));
        c->rec_off_cap = (size_t)n_targets * c->M;
    }
    if (need > c->acc_cap) {
        if (c->d_acc) { HIP_TRY(hipStreamSynchronize(stream)); HIP_TRY(hipFree(c->d_acc)); c->d_acc = nullptr; }
        HIP_TRY(hipMalloc((void **)&c->d_acc, need * sizeof(double)));
        c->acc_cap = need;
    }
    if (!c->dense && (size_t)n_targets * c->M > c->items_cap) {
        if (c->d_items) { HIP_TRY(hipStreamSynchronize(stream)); HIP_TRY(hipFree(c->d_items)); c->d_items = nullptr; }
        HIP_TRY(hipMalloc((void **)&c->d_items, (size_t)n_targets * c->M * sizeof(int2)));
        c->items_cap = (size_t)n_targets * c->M;
    }
    // work list: n_chunks = number of chunks of the batch when the caller knows its targets on the host, else bounded
    // by the largest source (workgroups past the device-side total exit on one scalar load)
    const int n_visits = n_targets * c->M;
    const int n_wblk = (n_visits + WORK_NT - 1) / WORK_NT;
    // n_chunks: exact when the caller knows its targets on the host; else the chunks of the n_targets chunk-richest
    // sources (a bound for distinct targets; with repeated targets the list can be longer: the buffer is sized for
    // that, the pixel kernel's stride loop covers it)
    const size_t work_need = (size_t)(n_chunks >= 0 ? n_chunks : (int64_t)n_targets * c->max_src_chunks);
    const size_t grid_need = (size_t)(n_chunks >= 0 ? n_chunks
                                      : n_targets <= c->S ? c->h_top_chunks[n_targets] : (int64_t)n_targets * c->max_src_chunks);
    if ((size_t)n_targets * c->M * c->CH > 0x7fffffffull) return CELESTE_ERR_INVALID_ARG;
    if (work_need > c->work_cap) {
        if (c->d_work) { HIP_TRY(hipStreamSynchronize(stream)); HIP_TRY(hipFree(c->d_work)); c->d_work = nullptr; }
        HIP_TRY(hipMalloc((void **)&c->d_work, std::max<size_t>(work_need, 1) * sizeof(int32_t)));
        c->work_cap = work_need;
    }
    int G = chunk_group(n_targets);
    // small Hessian-mode fp64 batches: eval_fused_kernel instead of pixel_kernel + lift_kernel (below)
    const bool eval_fused = want_eval_fused(flags, n_targets, !render_only && !d_active_rank && !d_live && !d_h_pos, d_d, d_h);
    if (eval_fused) G = 1;        // one record per work item: the work-list total is the batch's number of records
    const int n_classes = WORK_CLASSES;   // work-list classes: full groups, then the patches' last groups by length
    if ((size_t)n_wblk * (n_classes + 1) > c->work_blk_cap) {   // + the row of chunk counts (rec_off)
        if (c->d_work_blk) { HIP_TRY(hipStreamSynchronize(stream)); HIP_TRY(hipFree(c->d_work_blk)); c->d_work_blk = nullptr; }
        HIP_TRY(hipMalloc((void **)&c->d_work_blk, (size_t)n_wblk * (n_classes + 1) * sizeof(int32_t)));
        c->work_blk_cap = (size_t)n_wblk * (n_classes + 1);
    }
    const bool derivs = (flags & (CELESTE_FLAG_GRAD | CELESTE_FLAG_HESS)) != 0;
    const bool split = (flags & CELESTE_FLAG_SPLIT) != 0;
    if (split) {
        if (!(flags & CELESTE_FLAG_HESS)) return CELESTE_ERR_INVALID_ARG;
        if (!c->d_rec) {
            HIP_TRY(hipStreamSynchronize(stream));
            if (dev_upload(&c->d_tile_off, c->h_tile_off.data(), c->h_tile_off.size()) != CELESTE_OK) return CELESTE_ERR_HIP;
            if (hipMalloc((void **)&c->d_rec, (size_t)std::max<int64_t>(c->n_tiles, 1) * ACC_N * 64 * sizeof(double)) != hipSuccess)
                return CELESTE_ERR_ALLOC;
        }
        const size_t need_s = (size_t)n_targets * c->M * c->RCH * ACC_N;
        if (need_s > c->acc_split_cap) {
            if (c->d_acc_split) { HIP_TRY(hipStreamSynchronize(stream)); HIP_TRY(hipFree(c->d_acc_split)); c->d_acc_split = nullptr; }
            HIP_TRY(hipMalloc((void **)&c->d_acc_split, need_s * sizeof(double)));
            c->acc_split_cap = need_s;
        }
    }
    if (c->timing) HIP_TRY(hipEventRecord(c->ev[0], stream));
    if (render_neighbors && ++c->stamp == 0x7fffffff) {   // (the marks are batch stamps; 0 = never a target)
        HIP_TRY(hipMemsetAsync(c->d_needed, 0, (size_t)c->S * sizeof(int32_t), stream));
        c->stamp = 1;
    }
    // SrcGeo: of every source when the neighbours are (re)rendered, else of the targets only (setup_thread)
    const int geo_S = render_neighbors ? c->S : -1;
    const size_t setup_threads = std::max<size_t>(render_neighbors ? (size_t)c->S : 0, (size_t)n_targets * (c->dense ? 1 : c->M));
    // the sources whose tables this launch fills are marked by the setup kernel (targets + neighbours)
    int32_t *const prep_mark = render_neighbors && !tables_current && !prep_all ? c->d_prep_mark : nullptr;
    bool prep_fused = false;
    bool records_described = false;   // eval_fused: block 0 of the one-launch list has written chunk_desc / tgt_rec (no fused_setup_kernel)
    if (eval_fused) { int stb = fused_buffers(c, (size_t)n_targets, rec_cap, stream); if (stb != CELESTE_OK) return stb; }
    if (n_visits <= WORK1_MAX_VISITS && !getenv("CELESTE_PARALLEL_WORKLIST")) {
        const unsigned setup_blocks = (unsigned)((setup_threads + WORK1_SETUP - 1) / WORK1_SETUP);
        // neighbours frozen: the targets' tables are filled by extra blocks of this launch (one launch less per iteration)
        prep_fused = !render_neighbors && !getenv("CELESTE_NO_FUSED_PREP");
        // neighbours (re)rendered: every visit's tables by this launch as well when the context has few of them (a one-field
        // context: 10 000 visits, 15 us of work that hides under the list builder's block) -- a small batch's chain is one
        // launch shorter
        // (a handful of targets touch a handful of sources: there the marked tables of prep_kernel are the cheaper route)
        // (... unless the context is tiny -- a per-source context, a source and its neighbours: ten visits -- where filling
        // every table inside this launch beats a launch of its own whatever the batch: a one-target call 71 -> 67 us)
        const bool prep_all_here = render_neighbors && !tables_current && c->V > 0 && c->V <= WORK1_PREP_ALL_MAX &&
                                   (n_targets >= WORK1_PREP_ALL_MIN_TARGETS || c->V <= WORK1_PREP_ALL_TINY) && !getenv("CELESTE_NO_FUSED_PREP");
        const int prep_n = prep_all_here ? (int)c->V : n_visits;
        if (prep_all_here) prep_fused = true;
        const unsigned prep_blocks = prep_fused ? (unsigned)((prep_n + WORK1_NT / 64 - 1) / (WORK1_NT / 64)) : 0u;
        const bool records_described_here = eval_fused && c->dense && !d_live && !getenv("CELESTE_NO_FUSED_DESCRIBE");
        hipLaunchKernelGGL(setup_worklist_kernel, dim3(1 + setup_blocks + prep_blocks), dim3(WORK1_NT),
                           0, stream, d_vp, geo_S, c->d_geo, d_targets, n_targets, c->d_vis_off, c->d_vis_img, c->M,
                           c->dense ? nullptr : c->d_items, render_neighbors ? c->d_needed : nullptr, c->stamp, c->d_patches,
                           c->N, CH, chunk_px, G, (int)c->dense, c->d_work, c->d_work_total, d_live, prep_mark,
                           c->d_nbr_off, c->d_nbr_idx, c->d_rec_off, (int)setup_blocks, c->d_images, c->K, c->d_srcimg,
                           c->d_comps, prep_all_here ? (int)c->V : 0, c->d_vis_src,
                           records_described_here ? c->fused.d_chunk_desc : nullptr, records_described_here ? c->fused.d_tgt_rec : nullptr,
                           c->chunk_px);
        records_described = records_described_here;
    } else {
        // (the work-list kernels depend on nothing setup / prep / value produce; built on a second stream beside them and
        // joined in front of the pixel kernel they measured no faster -- 0.6519 ms per sweep of the bench field either way --
        // and a stream more per context is not free: round 5, removed)
        hipLaunchKernelGGL(setup_kernel, dim3((unsigned)((setup_threads + 63) / 64)), dim3(64), 0, stream, d_vp, geo_S,
                           c->d_geo, d_targets, n_targets, c->d_vis_off, c->d_vis_img, c->M, c->dense ? nullptr : c->d_items,
                           render_neighbors ? c->d_needed : nullptr, c->stamp, prep_mark, c->d_nbr_off, c->d_nbr_idx, d_live);
        hipLaunchKernelGGL(work_count_kernel, dim3(n_wblk), dim3(WORK_NT), 0, stream, d_targets, n_visits, c->d_patches,
                           c->d_vis_off, c->d_vis_img, c->N, c->M, chunk_px, G, (int)c->dense, c->d_work_blk, d_live);
        hipLaunchKernelGGL(work_scan_kernel, dim3(1), dim3(1024), 0, stream, c->d_work_blk, n_wblk * (n_classes + 1),
                           c->d_work_total, n_wblk * n_classes);
        hipLaunchKernelGGL(work_fill_kernel, dim3(n_wblk), dim3(WORK_NT), 0, stream, d_targets, n_visits, c->d_patches,
                           c->d_vis_off, c->d_vis_img, c->N, c->M, CH, chunk_px, G, (int)c->dense, c->d_work_blk, c->d_work, d_live,
                           c->d_rec_off);
    }
    // per-(source, image) constants: of every source when the neighbours are (re)rendered, else of the targets only
    if (render_neighbors) {
        if (c->V > 0 && !tables_current && !prep_fused)
            hipLaunchKernelGGL(prep_kernel, dim3((unsigned)c->V), dim3(64), 0, stream, d_vp, c->d_images, c->d_patches,
                               c->d_vis_src, c->d_vis_img, c->N, c->K, c->d_srcimg, c->d_comps, nullptr, c->d_vis_off, c->M,
                               (int)c->dense, nullptr, prep_mark, c->stamp);
    } else if (!prep_fused) {
        hipLaunchKernelGGL(prep_kernel, dim3((unsigned)std::max(n_visits, 1)), dim3(64), 0, stream, d_vp, c->d_images,
                           c->d_patches, c->d_vis_src, c->d_vis_img, c->N, c->K, c->d_srcimg, c->d_comps, d_targets,
                           c->d_vis_off, c->M, (int)c->dense, d_live, nullptr, 0);
    }
    if (render_neighbors) {
    if (c->n_value_items > 0)
    {
        // (single-precision mode: the neighbours' densities in fp32 too, their moments in fp64)
        // small batches leave the chip mostly idle: an item's four 64-pixel iterations then run side by side on four
        // wavefronts (same values; chunk_px = 256 is what the items were cut for)
        const bool wide_items = n_targets <= VALUE_WIDE_MAX && c->chunk_px == 256 && !getenv("CELESTE_NO_WIDE_VALUE");
#define LAUNCH_VALUE(R, WAVES)                                                                                              \
        hipLaunchKernelGGL((value_kernel<R, WAVES>), dim3((unsigned)c->n_value_items), dim3(64 * WAVES), 0, stream,       \
                           c->d_patches, c->d_coefs, c->d_srcimg, c->d_comps, c->d_needed, c->stamp, c->d_val_off,          \
                           c->d_value_items, c->NC, c->chunk_px, c->d_val, c->d_coefs_f)
        // (single precision: value_pixels_f2 for every batch size -- two wavefronts x 128 pixels when wide -- so that a
        // target's fp32 result does not depend on the size of the batch it is in)
        if (flags & CELESTE_FLAG_FP32) { if (wide_items) LAUNCH_VALUE(float, 2); else LAUNCH_VALUE(float, 1); }
        else { if (wide_items) LAUNCH_VALUE(double, 4); else LAUNCH_VALUE(double, 1); }
#undef LAUNCH_VALUE
    }
    }
    if (render_only) { HIP_TRY(hipGetLastError()); return CELESTE_OK; }
    if (c->timing) HIP_TRY(hipEventRecord(c->ev[1], stream));
    if (eval_fused) {
        // small batch: one workgroup per chunk record (four wavefronts, one 64-pixel iteration each), the lift by the
        // workgroup that completes a target -- eval_fused_kernel; same records, same results as pixel_kernel + lift_kernel
        auto &fb = c->fused;
        if (fb.arrivals_dirty) {
            HIP_TRY(hipMemsetAsync(fb.d_arrivals, 0, fb.cap_t * sizeof(int32_t), stream));
            fb.arrivals_dirty = false;
        }
        if (!records_described)
            hipLaunchKernelGGL(fused_setup_kernel, dim3((unsigned)((n_targets + 63) / 64)), dim3(64), 0, stream, d_targets, n_targets,
                               c->d_patches, c->d_vis_off, c->dense ? nullptr : c->d_items, c->N, c->M, c->chunk_px, c->d_rec_off,
                               fb.d_chunk_desc, fb.d_tgt_rec, (int32_t *)nullptr, (int32_t *)nullptr);
        FusedArgs A;
        fused_args_tables(c, A);
        A.targets = d_targets; A.n_targets = n_targets; A.vp = const_cast<double *>(d_vp);
        A.chunk_desc = fb.d_chunk_desc; A.tgt_rec = fb.d_tgt_rec; A.arrivals = fb.d_arrivals; A.flags = flags;
        memset(&A.op, 0, sizeof A.op);
        // no stride loop in this kernel: the grid must cover every record.  h_top_chunks bounds DISTINCT targets only, and
        // the device-pointer entry allows repeats -- there the bound is n_targets x the chunk-richest source
        const unsigned rec_bound = (unsigned)std::max<size_t>(n_chunks >= 0 ? grid_need : work_need, 1);
        hipLaunchKernelGGL(eval_fused_kernel, dim3(rec_bound + (unsigned)n_targets), dim3(FUSED_NT), 0, stream, A, c->d_srcimg,
                           c->d_comps, c->d_work_total, (int)rec_bound, d_v, d_d, d_h, d_counters, d_status);
        if (c->timing) { HIP_TRY(hipEventRecord(c->ev[2], stream)); HIP_TRY(hipEventRecord(c->ev[3], stream)); c->ev_valid = 1; c->ev_split = 0; }
        HIP_TRY(hipGetLastError());
        return CELESTE_OK;
    }
    const dim3 grid((unsigned)std::max<size_t>(grid_need, 1));
#define PIXEL_ARGS                                                                                                \
    c->d_images, c->d_patches, c->d_coefs, c->d_bitmaps, c->d_srcimg, c->d_comps, c->d_nbr_off, c->d_nbr_idx,       \
    c->d_val_off, c->d_val, d_targets, c->N, c->NC, CH, chunk_px, G, c->d_acc, c->d_tile_off, c->d_rec, \
    d_active_rank, c->d_items, c->M, c->d_work, c->d_work_total, c->d_nv_base, c->d_nbr_vis, c->d_rec_off, c->d_coefs_f
#define LAUNCH_PIXEL_T(MODE, R) hipLaunchKernelGGL((pixel_kernel<MODE, R>), grid, dim3(64), 0, stream, PIXEL_ARGS)
#define LAUNCH_PIXEL_M(MODE) hipLaunchKernelGGL((pixel_kernel<MODE, double, true>), grid, dim3(64), 0, stream, PIXEL_ARGS)
#define LAUNCH_PIXEL(MODE) do { if (flags & CELESTE_FLAG_FP32) LAUNCH_PIXEL_T(MODE, float); else LAUNCH_PIXEL_T(MODE, double); } while (0)
    if (d_active_rank) {   // several active sources: fp64, fused
        if (flags & CELESTE_FLAG_HESS) LAUNCH_PIXEL_M(2);
        else if (derivs) LAUNCH_PIXEL_M(1);
        else LAUNCH_PIXEL_M(0);
    }
    else if (split) LAUNCH_PIXEL(3);
    else if (flags & CELESTE_FLAG_HESS) LAUNCH_PIXEL(2);
    else if (derivs) LAUNCH_PIXEL(1);
    else LAUNCH_PIXEL_T(0, double);
#undef LAUNCH_PIXEL
#undef LAUNCH_PIXEL_M
#undef PIXEL_ARGS
#undef LAUNCH_PIXEL_T
    if (c->timing) HIP_TRY(hipEventRecord(c->ev[2], stream));
    c->ev_split = 0;
    // every gradient / Hessian entry is owned by one thread whatever the block size: 512 threads halve the latency of
    // a batch that leaves the chip mostly idle anyway; 256 keep 8 workgroups per CU for a 2000-target sweep
    const int lift_nt = n_targets <= 1024 ? 512 : 256;
    // (beyond one round of 8 workgroups per CU the spill-free instantiation: see lift_kernel; CELESTE_LIFT_WAVES=8 / 7 forces one)
    bool lift7 = n_targets > 4096;
    if (const char *e = getenv("CELESTE_LIFT_WAVES")) lift7 = atoi(e) == 7;
#define LAUNCH_LIFT(...) do { if (lift7) hipLaunchKernelGGL(lift_kernel<7>, __VA_ARGS__); else hipLaunchKernelGGL(lift_kernel<8>, __VA_ARGS__); } while (0)
    if (split) {
        // per-patch sums of the records, then the lift reads one record per (target, image): CH = 1
        // its own (part, patch) grid, part index slowest: streaming order matters more to this kernel than the idle
        // workgroups do (run over the pixel kernel's longest-first work list it lost 5 %)
        hipLaunchKernelGGL(record_sum_kernel, dim3((unsigned)((size_t)n_targets * c->M * c->RCH)), dim3(RSUM_NT), 0,
                           stream, c->d_patches, d_targets, c->d_tile_off, reinterpret_cast<const double2 *>(c->d_rec),
                           c->d_items, c->N, c->M, c->RCH, c->sum_tiles, c->d_acc_split, nullptr, c->d_work_total);
        if (c->timing) { HIP_TRY(hipEventRecord(c->ev[4], stream)); c->ev_split = 1; }
        LAUNCH_LIFT(dim3(n_targets), dim3(lift_nt), 0, stream, d_vp, c->d_images, c->d_patches, c->d_geo,
                           c->d_nbr_off, c->d_nbr_idx, d_targets, c->d_acc_split, c->d_prior, c->d_vis_off, c->d_vis_img, c->N, c->M,
                           c->RCH, c->sum_tiles * 64, flags,
                           d_v, d_d, d_h, d_counters, d_status, d_live, d_active_rank ? nullptr : c->d_lg_sum, nullptr, d_h_pos);
    } else
    LAUNCH_LIFT(dim3(n_targets), dim3(lift_nt), 0, stream, d_vp, c->d_images, c->d_patches, c->d_geo,
                       c->d_nbr_off, c->d_nbr_idx, d_targets, c->d_acc, c->d_prior, c->d_vis_off, c->d_vis_img, c->N, c->M, CH,
                       chunk_px, flags,
                       d_v, d_d, d_h, d_counters, d_status, d_live, d_active_rank ? nullptr : c->d_lg_sum, c->d_rec_off, d_h_pos);
#undef LAUNCH_LIFT
    if (c->timing) { HIP_TRY(hipEventRecord(c->ev[3], stream)); c->ev_valid = 1; }
    HIP_TRY(hipGetLastError());
    return CELESTE_OK;
}

// ---- cross blocks of several active sources (celeste_elbo_eval_multi, the blend library) ----------------------------------
// does source s list source t as a neighbour?  (of a pair of active sources that light common pixels, the one that lists the
// other comes first)
static bool nbr_lists(const celeste_ctx_t *c, int s, int t) {
    for (int64_t q = c->h_nbr_off[s]; q < c->h_nbr_off[s + 1]; ++q) if (c->h_nbr_idx[q] == t) return true;
    return false;
}

// the cross blocks of np pairs (d_pa[k], d_pb[k]) at the table d_vp: per pair and image the record of the common pixels
// (d_rec, np x N x ZV x ZV), then d2 / d theta_a d theta_b into d_x (np x LIFT_NP x LIFT_NP)
static void launch_cross(celeste_ctx_t *c, const double *d_vp, size_t np, const int32_t *d_pa, const int32_t *d_pb,
                         double *d_rec, double *d_x, hipStream_t stream) {
    hipLaunchKernelGGL(cross_kernel, dim3((unsigned)(np * c->N)), dim3(64), 0, stream, c->d_images, c->d_patches,
                       c->d_coefs, c->d_bitmaps, c->d_srcimg, c->d_comps, c->d_nbr_off, c->d_nbr_idx, c->d_val_off,
                       c->d_val, d_pa, d_pb, c->N, c->NC, d_rec, c->d_vis_off, c->d_vis_img, (int)c->dense);
    hipLaunchKernelGGL(cross_lift_kernel, dim3((unsigned)np), dim3(256), 0, stream, d_vp, c->d_images, c->d_patches,
                       c->d_geo, d_pa, d_pb, d_rec, c->N, d_x, c->d_vis_off, c->d_vis_img, (int)c->dense);
}

// a caller's optimiser settings (nullptr: the defaults), checked, as the kernels' OptParams and the flags of maximize!'s evaluations
static int optim_config(const celeste_optim_config_t *cfg_in, OptParams *op, uint32_t *flags) {
    celeste_optim_config_t cfg = {1e-4, 1.0, 50, 1, 1e-7, 1e-6, 1e-8, 1.0, 1e9, 0, 0};
    if (cfg_in) cfg = *cfg_in;
    if (!(cfg.loc_width > 0) || !(cfg.loc_scale > 0) || cfg.max_iters < 0 || cfg.tr_secular_iters < 0)
        return CELESTE_ERR_INVALID_ARG;
    op->loc_width = cfg.loc_width; op->loc_scale = cfg.loc_scale; op->xtol_abs = cfg.xtol_abs; op->ftol_rel = cfg.ftol_rel;
    op->gtol = cfg.gtol; op->initial_delta = cfg.initial_delta; op->delta_hat = cfg.delta_hat; op->max_iters = cfg.max_iters;
    op->secular_iters = cfg.tr_secular_iters > 0 ? cfg.tr_secular_iters : 20;
    // CELESTE_TR_SOLVER=eig: full eigen-decomposition for every sub-problem (cross-check of the default
    // tridiagonal-space solve)
    const char *env_solver = getenv("CELESTE_TR_SOLVER");
    op->solver = (env_solver && strcmp(env_solver, "eig") == 0) ? 1 : 0;
    op->pad = 0;
    *flags = CELESTE_FLAG_GRAD | CELESTE_FLAG_HESS | (cfg.include_kl ? CELESTE_FLAG_KL : 0);
    return CELESTE_OK;
}
