// celeste_abi.hip -- host side of the C ABI declared in include/celeste_mi355x.h.
//
// The context (engine_context.h) owns the device copies of the problem (images, patches, spline coefficients,
// neighbour graph); the evaluation launcher (engine_eval.h: launch_eval) launches prep_kernel -> pixel_kernel ->
// lift_kernel on one HIP stream; this file holds the entry points over them: host batches, prepared target lists, the
// optimiser's drivers, joint inference, the renderer and the device groups (group.h).  Only this library compiles them.
// There is deliberately no CPU evaluation path: without a HIP device every entry point
// that computes returns CELESTE_ERR_NO_DEVICE.
#include "elbo_kernels.h"
#include "optim_kernels.h"
#include "fused_kernels.h"

struct celeste_group;

#include "engine_eval.h"

extern "C" int celeste_elbo_eval_batch_device(celeste_ctx_t *c, const double *d_vp, int32_t n_targets,
                                              const int32_t *d_targets, uint32_t flags, double *d_v, double *d_d,
                                              double *d_h, int64_t *d_counters, int32_t *d_status, void *stream_) try {
    return launch_eval(c, d_vp, n_targets, d_targets, flags, d_v, d_d, d_h, d_counters, d_status, stream_, true);
} ABI_CATCH

// the events of the first n parts of a host-pointer sweep (created on first use; the calling thread's device is the context's)
static int ensure_part_events(celeste_ctx_t *c, int n) {
    for (int k = 0; k < n && k < celeste_ctx::MAX_PARTS; ++k) {
        if (!c->part_done[k]) HIP_TRY(hipEventCreateWithFlags(&c->part_done[k], hipEventDisableTiming));
        if (!c->part_copied[k]) HIP_TRY(hipEventCreateWithFlags(&c->part_copied[k], hipEventDisableTiming));
    }
    return CELESTE_OK;
}

// ---- prepared target lists -------------------------------------------------------------------------------------------
// A sweep's work list, record offsets, visit items, target marks and the choice of tables to fill and neighbour items
// to render depend on (context, target list, chunk size, G) and not on vp.  A caller that evaluates ONE target list
// again and again (a rank draining its shard: DeviceShardedSweep, celeste_group_sweep) has them made once, by the same
// kernels, into buffers the list owns; a prepared sweep is then four launches -- SrcGeo + the listed visits' tables (geo_prep_kernel),
// value_union_kernel over the list's neighbour pixels (each once: value_union.h), pixel_kernel, lift_kernel -- instead of
// eight.  Same records in the same order, same arithmetic: the results are those of launch_eval bit for bit.  Nothing of the context's per-call scratch that launch_eval
// rewrites (d_work, d_rec_off, d_items, d_needed, d_prep_mark, stamp) is touched; d_acc is shared.
// (struct celeste_targets, LIST_STAMP and targets_free stand in engine_context.h: celeste_ctx_destroy frees the lists left.)

// targets: host copy of the list, validated by the caller
static int targets_build(celeste_ctx_t *c, const std::vector<int32_t> &tg, celeste_targets_t **out) {
    const int32_t n = (int32_t)tg.size();
    if ((size_t)n * c->M * c->CH > 0x7fffffffull) return CELESTE_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(c->device));
    celeste_targets *t = new celeste_targets;
    t->ctx = c; t->n = n; t->G = chunk_group(n);
    int32_t *d_blk = nullptr;
    auto fail = [&](int st) { if (d_blk) (void)hipFree(d_blk); (void)hipGetLastError(); targets_free(t); return st; };
#define LIST_TRY(expr) do { if ((expr) != hipSuccess) return fail(CELESTE_ERR_HIP); } while (0)
#define LIST_ALLOC(p, bytes) do { if (hipMalloc((void **)&(p), (bytes)) != hipSuccess) return fail(CELESTE_ERR_ALLOC); } while (0)
    // the compact lists, from the host mirrors: the visits of the targets and of their neighbours (in visit order, as
    // prep_kernel's grid runs), and the value items of the targets (in the order of d_value_items: longest first)
    std::vector<char> is_tgt((size_t)c->S, 0), reads((size_t)c->S, 0);
    for (int32_t s : tg) {
        is_tgt[s] = 1; reads[s] = 1;
        for (int64_t q = c->h_nbr_off[s]; q < c->h_nbr_off[s + 1]; ++q) reads[c->h_nbr_idx[q]] = 1;
        t->n_records += c->h_src_chunks[s];
    }
    std::vector<int32_t> visits, vitems;
    for (int s = 0; s < c->S; ++s)
        if (reads[s]) for (int v = c->h_vis_off[s]; v < c->h_vis_off[s + 1]; ++v) visits.push_back(v);
    for (size_t i = 0; i < c->h_vitem_tgt.size(); ++i) if (is_tgt[c->h_vitem_tgt[i]]) vitems.push_back((int32_t)i);
    // the pixels of those items' rectangles, each once, and the items over them (value_union.h)
    std::vector<int32_t> upx;
    std::vector<ValueUnionItem> uitems;
    {
        static_assert(sizeof(ValueUnionBox) == 4 * sizeof(int32_t) && sizeof(ValueUnionItem) == sizeof(int4), "layout");
        std::vector<ValueUnionBox> boxes(c->h_patches.size());
        for (size_t v = 0; v < boxes.size(); ++v) { const DevPatch &q = c->h_patches[v]; boxes[v] = {q.off_h, q.off_w, q.H2, q.W2}; }
        std::vector<ValueUnionLink> links;
        links.reserve(vitems.size());
        for (int32_t i : vitems) links.push_back(c->h_vitem_link[(size_t)i]);      // (every chunk of a link: duplicates are dropped)
        if (!value_union_build(boxes.data(), std::move(links), c->chunk_px, upx, uitems)) return fail(CELESTE_ERR_INVALID_ARG);
    }
    t->n_visits = (int64_t)visits.size(); t->n_vitems = (int64_t)vitems.size(); t->n_uitems = (int64_t)uitems.size();
    const int n_cand = n * c->M;                                 // candidate visits k = ti * M + j
    const int n_wblk = (n_cand + WORK_NT - 1) / WORK_NT;
    const size_t n_blk = (size_t)n_wblk * (WORK_CLASSES + 1);
    LIST_ALLOC(t->d_targets, (size_t)n * sizeof(int32_t));
    LIST_ALLOC(t->d_work, std::max<size_t>((size_t)t->n_records, 1) * sizeof(int32_t));
    LIST_ALLOC(t->d_work_total, sizeof(int32_t));
    LIST_ALLOC(t->d_rec_off, (size_t)n_cand * sizeof(int32_t));
    if (!c->dense) LIST_ALLOC(t->d_items, (size_t)n_cand * sizeof(int2));
    LIST_ALLOC(t->d_needed, (size_t)c->S * sizeof(int32_t));
    LIST_ALLOC(t->d_visits, std::max<size_t>(visits.size(), 1) * sizeof(int32_t));
    LIST_ALLOC(t->d_vitems, std::max<size_t>(vitems.size(), 1) * sizeof(int32_t));
    LIST_ALLOC(t->d_uitems, std::max<size_t>(uitems.size(), 1) * sizeof(int4));
    LIST_ALLOC(t->d_upx, std::max<size_t>(upx.size(), 1) * sizeof(int32_t));
    LIST_ALLOC(d_blk, n_blk * sizeof(int32_t));
    LIST_TRY(hipMemcpy(t->d_targets, tg.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    if (!visits.empty()) LIST_TRY(hipMemcpy(t->d_visits, visits.data(), visits.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (!vitems.empty()) LIST_TRY(hipMemcpy(t->d_vitems, vitems.data(), vitems.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (!uitems.empty()) LIST_TRY(hipMemcpy(t->d_uitems, uitems.data(), uitems.size() * sizeof(int4), hipMemcpyHostToDevice));
    if (!upx.empty()) LIST_TRY(hipMemcpy(t->d_upx, upx.data(), upx.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    LIST_TRY(hipMemset(t->d_needed, 0, (size_t)c->S * sizeof(int32_t)));
    // the half of setup_thread that depends on the targets alone (vp == nullptr: no SrcGeo): visit items and target marks
    const size_t setup_threads = (size_t)n * (c->dense ? 1 : c->M);
    hipLaunchKernelGGL(setup_kernel, dim3((unsigned)((setup_threads + 63) / 64)), dim3(64), 0, nullptr, (const double *)nullptr, -1,
                       (SrcGeo *)nullptr, t->d_targets, n, c->d_vis_off, c->d_vis_img, c->M, t->d_items, t->d_needed, LIST_STAMP,
                       (int32_t *)nullptr, c->d_nbr_off, c->d_nbr_idx, (const int32_t *)nullptr);
    hipLaunchKernelGGL(work_count_kernel, dim3(n_wblk), dim3(WORK_NT), 0, nullptr, t->d_targets, n_cand, c->d_patches,
                       c->d_vis_off, c->d_vis_img, c->N, c->M, c->chunk_px, t->G, (int)c->dense, d_blk, (const int32_t *)nullptr);
    hipLaunchKernelGGL(work_scan_kernel, dim3(1), dim3(1024), 0, nullptr, d_blk, (int)n_blk, t->d_work_total, n_wblk * WORK_CLASSES);
    hipLaunchKernelGGL(work_fill_kernel, dim3(n_wblk), dim3(WORK_NT), 0, nullptr, t->d_targets, n_cand, c->d_patches,
                       c->d_vis_off, c->d_vis_img, c->N, c->M, c->CH, c->chunk_px, t->G, (int)c->dense, d_blk, t->d_work,
                       (const int32_t *)nullptr, t->d_rec_off);
    LIST_TRY(hipGetLastError());
    LIST_TRY(hipMemcpy(&t->n_work, t->d_work_total, sizeof(int32_t), hipMemcpyDeviceToHost));   // (waits for the kernels)
    LIST_TRY(hipFree(d_blk)); d_blk = nullptr;
    if (t->n_work < 0 || (int64_t)t->n_work > t->n_records) return fail(CELESTE_ERR_HIP);   // (a group holds at least one record)
    // The items' descriptors (work_sequences.h): the list's work items and record offsets come back (4 B per item and per
    // candidate visit) and every item that has pixels is described from the host mirrors as pixel_kernel's prologue would
    // find it.  Most trips first (ties in work-list order): the work list's own order, without its quantisation.
    {
        std::vector<int32_t> h_work((size_t)t->n_work), h_rec_off((size_t)n_cand);
        if (t->n_work > 0) LIST_TRY(hipMemcpy(h_work.data(), t->d_work, h_work.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (n_cand > 0) LIST_TRY(hipMemcpy(h_rec_off.data(), t->d_rec_off, h_rec_off.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        std::vector<WorkSeqDesc> items;
        std::vector<int32_t> trips, order;
        items.reserve(h_work.size()); trips.reserve(h_work.size());
        for (int32_t wg0 : h_work) {
            if (wg0 < 0 || wg0 / c->CH >= n_cand) return fail(CELESTE_ERR_HIP);
            const int tn = wg0 / c->CH, ch0 = wg0 - tn * c->CH, ti = tn / c->M, j = tn - ti * c->M, s = tg[(size_t)ti];
            if (j >= c->h_vis_off[s + 1] - c->h_vis_off[s]) continue;       // (pixel_kernel: v < 0)
            const int32_t v = c->h_vis_off[s] + j;
            const DevPatch &q = c->h_patches[(size_t)v];
            const int n_trips = work_item_trips(q.H2 > 0 && q.W2 > 0 ? (int64_t)q.H2 * q.W2 : 0, ch0, t->G, c->chunk_px);
            if (n_trips <= 0) continue;                                     // (pixel_kernel: empty chunk range)
            const int64_t nbn = c->h_nbr_off[s + 1] - c->h_nbr_off[s];
            if (nbn > 0x7fffffffll) return fail(CELESTE_ERR_INVALID_ARG);
            WorkSeqDesc D{};
            D.off_h = q.off_h; D.off_w = q.off_w; D.H2 = q.H2; D.W2 = q.W2; D.bitmap_off = q.bitmap_off; D.stamp = q.stamp;
            D.nb0 = c->h_nbr_off[s]; D.nbn = (int32_t)nbn; D.nv_row = c->dense ? 0 : c->h_nv_base[s] + (int64_t)j * nbn;
            D.v = v; D.n = c->h_vis_img[(size_t)v]; D.rec_base = h_rec_off[(size_t)tn]; D.ch0 = ch0;
            order.push_back((int32_t)items.size()); items.push_back(D); trips.push_back(n_trips);
        }
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return trips[(size_t)a] > trips[(size_t)b]; });
        std::vector<WorkSeqDesc> sorted(items.size());
        for (size_t i = 0; i < order.size(); ++i) sorted[i] = items[(size_t)order[i]];
        t->n_desc = (int32_t)sorted.size();
        LIST_ALLOC(t->d_desc, std::max<size_t>(sorted.size(), 1) * sizeof(WorkSeqDesc));
        if (!sorted.empty()) LIST_TRY(hipMemcpy(t->d_desc, sorted.data(), sorted.size() * sizeof(WorkSeqDesc), hipMemcpyHostToDevice));
    }
#undef LIST_TRY
#undef LIST_ALLOC
    c->lists.push_back(t);
    *out = t;
    return CELESTE_OK;
}

extern "C" int celeste_targets_create(celeste_ctx_t *c, int32_t n_targets, const int32_t *targets, celeste_targets_t **out) try {
    if (!c || !out || !targets || n_targets <= 0) return CELESTE_ERR_INVALID_ARG;
    *out = nullptr;
    for (int32_t i = 0; i < n_targets; ++i) if (targets[i] < 0 || targets[i] >= c->S) return CELESTE_ERR_INVALID_ARG;
    return targets_build(c, std::vector<int32_t>(targets, targets + n_targets), out);
} ABI_CATCH

extern "C" int celeste_targets_create_device(celeste_ctx_t *c, int32_t n_targets, const int32_t *d_targets, void *stream_,
                                             celeste_targets_t **out) try {
    if (!c || !out || !d_targets || n_targets <= 0) return CELESTE_ERR_INVALID_ARG;
    *out = nullptr;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<int32_t> tg((size_t)n_targets);
    HIP_TRY(hipMemcpyAsync(tg.data(), d_targets, (size_t)n_targets * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream_));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream_));      // (what the caller queued on `stream` has written the list)
    for (int32_t s : tg) if (s < 0 || s >= c->S) return CELESTE_ERR_INVALID_ARG;
    return targets_build(c, tg, out);
} ABI_CATCH

// the list leaves its context and is freed; the caller has made the list's device current and knows no sweep over it in flight
static void targets_release(celeste_targets_t *t) {
    celeste_ctx_t *c = t->ctx;
    auto it = std::find(c->lists.begin(), c->lists.end(), t);
    if (it != c->lists.end()) c->lists.erase(it);
    targets_free(t);
}

extern "C" void celeste_targets_destroy(celeste_targets_t *t) {
    if (!t) return;
    (void)hipSetDevice(t->ctx->device);
    (void)hipDeviceSynchronize();        // (a sweep over the list may be in flight on any stream)
    targets_release(t);
}

// A sweep over a prepared list.  What the prepared path does not serve goes to launch_eval with the list's own copy of the
// targets: single precision (its 512-pixel chunks need lists of their own), the split variant, batches small enough for
// eval_fused_kernel, CELESTE_NO_PREPARED=1 (the A/B switch).
static int launch_prepared(celeste_ctx_t *c, const celeste_targets_t *t, const double *d_vp, uint32_t flags, double *d_v,
                           double *d_d, double *d_h, int64_t *d_counters, int32_t *d_status, void *stream_) {
    if (!c || !t || t->ctx != c) return CELESTE_ERR_INVALID_ARG;
    const int32_t n_targets = t->n;
    const char *off = getenv("CELESTE_NO_PREPARED");
    if ((off && atoi(off) != 0) || (flags & (CELESTE_FLAG_FP32 | CELESTE_FLAG_SPLIT)) ||
        want_eval_fused(flags, n_targets, true, d_d, d_h))
        return launch_eval(c, d_vp, n_targets, t->d_targets, flags, d_v, d_d, d_h, d_counters, d_status, stream_, true, nullptr,
                           t->n_records);    // (the list knows its chunk count)
    if (!d_vp || !d_v || !d_status) return CELESTE_ERR_INVALID_ARG;
    if ((flags & CELESTE_FLAG_HESS) && !d_h) return CELESTE_ERR_INVALID_ARG;
    if ((flags & (CELESTE_FLAG_GRAD | CELESTE_FLAG_HESS)) && !d_d) return CELESTE_ERR_INVALID_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    const size_t need = std::max<size_t>((size_t)t->n_records, 1) * ACC_N;
    if (need > c->acc_cap) {
        if (c->d_acc) { HIP_TRY(hipStreamSynchronize(stream)); HIP_TRY(hipFree(c->d_acc)); c->d_acc = nullptr; }
        HIP_TRY(hipMalloc((void **)&c->d_acc, need * sizeof(double)));
        c->acc_cap = need;
    }
    const int CH = c->CH, chunk_px = c->chunk_px;
    if (c->timing) HIP_TRY(hipEventRecord(c->ev[0], stream));
    // SrcGeo of every source (64 per workgroup) and the tables of the listed visits, side by side in one launch
    const unsigned geo_blocks = (unsigned)((c->S + 63) / 64);
    hipLaunchKernelGGL(geo_prep_kernel, dim3(geo_blocks + (unsigned)t->n_visits), dim3(64), 0, stream, d_vp, c->d_images,
                       c->d_patches, c->d_vis_src, c->d_vis_img, c->K, c->d_srcimg, c->d_comps, t->d_visits, (int)geo_blocks,
                       c->S, c->d_geo);
    // the neighbours' light: every pixel the list wants once (value_union_kernel over the list's own items);
    // CELESTE_NO_VALUE_UNION=1 (the A/B switch, read per call): once per link, the context's items of the list's targets
    const char *no_union = getenv("CELESTE_NO_VALUE_UNION");
    if (!(no_union && atoi(no_union) != 0)) {
        if (t->n_uitems > 0) {
            const bool wide_items = n_targets <= VALUE_WIDE_MAX && c->chunk_px == 256 && !getenv("CELESTE_NO_WIDE_VALUE");
#define LAUNCH_UNION(WAVES)                                                                                                 \
            hipLaunchKernelGGL((value_union_kernel<WAVES>), dim3((unsigned)t->n_uitems), dim3(64 * WAVES), 0, stream,       \
                               c->d_patches, c->d_coefs, c->d_srcimg, c->d_comps, c->d_val_off, t->d_uitems, t->d_upx,      \
                               c->NC, c->d_val)
            if (wide_items) LAUNCH_UNION(4); else LAUNCH_UNION(1);
#undef LAUNCH_UNION
        }
    } else if (t->n_vitems > 0) {
        const bool wide_items = n_targets <= VALUE_WIDE_MAX && c->chunk_px == 256 && !getenv("CELESTE_NO_WIDE_VALUE");
#define LAUNCH_VALUE(WAVES)                                                                                                 \
        hipLaunchKernelGGL((value_kernel<double, WAVES>), dim3((unsigned)t->n_vitems), dim3(64 * WAVES), 0, stream,        \
                           c->d_patches, c->d_coefs, c->d_srcimg, c->d_comps, t->d_needed, LIST_STAMP, c->d_val_off,        \
                           c->d_value_items, c->NC, c->chunk_px, c->d_val, c->d_coefs_f, t->d_vitems)
        if (wide_items) LAUNCH_VALUE(4); else LAUNCH_VALUE(1);
#undef LAUNCH_VALUE
    }
    if (c->timing) HIP_TRY(hipEventRecord(c->ev[1], stream));
    // one workgroup per described item (pixel_desc_kernel); CELESTE_NO_SEQUENCES=1 (the A/B switch, read per call): pixel_kernel
    // over the list's d_work
    const char *no_seq = getenv("CELESTE_NO_SEQUENCES");
    const bool sequences = !(no_seq && atoi(no_seq) != 0);
    const dim3 grid((unsigned)std::max<int32_t>(sequences ? t->n_desc : t->n_work, 1));
#define LAUNCH_SEQ(MODE)                                                                                                    \
    hipLaunchKernelGGL((pixel_desc_kernel<MODE>), grid, dim3(64), 0, stream, c->d_images, c->d_patches, c->d_coefs,         \
                       c->d_bitmaps, c->d_srcimg, c->d_comps, c->d_nbr_idx, c->d_val_off, c->d_val, c->N, c->NC, chunk_px,  \
                       t->G, c->d_acc, t->d_desc, t->n_desc, c->d_nbr_vis, c->d_coefs_f)
    if (!sequences) { }
    else if (flags & CELESTE_FLAG_HESS) LAUNCH_SEQ(2);
    else if (flags & CELESTE_FLAG_GRAD) LAUNCH_SEQ(1);
    else LAUNCH_SEQ(0);
#undef LAUNCH_SEQ
#define LAUNCH_PIXEL(MODE)                                                                                                  \
    hipLaunchKernelGGL((pixel_kernel<MODE, double>), grid, dim3(64), 0, stream, c->d_images, c->d_patches, c->d_coefs,      \
                       c->d_bitmaps, c->d_srcimg, c->d_comps, c->d_nbr_off, c->d_nbr_idx, c->d_val_off, c->d_val,           \
                       t->d_targets, c->N, c->NC, CH, chunk_px, t->G, c->d_acc, c->d_tile_off, c->d_rec,                    \
                       (const int32_t *)nullptr, t->d_items, c->M, t->d_work, t->d_work_total, c->d_nv_base, c->d_nbr_vis,  \
                       t->d_rec_off, c->d_coefs_f)
    if (sequences) { }
    else if (flags & CELESTE_FLAG_HESS) LAUNCH_PIXEL(2);
    else if (flags & CELESTE_FLAG_GRAD) LAUNCH_PIXEL(1);
    else LAUNCH_PIXEL(0);
#undef LAUNCH_PIXEL
    if (c->timing) HIP_TRY(hipEventRecord(c->ev[2], stream));
    c->ev_split = 0;
    const int lift_nt = n_targets <= 1024 ? 512 : 256;     // (as launch_eval)
    bool lift7 = n_targets > 4096;
    if (const char *e = getenv("CELESTE_LIFT_WAVES")) lift7 = atoi(e) == 7;
#define LIFT_ARGS dim3(n_targets), dim3(lift_nt), 0, stream, d_vp, c->d_images, c->d_patches, c->d_geo, c->d_nbr_off,       \
                  c->d_nbr_idx, t->d_targets, c->d_acc, c->d_prior, c->d_vis_off, c->d_vis_img, c->N, c->M, CH, chunk_px,   \
                  flags, d_v, d_d, d_h, d_counters, d_status, (const int32_t *)nullptr, c->d_lg_sum, t->d_rec_off, \
                  (const int32_t *)nullptr
    if (lift7) hipLaunchKernelGGL(lift_kernel<7>, LIFT_ARGS); else hipLaunchKernelGGL(lift_kernel<8>, LIFT_ARGS);
#undef LIFT_ARGS
    if (c->timing) { HIP_TRY(hipEventRecord(c->ev[3], stream)); c->ev_valid = 1; }
    HIP_TRY(hipGetLastError());
    return CELESTE_OK;
}

extern "C" int celeste_elbo_eval_targets_device(celeste_ctx_t *c, const celeste_targets_t *t, const double *d_vp, uint32_t flags,
                                                double *d_v, double *d_d, double *d_h, int64_t *d_counters,
                                                int32_t *d_status, void *stream_) try {
    return launch_prepared(c, t, d_vp, flags, d_v, d_d, d_h, d_counters, d_status, stream_);
} ABI_CATCH

// ---- a copy stream whose copies really run beside the kernels -------------------------------------------------------
// HIP maps streams onto a few hardware queues in the order of their first use, and what else a queue carries decides
// whether a device-to-host copy on the copy stream overlaps a kernel on `stream` at all: one context in four or so drew a
// stream whose copies waited for the kernels (2.0 - 2.4 ms per host-pointer sweep of 2000 sources instead of 1.35;
// profiles/r06_stream_lottery.txt), and creating the stream at another priority only moved the draw.  So the first batch
// that relies on the overlap MEASURES it: a 4 MB copy on the candidate stream against a 300 us spin on `stream`; a
// candidate whose copy ends inside the spin is kept, otherwise up to three fresh streams are tried and the quickest wins.
// About a millisecond, once per context (CELESTE_COPY_STREAM_CHECK=0 skips it).
__global__ void spin_kernel(long long ticks) {
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
static int pick_copy_stream(celeste_ctx_t *c) {
    if (c->copy_stream_checked) return CELESTE_OK;
    c->copy_stream_checked = true;
    if (const char *e = getenv("CELESTE_COPY_STREAM_CHECK")) if (atoi(e) == 0) return CELESTE_OK;
    const size_t bytes = 4u << 20;
    void *d_buf = nullptr, *h_buf = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipMalloc(&d_buf, bytes) != hipSuccess || hipHostMalloc(&h_buf, bytes, hipHostMallocDefault) != hipSuccess ||
        hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
        (void)hipGetLastError();
        if (d_buf) (void)hipFree(d_buf);
        if (h_buf) (void)hipHostFree(h_buf);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        return CELESTE_OK;       // (no measurement: the stream stays as it is)
    }
    const float spin_ms = 0.3f;
    auto measure = [&](hipStream_t s, float *ms) -> bool {   // copy end relative to the spin's start
        if (hipEventRecord(e0, c->stream) != hipSuccess) return false;
        hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, c->stream, (long long)(spin_ms * 1e5));   // wall_clock64: 100 MHz
        if (hipStreamWaitEvent(s, e0, 0) != hipSuccess || hipMemcpyAsync(h_buf, d_buf, bytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipEventRecord(e1, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
            return false;
        return hipEventElapsedTime(ms, e0, e1) == hipSuccess;
    };
    float best = 0;
    hipStream_t retired[3]; int n_retired = 0;   // (back to the pool only at the end: a retired stream must not be drawn again here)
    bool ok = measure(c->copy_stream, &best) && measure(c->copy_stream, &best);     // (the first use of a stream creates its queue)
    for (int k = 0; ok && best > spin_ms && k < 3; ++k) {
        hipStream_t s = nullptr;
        float ms = 0;
        if (stream_acquire(c->device, &s) != hipSuccess) break;
        if (measure(s, &ms) && measure(s, &ms) && ms < best) { std::swap(s, c->copy_stream); best = ms; }
        retired[n_retired++] = s;
    }
    for (int k = 0; k < n_retired; ++k) stream_retire(c->device, retired[k]);
    (void)hipGetLastError();
    (void)hipFree(d_buf); (void)hipHostFree(h_buf); (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return CELESTE_OK;
}

// ---- page-locked host memory ---------------------------------------------------------------------------------
extern "C" void *celeste_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, std::max<size_t>(bytes, 1), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
extern "C" void celeste_host_free(void *ptr) { if (ptr) (void)hipHostFree(ptr); }
extern "C" int celeste_host_register(void *ptr, size_t bytes) try {
    if (!ptr || bytes == 0) return CELESTE_ERR_INVALID_ARG;
    if (hipHostRegister(ptr, bytes, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); return CELESTE_ERR_HIP; }
    return CELESTE_OK;
} ABI_CATCH
extern "C" int celeste_host_unregister(void *ptr) try {
    if (!ptr) return CELESTE_ERR_INVALID_ARG;
    if (hipHostUnregister(ptr) != hipSuccess) { (void)hipGetLastError(); return CELESTE_ERR_HIP; }
    return CELESTE_OK;
} ABI_CATCH
// is [ptr, ptr + bytes) page-locked memory the DMA engines can write directly?
static bool is_pinned(const void *ptr, size_t bytes) {
    if (!ptr || bytes == 0) return false;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, ptr) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (a.type != hipMemoryTypeHost) return false;
    if (hipPointerGetAttributes(&a, (const char *)ptr + bytes - 1) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

template <class T>
static int pinned_grow(T **p, size_t n) {
    if (*p) { staging_free(*p); *p = nullptr; }
    HIP_TRY(staging_alloc((void **)p, std::max<size_t>(n, 1) * sizeof(T)));
    return CELESTE_OK;
}

// A few targets per call (the literal drop-in: one elbo() per call): two copies instead of seven and no second stream --
// the table and the target list go up as ONE block, every output comes down as ONE block on the context's stream.
#define EVAL_SMALL_MAX 32
static int eval_small(celeste_ctx_t *c, const double *vp, int32_t n_targets, const int32_t *targets, uint32_t flags, double *v,
                      double *d, double *h, int64_t *counters, int32_t *status) {
    const size_t n = (size_t)n_targets, HS = (flags & CELESTE_FLAG_PACKED_HESS) ? CELESTE_HP : (size_t)CEL_P * CEL_P;
    const size_t vp_n = (size_t)c->S * CEL_P;
    const size_t in_n = vp_n + EVAL_SMALL_MAX / 2;                                     // doubles: table, then 32 int32
    const size_t per = 1 + CEL_P + (size_t)CEL_P * CEL_P + 2 + 1, out_n = EVAL_SMALL_MAX * per;
    if (!c->d_small_in) HIP_TRY(hipMalloc((void **)&c->d_small_in, in_n * sizeof(double)));
    if (!c->p_small_in) HIP_TRY(staging_alloc((void **)&c->p_small_in, in_n * sizeof(double)));
    if (!c->d_small_out) HIP_TRY(hipMalloc((void **)&c->d_small_out, out_n * sizeof(double)));
    if (!c->p_small_out) HIP_TRY(staging_alloc((void **)&c->p_small_out, out_n * sizeof(double)));
    memcpy(c->p_small_in, vp, vp_n * sizeof(double));
    memcpy(c->p_small_in + vp_n, targets, n * sizeof(int32_t));
    HIP_TRY(hipMemcpyAsync(c->d_small_in, c->p_small_in, (vp_n + (n + 1) / 2) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    // the block of outputs: v[n], d[n x 44], h[n x HS], counters[n x 2], status[n].  The kernels write it straight into the
    // page-locked host block: no copy down (84 -> 81 us per call on a per-source context; CELESTE_SMALL_ZERO_COPY=0: device
    // block + copy)
    static const bool zero_copy = !(getenv("CELESTE_SMALL_ZERO_COPY") && atoi(getenv("CELESTE_SMALL_ZERO_COPY")) == 0);
    double *out_dev = c->d_small_out;
    if (zero_copy) HIP_TRY(hipHostGetDevicePointer((void **)&out_dev, c->p_small_out, 0));
    double *const b_v = out_dev, *const b_d = b_v + n, *const b_h = b_d + n * CEL_P;
    int64_t *const b_c = reinterpret_cast<int64_t *>(b_h + n * HS);
    int32_t *const b_s = reinterpret_cast<int32_t *>(b_c + 2 * n);
    const size_t bytes = (n * (1 + CEL_P + HS + 2)) * sizeof(double) + n * sizeof(int32_t);
    int64_t n_chunks = 0;
    for (int t = 0; t < n_targets; ++t) n_chunks += c->h_src_chunks[targets[t]];
    int st = launch_eval(c, c->d_small_in, n_targets, reinterpret_cast<const int32_t *>(c->d_small_in + vp_n), flags, b_v, b_d, b_h,
                         b_c, b_s, c->stream, true, nullptr, n_chunks);
    if (st != CELESTE_OK) { (void)hipStreamSynchronize(c->stream); return st; }
    if ((!zero_copy && hipMemcpyAsync(c->p_small_out, c->d_small_out, bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
        hipStreamSynchronize(c->stream) != hipSuccess) { (void)hipStreamSynchronize(c->stream); return CELESTE_ERR_HIP; }
    const double *const o_v = c->p_small_out, *const o_d = o_v + n, *const o_h = o_d + n * CEL_P;
    const int64_t *const o_c = reinterpret_cast<const int64_t *>(o_h + n * HS);
    const int32_t *const o_s = reinterpret_cast<const int32_t *>(o_c + 2 * n);
    if (v) memcpy(v, o_v, n * sizeof(double));
    if (d && (flags & (CELESTE_FLAG_GRAD | CELESTE_FLAG_HESS))) memcpy(d, o_d, n * CEL_P * sizeof(double));
    if (h && (flags & CELESTE_FLAG_HESS)) memcpy(h, o_h, n * HS * sizeof(double));
    if (counters) memcpy(counters, o_c, n * 2 * sizeof(int64_t));
    int worst = CELESTE_OK;
    for (int t = 0; t < n_targets; ++t) {
        if (status) status[t] = o_s[t];
        if (o_s[t] != CELESTE_OK && worst == CELESTE_OK) worst = o_s[t];
    }
    return worst;
}

// The host-pointer sweep (what the Julia shim calls).  vp and the target list go up through page-locked staging.  A page-locked
// Hessian array (celeste_host_alloc / celeste_host_register) is written by the lift kernel itself through its device address:
// one launch chain, nothing to copy.  Otherwise the batch is cut into up to MAX_PARTS parts that are evaluated back to back on
// the context's stream while each finished part's results are copied down on the copy stream into page-locked staging,
// followed by a host copy of that part (which overlaps the device work of the following parts).  Only the context's own
// streams are waited for.
extern "C" int celeste_elbo_eval_batch(celeste_ctx_t *c, const double *vp, int32_t n_targets, const int32_t *targets,
                                       uint32_t flags, double *v, double *d, double *h, int64_t *counters,
                                       int32_t *status) try {
    if (!c || !vp || !targets || n_targets < 0) return CELESTE_ERR_INVALID_ARG;
    if (n_targets == 0) return CELESTE_OK;
    for (int t = 0; t < n_targets; ++t) if (targets[t] < 0 || targets[t] >= c->S) return CELESTE_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(c->device));
    if (n_targets <= EVAL_SMALL_MAX && !c->timing && v) return eval_small(c, vp, n_targets, targets, flags, v, d, h, counters, status);
    const bool want_h = h && (flags & CELESTE_FLAG_HESS);
    const bool want_d = d && (flags & (CELESTE_FLAG_GRAD | CELESTE_FLAG_HESS));
    const size_t HS = (flags & CELESTE_FLAG_PACKED_HESS) ? CELESTE_HP : (size_t)CEL_P * CEL_P;   // doubles per Hessian
    const size_t n = (size_t)n_targets;
    const size_t vp_bytes = (size_t)c->S * CEL_P * sizeof(double);
    if (!c->d_vp) HIP_TRY(hipMalloc((void **)&c->d_vp, vp_bytes));
    if (!c->p_vp) { int st = pinned_grow(&c->p_vp, (size_t)c->S * CEL_P); if (st != CELESTE_OK) return st; }
    if (n > c->stage_cap) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        void **ps[] = {(void **)&c->d_targets, (void **)&c->d_v, (void **)&c->d_d, (void **)&c->d_h, (void **)&c->d_cnt, (void **)&c->d_status};
        for (void **p : ps) if (*p) { HIP_TRY(hipFree(*p)); *p = nullptr; }
        c->stage_cap = 0;
        HIP_TRY(hipMalloc((void **)&c->d_targets, n * sizeof(int32_t)));
        HIP_TRY(hipMalloc((void **)&c->d_v, n * sizeof(double)));
        HIP_TRY(hipMalloc((void **)&c->d_d, n * CEL_P * sizeof(double)));
        HIP_TRY(hipMalloc((void **)&c->d_h, n * CEL_P * CEL_P * sizeof(double)));
        HIP_TRY(hipMalloc((void **)&c->d_cnt, n * 2 * sizeof(int64_t)));
        HIP_TRY(hipMalloc((void **)&c->d_status, n * sizeof(int32_t)));
        c->stage_cap = n;
    }
    // which outputs need staging on the host
    const bool pin_v = is_pinned(v, n * sizeof(double)), pin_d = !want_d || is_pinned(d, n * CEL_P * sizeof(double));
    const bool pin_h = !want_h || is_pinned(h, n * HS * sizeof(double));
    const bool pin_c = !counters || is_pinned(counters, n * 2 * sizeof(int64_t));
    if (n > c->pin_cap) {
        c->pin_cap = 0;
        int st = pinned_grow(&c->p_targets, n);
        if (st == CELESTE_OK) st = pinned_grow(&c->p_status, n);
        if (st == CELESTE_OK) st = pinned_grow(&c->p_v, n);
        if (st == CELESTE_OK) st = pinned_grow(&c->p_d, n * CEL_P);
        if (st == CELESTE_OK) st = pinned_grow(&c->p_cnt, n * 2);
        if (st == CELESTE_OK) st = pinned_grow(&c->p_h, n * CEL_P * CEL_P);
        if (st != CELESTE_OK) return st;
        c->pin_cap = n;
    }
    // inputs: through page-locked staging unless the caller's vp already is page-locked
    const double *vp_src = vp;
    if (!is_pinned(vp, vp_bytes)) { memcpy(c->p_vp, vp, vp_bytes); vp_src = c->p_vp; }
    memcpy(c->p_targets, targets, n * sizeof(int32_t));
    HIP_TRY(hipMemcpyAsync(c->d_vp, vp_src, vp_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_targets, c->p_targets, n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));

    // parts: at least 192 targets each so that a part still fills the chip; one part when nothing large comes back
    int n_parts = 1;
    if (want_h) n_parts = (int)std::min<size_t>(celeste_ctx::MAX_PARTS, std::max<size_t>(1, n / 192));
    if (c->timing) n_parts = 1;   // the kernel timers describe one launch
    // Page-locked Hessians: the lift kernel writes them STRAIGHT into the caller's array (the device address of the mapped host
    // block) -- no copy engine, no second stream, no cross-stream dependency per part, whose latency is what made one context in
    // four slow (pick_copy_stream); the PCIe writes are the lift's own (CELESTE_HOST_ZERO_COPY=0: the copied parts).
    static const bool zero_copy_h = !(getenv("CELESTE_HOST_ZERO_COPY") && atoi(getenv("CELESTE_HOST_ZERO_COPY")) == 0);
    double *h_mapped = nullptr;
    if (want_h && pin_h && zero_copy_h && !c->timing && hipHostGetDevicePointer((void **)&h_mapped, h, 0) == hipSuccess && h_mapped) n_parts = 1;
    else { h_mapped = nullptr; (void)hipGetLastError(); }
    if (n_parts > 1) (void)pick_copy_stream(c);
    double *const o_v = pin_v ? v : c->p_v;
    double *const o_d = want_d ? (pin_d ? d : c->p_d) : nullptr;
    double *const o_h = want_h ? (pin_h ? h : c->p_h) : nullptr;
    int64_t *const o_c = counters ? (pin_c ? counters : c->p_cnt) : nullptr;
    // From here on copies into the CALLER's buffers may be in flight on the copy stream: an error return first waits for
    // both streams, so that no DMA writes into memory the caller believes is his again (page-locked blocks are recycled)
#define EB_TRY(expr)                                                                                             \
    do {                                                                                                         \
        hipError_t e__ = (expr);                                                                                 \
        if (e__ != hipSuccess) {                                                                                 \
            fprintf(stderr, "celeste_mi355x: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            (void)hipStreamSynchronize(c->stream); (void)hipStreamSynchronize(c->copy_stream);                   \
            return CELESTE_ERR_HIP;                                                                              \
        }                                                                                                        \
    } while (0)
    int part_lo[celeste_ctx::MAX_PARTS + 1];
    for (int k = 0; k <= n_parts; ++k) part_lo[k] = (int)((int64_t)n_targets * k / n_parts);
    { int st_e = ensure_part_events(c, n_parts); if (st_e != CELESTE_OK) return st_e; }
    for (int k = 0; k < n_parts; ++k) {
        const int lo = part_lo[k], cnt = part_lo[k + 1] - lo;
        int64_t n_chunks = 0;   // the targets are known here: exact size of the pixel kernel's work list
        for (int t = lo; t < lo + cnt; ++t) n_chunks += c->h_src_chunks[targets[t]];
        int st = launch_eval(c, c->d_vp, cnt, c->d_targets + lo, flags, c->d_v + lo, c->d_d + (size_t)lo * CEL_P,
                             h_mapped ? h_mapped + (size_t)lo * HS : c->d_h + (size_t)lo * HS, c->d_cnt + 2 * (size_t)lo,
                             c->d_status + lo, c->stream, true, nullptr, n_chunks, k > 0, nullptr, n_parts > 1);
        if (st != CELESTE_OK) { (void)hipStreamSynchronize(c->stream); (void)hipStreamSynchronize(c->copy_stream); return st; }
        EB_TRY(hipEventRecord(c->part_done[k], c->stream));
        EB_TRY(hipStreamWaitEvent(c->copy_stream, c->part_done[k], 0));
        if (o_h && !h_mapped) EB_TRY(hipMemcpyAsync(o_h + (size_t)lo * HS, c->d_h + (size_t)lo * HS, (size_t)cnt * HS * sizeof(double),
                                                     hipMemcpyDeviceToHost, c->copy_stream));
        if (o_d) EB_TRY(hipMemcpyAsync(o_d + (size_t)lo * CEL_P, c->d_d + (size_t)lo * CEL_P,
                                        (size_t)cnt * CEL_P * sizeof(double), hipMemcpyDeviceToHost, c->copy_stream));
        EB_TRY(hipMemcpyAsync(o_v + lo, c->d_v + lo, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost, c->copy_stream));
        if (o_c) EB_TRY(hipMemcpyAsync(o_c + 2 * (size_t)lo, c->d_cnt + 2 * (size_t)lo, (size_t)cnt * 2 * sizeof(int64_t),
                                        hipMemcpyDeviceToHost, c->copy_stream));
        EB_TRY(hipMemcpyAsync(c->p_status + lo, c->d_status + lo, (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToHost,
                               c->copy_stream));
        EB_TRY(hipEventRecord(c->part_copied[k], c->copy_stream));
    }
    for (int k = 0; k < n_parts; ++k) {   // staged outputs: host copy of part k while later parts are still in flight
        const int lo = part_lo[k], cnt = part_lo[k + 1] - lo;
        EB_TRY(hipEventSynchronize(c->part_copied[k]));
        if (v && !pin_v) memcpy(v + lo, c->p_v + lo, (size_t)cnt * sizeof(double));
        if (want_d && !pin_d) memcpy(d + (size_t)lo * CEL_P, c->p_d + (size_t)lo * CEL_P, (size_t)cnt * CEL_P * sizeof(double));
        if (want_h && !pin_h) memcpy(h + (size_t)lo * HS, c->p_h + (size_t)lo * HS, (size_t)cnt * HS * sizeof(double));
        if (counters && !pin_c) memcpy(counters + 2 * (size_t)lo, c->p_cnt + 2 * (size_t)lo, (size_t)cnt * 2 * sizeof(int64_t));
    }
    EB_TRY(hipStreamSynchronize(c->stream));
#undef EB_TRY
    int worst = CELESTE_OK;
    for (int t = 0; t < n_targets; ++t) {
        const int32_t s1 = c->p_status[t];
        if (status) status[t] = s1;
        if (s1 != CELESTE_OK && worst == CELESTE_OK) worst = s1;
    }
    return worst;
} ABI_CATCH

extern "C" int celeste_elbo_eval(celeste_ctx_t *c, const double *vp, int32_t target, uint32_t flags, double *v,
                                 double *d, double *h, int64_t *n_active_px, int64_t *n_inactive_px) try {
    int64_t cnt[2] = {0, 0};
    int32_t st1 = 0;
    double vv = 0;
    int st = celeste_elbo_eval_batch(c, vp, 1, &target, flags, &vv, d, h, cnt, &st1);
    if (v) *v = vv;
    if (n_active_px) *n_active_px = cnt[0];
    if (n_inactive_px) *n_inactive_px = cnt[1];
    return st;
} ABI_CATCH

// ---- elbo() with several active sources (ElboArgs.active_sources, elbo_args.jl:165-211) -------------------
extern "C" int celeste_elbo_eval_multi(celeste_ctx_t *c, const double *vp, int32_t n_active, const int32_t *active,
                                       uint32_t flags, double *v, double *d, double *h, int64_t *n_active_px,
                                       int64_t *n_inactive_px) try {
    if (!c || !vp || !active || n_active < 1 || (flags & (CELESTE_FLAG_SPLIT | CELESTE_FLAG_PACKED_HESS))) return CELESTE_ERR_INVALID_ARG;
    const int Sa = n_active;
    for (int a = 0; a < Sa; ++a) {
        if (active[a] < 0 || active[a] >= c->S) return CELESTE_ERR_INVALID_ARG;
        for (int b = 0; b < a; ++b) if (active[b] == active[a]) return CELESTE_ERR_INVALID_ARG;
    }
    const bool want_hess = (flags & CELESTE_FLAG_HESS) != 0;
    const bool want_grad = want_hess || (flags & CELESTE_FLAG_GRAD) != 0;
    if ((want_grad && !d) || (want_hess && !h)) return CELESTE_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(c->device));
    const size_t PT = (size_t)CEL_P * Sa;
    std::vector<double> hv(Sa), hd((size_t)Sa * CEL_P), hh(want_hess ? (size_t)Sa * CEL_P * CEL_P : 0);
    std::vector<int64_t> hcnt((size_t)Sa * 2);
    std::vector<int32_t> hst(Sa), rank((size_t)c->S, -1);
    for (int a = 0; a < Sa; ++a) rank[active[a]] = a;
    // pairs of active sources that light common pixels; the first of a pair must list the second as a neighbour
    std::vector<int32_t> pa, pb, pia, pib;
    if (want_hess)
        for (int ia = 0; ia < Sa; ++ia) for (int ib = ia + 1; ib < Sa; ++ib) {
            if (nbr_lists(c, active[ia], active[ib])) { pa.push_back(active[ia]); pb.push_back(active[ib]); pia.push_back(ia); pib.push_back(ib); }
            else if (nbr_lists(c, active[ib], active[ia])) { pa.push_back(active[ib]); pb.push_back(active[ia]); pia.push_back(ib); pib.push_back(ia); }
        }
    const size_t np = pa.size();
    double *d_vp = nullptr, *d_v = nullptr, *d_d = nullptr, *d_h = nullptr, *d_rec = nullptr, *d_x = nullptr;
    int32_t *d_t = nullptr, *d_st = nullptr, *d_rank = nullptr, *d_pa = nullptr, *d_pb = nullptr;
    int64_t *d_cnt = nullptr;
    int rc = CELESTE_OK;
    std::vector<double> hx(np * LIFT_NP * LIFT_NP);
#define MU_TRY(expr) do { if ((expr) != hipSuccess) { rc = CELESTE_ERR_HIP; goto done; } } while (0)
    MU_TRY(scratch_get(c, 0, (size_t)c->S * CEL_P * sizeof(double), &d_vp));
    MU_TRY(scratch_get(c, 1, Sa * sizeof(double), &d_v));
    MU_TRY(scratch_get(c, 2, (size_t)Sa * CEL_P * sizeof(double), &d_d));
    MU_TRY(scratch_get(c, 3, (size_t)Sa * CEL_P * CEL_P * sizeof(double), &d_h));
    MU_TRY(scratch_get(c, 4, Sa * sizeof(int32_t), &d_t));
    MU_TRY(scratch_get(c, 5, Sa * sizeof(int32_t), &d_st));
    MU_TRY(scratch_get(c, 6, (size_t)Sa * 2 * sizeof(int64_t), &d_cnt));
    MU_TRY(scratch_get(c, 7, (size_t)c->S * sizeof(int32_t), &d_rank));
    MU_TRY(hipMemcpyAsync(d_vp, vp, (size_t)c->S * CEL_P * sizeof(double), hipMemcpyHostToDevice, c->stream));
    MU_TRY(hipMemcpyAsync(d_t, active, Sa * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    MU_TRY(hipMemcpyAsync(d_rank, rank.data(), (size_t)c->S * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    rc = launch_eval(c, d_vp, Sa, d_t, flags, d_v, d_d, d_h, d_cnt, d_st, c->stream, true, d_rank);
    if (rc != CELESTE_OK) goto done;
    if (np > 0) {
        MU_TRY(scratch_get(c, 8, np * sizeof(int32_t), &d_pa));
        MU_TRY(scratch_get(c, 9, np * sizeof(int32_t), &d_pb));
        MU_TRY(scratch_get(c, 10, np * c->N * ZV * ZV * sizeof(double), &d_rec));
        MU_TRY(scratch_get(c, 11, np * LIFT_NP * LIFT_NP * sizeof(double), &d_x));
        MU_TRY(hipMemcpyAsync(d_pa, pa.data(), np * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        MU_TRY(hipMemcpyAsync(d_pb, pb.data(), np * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        launch_cross(c, d_vp, np, d_pa, d_pb, d_rec, d_x, c->stream);
        MU_TRY(hipMemcpyAsync(hx.data(), d_x, hx.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    MU_TRY(hipMemcpyAsync(hv.data(), d_v, Sa * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    MU_TRY(hipMemcpyAsync(hst.data(), d_st, Sa * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    MU_TRY(hipMemcpyAsync(hcnt.data(), d_cnt, hcnt.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    if (want_grad) MU_TRY(hipMemcpyAsync(hd.data(), d_d, hd.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (want_hess) MU_TRY(hipMemcpyAsync(hh.data(), d_h, hh.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    MU_TRY(hipStreamSynchronize(c->stream));
    {
        double vs = 0; int64_t na = 0, ni = 0;
        for (int a = 0; a < Sa; ++a) {
            vs += hv[a]; na += hcnt[2 * a]; ni += hcnt[2 * a + 1];
            if (hst[a] != CELESTE_OK && rc == CELESTE_OK) rc = hst[a];
        }
        if (v) *v = vs;
        if (n_active_px) *n_active_px = na;
        if (n_inactive_px) *n_inactive_px = ni;
        if (want_grad) memcpy(d, hd.data(), hd.size() * sizeof(double));   // P x Sa, column per active source
        if (want_hess) {
            memset(h, 0, PT * PT * sizeof(double));
            for (int a = 0; a < Sa; ++a)
                for (int j = 0; j < CEL_P; ++j) for (int i = 0; i < CEL_P; ++i)
                    h[(CEL_P * a + i) + PT * (CEL_P * a + j)] = hh[(size_t)a * CEL_P * CEL_P + i + CEL_P * j];
            for (size_t k = 0; k < np; ++k)
                for (int p2 = 0; p2 < LIFT_NP; ++p2) for (int p1 = 0; p1 < LIFT_NP; ++p1) {
                    const double x = hx[k * LIFT_NP * LIFT_NP + p1 + LIFT_NP * p2];   // d2 / d theta_a[p1] d theta_b[p2]
                    if (!std::isfinite(x) && rc == CELESTE_OK) rc = CELESTE_ERR_NONFINITE_RESULT;
                    h[(CEL_P * pia[k] + p1) + PT * (CEL_P * pib[k] + p2)] = x;
                    h[(CEL_P * pib[k] + p2) + PT * (CEL_P * pia[k] + p1)] = x;
                }
        }
    }
done:
#undef MU_TRY
    (void)hipStreamSynchronize(c->stream);   // nothing of this call is in flight when it returns
    return rc;
} ABI_CATCH

extern "C" int celeste_ctx_enable_timing(celeste_ctx_t *c, int enable) try {
    if (!c) return CELESTE_ERR_INVALID_ARG;
    if (enable && !c->ev[4]) {      // (created on first use; the caller's current device is left as it was)
        int prev = -1;
        (void)hipGetDevice(&prev);
        HIP_TRY(hipSetDevice(c->device));
        for (int i = 0; i < 5; ++i) if (!c->ev[i]) HIP_TRY(hipEventCreate(&c->ev[i]));
        if (prev >= 0 && prev != c->device) HIP_TRY(hipSetDevice(prev));
    }
    c->timing = enable ? 1 : 0;
    c->ev_valid = 0;
    return CELESTE_OK;
} ABI_CATCH

extern "C" int celeste_ctx_last_kernel_ms(celeste_ctx_t *c, float ms[3]) try {
    if (!c || !ms || !c->ev_valid) return CELESTE_ERR_INVALID_ARG;
    HIP_TRY(hipEventSynchronize(c->ev[3]));
    for (int i = 0; i < 3; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], c->ev[i], c->ev[i + 1]));
    if (c->ev_split) HIP_TRY(hipEventElapsedTime(&ms[2], c->ev[4], c->ev[3]));  // lift alone
    return CELESTE_OK;
} ABI_CATCH

extern "C" int celeste_ctx_last_record_sum_ms(celeste_ctx_t *c, float *ms) try {
    if (!c || !ms || !c->ev_valid || !c->ev_split) return CELESTE_ERR_INVALID_ARG;
    HIP_TRY(hipEventSynchronize(c->ev[3]));
    HIP_TRY(hipEventElapsedTime(ms, c->ev[2], c->ev[4]));
    return CELESTE_OK;
} ABI_CATCH

extern "C" int celeste_ctx_work_stats(celeste_ctx_t *c, int32_t n_targets, const int32_t *targets,
                                      celeste_work_stats_t *out) try {
    if (!c || !out || (n_targets > 0 && !targets)) return CELESTE_ERR_INVALID_ARG;
    memset(out, 0, sizeof *out);
    out->n_targets = n_targets;
    for (int q = 0; q < n_targets; ++q) {
        const int t = targets[q];
        if (t < 0 || t >= c->S) return CELESTE_ERR_INVALID_ARG;
        int64_t A = 0, R = 0, PC = 0;   // PC: non-empty (source, image) patches whose constants are read
        for (int v = c->h_vis_off[t]; v < c->h_vis_off[t + 1]; ++v) {
            const DevPatch &p = c->h_patches[v];
            if (p.H2 * p.W2 > 0) {
                A += (int64_t)p.H2 * p.W2;  // upper bound of visited pixels (NaN / masked pixels are skipped)
                R += p.H2;
                PC += 1;
                out->record_bytes += (int64_t)ACC_N * 8 * ((int64_t)p.H2 * p.W2 + 1);
                out->record_tiles += ((int64_t)p.H2 * p.W2 + 63) / 64;
            }
        }
        const int64_t Kn = c->h_nbr_off[t + 1] - c->h_nbr_off[t];
        for (int64_t q2 = c->h_nbr_off[t]; q2 < c->h_nbr_off[t + 1]; ++q2) {
            const int s2 = c->h_nbr_idx[q2];
            for (int v = c->h_vis_off[s2]; v < c->h_vis_off[s2 + 1]; ++v) PC += c->h_patches[v].H2 * c->h_patches[v].W2 > 0;
        }
        out->active_pixel_visits += A;
        out->patch_rows += R;
        out->neighbor_links += Kn;
        // 9 A + 4 R + 352 (1 + K) + 200 per (source, image) patch of the target and its neighbours
        // (= 200 N (1 + K) when every source is in every image) + 8288
        out->algorithmic_bytes += 9 * A + 4 * R + 352 * (1 + Kn) + 200 * PC + 8288;
    }
    return CELESTE_OK;
} ABI_CATCH

extern "C" int celeste_ctx_spline_coefficients(celeste_ctx_t *c, int32_t stamp, double *coef53) try {
    if (!c || !coef53 || stamp < 0 || stamp >= c->n_stamps) return CELESTE_ERR_INVALID_ARG;
    int st = select_device(c->device);
    if (st != CELESTE_OK) return st;
    HIP_TRY(hipMemcpy(coef53, c->d_coefs + (size_t)stamp * CEL_COEF * CEL_COEF, sizeof(double) * CEL_COEF * CEL_COEF, hipMemcpyDeviceToHost));
    return CELESTE_OK;
} ABI_CATCH

extern "C" int celeste_psf_raster(int device, const double *psf, int32_t K, const double *rows, int32_t n_rows,
                                  const double *cols, int32_t n_cols, double *out) try {
    if (!psf || K <= 0 || !rows || !cols || n_rows <= 0 || n_cols <= 0 || !out) return CELESTE_ERR_INVALID_ARG;
    int st = select_device(device);
    if (st != CELESTE_OK) return st;
    double *d_psf = nullptr, *d_rows = nullptr, *d_cols = nullptr, *d_out = nullptr;
    st = dev_upload(&d_psf, psf, (size_t)K * 6);
    if (st == CELESTE_OK) st = dev_upload(&d_rows, rows, (size_t)n_rows);
    if (st == CELESTE_OK) st = dev_upload(&d_cols, cols, (size_t)n_cols);
    if (st == CELESTE_OK) st = dev_upload<double>(&d_out, nullptr, (size_t)n_rows * n_cols);
    if (st == CELESTE_OK) {
        const int n = n_rows * n_cols;
        hipLaunchKernelGGL(psf_raster_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, d_psf, K, d_rows, n_rows,
                           d_cols, n_cols, d_out);
        if (hipMemcpy(out, d_out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) st = CELESTE_ERR_HIP;
    }
    (void)hipFree(d_psf); (void)hipFree(d_rows); (void)hipFree(d_cols); (void)hipFree(d_out);
    return st;
} ABI_CATCH


// ---- maximize! for a batch of targets (ElboMaximize.jl:228-242; neighbours frozen at the input vp) ----------
// Two drivers of the same device functions:
//  * fused (optim_fused_kernel, fused_kernels.h): ONE persistent launch in which every target iterates at its own pace --
//    the default for batches of up to FUSED_AUTO_MAX targets (Cyclades layers, a rank's shard at N >= 4), where the chained
//    driver's four dependent launches per Newton iteration leave the chip idle;
//  * chained: work list -> pixel_kernel -> lift_kernel -> optim_step_kernel per Newton iteration, all targets in
//    lock-step, for large batches that fill the chip kernel by kernel.  Its Newton loop is device resident: the host
//    enqueues iteration `it` while the device is still two iterations behind, sizing the grids by the number of
//    unconverged targets two iterations ago (an upper bound: the count never grows); the true count lives in device
//    memory and the kernels that depend on it read it there.  The counts come back through page-locked slots with an
//    event each, so the host never waits for the iteration it just enqueued.
// Results are bit-identical (tests/test_gpu_fused.py).  CELESTE_OPT_FUSED=0 / 1 forces one or the other.
#define FUSED_SMALL_TARGETS 160    // batches up to this size run the fused launch with one workgroup per CU (measured: 96 ... 256 alike, 400 loses)
#define FUSED_AUTO_MAX 880          // (measured, config 3, end of round 4: 500 targets 9.1 vs 11.2 ms chained, 750: 12.5 vs 13.1, 1000: 16.2 vs 15.6)
#define JOINT_DATAFLOW_WIDEST 4096  // widest layer of a schedule that still runs as one dataflow launch (measured: 3821 -> 0.158 s against 0.185 layer by layer; 14 782 -> 0.64 against 0.52)

// per-target buffers of the optimiser at capacity >= n
static int optim_buffers(celeste_ctx_t *c, size_t n, hipStream_t stream) {
    auto &ob = c->opt;
    const size_t vp_bytes = (size_t)c->S * CEL_P * sizeof(double);
    if (n > ob.cap) {   // (re)allocate every per-target buffer at the new capacity
        void **grow[] = {(void **)&ob.d_v, (void **)&ob.d_d, (void **)&ob.d_h, (void **)&ob.d_H, (void **)&ob.d_pos,
                         (void **)&ob.d_targets, (void **)&ob.d_act[0], (void **)&ob.d_act[1], (void **)&ob.d_evt[0],
                         (void **)&ob.d_evt[1], (void **)&ob.d_st, &ob.d_state, (void **)&ob.d_T, (void **)&ob.d_S};
        const size_t bytes[] = {sizeof(double), CEL_P * sizeof(double), CEL_P * CEL_P * sizeof(double), NF * NF * sizeof(double),
                                2 * sizeof(double), sizeof(int32_t), sizeof(int32_t), sizeof(int32_t), sizeof(int32_t),
                                sizeof(int32_t), sizeof(int32_t), sizeof(OptState), TRI_STATE * sizeof(double), 2 * SPEC_STATE * sizeof(double)};
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        ob.cap = 0;
        for (int k = 0; k < 14; ++k) {
            if (*grow[k]) { (void)hipFree(*grow[k]); *grow[k] = nullptr; }
            HIP_TRY(hipMalloc(grow[k], n * bytes[k]));
        }
        if (ob.h_state) { staging_free(ob.h_state); ob.h_state = nullptr; }
        HIP_TRY(staging_alloc(&ob.h_state, n * sizeof(OptState)));
        ob.cap = n;
    }
    if (!ob.d_vp) HIP_TRY(hipMalloc((void **)&ob.d_vp, vp_bytes));
    if (!ob.d_count) HIP_TRY(hipMalloc((void **)&ob.d_count, 3 * sizeof(int32_t)));   // two counters + blocks_done
    if (!ob.h_vp) HIP_TRY(staging_alloc((void **)&ob.h_vp, 2 * vp_bytes));
    if (!ob.h_count) {
        HIP_TRY(staging_alloc((void **)&ob.h_count, celeste_ctx::OptBuffers::RING * sizeof(int32_t)));
        for (int k = 0; k < celeste_ctx::OptBuffers::RING; ++k) HIP_TRY(hipEventCreateWithFlags(&ob.ev[k], hipEventDisableTiming));
    }
    return CELESTE_OK;
}

// the neighbours of the batch's targets as they act during the optimisation: rendered once, from the table at d_table
// (ParallelRun.process_source, ParallelRun.jl:468-498), together with the batch's bookkeeping
static int optim_render(celeste_ctx_t *c, const double *d_table, int32_t n_targets, const int32_t *d_targets,
                        int64_t n_chunks, hipStream_t stream) {
    return launch_eval(c, d_table, n_targets, d_targets, 0, c->opt.d_v, nullptr, nullptr, nullptr, c->opt.d_st, stream, true,
                       nullptr, n_chunks, false, nullptr, false, /*render_only=*/true);
}

// how the batch is optimised: 1 = fused launch, 0 = chained
static bool optim_use_fused(celeste_ctx_t *c, int32_t n_targets, int64_t n_chunks, const OptParams &op, bool any_size = false) {
    int mode = -1;
    if (const char *e = getenv("CELESTE_OPT_FUSED")) mode = atoi(e);
    if (mode == 0) return false;
    const int64_t rec = n_chunks >= 0 ? n_chunks : std::min<int64_t>((int64_t)n_targets * c->max_src_chunks, (int64_t)n_targets * c->M * c->CH);
    const int64_t q = (rec + n_targets) * ((int64_t)op.max_iters + 2) + 4096;
    if (q > (int64_t)1 << 28) return false;   // a queue of more than 1 GiB of tickets: lock-step is the better tool
    if (mode == 1 || any_size) return true;
    return n_targets <= FUSED_AUTO_MAX;
}

// The fused launch.  The targets have been initialised (optim_init_kernel) and rendered (optim_render) on `stream`;
// asynchronous.  c->fused.h_ctl[FQC_ABORT] != 0 after the stream has drained: the launch gave up (see fused_kernels.h).
// joint mode (celeste_joint_infer): the entries' dependency counters and successor lists, per-entry scratch
struct JointLaunch {
    int32_t *d_dep; const int32_t *d_succ_off, *d_succ; int32_t *d_render_arr; double *d_saved; const double *d_pos;
    int gshift; size_t render_groups;   // bits of a render-group index; groups of the whole schedule
};
static int optim_run_fused(celeste_ctx_t *c, double *d_vp, int32_t n_targets, const int32_t *d_targets, int64_t n_chunks,
                           const OptParams &op, uint32_t flags, hipStream_t stream, const JointLaunch *J = nullptr) {
    auto &fb = c->fused;
    auto &ob = c->opt;
    const size_t n = (size_t)n_targets;
    const size_t rec = (size_t)(n_chunks >= 0 ? n_chunks
                                              : std::min<int64_t>((int64_t)n_targets * c->max_src_chunks, (int64_t)n_targets * c->M * c->CH));
    if (!fb.max_resident) {
        int per_cu = 0, cus = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, optim_fused_kernel<true>, FUSED_NT, 0));
        HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
        fb.max_resident = std::max(1, std::min(per_cu, 2) * cus);
        fb.cus = cus;
        if (const char *e = getenv("CELESTE_FUSED_GRID")) if (atoi(e) > 0) fb.max_resident = atoi(e);
    }
    // A small batch (one layer of a Cyclades schedule: 80 targets, ~900 records) gets ONE workgroup per CU: its wavefronts then
    // have their SIMDs to themselves in every phase (a chunk item takes 6 us instead of 11 next to a second workgroup's), and the
    // launch is latency-bound -- 86.7 -> 81.5 us per Newton iteration of the layer.  Larger batches need the second workgroup's
    // throughput (the joint schedule of config 3: 0.060 s with two per CU, 0.079 s with one; layers of up to 400: 0.183 s against
    // 0.171 layer by layer).  CELESTE_FUSED_SMALL overrides the threshold, CELESTE_FUSED_GRID the grid.
    static const int small_targets = getenv("CELESTE_FUSED_SMALL") ? atoi(getenv("CELESTE_FUSED_SMALL")) : FUSED_SMALL_TARGETS;
    size_t resident = (size_t)fb.max_resident;
    if (!J && n_targets <= small_targets && fb.cus > 0 && !getenv("CELESTE_FUSED_GRID")) resident = std::min<size_t>(resident, (size_t)fb.cus);
    const int G = (int)std::max<size_t>(1, std::min<size_t>(resident, rec + n));
    const size_t q_cap = (rec + n) * ((size_t)op.max_iters + 2) + (J ? n + J->render_groups : 0) + (size_t)G + 64;
    if (q_cap > 0x7fffffffull) return CELESTE_ERR_INVALID_ARG;
    { int stb = fused_buffers(c, n, rec, stream); if (stb != CELESTE_OK) return stb; }
    if (q_cap > fb.cap_q) {
        HIP_TRY(hipStreamSynchronize(stream));
        if (fb.d_q_items) { (void)hipFree(fb.d_q_items); fb.d_q_items = nullptr; }
        fb.cap_q = 0;
        HIP_TRY(hipMalloc((void **)&fb.d_q_items, q_cap * sizeof(int32_t)));
        fb.cap_q = q_cap;
    }
    if (!fb.d_q_ctl) HIP_TRY(hipMalloc((void **)&fb.d_q_ctl, FQC_WORDS * sizeof(int32_t)));
    if (!fb.h_ctl) HIP_TRY(staging_alloc((void **)&fb.h_ctl, FQC_WORDS * sizeof(int32_t)));
    // every polled word is reset before every launch
    HIP_TRY(hipMemsetAsync(fb.d_q_items, 0xFF, q_cap * sizeof(int32_t), stream));
    HIP_TRY(hipMemsetAsync(fb.d_q_ctl, 0, FQC_WORDS * sizeof(int32_t), stream));
    HIP_TRY(hipMemsetAsync(fb.d_arrivals, 0, n * sizeof(int32_t), stream));
    fb.arrivals_dirty = true;      // (clean again only if the launch runs to its end: eval_fused re-checks)
    hipLaunchKernelGGL(fused_setup_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, d_targets, n_targets,
                       c->d_patches, c->d_vis_off, c->dense ? nullptr : c->d_items, c->N, c->M, c->chunk_px, c->d_rec_off,
                       fb.d_chunk_desc, fb.d_tgt_rec, fb.d_q_items, fb.d_q_ctl, J ? J->d_dep : nullptr, (int)rec);
    FusedArgs A;
    fused_args_tables(c, A);
    A.targets = d_targets; A.n_targets = n_targets; A.vp = d_vp;
    A.chunk_desc = fb.d_chunk_desc; A.tgt_rec = fb.d_tgt_rec;
    A.st = (OptState *)ob.d_state; A.Hstate = ob.d_H; A.Tstate = ob.d_T; A.op = op; A.flags = flags;
    A.Spec = ob.d_S;
    if (const char *e = getenv("CELESTE_FUSED_SPEC")) if (atoi(e) == 0) A.Spec = nullptr;
    if (A.Spec) HIP_TRY(hipMemsetAsync(ob.d_S, 0xFF, n * 2 * SPEC_STATE * sizeof(double), stream));   // no tag matches an iteration
    if (J) {
        A.j_R = (int)rec; A.j_gshift = J->gshift; A.j_dep = J->d_dep; A.j_succ_off = J->d_succ_off; A.j_succ = J->d_succ;
        A.j_vitem_off = c->d_vitem_off; A.j_vitems = c->d_vitems_src; A.j_render_arr = J->d_render_arr; A.j_saved = J->d_saved;
        A.j_pos = J->d_pos; A.j_srcimg = c->d_srcimg; A.j_comps = c->d_comps; A.j_geo = c->d_geo;
    }
    A.q_items = fb.d_q_items; A.q_ctl = fb.d_q_ctl; A.arrivals = fb.d_arrivals; A.q_cap = (int)std::min<size_t>(q_cap, 0x7fffffff);
    double tmo_s = 10.0;
    if (const char *e = getenv("CELESTE_FUSED_TIMEOUT_S")) if (atof(e) > 0) tmo_s = atof(e);
    A.timeout_ticks = (long long)(tmo_s * 1e8);   // wall_clock64: 100 MHz
    if (J) hipLaunchKernelGGL(optim_fused_kernel<true>, dim3((unsigned)G), dim3(FUSED_NT), 0, stream, A);
    else hipLaunchKernelGGL(optim_fused_kernel<false>, dim3((unsigned)G), dim3(FUSED_NT), 0, stream, A);
    HIP_TRY(hipMemcpyAsync(fb.h_ctl, fb.d_q_ctl, FQC_WORDS * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipGetLastError());
    return CELESTE_OK;
}

// The chained driver.  Blocks the host until the batch has converged.
static int optim_run_chained(celeste_ctx_t *c, double *d_vp, int32_t n_targets, const int32_t *d_targets, const OptParams &op,
                             uint32_t flags, hipStream_t stream) {
    auto &ob = c->opt;
    const size_t n = (size_t)n_targets;
    double *const d_v = ob.d_v, *const d_d = ob.d_d, *const d_h = ob.d_h, *const d_H = ob.d_H;
    int32_t *const d_st = ob.d_st;
    int32_t *const d_cnt[2] = {ob.d_count, ob.d_count + 1};
    int32_t *const *d_act = ob.d_act, *const *d_evt = ob.d_evt;
    OptState *const d_state = (OptState *)ob.d_state;
    constexpr int RING = celeste_ctx::OptBuffers::RING;
    HIP_TRY(hipMemsetAsync(ob.d_count, 0, 3 * sizeof(int32_t), stream));   // (an earlier call may have stopped mid-loop)
    // both lists start as the full target list: the step kernel only rewrites the first *next_count entries of the other
    // list, and the launches are sized by a count two iterations old -- entries past the live count must be valid ids
    HIP_TRY(hipMemcpyAsync(d_evt[0], d_targets, n * sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_evt[1], d_targets, n * sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
    int32_t n_upper = n_targets;
    int cur = 0;
    for (int it = 0; it <= op.max_iters + 1; ++it) {
        if (it >= 2) {   // the count two iterations back: an upper bound of the live targets, 0 = all converged
            HIP_TRY(hipEventSynchronize(ob.ev[(it - 2) % RING]));
            n_upper = ob.h_count[(it - 2) % RING];
            if (n_upper <= 0) break;
        }
        const int32_t *d_live = it == 0 ? nullptr : d_cnt[cur];
        int st1 = launch_eval(c, d_vp, n_upper, d_evt[cur], flags, d_v, d_d, d_h, nullptr, d_st, stream, false, nullptr,
                              -1, false, d_live);
        if (st1 != CELESTE_OK) return st1;
        hipLaunchKernelGGL(optim_step_kernel, dim3(n_upper), dim3(64), 0, stream, d_vp, d_targets, d_act[cur],
                           d_v, d_d, d_h, d_st, op, d_state, d_H, d_act[1 - cur], d_evt[1 - cur], d_cnt[1 - cur],
                           it == 0 ? nullptr : d_cnt[cur], ob.d_count + 2, &ob.h_count[it % RING], ob.d_T);
        HIP_TRY(hipEventRecord(ob.ev[it % RING], stream));
        cur = 1 - cur;
    }
    return CELESTE_OK;
}

// maximize! of the targets against the table at d_vp (rendering done): save the rows, initialise, run, write the
// per-target outputs (device pointers, may be NULL) and give failed targets their rows back.  *fused_out: which driver.
static int optim_run(celeste_ctx_t *c, double *d_vp, const double *d_pos, int32_t n_targets, const int32_t *d_targets,
                     int64_t n_chunks, const OptParams &op, uint32_t flags, int32_t *d_iterations, int32_t *d_f_evals,
                     double *d_elbo, int32_t *d_status, hipStream_t stream, bool *fused_out) {
    auto &ob = c->opt;
    auto &fb = c->fused;
    const size_t n = (size_t)n_targets;
    if (n * CEL_P > fb.cap_saved) {
        HIP_TRY(hipStreamSynchronize(stream));
        if (fb.d_saved) { (void)hipFree(fb.d_saved); fb.d_saved = nullptr; }
        fb.cap_saved = 0;
        HIP_TRY(hipMalloc((void **)&fb.d_saved, n * CEL_P * sizeof(double)));
        fb.cap_saved = n * CEL_P;
    }
    hipLaunchKernelGGL(save_rows_kernel, dim3((unsigned)((n * CEL_P + 255) / 256)), dim3(256), 0, stream, d_vp, d_targets,
                       n_targets, fb.d_saved);
    // (no reduced form yet: NaN everywhere -- the first sub-problem of every target starts its eigenvalue search cold)
    HIP_TRY(hipMemsetAsync(ob.d_T, 0xFF, n * TRI_STATE * sizeof(double), stream));
    hipLaunchKernelGGL(optim_init_kernel, dim3((n_targets + 63) / 64), dim3(64), 0, stream, d_vp, d_targets, n_targets, op,
                       (OptState *)ob.d_state, ob.d_act[0], d_pos);
    const bool fused = optim_use_fused(c, n_targets, n_chunks, op);
    if (fused_out) *fused_out = fused;
    int st = fused ? optim_run_fused(c, d_vp, n_targets, d_targets, n_chunks, op, flags, stream)
                   : optim_run_chained(c, d_vp, n_targets, d_targets, op, flags, stream);
    if (st != CELESTE_OK) return st;
    hipLaunchKernelGGL(optim_finalize_kernel, dim3((n_targets + 63) / 64), dim3(64), 0, stream, (const OptState *)ob.d_state,
                       d_targets, n_targets, d_vp, fb.d_saved, d_iterations, d_f_evals, d_elbo, d_status,
                       fused ? fb.d_q_ctl : nullptr);
    HIP_TRY(hipGetLastError());
    return CELESTE_OK;
}

// did the last fused launch on this context give up?  (after the stream has been synchronised)
static int fused_abort_status(celeste_ctx_t *c) {
    const int code = c->fused.h_ctl ? c->fused.h_ctl[FQC_ABORT] : 0;
    if (code == 0) return CELESTE_OK;
    fprintf(stderr, "celeste_mi355x: the fused optimiser launch gave up (%s)\n",
            code == 1 ? "a workgroup waited longer than CELESTE_FUSED_TIMEOUT_S for work" : "queue capacity exceeded");
    return CELESTE_ERR_HIP;
}

extern "C" int celeste_maximize_batch_device(celeste_ctx_t *c, double *d_vp, const double *d_vp_neighbors,
                                             const double *d_pos_centers, int32_t n_targets, const int32_t *d_targets,
                                             const celeste_optim_config_t *cfg_in, int32_t *d_iterations, int32_t *d_f_evals,
                                             double *d_elbo, int32_t *d_status, void *stream_) try {
    if (!c || !d_vp || !d_targets || n_targets < 0) return CELESTE_ERR_INVALID_ARG;
    if (n_targets == 0) return CELESTE_OK;
    OptParams op;
    uint32_t flags;
    int st = optim_config(cfg_in, &op, &flags);
    if (st != CELESTE_OK) return st;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = (hipStream_t)stream_;
    st = optim_buffers(c, (size_t)n_targets, stream);
    if (st != CELESTE_OK) return st;
    st = optim_render(c, d_vp_neighbors ? d_vp_neighbors : d_vp, n_targets, d_targets, -1, stream);
    if (st != CELESTE_OK) return st;
    return optim_run(c, d_vp, d_pos_centers, n_targets, d_targets, -1, op, flags, d_iterations, d_f_evals, d_elbo, d_status,
                     stream, nullptr);
} ABI_CATCH

static int check_distinct_targets(celeste_ctx_t *c, int32_t n, const int32_t *targets, std::vector<uint8_t> &seen) {
    seen.assign((size_t)c->S, 0);   // two optimisations of one source would share its row of vp
    for (int t = 0; t < n; ++t) {
        if (targets[t] < 0 || targets[t] >= c->S || seen[targets[t]]) return CELESTE_ERR_INVALID_ARG;
        seen[targets[t]] = 1;
    }
    return CELESTE_OK;
}

extern "C" int celeste_maximize_batch(celeste_ctx_t *c, double *vp, const double *vp_neighbors,
                                      const double *pos_centers, int32_t n_targets, const int32_t *targets,
                                      const celeste_optim_config_t *cfg_in, int32_t *iterations, int32_t *f_evals,
                                      double *elbo, int32_t *status) try {
    if (!c || !vp || !targets || n_targets < 0) return CELESTE_ERR_INVALID_ARG;
    if (n_targets == 0) return CELESTE_OK;
    std::vector<uint8_t> seen;
    if (check_distinct_targets(c, n_targets, targets, seen) != CELESTE_OK) return CELESTE_ERR_INVALID_ARG;
    OptParams op;
    uint32_t flags;
    int rc = optim_config(cfg_in, &op, &flags);
    if (rc != CELESTE_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)n_targets;
    const size_t vp_bytes = (size_t)c->S * CEL_P * sizeof(double);
    auto &ob = c->opt;
    hipStream_t stream = c->stream;
    rc = optim_buffers(c, n, stream);
    if (rc != CELESTE_OK) return rc;
    int64_t n_chunks = 0;
    for (int t = 0; t < n_targets; ++t) n_chunks += c->h_src_chunks[targets[t]];
#define MX_TRY(expr) do { if ((expr) != hipSuccess) { rc = CELESTE_ERR_HIP; goto cleanup; } } while (0)
    {
    double *const d_vp = ob.d_vp;
    double *const d_pos = pos_centers ? ob.d_pos : nullptr;
    int32_t *const d_targets = ob.d_targets;
    double *const h_vp0 = ob.h_vp, *const h_vp1 = ob.h_vp + (size_t)c->S * CEL_P;
    MX_TRY(hipMemcpyAsync(d_targets, targets, n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    if (pos_centers) MX_TRY(hipMemcpyAsync(d_pos, pos_centers, n * 2 * sizeof(double), hipMemcpyHostToDevice, stream));
    // neighbours are rendered once, from their frozen parameters, before any target moves
    memcpy(h_vp0, vp_neighbors ? vp_neighbors : vp, vp_bytes);
    MX_TRY(hipMemcpyAsync(d_vp, h_vp0, vp_bytes, hipMemcpyHostToDevice, stream));
    rc = optim_render(c, d_vp, n_targets, d_targets, n_chunks, stream);
    if (rc != CELESTE_OK) goto cleanup;
    if (vp_neighbors) {
        memcpy(h_vp1, vp, vp_bytes);
        MX_TRY(hipMemcpyAsync(d_vp, h_vp1, vp_bytes, hipMemcpyHostToDevice, stream));
    }
    bool fused = false;
    rc = optim_run(c, d_vp, d_pos, n_targets, d_targets, n_chunks, op, flags, nullptr, nullptr, nullptr, nullptr, stream, &fused);
    if (rc != CELESTE_OK) goto cleanup;
    OptState *const hs = (OptState *)ob.h_state;
    MX_TRY(hipMemcpyAsync(hs, ob.d_state, n * sizeof(OptState), hipMemcpyDeviceToHost, stream));
    MX_TRY(hipMemcpyAsync(h_vp0, d_vp, vp_bytes, hipMemcpyDeviceToHost, stream));
    MX_TRY(hipStreamSynchronize(stream));
    if (fused && (rc = fused_abort_status(c)) != CELESTE_OK) goto cleanup;
    for (int t = 0; t < n_targets; ++t) {
        // a target that failed keeps its input row; the others are unaffected (ParallelRun.jl:582-597)
        if (hs[t].status == CELESTE_OK)
            memcpy(vp + (size_t)targets[t] * CEL_P, h_vp0 + (size_t)targets[t] * CEL_P, CEL_P * sizeof(double));
        if (iterations) iterations[t] = hs[t].iter;
        if (f_evals) f_evals[t] = hs[t].evals;
        if (elbo) elbo[t] = -hs[t].f;
        if (status) status[t] = hs[t].status;
        if (hs[t].status != CELESTE_OK && rc == CELESTE_OK) rc = hs[t].status;
    }
    }
cleanup:
#undef MX_TRY
    if (rc == CELESTE_ERR_HIP) (void)hipStreamSynchronize(stream);
    return rc;
} ABI_CATCH


// ---- joint inference as ONE launch: the schedule's entries as a dataflow (fused_kernels.h, joint mode) ----------------
#define JOINT_DATAFLOW_MAX 262144
// *ran = false (and CELESTE_OK): the schedule does not fit the launch's encodings -- the caller runs it layer by layer
// d_table: the parameter table the schedule runs against (n_sources x 44, HBM); d_restore: a device copy of it as it was on
// entry (the launch may give up half way -- queue capacity -- and the layered driver then starts from the entry state)
static int joint_dataflow(celeste_ctx_t *c, double *d_table, const double *d_restore, int64_t total, const int32_t *targets,
                          const int32_t *d_all, const double *d_pos,
                          const OptParams &op, uint32_t flags, int32_t *d_it, int32_t *d_ev, double *d_el, int32_t *d_stt,
                          hipStream_t stream, bool *ran) {
    *ran = false;
    const int E = (int)total;
    // a flattened schedule too large for one batch's index space (launch_eval's n_targets x M x CH bound) is a limit of THIS
    // driver, not of the call: the caller runs it layer by layer.  Every other CELESTE_ERR_INVALID_ARG below is an error.
    if ((size_t)E * c->M * c->CH > 0x7fffffffull) return CELESTE_OK;
    auto &ob = c->opt;
    auto &fb = c->fused;
    // An entry waits for the last earlier entry that wrote a row it reads -- its source's, its neighbours' -- and for
    // the earlier entries that read the row it writes: the order the layer-by-layer schedule enforces with barriers.
    std::vector<int32_t> last((size_t)c->S, -1), dep((size_t)E, 0), deps;
    std::vector<std::vector<int32_t>> readers((size_t)c->S), succ((size_t)E);
    int64_t n_chunks = 0;
    size_t groups = 0, gmax = 1;
    for (int e = 0; e < E; ++e) {
        const int t = targets[e];
        deps.clear();
        if (last[t] >= 0) deps.push_back(last[t]);
        for (int64_t q = c->h_nbr_off[t]; q < c->h_nbr_off[t + 1]; ++q) if (last[c->h_nbr_idx[q]] >= 0) deps.push_back(last[c->h_nbr_idx[q]]);
        deps.insert(deps.end(), readers[t].begin(), readers[t].end());
        std::sort(deps.begin(), deps.end());
        deps.erase(std::unique(deps.begin(), deps.end()), deps.end());
        for (int32_t d : deps) succ[(size_t)d].push_back(e);
        dep[(size_t)e] = (int32_t)deps.size();
        last[t] = e;
        readers[t].clear();
        for (int64_t q = c->h_nbr_off[t]; q < c->h_nbr_off[t + 1]; ++q) readers[c->h_nbr_idx[q]].push_back(e);
        n_chunks += c->h_src_chunks[t];
        const size_t g = ((size_t)(c->h_vitem_off[t + 1] - c->h_vitem_off[t]) + FUSED_WAVES - 1) / FUSED_WAVES;
        groups += g; gmax = std::max(gmax, g);
    }
    std::vector<int32_t> succ_off((size_t)E + 1, 0), succ_flat;
    size_t most = 0;
    for (int e = 0; e < E; ++e) {
        succ_off[(size_t)e + 1] = succ_off[(size_t)e] + (int32_t)succ[(size_t)e].size();
        succ_flat.insert(succ_flat.end(), succ[(size_t)e].begin(), succ[(size_t)e].end());
        most = std::max(most, succ[(size_t)e].size());
    }
    int gshift = 1;
    while (((size_t)1 << gshift) < gmax) ++gshift;
    // item codes are int32: records, then one START per entry, then (entry, render group); the ready list of an ending
    // entry is staged in 2048 LDS words
    if (most > 2048 || (uint64_t)n_chunks + (uint64_t)E + ((uint64_t)E << gshift) >= 0x7fffffffull) return CELESTE_OK;
    if (!optim_use_fused(c, E, n_chunks, op, /*any_size=*/true)) return CELESTE_OK;
    int32_t *d_dep = nullptr, *d_succ_off = nullptr, *d_succ = nullptr, *d_rarr = nullptr;
    int rc = CELESTE_OK;
#define JD_TRY(expr) do { if ((expr) != hipSuccess) { rc = CELESTE_ERR_HIP; goto out; } } while (0)
    // (kept between calls: a schedule per box is the normal use)
    JD_TRY(scratch_get(c, 19, (size_t)E * sizeof(int32_t), &d_dep));
    JD_TRY(scratch_get(c, 20, ((size_t)E + 1) * sizeof(int32_t), &d_succ_off));
    JD_TRY(scratch_get(c, 21, std::max<size_t>(succ_flat.size(), 1) * sizeof(int32_t), &d_succ));
    JD_TRY(scratch_get(c, 22, (size_t)E * sizeof(int32_t), &d_rarr));
    if ((size_t)E * CEL_P > fb.cap_saved) {
        JD_TRY(hipStreamSynchronize(stream));
        if (fb.d_saved) { (void)hipFree(fb.d_saved); fb.d_saved = nullptr; }
        fb.cap_saved = 0;
        JD_TRY(hipMalloc((void **)&fb.d_saved, (size_t)E * CEL_P * sizeof(double)));
        fb.cap_saved = (size_t)E * CEL_P;
    }
    JD_TRY(hipMemcpyAsync(d_dep, dep.data(), (size_t)E * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    JD_TRY(hipMemcpyAsync(d_succ_off, succ_off.data(), ((size_t)E + 1) * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    if (!succ_flat.empty())
        JD_TRY(hipMemcpyAsync(d_succ, succ_flat.data(), succ_flat.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    JD_TRY(hipMemsetAsync(d_rarr, 0, (size_t)E * sizeof(int32_t), stream));
    // the batch's bookkeeping for all entries (visit items, record offsets), every source's tables and shape derivatives
    // from the input table; the entries refresh them as they end
    rc = optim_render(c, d_table, E, d_all, n_chunks, stream);
    if (rc != CELESTE_OK) goto out;
    {
        JD_TRY(hipMemsetAsync(ob.d_T, 0xFF, (size_t)E * TRI_STATE * sizeof(double), stream));
        JointLaunch J = {d_dep, d_succ_off, d_succ, d_rarr, fb.d_saved, d_pos, gshift, groups};
        rc = optim_run_fused(c, d_table, E, d_all, n_chunks, op, flags, stream, &J);
        if (rc != CELESTE_OK) goto out;
        // (failed entries gave their rows back in flight: no saved rows here)
        hipLaunchKernelGGL(optim_finalize_kernel, dim3((unsigned)((E + 63) / 64)), dim3(64), 0, stream, (const OptState *)ob.d_state,
                           d_all, E, d_table, (const double *)nullptr, d_it, d_ev, d_el, d_stt, fb.d_q_ctl);
        JD_TRY(hipGetLastError());
        JD_TRY(hipStreamSynchronize(stream));      // (the host vectors above are in flight until here)
        if (fb.h_ctl && fb.h_ctl[FQC_ABORT] == 2) {
            // the launch ran out of queue capacity (a time-out stays an error: something is wrong with the device): the
            // table is partly optimised -- put the entry state back and let the layered driver run the schedule
            JD_TRY(hipMemcpyAsync(d_table, d_restore, (size_t)c->S * CEL_P * sizeof(double), hipMemcpyDefault, stream));
            fb.h_ctl[FQC_ABORT] = 0;               // (the layered driver's own launches set it again if THEY give up)
            goto out;
        }
        *ran = true;
    }
out:
#undef JD_TRY
    if (rc != CELESTE_OK) (void)hipStreamSynchronize(stream);
    return rc;
}

// ---- joint inference: a schedule of layers against one device-resident parameter table -------------------------
// The schedule against the table at d_table (n_sources x 44, HBM, updated in place).  d_entry: a device snapshot of the
// table as it is on entry, or nullptr -- then ob.h_vp (page-locked) must hold it.  Blocks until the schedule is done; the
// per-entry outputs are host pointers (may be NULL).
static int joint_run(celeste_ctx_t *c, double *d_table, const double *d_entry, int32_t n_layers, const int64_t *layer_offsets,
                     const int32_t *layer_targets, const double *pos_centers, const celeste_optim_config_t *cfg_in,
                     int32_t *iterations, int32_t *f_evals, double *elbo, int32_t *status, bool validate) {
    const int64_t total = layer_offsets[n_layers];
    size_t widest = 0;
    std::vector<uint8_t> seen;
    std::vector<int64_t> layer_chunks((size_t)n_layers, 0);
    for (int l = 0; l < n_layers; ++l) {
        const int64_t lo = layer_offsets[l], hi = layer_offsets[l + 1];
        if (hi < lo || hi - lo > 0x7fffffff) return CELESTE_ERR_INVALID_ARG;
        if (validate && check_distinct_targets(c, (int32_t)(hi - lo), layer_targets + lo, seen) != CELESTE_OK) return CELESTE_ERR_INVALID_ARG;
        // the sources of a layer are optimised simultaneously: none may be another's neighbour
        for (int64_t e = lo; e < hi; ++e) {
            const int t = layer_targets[e];
            if (validate)
                for (int64_t q = c->h_nbr_off[t]; q < c->h_nbr_off[t + 1]; ++q) if (seen[c->h_nbr_idx[q]]) return CELESTE_ERR_INVALID_ARG;
            layer_chunks[l] += c->h_src_chunks[t];
        }
        widest = std::max(widest, (size_t)(hi - lo));
    }
    if (total == 0) return CELESTE_OK;
    OptParams op;
    uint32_t flags;
    int rc = optim_config(cfg_in, &op, &flags);
    if (rc != CELESTE_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = c->stream;
    // One dataflow launch for the whole schedule when its layers are of the size the fused launch is the better driver
    // for (Cyclades batches); schedules with huge layers (a greedy colouring of a 30 000-source scene: 15 000 sources in
    // the first) run layer by layer, where the lock-step kernels spend half the chip time per evaluation (measured on
    // config 5's scene: colouring 0.60 s layered / 0.99 s dataflow, Cyclades 2.39 s layered / 0.99 s dataflow).
    // CELESTE_JOINT_DATAFLOW=0 / 1 forces one or the other.
    const bool can_dataflow = total <= JOINT_DATAFLOW_MAX && optim_use_fused(c, 1, 1, op);
    bool dataflow = can_dataflow && widest <= JOINT_DATAFLOW_WIDEST;
    if (const char *e = getenv("CELESTE_JOINT_DATAFLOW")) dataflow = can_dataflow && atoi(e) != 0;
    rc = optim_buffers(c, dataflow ? (size_t)total : widest, stream);
    if (rc != CELESTE_OK) return rc;
    auto &ob = c->opt;
    // the whole schedule and the per-entry outputs live on the device for the duration of the call
    int32_t *d_all = nullptr, *d_it = nullptr, *d_ev = nullptr, *d_stt = nullptr;
    double *d_pos = nullptr, *d_el = nullptr;
    std::vector<int32_t> h_it((size_t)total), h_ev((size_t)total), h_st((size_t)total);
    std::vector<double> h_el((size_t)total);
    bool any_fused = false;
    int abort_rc = CELESTE_OK;
#define JI_TRY(expr) do { if ((expr) != hipSuccess) { rc = CELESTE_ERR_HIP; goto done; } } while (0)
    JI_TRY(scratch_get(c, 13, (size_t)total * sizeof(int32_t), &d_all));
    JI_TRY(scratch_get(c, 14, (size_t)total * sizeof(int32_t), &d_it));
    JI_TRY(scratch_get(c, 15, (size_t)total * sizeof(int32_t), &d_ev));
    JI_TRY(scratch_get(c, 16, (size_t)total * sizeof(int32_t), &d_stt));
    JI_TRY(scratch_get(c, 17, (size_t)total * sizeof(double), &d_el));
    if (pos_centers) JI_TRY(scratch_get(c, 18, (size_t)total * 2 * sizeof(double), &d_pos));
    JI_TRY(hipMemcpyAsync(d_all, layer_targets, (size_t)total * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    if (pos_centers) JI_TRY(hipMemcpyAsync(d_pos, pos_centers, (size_t)total * 2 * sizeof(double), hipMemcpyHostToDevice, stream));
    if (dataflow) {
        // one launch for the whole schedule (fused_kernels.h, joint mode)
        rc = joint_dataflow(c, d_table, d_entry ? d_entry : ob.h_vp, total, layer_targets, d_all, d_pos, op, flags, d_it, d_ev,
                            d_el, d_stt, stream, &dataflow);
        if (rc != CELESTE_OK) goto done;
        any_fused = dataflow;
    }
    if (!dataflow)
    for (int l = 0; l < n_layers; ++l) {
        const int64_t lo = layer_offsets[l];
        const int32_t n = (int32_t)(layer_offsets[l + 1] - lo);
        if (n == 0) continue;
        // every layer sees the table as the layers before it left it (ParallelRun.jl:372-397)
        rc = optim_render(c, d_table, n, d_all + lo, layer_chunks[l], stream);
        if (rc != CELESTE_OK) goto done;
        bool fused = false;
        rc = optim_run(c, d_table, d_pos ? d_pos + 2 * lo : nullptr, n, d_all + lo, layer_chunks[l], op, flags, d_it + lo,
                       d_ev + lo, d_el + lo, d_stt + lo, stream, &fused);
        if (rc != CELESTE_OK) goto done;
        any_fused |= fused;
    }
    JI_TRY(hipMemcpyAsync(h_it.data(), d_it, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    JI_TRY(hipMemcpyAsync(h_ev.data(), d_ev, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    JI_TRY(hipMemcpyAsync(h_st.data(), d_stt, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    JI_TRY(hipMemcpyAsync(h_el.data(), d_el, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, stream));
    JI_TRY(hipStreamSynchronize(stream));
    if (any_fused) abort_rc = fused_abort_status(c);   // (of the last fused layer; an earlier one shows in the statuses)
    for (int64_t e = 0; e < total; ++e) {
        if (h_st[e] == CELESTE_ERR_HIP) abort_rc = CELESTE_ERR_HIP;
        if (iterations) iterations[e] = h_it[e];
        if (f_evals) f_evals[e] = h_ev[e];
        if (elbo) elbo[e] = h_el[e];
        if (status) status[e] = h_st[e];
        if (h_st[e] != CELESTE_OK && rc == CELESTE_OK) rc = h_st[e];
    }
    if (abort_rc != CELESTE_OK) rc = abort_rc;
done:
#undef JI_TRY
    (void)hipStreamSynchronize(stream);
    return rc;
}

extern "C" int celeste_joint_infer(celeste_ctx_t *c, double *vp, int32_t n_layers, const int64_t *layer_offsets,
                                   const int32_t *layer_targets, const double *pos_centers,
                                   const celeste_optim_config_t *cfg_in, int32_t *iterations, int32_t *f_evals,
                                   double *elbo, int32_t *status) try {
    if (!c || !vp || n_layers < 0 || (n_layers > 0 && (!layer_offsets || !layer_targets))) return CELESTE_ERR_INVALID_ARG;
    if (n_layers == 0) return CELESTE_OK;
    if (layer_offsets[0] != 0) return CELESTE_ERR_INVALID_ARG;
    if (layer_offsets[n_layers] == 0) return CELESTE_OK;
    HIP_TRY(hipSetDevice(c->device));
    // vp is uploaded once, stays in HBM across all layers and is written back at the end
    int rc = optim_buffers(c, 1, c->stream);
    if (rc != CELESTE_OK) return rc;
    auto &ob = c->opt;
    const size_t vp_bytes = (size_t)c->S * CEL_P * sizeof(double);
    memcpy(ob.h_vp, vp, vp_bytes);
    HIP_TRY(hipMemcpyAsync(ob.d_vp, ob.h_vp, vp_bytes, hipMemcpyHostToDevice, c->stream));
    rc = joint_run(c, ob.d_vp, nullptr, n_layers, layer_offsets, layer_targets, pos_centers, cfg_in, iterations, f_evals, elbo,
                   status, true);
    // failed targets already hold their pre-layer rows (optim_finalize_kernel); a launch that gave up leaves vp untouched
    if (rc == CELESTE_OK || rc == CELESTE_ERR_NONFINITE_INPUT || rc == CELESTE_ERR_NONFINITE_RESULT) {
        double *const h_out = ob.h_vp + (size_t)c->S * CEL_P;
        if (hipMemcpyAsync(h_out, ob.d_vp, vp_bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) return CELESTE_ERR_HIP;
        memcpy(vp, h_out, vp_bytes);
    }
    return rc;
} ABI_CATCH

extern "C" int celeste_optim_stats(int reset, uint64_t out[5]) try {
    unsigned long long h[5] = {0, 0, 0, 0, 0};
    if (out) {
        HIP_TRY(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_optim_stats), sizeof h));
        for (int i = 0; i < 5; ++i) out[i] = h[i];
    }
    if (reset) { unsigned long long z[5] = {0, 0, 0, 0, 0}; HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_optim_stats), z, sizeof z)); }
    return CELESTE_OK;
} ABI_CATCH

extern "C" int celeste_tr_solve_batch(int device, int32_t n, const double *H, const double *g, const double *delta,
                                      int32_t solver, int32_t secular_iters, double *p, double *m, int32_t *interior,
                                      int32_t *fell_back) try {
    if (n < 0 || !H || !g || !delta || !p || solver < 0 || solver > 2 || secular_iters < 0) return CELESTE_ERR_INVALID_ARG;
    if (n == 0) return CELESTE_OK;
    int st = select_device(device);
    if (st != CELESTE_OK) return st;
    double *d_H = nullptr, *d_g = nullptr, *d_delta = nullptr, *d_p = nullptr, *d_m = nullptr;
    int32_t *d_i = nullptr, *d_f = nullptr;
    st = dev_upload(&d_H, H, (size_t)n * NF * NF);
    if (st == CELESTE_OK) st = dev_upload(&d_g, g, (size_t)n * NF);
    if (st == CELESTE_OK) st = dev_upload(&d_delta, delta, (size_t)n);
    if (st == CELESTE_OK) st = dev_upload<double>(&d_p, nullptr, (size_t)n * NF);
    if (st == CELESTE_OK) st = dev_upload<double>(&d_m, nullptr, (size_t)n);
    if (st == CELESTE_OK) st = dev_upload<int32_t>(&d_i, nullptr, (size_t)n);
    if (st == CELESTE_OK) st = dev_upload<int32_t>(&d_f, nullptr, (size_t)n);
    if (st == CELESTE_OK) {
        hipLaunchKernelGGL(tr_solve_kernel, dim3((unsigned)n), dim3(64), 0, nullptr, d_H, d_g, d_delta, (int)solver,
                           secular_iters > 0 ? (int)secular_iters : 20, d_p, d_m, d_i, d_f);
        std::vector<int32_t> hi((size_t)n), hf((size_t)n);
        std::vector<double> hm((size_t)n);
        if (hipMemcpy(p, d_p, (size_t)n * NF * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(hm.data(), d_m, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(hi.data(), d_i, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(hf.data(), d_f, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) st = CELESTE_ERR_HIP;
        for (int k = 0; k < n && st == CELESTE_OK; ++k) {
            if (m) m[k] = hm[k];
            if (interior) interior[k] = hi[k];
            if (fell_back) fell_back[k] = hf[k];
        }
    }
    (void)hipFree(d_H); (void)hipFree(d_g); (void)hipFree(d_delta); (void)hipFree(d_p); (void)hipFree(d_m);
    (void)hipFree(d_i); (void)hipFree(d_f);
    return st;
} ABI_CATCH

#ifdef OPTIM_DEBUG_T
extern "C" int celeste_debug_T(int32_t n, double *out) {   // n = 0: allocate for 4096 problems; n > 0: fetch n records
    static double *buf = nullptr;
    if (!buf) { HIP_TRY(hipMalloc((void **)&buf, (size_t)4096 * 4 * NF * sizeof(double))); HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_dbg_T), &buf, sizeof buf)); }
    if (n > 0) HIP_TRY(hipMemcpy(out, buf, (size_t)n * 4 * NF * sizeof(double), hipMemcpyDeviceToHost));
    return CELESTE_OK;
}
#endif
#ifdef VALUE_TIMING
extern "C" int celeste_value_clocks(int reset, uint64_t out[8]) {   // debug builds only (tools/variants)
    unsigned long long h[8] = {0};
    HIP_TRY(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_value_clk), sizeof h));
    for (int i = 0; i < 8; ++i) out[i] = h[i];
    if (reset) { unsigned long long z[8] = {0}; HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_value_clk), z, sizeof z)); }
    return CELESTE_OK;
}
#endif
#ifdef LIFT_TIMING
extern "C" int celeste_lift_clocks(int reset, uint64_t out[16]) {   // debug builds only (tools/variants)
    unsigned long long h[16] = {0};
    HIP_TRY(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_lift_clk), sizeof h));
    for (int i = 0; i < 16; ++i) out[i] = h[i];
    if (reset) { unsigned long long z[16] = {0}; HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_lift_clk), z, sizeof z)); }
    return CELESTE_OK;
}
#endif
#ifdef FUSED_TIMING
extern "C" int celeste_fused_clocks(int reset, uint64_t out[16]) {   // debug builds only (tools/variants)
    unsigned long long h[16] = {0};
    HIP_TRY(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_fused_clk), sizeof h));
    for (int i = 0; i < 16; ++i) out[i] = h[i];
    if (reset) { unsigned long long z[16] = {0}; HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_fused_clk), z, sizeof z)); }
    return CELESTE_OK;
}
#endif
#ifdef OPTIM_TIMING
extern "C" int celeste_optim_clocks(int reset, uint64_t out[16]) {   // debug builds only (tools/variants)
    unsigned long long h[16] = {0};
    HIP_TRY(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_optim_clk), sizeof h));
    for (int i = 0; i < 16; ++i) out[i] = h[i];
    if (reset) { unsigned long long z[16] = {0}; HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_optim_clk), z, sizeof z)); }
    return CELESTE_OK;
}
#endif

// ---- expected-image renderer (bin/write_celeste_expectation.jl:112-156, fsm_util.jl:349-400) ------------
extern "C" int celeste_render_expected(celeste_ctx_t *c, const double *vp, int32_t image, double *out_plane) try {
    if (!c || !vp || !out_plane || image < 0 || image >= c->N) return CELESTE_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(c->device));
    const DevImage &im = c->imgs->h_images[image];
    const size_t npix = (size_t)im.H * im.W;
    double *d_plane = nullptr;
    if (!c->d_vp) HIP_TRY(hipMalloc((void **)&c->d_vp, (size_t)c->S * CEL_P * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(c->d_vp, vp, (size_t)c->S * CEL_P * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(scratch_get(c, 12, npix * sizeof(double), &d_plane));
    int rc = CELESTE_OK;
    if (hipMemsetAsync(d_plane, 0, npix * sizeof(double), c->stream) != hipSuccess) rc = CELESTE_ERR_HIP;
    if (rc == CELESTE_OK) {
        if (c->V > 0)
            hipLaunchKernelGGL(prep_kernel, dim3((unsigned)c->V), dim3(64), 0, c->stream, c->d_vp, c->d_images,
                               c->d_patches, c->d_vis_src, c->d_vis_img, c->N, c->K, c->d_srcimg, c->d_comps, nullptr,
                               c->d_vis_off, c->M, (int)c->dense, nullptr, nullptr, 0);
        hipLaunchKernelGGL(render_kernel, dim3((unsigned)((size_t)c->S * c->CH)), dim3(64), 0, c->stream, c->d_patches,
                           c->d_coefs, c->d_bitmaps, im.pixels, c->d_srcimg, c->d_comps, (int)image, c->N, c->NC,
                           c->CH, c->chunk_px, im.H, d_plane, c->d_vis_off, c->d_vis_img, (int)c->dense);
        if (hipMemcpyAsync(out_plane, d_plane, npix * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = CELESTE_ERR_HIP;
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) rc = CELESTE_ERR_HIP;
    return rc;
} ABI_CATCH

// ---- one process, N devices (celeste_group_*) ----------------------------------------------------------------------
#include "group.h"
