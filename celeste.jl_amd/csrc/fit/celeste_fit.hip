// celeste_fit.hip -- libceleste_fit.so: per-source goodness of fit (include/celeste_fit.h).
//
// The engine's context code (engine_context.h) and its kernels' header are compiled into this library, unchanged: the patch table, the
// per-visit tables of prep_kernel, the spline coefficients, the bitmaps and the neighbour lists are the engine's, and the
// two densities are its star_value and galaxy_value.  The context, the work list and the pixel walk (the target's own light m
// and the neighbours' light B of every pixel) are engine_client.h's; this file adds two kernels.  One call:
//   prep_kernel          (the engine's) SrcImg and Comp of every visit of the context at the call's table
//   fit_pixel_kernel     one wavefront per work item; from m and B a lane forms lam, the stamp value if asked, and the seven
//                        terms; the wavefront sums them in a fixed butterfly and lane 0 writes the tile's record
//   fit_reduce_kernel    one wavefront per target adds its tile records one after another, in ascending (image, tile) order,
//                        into its band rows (lane = band x statistic) and writes its status
// A tile is 64 consecutive pixels of a patch whatever the chunk size is (chunks are multiples of 64 pixels), so the sums do not
// depend on it.  No floating-point atomics.
#include "../engine_context.h"
#include "../engine_client.h"
#include "../../../include/celeste_fit.h"

// Mutation testing (tests/test_satellite_mutants.py builds this library with -DCELESTE_FIT_MUTANT=k and checks that
// tests/test_gpu_fit.py notices).  A mutant changes arithmetic, or reads fewer records of the same array; never a size, a launch,
// a barrier or anything that could leave an array.  0 = the product;
//   1 = SELF ignores B (m / (m + B) becomes 1)
//   2 = an unvisited pixel's stamp gets lam instead of NaN
//   3 = fit_reduce_kernel adds MAX_Z instead of taking the maximum
//   4 = fit_reduce_kernel starts at tr.x + 1 when tr.y > 1: the first tile is dropped (a later start inside [tr.x, tr.x + tr.y))
//   5 = the tiles' bad flag is not reported: never NONFINITE_RESULT
// Never defined in the shipped build.
#ifndef CELESTE_FIT_MUTANT
#define CELESTE_FIT_MUTANT 0
#endif

#define FIT_NB CELESTE_FIT_BANDS
#define FIT_NS CELESTE_FIT_NSTATS
#define FIT_REC 8                      // doubles of a tile record: the seven statistics, one unused

struct FitTileInfo { int32_t n_pix, bad, band, pad; };   // visited pixels; lam non-finite or <= 0 at one of them; band 0..4

// (a work item's px_off: where the visit's stamp starts in the stamp buffer; its tiles number the tile records)
__global__ void __launch_bounds__(64)
fit_pixel_kernel(const VisitItem *__restrict__ items, const DevImage *__restrict__ images, const DevPatch *__restrict__ patches,
                 const double *__restrict__ coefs, const uint8_t *__restrict__ bitmaps, const SrcImg *__restrict__ srcimg,
                 const Comp *__restrict__ comps, const int64_t *__restrict__ nbr_off, const int32_t *__restrict__ nbr_idx,
                 const int32_t *__restrict__ vis_off, const int32_t *__restrict__ vis_img, const int32_t *__restrict__ vis_src,
                 int dense, int N, int NC, int chunk_px, double *__restrict__ rec, FitTileInfo *__restrict__ info,
                 double *__restrict__ stamps) {
    const VisitItem it = items[blockIdx.x];
    const int lane = threadIdx.x;
    visit_pixel_walk(it, images, patches, coefs, bitmaps, srcimg, comps, nbr_off, nbr_idx, vis_off, vis_img, vis_src, dense, N, NC,
                     chunk_px, [&](const DevImage &img, const VisitPixel &px) {
        const int tile = px.tile, idx = px.idx;
        const bool inp = px.inp, valid = px.valid;
        const float xf = px.xf, skyf = px.skyf;
        const double iota = px.iota, m = px.m, B = px.B;
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
#if CELESTE_FIT_MUTANT == 1
            t[CELESTE_FIT_SELF] = m != 0.0 ? __dmul_rn(own, 1.0) : 0.0;
#else
            t[CELESTE_FIT_SELF] = m != 0.0 ? __dmul_rn(own, m / (m + B)) : 0.0;   // (m / (m + 0) = 1: self = own to the bit without neighbours)
#endif
            t[CELESTE_FIT_WRES] = __dmul_rn(own, r) / lam;
            t[CELESTE_FIT_WINFO] = __dmul_rn(own, own) / lam;
            t[CELESTE_FIT_MAX_Z] = fabs(r) / sqrt(lam);
        }
#if CELESTE_FIT_MUTANT == 2
        if (stamps && inp) stamps[it.px_off + idx] = lam;
#else
        if (stamps && inp) stamps[it.px_off + idx] = valid ? lam : (double)NAN;
#endif
#pragma unroll
        for (int k = 0; k < FIT_NS - 1; ++k) t[k] = wave_sum(t[k]);
        t[CELESTE_FIT_MAX_Z] = wave_max(t[CELESTE_FIT_MAX_Z]);
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
    });
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
#if CELESTE_FIT_MUTANT == 4
    for (int r = tr.x + (tr.y > 1 ? 1 : 0); r < tr.x + tr.y; ++r) {
#else
    for (int r = tr.x; r < tr.x + tr.y; ++r) {
#endif
        const FitTileInfo fi = info[r];
        const double x = rec[(size_t)r * FIT_REC + col];
#if CELESTE_FIT_MUTANT == 5
        bad |= 0;
#else
        bad |= fi.bad;
#endif
        const bool mine = fi.band == b;
        if (k < CELESTE_FIT_MAX_Z) acc = mine ? acc + x : acc;
#if CELESTE_FIT_MUTANT == 3
        else if (k == CELESTE_FIT_MAX_Z) acc = mine ? acc + x : acc;
#else
        else if (k == CELESTE_FIT_MAX_Z) acc = mine ? fmax(acc, x) : acc;
#endif
        else cnt += mine ? fi.n_pix : 0;
    }
    const double *vs = vp + (size_t)targets[ti] * CEL_P;
    const int nonfinite = __any(row_nonfinite(vs, lane));
    const int st = nonfinite ? CELESTE_ERR_NONFINITE_INPUT : (bad ? CELESTE_ERR_NONFINITE_RESULT : CELESTE_OK);
    if (b < FIT_NB) {
        if (k < FIT_NS) stats[((size_t)ti * FIT_NB + b) * FIT_NS + k] = st != CELESTE_OK ? (double)NAN : acc;
        else n_pix[(size_t)ti * FIT_NB + b] = cnt;
    }
    if (lane == 0) status[ti] = st;
}

// ---- host side ----------------------------------------------------------------------------------------------------------
struct celeste_fit_ctx : ClientCtx<10, 4, 3> {
    // host staging of one call: kept here so that it outlives the asynchronous copies
    std::vector<VisitItem> items;
    std::vector<int2> tgt_rec;
};

extern "C" int celeste_fit_version(void) { return CELESTE_FIT_ABI_VERSION; }

extern "C" const char *celeste_fit_strerror(int status) { return celeste_strerror(status); }

extern "C" int celeste_fit_ctx_create(const celeste_problem_t *problem, int device, celeste_fit_ctx_t **out) try {
    return client_create(problem, device, out);
} ABI_CATCH

extern "C" void celeste_fit_ctx_destroy(celeste_fit_ctx_t *f) { client_destroy(f); }

extern "C" int celeste_fit_stats(celeste_fit_ctx_t *f, const double *vp, int32_t n_targets, const int32_t *targets,
                                 int64_t *n_pix, double *stats, int32_t *status, int64_t *stamp_offsets, double *stamps) try {
    if (!f || !f->c || !vp || n_targets < 0 || (stamps && !stamp_offsets)) return CELESTE_ERR_INVALID_ARG;
    if (n_targets > 0 && (!targets || !n_pix || !stats || !status)) return CELESTE_ERR_INVALID_ARG;
    celeste_ctx_t *c = f->c;
    if (!client_targets_ok(c, n_targets, targets)) return CELESTE_ERR_INVALID_ARG;
    if (n_targets == 0) return CELESTE_OK;
    // the work list; a target's tile records follow each other, and so do the stamps of the call's entries
    std::vector<VisitItem> &items = f->items;
    std::vector<int2> &tgt_rec = f->tgt_rec;
    tgt_rec.assign((size_t)n_targets, make_int2(0, 0));
    int64_t n_rec = 0, soff = 0, n_ent = 0;
    if (!client_walk(c, n_targets, targets, items, n_rec, soff, [&](int ti, int, int, int64_t tile0, int64_t tile1, int64_t px_off) {
            if (tgt_rec[ti].y == 0) tgt_rec[ti].x = (int)tile0;
            tgt_rec[ti].y = (int)tile1 - tgt_rec[ti].x;
            if (stamp_offsets) stamp_offsets[n_ent] = px_off;
            ++n_ent;
            return true;
        })) return CELESTE_ERR_INVALID_ARG;
    if (stamp_offsets) stamp_offsets[n_ent] = soff;
    HIP_TRY(hipSetDevice(c->device));
    const int chunk = c->chunk_px;
    const size_t nt = (size_t)n_targets, ni = items.size();
    double *d_vp = nullptr, *d_rec = nullptr, *d_stats = nullptr, *d_stamps = nullptr;
    VisitItem *d_items = nullptr;
    FitTileInfo *d_info = nullptr;
    int2 *d_tgt_rec = nullptr;
    int32_t *d_targets = nullptr, *d_status = nullptr;
    int64_t *d_npix = nullptr;
    if (client_get(f, 0, (size_t)c->S * CEL_P * sizeof(double), &d_vp) != hipSuccess ||
        client_get(f, 1, ni * sizeof(VisitItem), &d_items) != hipSuccess ||
        client_get(f, 2, (size_t)n_rec * FIT_REC * sizeof(double), &d_rec) != hipSuccess ||
        client_get(f, 3, (size_t)n_rec * sizeof(FitTileInfo), &d_info) != hipSuccess ||
        client_get(f, 4, nt * sizeof(int2), &d_tgt_rec) != hipSuccess ||
        client_get(f, 5, nt * sizeof(int32_t), &d_targets) != hipSuccess ||
        client_get(f, 6, nt * FIT_NB * FIT_NS * sizeof(double), &d_stats) != hipSuccess ||
        client_get(f, 7, nt * FIT_NB * sizeof(int64_t), &d_npix) != hipSuccess ||
        client_get(f, 8, nt * sizeof(int32_t), &d_status) != hipSuccess ||
        (stamps && client_get(f, 9, (size_t)soff * sizeof(double), &d_stamps) != hipSuccess))
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
    client_stage_ms(f);
    return client_first_status(status, n_targets);
} ABI_CATCH

extern "C" int celeste_fit_last_ms(celeste_fit_ctx_t *f, float ms[3]) { return client_last_ms(f, ms); }
