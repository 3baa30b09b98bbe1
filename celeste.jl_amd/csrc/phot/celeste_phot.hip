// celeste_phot.hip -- libceleste_phot.so: per-exposure forced photometry (include/celeste_phot.h).
//
// The engine's context code (engine_context.h) and its kernels' header are compiled into this library, unchanged, as for the
// fit library: the patch table, the per-visit tables of prep_kernel, the spline coefficients, the bitmaps, the neighbour
// lists, star_value and galaxy_value are the engine's.  The context, the work list and the pixel walk (the target's own light
// m and the neighbours' light B of every pixel) are engine_client.h's; this file adds three kernels.  One call:
//   prep_kernel          (the engine's) SrcImg and Comp of every visit of the context at the call's table
//   phot_pixel_kernel    one wavefront per work item; from m and B -- the expensive part, once per pixel -- a lane writes
//                        a = iota m, b = iota (eps + B) and x to the entry's scratch in device memory (CSR by entry, one plane
//                        each); a pixel that is not visited is written as a = b = x = 0 (b > 0 marks a visited pixel of a
//                        sound entry)
//   phot_solve_kernel    one workgroup of four wavefronts per entry runs every Newton iteration.  <true>: a, b, x are staged
//                        once into LDS (24 B per pixel, up to CELESTE_PHOT_LDS_PIXELS pixels); <false>: they are read from
//                        the scratch on every iteration.  Both run the same pass: wavefront w sums tiles w, w + 4, ... (a tile
//                        = 64 consecutive pixels, a fixed butterfly), lane 0 leaves the tile's sums in LDS, and after a barrier
//                        EVERY thread adds the tiles in ascending order -- all threads hold the same sums, so the iteration's
//                        control flow is uniform without a broadcast.  Tiles are taken in rounds of PHOT_PT, the rounds
//                        alternating between two buffers (one barrier per round).
//   phot_summary_kernel  one wavefront per target: lane b adds the OK entries of band b in ascending image order; status
// No floating-point atomics; every rounded operation of a pass is spelled out (no contraction), so both paths agree bit for bit.
#include "../engine_context.h"
#include "../engine_client.h"
#include "../../../include/celeste_phot.h"

// Mutation testing (tests/test_satellite_mutants.py builds this library with -DCELESTE_PHOT_MUTANT=k and checks that
// tests/test_gpu_phot.py notices).  A mutant changes arithmetic, or an index that stays under the same p < npx test; never a
// size, a launch, a barrier or a loop.  0 = the product;
//   1 = phot_pass reads pixel t * 64 + lane: t0 is dropped (t < nt <= n_tiles, and p < npx is still tested)
//   2 = b leaves out the neighbours' light
//   3 = elec tests px[p] >= 0.0: AT_BOUND is never reached
//   4 = the summary weights are 1 / sigma instead of 1 / sigma^2
//   5 = the convergence test compares fabs(step) with tol_sigma itself
//   6 = the second pass's sigma is 1 / s0 without the square root
// Never defined in the shipped build.
#ifndef CELESTE_PHOT_MUTANT
#define CELESTE_PHOT_MUTANT 0
#endif

#define PHOT_NB CELESTE_PHOT_BANDS
#define PHOT_NSUM CELESTE_PHOT_NSUMMARY
#define PHOT_THREADS 256
#define PHOT_WAVES (PHOT_THREADS / 64)
#define PHOT_PT 128                     // tiles of a round: 2 buffers x 128 tiles x 3 sums x 8 B = 6 KiB of LDS
#define PHOT_CLASSES 4                  // size classes of the LDS path: one launch each

struct PhotEntry {
    int64_t px_off;                    // first pixel in the scratch planes
    int32_t npx, tile0;                // pixels of the patch; first tile
    int32_t n, ti;                     // image; index of the target in the call
    int32_t pad[2];
};

struct PhotTileInfo { int32_t n_pix, bad; };   // visited pixels; a or b unsound at one of them

// ---- pixel pass ------------------------------------------------------------------------------------------------------------
// (a work item's px_off: where the entry's pixels start in the scratch planes)
__global__ void __launch_bounds__(64)
phot_pixel_kernel(const VisitItem *__restrict__ items, const DevImage *__restrict__ images, const DevPatch *__restrict__ patches,
                  const double *__restrict__ coefs, const uint8_t *__restrict__ bitmaps, const SrcImg *__restrict__ srcimg,
                  const Comp *__restrict__ comps, const int64_t *__restrict__ nbr_off, const int32_t *__restrict__ nbr_idx,
                  const int32_t *__restrict__ vis_off, const int32_t *__restrict__ vis_img, const int32_t *__restrict__ vis_src,
                  int dense, int N, int NC, int chunk_px, double *__restrict__ sa, double *__restrict__ sb,
                  double *__restrict__ sx, PhotTileInfo *__restrict__ info) {
    const VisitItem it = items[blockIdx.x];
    const int lane = threadIdx.x;
    visit_pixel_walk(it, images, patches, coefs, bitmaps, srcimg, comps, nbr_off, nbr_idx, vis_off, vis_img, vis_src, dense, N, NC,
                     chunk_px, [&](const DevImage &, const VisitPixel &px) {
        const int tile = px.tile, idx = px.idx;
        const bool inp = px.inp, valid = px.valid;
        const float xf = px.xf, skyf = px.skyf;
        const double iota = px.iota, m = px.m, B = px.B;
#if CELESTE_PHOT_MUTANT == 2
        const double a = __dmul_rn(iota, m), b = __dmul_rn(iota, (double)skyf);
#else
        const double a = __dmul_rn(iota, m), b = __dmul_rn(iota, (double)skyf + B);
#endif
        const bool bad = valid && !(isfinite(a) && isfinite(b) && a >= 0.0 && b > 0.0);
        if (inp) {                                            // idx < npx: inside the entry's planes
            const int64_t o = it.px_off + idx;
            sa[o] = valid ? a : 0.0;
            sb[o] = valid ? b : 0.0;
            sx[o] = valid ? (double)xf : 0.0;
        }
        const int n_valid = __popcll(__ballot(valid));
        const int any_bad = __any(bad);
        if (lane == 0) {
            PhotTileInfo ti;
            ti.n_pix = n_valid; ti.bad = any_bad;
            info[tile] = ti;
        }
    });
}

// ---- solve pass ------------------------------------------------------------------------------------------------------------
// One pass over the entry's pixels at alpha.  MODE 0: s0 = g, s1 = D, s2 = I.  MODE 1: s0 = I, s1 = chi2.
// part: the two round buffers; round: the running round count of the workgroup (selects the buffer).
template <int MODE>
__device__ __forceinline__ void phot_pass(const double *pa, const double *pb, const double *px, int npx, int n_tiles, double alpha,
                                          double (*part)[PHOT_PT][3], int &round, double &s0, double &s1, double &s2) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    s0 = 0.0; s1 = 0.0; s2 = 0.0;
    for (int t0 = 0; t0 < n_tiles; t0 += PHOT_PT, ++round) {
        double (*buf)[3] = part[round & 1];
        const int nt = min(n_tiles - t0, PHOT_PT);
        for (int t = wave; t < nt; t += PHOT_WAVES) {
#if CELESTE_PHOT_MUTANT == 1
            const int p = t * 64 + lane;
#else
            const int p = (t0 + t) * 64 + lane;
#endif
            double a = 0.0, b = 0.0, x = 0.0;
            if (p < npx) { a = pa[p]; b = pb[p]; x = px[p]; }
            double u0 = 0.0, u1 = 0.0, u2 = 0.0;
            if (b > 0.0) {                                    // a visited pixel
                const double lam = __dadd_rn(b, __dmul_rn(alpha, a));
                const double inv = 1.0 / lam;
                const double r = __dmul_rn(a, inv);           // a / lam
                if (MODE == 0) {
                    u0 = __dmul_rn(a, __dsub_rn(__dmul_rn(x, inv), 1.0));
                    u1 = __dmul_rn(x, __dmul_rn(r, r));
                    u2 = __dmul_rn(a, r);
                } else {
                    const double d = __dsub_rn(x, lam);
                    u0 = __dmul_rn(a, r);
                    u1 = __dmul_rn(__dmul_rn(d, d), inv);
                }
            }
            u0 = wave_sum(u0);
            u1 = wave_sum(u1);
            if (MODE == 0) u2 = wave_sum(u2);
            if (lane == 0) { buf[t][0] = u0; buf[t][1] = u1; buf[t][2] = u2; }
        }
        __syncthreads();
        for (int t = 0; t < nt; ++t) {                        // every thread: the tiles in ascending order
            s0 = __dadd_rn(s0, buf[t][0]);
            s1 = __dadd_rn(s1, buf[t][1]);
            if (MODE == 0) s2 = __dadd_rn(s2, buf[t][2]);
        }
    }
}

template <bool LDS>
__global__ void __launch_bounds__(PHOT_THREADS)
phot_solve_kernel(const int32_t *__restrict__ list, const PhotEntry *__restrict__ entries, const PhotTileInfo *__restrict__ info,
                  const int32_t *__restrict__ targets, const double *__restrict__ vp, const DevImage *__restrict__ images,
                  const double *__restrict__ sa, const double *__restrict__ sb, const double *__restrict__ sx, double tol_sigma,
                  int max_iters, int32_t *__restrict__ o_image, int32_t *__restrict__ o_band, double *__restrict__ o_alpha,
                  double *__restrict__ o_sigma, double *__restrict__ o_chi2, int32_t *__restrict__ o_npix,
                  int32_t *__restrict__ o_iters, int32_t *__restrict__ o_flag) {
    extern __shared__ double px_lds[];                        // <true>: a, b, x of the entry, each padded to whole tiles
    __shared__ double part[2][PHOT_PT][3];
    __shared__ double red[PHOT_WAVES];
    __shared__ int cnt[2];
    const int e = list[blockIdx.x];
    const PhotEntry E = entries[e];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int npx = E.npx, n_tiles = (npx + 63) >> 6;
    if (tid < 2) cnt[tid] = 0;
    const double *vs = vp + (size_t)targets[E.ti] * CEL_P;
    const int nonfinite = __syncthreads_or(row_nonfinite(vs, tid));
    {
        int np = 0, bd = 0;
        for (int t = tid; t < n_tiles; t += PHOT_THREADS) { const PhotTileInfo ti = info[E.tile0 + t]; np += ti.n_pix; bd |= ti.bad; }
        if (np) atomicAdd(&cnt[0], np);                       // (integers: the order does not matter)
        if (bd) atomicOr(&cnt[1], 1);
    }
    __syncthreads();
    const int n_pix = cnt[0], bad = cnt[1];
    int flag = CELESTE_PHOT_BAD_MODEL, iters = 0;
    double alpha = (double)NAN, sigma = (double)NAN, chi2 = (double)NAN;
    if (!nonfinite && !bad) {
        const double *pa = sa + E.px_off, *pb = sb + E.px_off, *px = sx + E.px_off;
        if (LDS) {
            const int pad = n_tiles * 64;
            double *la = px_lds, *lb = px_lds + pad, *lx = px_lds + 2 * pad;
            for (int p = tid; p < pad; p += PHOT_THREADS) {
                const bool in = p < npx;
                la[p] = in ? pa[p] : 0.0;
                lb[p] = in ? pb[p] : 0.0;
                lx[p] = in ? px[p] : 0.0;
            }
            __syncthreads();
            pa = la; pb = lb; px = lx;
        }
        // the domain and the two degenerate cases: maxima and flags, which do not depend on an order
        double amin = -INFINITY;
        int light = 0, elec = 0;
        for (int p = tid; p < npx; p += PHOT_THREADS) {
            const double a = pa[p], b = pb[p];
            if (b > 0.0 && a > 0.0) {
                light = 1;
                amin = fmax(amin, -b / a);
#if CELESTE_PHOT_MUTANT == 3
                if (px[p] >= 0.0) elec = 1;
#else
                if (px[p] > 0.0) elec = 1;
#endif
            }
        }
        amin = wave_max(amin);
        if (lane == 0) red[wave] = amin;
        light = __syncthreads_or(light);
        elec = __syncthreads_or(elec);
        amin = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
        int round = 0;
        double s0, s1, s2;
        if (!light) {
            flag = CELESTE_PHOT_NO_LIGHT;
            phot_pass<1>(pa, pb, px, npx, n_tiles, 0.0, part, round, s0, s1, s2);
            chi2 = s1;
        } else if (!elec) {
            flag = CELESTE_PHOT_AT_BOUND;
            alpha = amin;
        } else {
            flag = CELESTE_PHOT_NOT_CONVERGED;
            alpha = 1.0;
            while (iters < max_iters) {
                phot_pass<0>(pa, pb, px, npx, n_tiles, alpha, part, round, s0, s1, s2);
                const double step = s0 / s1;
                ++iters;
                if (!isfinite(step)) break;
                double next = __dadd_rn(alpha, step);
                const bool inside = next > amin;
                if (!inside) next = __dadd_rn(alpha, __dmul_rn(0.5, __dsub_rn(amin, alpha)));
                alpha = next;
#if CELESTE_PHOT_MUTANT == 5
                if (inside && fabs(step) <= tol_sigma) { flag = CELESTE_PHOT_OK; break; }
#else
                if (inside && fabs(step) <= tol_sigma / sqrt(s2)) { flag = CELESTE_PHOT_OK; break; }
#endif
            }
            phot_pass<1>(pa, pb, px, npx, n_tiles, alpha, part, round, s0, s1, s2);
#if CELESTE_PHOT_MUTANT == 6
            sigma = 1.0 / s0;
#else
            sigma = 1.0 / sqrt(s0);
#endif
            chi2 = s1;
        }
    }
    if (tid == 0) {
        o_image[e] = E.n;
        o_band[e] = images[E.n].band - 1;
        o_alpha[e] = alpha;
        o_sigma[e] = sigma;
        o_chi2[e] = chi2;
        o_npix[e] = n_pix;
        o_iters[e] = iters;
        o_flag[e] = flag;
    }
}

// ---- band summaries --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
phot_summary_kernel(const int64_t *__restrict__ eoff, const int32_t *__restrict__ targets, const double *__restrict__ vp,
                    const int32_t *__restrict__ band, const int32_t *__restrict__ flag, const double *__restrict__ alpha,
                    const double *__restrict__ sigma, int32_t *__restrict__ n_epochs, double *__restrict__ summary,
                    int32_t *__restrict__ status) {
    const int ti = blockIdx.x, lane = threadIdx.x;
    const int64_t e0 = eoff[ti], e1 = eoff[ti + 1];
    int bad = 0;
    for (int64_t e = e0 + lane; e < e1; e += 64) bad |= flag[e] == CELESTE_PHOT_BAD_MODEL;
    bad = __any(bad);
    const double *vs = vp + (size_t)targets[ti] * CEL_P;
    const int nonfinite = __any(row_nonfinite(vs, lane));
    if (lane < PHOT_NB) {
        int n = 0;
        double W = 0.0, SA = 0.0;
        for (int64_t e = e0; e < e1; ++e) {
            if (flag[e] != CELESTE_PHOT_OK || band[e] != lane) continue;
#if CELESTE_PHOT_MUTANT == 4
            const double sg = sigma[e], w = 1.0 / sg;
#else
            const double sg = sigma[e], w = 1.0 / __dmul_rn(sg, sg);
#endif
            ++n;
            W = __dadd_rn(W, w);
            SA = __dadd_rn(SA, __dmul_rn(w, alpha[e]));
        }
        double wmean = (double)NAN, wsig = (double)NAN, cv = (double)NAN;
        if (n > 0) {
            wmean = SA / W;
            wsig = 1.0 / sqrt(W);
            cv = 0.0;
            for (int64_t e = e0; e < e1; ++e) {
                if (flag[e] != CELESTE_PHOT_OK || band[e] != lane) continue;
#if CELESTE_PHOT_MUTANT == 4
                const double sg = sigma[e], w = 1.0 / sg, d = __dsub_rn(alpha[e], wmean);
#else
                const double sg = sigma[e], w = 1.0 / __dmul_rn(sg, sg), d = __dsub_rn(alpha[e], wmean);
#endif
                cv = __dadd_rn(cv, __dmul_rn(w, __dmul_rn(d, d)));
            }
        }
        n_epochs[(size_t)ti * PHOT_NB + lane] = n;
        double *o = summary + ((size_t)ti * PHOT_NB + lane) * PHOT_NSUM;
        o[CELESTE_PHOT_WMEAN] = wmean;
        o[CELESTE_PHOT_WMEAN_SIGMA] = wsig;
        o[CELESTE_PHOT_CHI2_VAR] = cv;
    }
    if (lane == 0) status[ti] = nonfinite ? CELESTE_ERR_NONFINITE_INPUT : (bad ? CELESTE_ERR_NONFINITE_RESULT : CELESTE_OK);
}

// ---- host side ----------------------------------------------------------------------------------------------------------
enum { PB_VP, PB_ITEMS, PB_ENTRIES, PB_INFO, PB_SA, PB_SB, PB_SX, PB_LIST, PB_TARGETS, PB_EOFF, PB_IMAGE, PB_BAND, PB_ALPHA,
       PB_SIGMA, PB_CHI2, PB_NPIX, PB_ITERS, PB_FLAG, PB_NEPOCHS, PB_SUMMARY, PB_STATUS, PB_COUNT };

struct celeste_phot_ctx : ClientCtx<PB_COUNT, 5, 4> {
    // host staging of one call: kept here so that it outlives the asynchronous copies
    std::vector<VisitItem> items;
    std::vector<PhotEntry> entries;
    std::vector<int32_t> list;         // the entries solved from LDS, class by class, then the streamed ones
    std::vector<int64_t> eoff;
};

extern "C" int celeste_phot_version(void) { return CELESTE_PHOT_ABI_VERSION; }

extern "C" const char *celeste_phot_strerror(int status) { return celeste_strerror(status); }

extern "C" int celeste_phot_ctx_create(const celeste_problem_t *problem, int device, celeste_phot_ctx_t **out) try {
    const int rc = client_create(problem, device, out);
    if (rc != CELESTE_OK) return rc;
    // the LDS path declares more than the 64 KiB a launch gets without asking
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(&phot_solve_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            CELESTE_PHOT_LDS_PIXELS * 24) != hipSuccess) {
        client_destroy(*out);
        *out = nullptr;
        return CELESTE_ERR_HIP;
    }
    return CELESTE_OK;
} ABI_CATCH

extern "C" void celeste_phot_ctx_destroy(celeste_phot_ctx_t *f) { client_destroy(f); }

extern "C" int celeste_phot_light_curves(celeste_phot_ctx_t *f, const double *vp, int32_t n_targets, const int32_t *targets,
                                         const celeste_phot_params_t *params, int64_t *entry_offsets, int32_t *image,
                                         double *alpha, double *sigma, double *chi2, int32_t *n_pix, int32_t *iters,
                                         int32_t *flag, int32_t *n_epochs, double *summary, int32_t *status) try {
    if (!f || !f->c || !vp || n_targets < 0) return CELESTE_ERR_INVALID_ARG;
    if (n_targets > 0 && (!targets || !entry_offsets || !image || !alpha || !sigma || !chi2 || !n_pix || !iters || !flag ||
                          !n_epochs || !summary || !status)) return CELESTE_ERR_INVALID_ARG;
    celeste_phot_params_t pr;
    pr.tol_sigma = 1e-9; pr.max_iters = 50; pr.lds_max_pixels = 0;
    if (params) pr = *params;
    if (!(pr.tol_sigma > 0.0 && std::isfinite(pr.tol_sigma)) || pr.max_iters < 1 || pr.lds_max_pixels < 0)
        return CELESTE_ERR_INVALID_ARG;
    celeste_ctx_t *c = f->c;
    if (!client_targets_ok(c, n_targets, targets)) return CELESTE_ERR_INVALID_ARG;
    if (n_targets == 0) return CELESTE_OK;
    const int lds_cap = pr.lds_max_pixels > 0 ? std::min<int>(pr.lds_max_pixels, CELESTE_PHOT_LDS_PIXELS) : CELESTE_PHOT_LDS_PIXELS;
    // the work list, and the entries in (target, image) order: eoff[ti] .. eoff[ti + 1] are target ti's
    std::vector<VisitItem> &items = f->items;
    std::vector<PhotEntry> &entries = f->entries;
    std::vector<int64_t> &eoff = f->eoff;
    entries.clear();
    eoff.assign((size_t)n_targets + 1, 0);
    int64_t n_tiles = 0, poff = 0;
    if (!client_walk(c, n_targets, targets, items, n_tiles, poff, [&](int ti, int v, int npx, int64_t tile0, int64_t, int64_t px_off) {
            if (entries.size() >= 0x7fffff00ull) return false;
            PhotEntry E;
            E.px_off = px_off; E.npx = npx; E.tile0 = (int32_t)tile0; E.n = c->h_vis_img[v]; E.ti = ti; E.pad[0] = E.pad[1] = 0;
            entries.push_back(E);
            ++eoff[ti + 1];
            return true;
        })) return CELESTE_ERR_INVALID_ARG;
    for (int ti = 0; ti < n_targets; ++ti) eoff[ti + 1] += eoff[ti];
    const int chunk = c->chunk_px;
    const size_t nt = (size_t)n_targets, ni = items.size(), ne = entries.size();
    // the solve lists: the entries solved from LDS by size class, one launch per class -- a launch declares the LDS of its
    // largest patch for every workgroup, and the classes end where another workgroup fits a CU's 160 KiB (6, 3, 2, 1 per CU)
    // -- then the streamed entries.  Which list an entry is on does not change its numbers.
    static const int class_px[PHOT_CLASSES] = {704, 1664, 3072, CELESTE_PHOT_LDS_PIXELS};
    std::vector<int32_t> &list = f->list;
    list.clear();
    size_t cls_n[PHOT_CLASSES];
    int cls_max[PHOT_CLASSES];
    for (int k = 0; k < PHOT_CLASSES; ++k) {
        const int lo = k ? class_px[k - 1] : 0, hi = std::min(class_px[k], lds_cap);
        const size_t first = list.size();
        cls_max[k] = 0;
        for (size_t e = 0; e < ne; ++e)
            if (entries[e].npx > lo && entries[e].npx <= hi) { list.push_back((int32_t)e); cls_max[k] = std::max(cls_max[k], entries[e].npx); }
        cls_n[k] = list.size() - first;
    }
    const size_t n_lds = list.size();
    for (size_t e = 0; e < ne; ++e) if (entries[e].npx > lds_cap) list.push_back((int32_t)e);
    for (int ti = 0; ti <= n_targets; ++ti) entry_offsets[ti] = eoff[ti];
    HIP_TRY(hipSetDevice(c->device));
    double *d_vp = nullptr, *d_sa = nullptr, *d_sb = nullptr, *d_sx = nullptr, *d_alpha = nullptr, *d_sigma = nullptr,
           *d_chi2 = nullptr, *d_summary = nullptr;
    VisitItem *d_items = nullptr;
    PhotEntry *d_entries = nullptr;
    PhotTileInfo *d_info = nullptr;
    int64_t *d_eoff = nullptr;
    int32_t *d_list = nullptr, *d_targets = nullptr, *d_image = nullptr, *d_band = nullptr, *d_npix = nullptr, *d_iters = nullptr,
            *d_flag = nullptr, *d_nepochs = nullptr, *d_status = nullptr;
    const size_t npl = (size_t)poff * sizeof(double);
    if (client_get(f, PB_VP, (size_t)c->S * CEL_P * sizeof(double), &d_vp) != hipSuccess ||
        client_get(f, PB_ITEMS, ni * sizeof(VisitItem), &d_items) != hipSuccess ||
        client_get(f, PB_ENTRIES, ne * sizeof(PhotEntry), &d_entries) != hipSuccess ||
        client_get(f, PB_INFO, (size_t)n_tiles * sizeof(PhotTileInfo), &d_info) != hipSuccess ||
        client_get(f, PB_SA, npl, &d_sa) != hipSuccess || client_get(f, PB_SB, npl, &d_sb) != hipSuccess ||
        client_get(f, PB_SX, npl, &d_sx) != hipSuccess ||
        client_get(f, PB_LIST, ne * sizeof(int32_t), &d_list) != hipSuccess ||
        client_get(f, PB_TARGETS, nt * sizeof(int32_t), &d_targets) != hipSuccess ||
        client_get(f, PB_EOFF, (nt + 1) * sizeof(int64_t), &d_eoff) != hipSuccess ||
        client_get(f, PB_IMAGE, ne * sizeof(int32_t), &d_image) != hipSuccess ||
        client_get(f, PB_BAND, ne * sizeof(int32_t), &d_band) != hipSuccess ||
        client_get(f, PB_ALPHA, ne * sizeof(double), &d_alpha) != hipSuccess ||
        client_get(f, PB_SIGMA, ne * sizeof(double), &d_sigma) != hipSuccess ||
        client_get(f, PB_CHI2, ne * sizeof(double), &d_chi2) != hipSuccess ||
        client_get(f, PB_NPIX, ne * sizeof(int32_t), &d_npix) != hipSuccess ||
        client_get(f, PB_ITERS, ne * sizeof(int32_t), &d_iters) != hipSuccess ||
        client_get(f, PB_FLAG, ne * sizeof(int32_t), &d_flag) != hipSuccess ||
        client_get(f, PB_NEPOCHS, nt * PHOT_NB * sizeof(int32_t), &d_nepochs) != hipSuccess ||
        client_get(f, PB_SUMMARY, nt * PHOT_NB * PHOT_NSUM * sizeof(double), &d_summary) != hipSuccess ||
        client_get(f, PB_STATUS, nt * sizeof(int32_t), &d_status) != hipSuccess)
        return CELESTE_ERR_HIP;
    hipStream_t st = c->stream;
    HIP_TRY(hipMemcpyAsync(d_vp, vp, (size_t)c->S * CEL_P * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_targets, targets, nt * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_eoff, eoff.data(), (nt + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    if (ni > 0) HIP_TRY(hipMemcpyAsync(d_items, items.data(), ni * sizeof(VisitItem), hipMemcpyHostToDevice, st));
    if (ne > 0) {
        HIP_TRY(hipMemcpyAsync(d_entries, entries.data(), ne * sizeof(PhotEntry), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_list, list.data(), ne * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipEventRecord(f->ev[0], st));
    client_launch_prep(c, d_vp, st);
    HIP_TRY(hipEventRecord(f->ev[1], st));
    if (ni > 0)
        hipLaunchKernelGGL(phot_pixel_kernel, dim3((unsigned)ni), dim3(64), 0, st, d_items, c->d_images, c->d_patches, c->d_coefs,
                           c->d_bitmaps, c->d_srcimg, c->d_comps, c->d_nbr_off, c->d_nbr_idx, c->d_vis_off, c->d_vis_img,
                           c->d_vis_src, (int)c->dense, c->N, c->NC, chunk, d_sa, d_sb, d_sx, d_info);
    HIP_TRY(hipEventRecord(f->ev[2], st));
    for (size_t k = 0, first = 0; k < PHOT_CLASSES; first += cls_n[k], ++k) {
        if (cls_n[k] == 0) continue;
        const size_t dyn = (size_t)((cls_max[k] + 63) / 64 * 64) * 24;   // <= CELESTE_PHOT_LDS_PIXELS * 24 (a multiple of 64 pixels)
        hipLaunchKernelGGL(phot_solve_kernel<true>, dim3((unsigned)cls_n[k]), dim3(PHOT_THREADS), dyn, st, d_list + first, d_entries,
                           d_info, d_targets, d_vp, c->d_images, d_sa, d_sb, d_sx, pr.tol_sigma, (int)pr.max_iters, d_image, d_band,
                           d_alpha, d_sigma, d_chi2, d_npix, d_iters, d_flag);
    }
    if (ne > n_lds)
        hipLaunchKernelGGL(phot_solve_kernel<false>, dim3((unsigned)(ne - n_lds)), dim3(PHOT_THREADS), 0, st, d_list + n_lds,
                           d_entries, d_info, d_targets, d_vp, c->d_images, d_sa, d_sb, d_sx, pr.tol_sigma, (int)pr.max_iters,
                           d_image, d_band, d_alpha, d_sigma, d_chi2, d_npix, d_iters, d_flag);
    HIP_TRY(hipEventRecord(f->ev[3], st));
    hipLaunchKernelGGL(phot_summary_kernel, dim3((unsigned)nt), dim3(64), 0, st, d_eoff, d_targets, d_vp, d_band, d_flag, d_alpha,
                       d_sigma, d_nepochs, d_summary, d_status);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(f->ev[4], st));
    if (ne > 0) {
        HIP_TRY(hipMemcpyAsync(image, d_image, ne * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(alpha, d_alpha, ne * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(sigma, d_sigma, ne * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(chi2, d_chi2, ne * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(n_pix, d_npix, ne * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(iters, d_iters, ne * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(flag, d_flag, ne * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(n_epochs, d_nepochs, nt * PHOT_NB * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(summary, d_summary, nt * PHOT_NB * PHOT_NSUM * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(status, d_status, nt * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    client_stage_ms(f);
    return client_first_status(status, n_targets);
} ABI_CATCH

extern "C" int celeste_phot_last_ms(celeste_phot_ctx_t *f, float ms[4]) { return client_last_ms(f, ms); }
