// celeste_prep_detected: detections of every image -> joined objects -> catalog entries and the patch table
// (include/celeste_prep.h states the arithmetic).  Included at the end of celeste_prep.hip.
//
//   prep_det_world_kernel            one thread per detection: its image, its world position
//   prep_det_unit_kernel, prep_match_angular_kernel
//                                    the same join by angular distance, when an image is TAN (celeste_prep.h)
//   prep_match_kernel                per image, one thread per detection: the nearest joined entry, the joined list through
//                                    LDS in tiles; the list's length is read from device memory
//   prep_append_kernel               per image, one workgroup: the unmatched detections go to the end of the list in object
//                                    order (a block scan per 256 detections)
//   prep_object_ranges_kernel        per object: where its detections start in the list sorted by joined index
//   prep_entry_kernel                one thread per object: fluxes and shape of its catalog entry, its (image, object) list
//   prep_detected_geometry_kernel    one thread per (object, image) pair: the detection box or the minimum box, clamped
// The search of the match kernel is exhaustive: every detection of a later image against every joined entry.
//
// CELESTE_PREP_MUTANT (celeste_prep.hip lists 1 to 16):
//   17 = prep_match_kernel joins at best <= match_radius
//   18 = prep_match_kernel: the highest index among equal distances
//   19 = prep_append_kernel appends a block's unmatched detections in reverse order
//   20 = prep_entry_kernel: the last band on a tie gives the shape
//   21 = prep_detected_geometry_kernel: the detection's box replaces the minimum box instead of being enclosed with it
//   22 = prep_match_angular_kernel compares half the separation with match_radius
#pragma once

#define PREP_TILE CELESTE_PREP_MATCH_TILE
static_assert(CELESTE_PREP_MATCH_BLOCK == PREP_BLOCK, "the match kernel runs workgroups of PREP_BLOCK threads");

// the image of detection d: the n with off[n] <= d < off[n + 1] (off[N] = D > d)
__device__ __forceinline__ int det_image_of(const int64_t *off, int N, int64_t d) {
    int lo = 0, hi = N;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= d) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(PREP_BLOCK) prep_det_world_kernel(const PrepImg *imgs, int N, const int64_t *off, const celeste_prep_detection_t *det,
                                                                    int64_t D, double2 *world, int32_t *dimg, int32_t *didx) {
    const int64_t d = (int64_t)blockIdx.x * PREP_BLOCK + threadIdx.x;
    if (d >= D) return;
    const int n = det_image_of(off, N, d);
    double w1, w2;
    pix_to_world(imgs[n], det[d].x, det[d].y, w1, w2);
    world[d] = make_double2(w1, w2);
    dimg[d] = n;
    didx[d] = (int32_t)d;
}

// detections first .. first + n of one image against the joined list jpos[0 .. *jcount): jidx = the nearest entry when it is
// closer than match_radius, else -1
__global__ void __launch_bounds__(PREP_BLOCK) prep_match_kernel(const double2 *world, int64_t first, int n, const double2 *jpos, const int32_t *jcount,
                                                                double match_radius, int32_t *jidx) {
    __shared__ double2 tile[PREP_TILE];
    const int i = blockIdx.x * PREP_BLOCK + threadIdx.x;
    const bool live = i < n;
    const double2 w = live ? world[first + i] : make_double2(0.0, 0.0);
    const int cnt = *jcount;                       // (uniform over the grid: the append launch of the image before wrote it)
    double best = INFINITY;
    int bi = -1;
    for (int t0 = 0; t0 < cnt; t0 += PREP_TILE) {
        const int m = min(PREP_TILE, cnt - t0);
        for (int k = threadIdx.x; k < m; k += PREP_BLOCK) tile[k] = jpos[t0 + k];
        __syncthreads();
        if (live)
            for (int k = 0; k < m; ++k) {
                const double dx = tile[k].x - w.x, dy = tile[k].y - w.y;
                const double d = sqrt(dx * dx + dy * dy);
#if CELESTE_PREP_MUTANT == 18
                if (d <= best) { best = d; bi = t0 + k; }
#else
                if (d < best) { best = d; bi = t0 + k; }      // strict: the lowest index among equal distances
#endif
            }
        __syncthreads();
    }
#if CELESTE_PREP_MUTANT == 17
    if (live) jidx[first + i] = (bi >= 0 && best <= match_radius) ? bi : -1;
#else
    if (live) jidx[first + i] = (bi >= 0 && best < match_radius) ? bi : -1;
#endif
}

struct PrepUnit { double x, y, z; };      // (cos dec cos ra, cos dec sin ra, sin dec)

// one thread per detection (launched when an image is TAN): the unit vector of its world position, (ra, dec) in degrees
__global__ void __launch_bounds__(PREP_BLOCK) prep_det_unit_kernel(const double2 *world, int64_t D, PrepUnit *unit) {
    const int64_t d = (int64_t)blockIdx.x * PREP_BLOCK + threadIdx.x;
    if (d >= D) return;
    double sl, cl, sb, cb;
    sincos(world[d].x * PREP_D2R, &sl, &cl);
    sincos(world[d].y * PREP_D2R, &sb, &cb);
    PrepUnit u;
    u.x = cb * cl; u.y = cb * sl; u.z = sb;
    unit[d] = u;
}

// prep_match_kernel with the angular distance: the chord between unit vectors orders the entries (strict <: the lowest index
// among equal chords); the nearest is joined when 2 asind(chord / 2) < match_radius, in degrees
__global__ void __launch_bounds__(PREP_BLOCK) prep_match_angular_kernel(const PrepUnit *unit, int64_t first, int n, const PrepUnit *junit,
                                                                        const int32_t *jcount, double match_radius, int32_t *jidx) {
    __shared__ PrepUnit tile[PREP_TILE];
    const int i = blockIdx.x * PREP_BLOCK + threadIdx.x;
    const bool live = i < n;
    PrepUnit w;
    w.x = 0.0; w.y = 0.0; w.z = 0.0;
    if (live) w = unit[first + i];
    const int cnt = *jcount;                       // (uniform over the grid)
    double best = INFINITY;
    int bi = -1;
    for (int t0 = 0; t0 < cnt; t0 += PREP_TILE) {
        const int m = min(PREP_TILE, cnt - t0);
        for (int k = threadIdx.x; k < m; k += PREP_BLOCK) tile[k] = junit[t0 + k];
        __syncthreads();
        if (live)
            for (int k = 0; k < m; ++k) {
                const double ex = tile[k].x - w.x, ey = tile[k].y - w.y, ez = tile[k].z - w.z;
                const double d = sqrt((ex * ex + ey * ey) + ez * ez);
                if (d < best) { best = d; bi = t0 + k; }
            }
        __syncthreads();
    }
    if (live) {
        const double h = best / 2.0;
#if CELESTE_PREP_MUTANT == 22
        const double sep = asin(h < 1.0 ? h : 1.0) * PREP_R2D;
#else
        const double sep = 2.0 * (asin(h < 1.0 ? h : 1.0) * PREP_R2D);
#endif
        jidx[first + i] = (bi >= 0 && sep < match_radius) ? bi : -1;
    }
}

// one workgroup: the detections of the image with jidx < 0 are appended in object order (their unit vectors too, when given)
__global__ void __launch_bounds__(PREP_BLOCK) prep_append_kernel(const double2 *world, int64_t first, int n, double2 *jpos, int32_t *jcount, int32_t *jidx,
                                                                 const PrepUnit *unit, PrepUnit *junit) {
    typedef hipcub::BlockScan<int, PREP_BLOCK> Scan;
    __shared__ typename Scan::TempStorage tmp;
    const int base = *jcount;
    int run = 0;
    for (int c0 = 0; c0 < n; c0 += PREP_BLOCK) {
        const int i = c0 + (int)threadIdx.x;
        const int flag = (i < n && jidx[first + i] < 0) ? 1 : 0;
        int ex, tot;
        Scan(tmp).ExclusiveSum(flag, ex, tot);
        __syncthreads();
        if (flag) {
#if CELESTE_PREP_MUTANT == 19
            const int k = base + run + (tot - 1 - ex);
#else
            const int k = base + run + ex;
#endif
            jidx[first + i] = k;
            jpos[k] = world[first + i];
            if (unit) junit[k] = unit[first + i];
        }
        run += tot;
    }
    __syncthreads();                               // (every thread has read *jcount)
    if (threadIdx.x == 0) *jcount = base + run;
}

// ooff[s] = the first position of key s in the sorted keys, s = 0 .. S (ooff[S] = D)
__global__ void __launch_bounds__(PREP_BLOCK) prep_object_ranges_kernel(const uint32_t *skey, int64_t D, int64_t S, int64_t *ooff) {
    const int64_t s = (int64_t)blockIdx.x * PREP_BLOCK + threadIdx.x;
    if (s > S) return;
    int64_t lo = 0, hi = D;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)skey[mid] < s) lo = mid + 1; else hi = mid;
    }
    ooff[s] = lo;
}

struct PrepCatalogOut { double *flux, *ratio, *angle, *radius; int32_t *det_image, *det_object; };

__global__ void __launch_bounds__(PREP_BLOCK) prep_entry_kernel(const PrepImg *imgs, const int64_t *off, const celeste_prep_detection_t *det,
                                                                const int32_t *dimg, const int32_t *sdet, const int64_t *ooff, int64_t S,
                                                                const double *angle, double c_radius, PrepCatalogOut O) {
    const int64_t s = (int64_t)blockIdx.x * PREP_BLOCK + threadIdx.x;
    if (s >= S) return;
    int32_t best[5] = {-1, -1, -1, -1, -1}, npix[5] = {0, 0, 0, 0, 0};
    for (int64_t j = ooff[s]; j < ooff[s + 1]; ++j) {
        const int32_t d = sdet[j];
        const int n = dimg[d];
        O.det_image[j] = n;
        O.det_object[j] = (int32_t)((int64_t)d - off[n]);
        const int b = imgs[n].band - 1;
        if (det[d].npix > npix[b]) { npix[b] = det[d].npix; best[b] = d; }
    }
    int bb = 0;
    for (int b = 0; b < 5; ++b) {
        O.flux[5 * s + b] = best[b] >= 0 ? det[best[b]].flux : 0.0;
#if CELESTE_PREP_MUTANT == 20
        if (npix[b] >= npix[bb]) bb = b;
#else
        if (npix[b] > npix[bb]) bb = b;                       // the first band on a tie
#endif
    }
    const int32_t d = best[bb];                               // (an object has a detection, and npix > 0)
    const double a = det[d].a, b = det[d].b;
    O.ratio[s] = b / a;
    O.angle[s] = det[d].theta + angle[dimg[d]];
    O.radius[s] = sqrt(a * b) * c_radius;
}

__device__ __forceinline__ int32_t clamp_i64(int64_t v) { return (int32_t)(v < -2000000000ll ? -2000000000ll : (v > 2000000000ll ? 2000000000ll : v)); }

// first - delta .. last + delta, delta = rint((dilate length) / 2), enclosed with m0 .. m1
__device__ __forceinline__ void dilate_enclose(int32_t first, int32_t last, double dilate, int32_t &m0, int32_t &m1) {
    const double len = (double)((int64_t)last - first + 1);
    const int64_t delta = (int64_t)round_even((dilate * len) / 2.0);
    const int32_t lo = clamp_i64((int64_t)first - delta), hi = clamp_i64((int64_t)last + delta);
#if CELESTE_PREP_MUTANT == 21
    m0 = lo;
#else
    m0 = lo < m0 ? lo : m0;
#endif
    m1 = hi > m1 ? hi : m1;
}

__global__ void __launch_bounds__(PREP_BLOCK) prep_detected_geometry_kernel(const PrepImg *imgs, int N, const int64_t *off, const celeste_prep_detection_t *det,
                                                                            const int32_t *sdet, const int64_t *ooff, const double2 *jpos, int64_t P,
                                                                            double min_radius, double dilate, int dense, int32_t *keep, int4 *pbox,
                                                                            int32_t *err) {
    const int64_t p = (int64_t)blockIdx.x * PREP_BLOCK + threadIdx.x;
    if (p >= P) return;
    const int64_t s = p / N;
    const int n = (int)(p - s * N);
    const PrepImg &im = imgs[n];
    const double2 pos = jpos[s];
    double pc1, pc2;
    world_to_pix(im, pos.x, pos.y, pc1, pc2);
    if (im.kind == CELESTE_PREP_WCS_TAN && !(fabs(pc1) < INFINITY && fabs(pc2) < INFINITY)) {   // behind the plane: the empty box
        keep[p] = dense ? 1 : 0; pbox[p] = make_int4(1, 0, 1, 0); return;
    }
    if (!(pc1 == pc1) || !(pc2 == pc2)) { err[0] = 1; keep[p] = 0; pbox[p] = make_int4(1, 0, 1, 0); return; }
    int32_t r0 = round_even(pc1 - min_radius), r1 = round_even(pc1 + min_radius);
    int32_t c0 = round_even(pc2 - min_radius), c1 = round_even(pc2 + min_radius);
    // the object's last detection in image n: its detections are sorted by their index, image n's are off[n] .. off[n + 1]
    int64_t lo = ooff[s], hi = ooff[s + 1];
    const int64_t a = lo, end = off[n + 1];
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)sdet[mid] < end) lo = mid + 1; else hi = mid;
    }
    if (lo > a && (int64_t)sdet[lo - 1] >= off[n]) {
        const celeste_prep_detection_t &d = det[sdet[lo - 1]];
        dilate_enclose(d.xmin, d.xmax, dilate, r0, r1);
        dilate_enclose(d.ymin, d.ymax, dilate, c0, c1);
    }
    int4 b;
    b.x = clampi(r0, 1, im.H + 1); b.y = clampi(r1, 0, im.H);
    b.z = clampi(c0, 1, im.W + 1); b.w = clampi(c1, 0, im.W);
    pbox[p] = b;
    const bool nonempty = b.y >= b.x && b.w >= b.z;
    keep[p] = (dense || nonempty) ? 1 : 0;
    if (nonempty) atomicMax(&err[1], b.y - b.x + 1);          // (an integer maximum: the neighbour search's row window)
}

extern "C" int celeste_prep_detected_last_ms(float ms[CELESTE_PREP_DETECTED_N_STAGES]) {
    if (!ms) return CELESTE_PREP_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_mu);
    for (int i = 0; i < CELESTE_PREP_DETECTED_N_STAGES; ++i) ms[i] = g_det_ms[i];
    return CELESTE_PREP_OK;
}

extern "C" int celeste_prep_result_get_catalog(const celeste_prep_result_t *result, celeste_prep_catalog_t *catalog) {
    if (!result || !catalog || !result->has_catalog) return CELESTE_PREP_ERR_INVALID_ARG;
    *catalog = result->catalog;
    return CELESTE_PREP_OK;
}

extern "C" int celeste_prep_detected_check(int32_t n_images, const int64_t *det_offsets, const celeste_prep_detection_t *dets,
                                           const double *x_vs_n_angle, double match_radius, double min_radius_pix, double dilate,
                                           uint32_t flags) {
    if (n_images <= 0 || !det_offsets || !x_vs_n_angle || (flags & ~(uint32_t)(CELESTE_PREP_FLAG_DENSE | CELESTE_PREP_FLAG_STAMPS)))
        return CELESTE_PREP_ERR_INVALID_ARG;
    if (!(match_radius >= 0.0) || !(min_radius_pix >= 0.0) || !std::isfinite(min_radius_pix) || !(dilate >= 0.0) || !std::isfinite(dilate))
        return CELESTE_PREP_ERR_INVALID_ARG;
    if (det_offsets[0] != 0) return CELESTE_PREP_ERR_INVALID_ARG;
    for (int n = 0; n < n_images; ++n)
        if (det_offsets[n + 1] < det_offsets[n] || !std::isfinite(x_vs_n_angle[n])) return CELESTE_PREP_ERR_INVALID_ARG;
    const int64_t D = det_offsets[n_images];
    if (D > 0x7fffffff || (D > 0 && !dets)) return CELESTE_PREP_ERR_INVALID_ARG;
    for (int64_t d = 0; d < D; ++d) {
        const celeste_prep_detection_t &t = dets[d];
        if (t.npix <= 0 || t.xmax < t.xmin || t.ymax < t.ymin || !std::isfinite(t.x) || !std::isfinite(t.y) || !std::isfinite(t.a) ||
            !std::isfinite(t.b) || !std::isfinite(t.theta) || !std::isfinite(t.flux) || !(t.a > 0.0))
            return CELESTE_PREP_ERR_INVALID_ARG;
    }
    return CELESTE_PREP_OK;
}

extern "C" int celeste_prep_detected(celeste_prep_images_t *handle, const int64_t *det_offsets, const celeste_prep_detection_t *dets,
                                     const double *x_vs_n_angle, double match_radius, double min_radius_pix, double dilate,
                                     uint32_t flags, celeste_prep_result_t **result) {
    // ---- arguments
    if (!result) return CELESTE_PREP_ERR_INVALID_ARG;
    *result = nullptr;
    if (!handle) return CELESTE_PREP_ERR_INVALID_ARG;
    const int N = handle->n_images;
    int st = celeste_prep_detected_check(N, det_offsets, dets, x_vs_n_angle, match_radius, min_radius_pix, dilate, flags);
    if (st) return st;
    const int64_t D = det_offsets[N];
    if (D * (int64_t)N > 0x7fffffff) return CELESTE_PREP_ERR_INVALID_ARG;      // (S <= D: the pairs fit an int)
    const bool dense = flags & CELESTE_PREP_FLAG_DENSE, want_stamps = (flags & CELESTE_PREP_FLAG_STAMPS) != 0;
    const double c_radius = std::sqrt(2.0 * std::log(2.0));

    std::lock_guard<std::mutex> lk(g_mu);
    PrepCall call;
    if ((st = call.open_detected(handle->device))) return st;
    hipStream_t q = call.stream;
    for (float &m : g_last_ms) m = 0.0f;
    for (float &m : g_det_ms) m = 0.0f;

    // ---- world positions, join, the detections by joined index
    int64_t *d_off, *d_ooff = nullptr; celeste_prep_detection_t *d_det; double *d_angle; double2 *d_world, *d_jpos;
    int32_t *d_dimg, *d_didx, *d_jidx, *d_jcount, *d_sdet; uint32_t *d_skey;
    const bool angular = handle->any_tan != 0;
    PrepUnit *d_unit = nullptr, *d_junit = nullptr;
    if (angular && ((st = call.alloc(&d_unit, (size_t)D)) || (st = call.alloc(&d_junit, (size_t)D)))) return st;
    if ((st = call.alloc(&d_off, (size_t)N + 1)) || (st = call.alloc(&d_det, (size_t)D)) || (st = call.alloc(&d_angle, (size_t)N)) ||
        (st = call.alloc(&d_world, (size_t)D)) || (st = call.alloc(&d_jpos, (size_t)D)) || (st = call.alloc(&d_dimg, (size_t)D)) ||
        (st = call.alloc(&d_didx, (size_t)D)) || (st = call.alloc(&d_jidx, (size_t)D)) || (st = call.alloc(&d_jcount, 1)) ||
        (st = call.alloc(&d_sdet, (size_t)D)) || (st = call.alloc(&d_skey, (size_t)D)))
        return st;
    PREP_HIP(hipEventRecord(call.dev[0], q));
    PREP_HIP(hipMemcpyAsync(d_off, det_offsets, ((size_t)N + 1) * sizeof(int64_t), hipMemcpyHostToDevice, q));
    PREP_HIP(hipMemcpyAsync(d_angle, x_vs_n_angle, (size_t)N * sizeof(double), hipMemcpyHostToDevice, q));
    PREP_HIP(hipMemsetAsync(d_jcount, 0, sizeof(int32_t), q));
    int64_t S = 0;
    if (D > 0) {
        PREP_HIP(hipMemcpyAsync(d_det, dets, (size_t)D * sizeof(celeste_prep_detection_t), hipMemcpyHostToDevice, q));
        hipLaunchKernelGGL(prep_det_world_kernel, dim3(blocks_for(D)), dim3(PREP_BLOCK), 0, q, handle->d_imgs, N, d_off, d_det, D, d_world,
                           d_dimg, d_didx);
        PREP_HIP(hipGetLastError());
        if (angular) {
            hipLaunchKernelGGL(prep_det_unit_kernel, dim3(blocks_for(D)), dim3(PREP_BLOCK), 0, q, d_world, D, d_unit);
            PREP_HIP(hipGetLastError());
        }
        for (int n = 0; n < N; ++n) {
            const int64_t first = det_offsets[n];
            const int cnt = (int)(det_offsets[n + 1] - first);
            if (cnt == 0) continue;
            if (angular)
                hipLaunchKernelGGL(prep_match_angular_kernel, dim3(blocks_for(cnt)), dim3(PREP_BLOCK), 0, q, d_unit, first, cnt, d_junit, d_jcount,
                                   match_radius, d_jidx);
            else
                hipLaunchKernelGGL(prep_match_kernel, dim3(blocks_for(cnt)), dim3(PREP_BLOCK), 0, q, d_world, first, cnt, d_jpos, d_jcount,
                                   match_radius, d_jidx);
            PREP_HIP(hipGetLastError());
            hipLaunchKernelGGL(prep_append_kernel, dim3(1), dim3(PREP_BLOCK), 0, q, d_world, first, cnt, d_jpos, d_jcount, d_jidx,
                               (const PrepUnit *)d_unit, d_junit);
            PREP_HIP(hipGetLastError());
        }
        const int end_bit = bits_for((uint64_t)D);
        size_t tb = 0;
        PREP_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, (const uint32_t *)d_jidx, d_skey, d_didx, d_sdet, (int)D, 0, end_bit, q));
        char *d_tmp;
        if ((st = call.alloc(&d_tmp, tb))) return st;
        PREP_HIP(hipcub::DeviceRadixSort::SortPairs(d_tmp, tb, (const uint32_t *)d_jidx, d_skey, d_didx, d_sdet, (int)D, 0, end_bit, q));
        int32_t count = 0;
        PREP_HIP(hipMemcpyAsync(&count, d_jcount, sizeof(int32_t), hipMemcpyDeviceToHost, q));
        PREP_HIP(hipStreamSynchronize(q));          // the one wait of the join: the pair arrays are sized by the object count
        S = count;
        if (S < 1 || S > D) return CELESTE_PREP_ERR_HIP;
    }
    const int64_t P = S * N;
    if ((st = call.alloc(&d_ooff, (size_t)S + 1))) return st;
    hipLaunchKernelGGL(prep_object_ranges_kernel, dim3(blocks_for(S + 1)), dim3(PREP_BLOCK), 0, q, d_skey, D, S, d_ooff);
    PREP_HIP(hipGetLastError());
    PREP_HIP(hipEventRecord(call.dev[1], q));

    // ---- catalog entries
    PrepCatalogOut O;
    if ((st = call.alloc(&O.flux, (size_t)S * 5)) || (st = call.alloc(&O.ratio, (size_t)S)) || (st = call.alloc(&O.angle, (size_t)S)) ||
        (st = call.alloc(&O.radius, (size_t)S)) || (st = call.alloc(&O.det_image, (size_t)D)) || (st = call.alloc(&O.det_object, (size_t)D)))
        return st;
    if (S > 0) {
        hipLaunchKernelGGL(prep_entry_kernel, dim3(blocks_for(S)), dim3(PREP_BLOCK), 0, q, handle->d_imgs, d_off, d_det, d_dimg, d_sdet,
                           d_ooff, S, d_angle, c_radius, O);
        PREP_HIP(hipGetLastError());
    }
    PREP_HIP(hipEventRecord(call.dev[2], q));

    // ---- boxes, then the table stages of celeste_prep_patches
    PrepPairs G;
    if ((st = G.alloc(call, P))) return st;
    PREP_HIP(hipEventRecord(call.ev[0], q));
    if (P > 0) {
        PREP_HIP(hipMemsetAsync(G.err, 0, 2 * sizeof(int32_t), q));
        hipLaunchKernelGGL(prep_detected_geometry_kernel, dim3(blocks_for(P)), dim3(PREP_BLOCK), 0, q, handle->d_imgs, N, d_off, d_det, d_sdet,
                           d_ooff, d_jpos, P, min_radius_pix, dilate, dense ? 1 : 0, G.keep, G.pbox, G.err);
        PREP_HIP(hipGetLastError());
    }
    PrepExtra X[8] = {{d_jpos, (size_t)S * 16, 0, nullptr},      {O.flux, (size_t)S * 40, 0, nullptr},
                      {O.ratio, (size_t)S * 8, 0, nullptr},      {O.angle, (size_t)S * 8, 0, nullptr},
                      {O.radius, (size_t)S * 8, 0, nullptr},     {d_ooff, (size_t)(S + 1) * 8, 0, nullptr},
                      {O.det_image, (size_t)D * 4, 0, nullptr},  {O.det_object, (size_t)D * 4, 0, nullptr}};
    if ((st = prep_table_stages(handle, call, S, P, G, -1, want_stamps, X, 8, result))) return st;
    celeste_prep_result *res = *result;
    celeste_prep_catalog_t &K = res->catalog;
    memset(&K, 0, sizeof K);
    K.n_objects = S; K.n_detections = D;
    K.pos = (const double *)X[0].host; K.flux = (const double *)X[1].host; K.gal_axis_ratio = (const double *)X[2].host;
    K.gal_angle = (const double *)X[3].host; K.gal_radius_px = (const double *)X[4].host; K.det_offsets = (const int64_t *)X[5].host;
    K.det_image = (const int32_t *)X[6].host; K.det_object = (const int32_t *)X[7].host;
    res->has_catalog = true;
    (void)hipEventElapsedTime(&g_det_ms[0], call.dev[0], call.dev[1]);
    (void)hipEventElapsedTime(&g_det_ms[1], call.dev[1], call.dev[2]);
    for (int i = 0; i < 4; ++i) g_det_ms[2 + i] = g_last_ms[i];
    return CELESTE_PREP_OK;
}
