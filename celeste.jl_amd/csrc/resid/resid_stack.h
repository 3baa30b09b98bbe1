// resid_stack.h -- the stack of a search's maps across images on a sky grid (include/celeste_resid.h, "The stack").
//
// Included by celeste_resid.hip after its kernels: the peak kernels, PeakImg, resid_subpixel and wave_max are used here.
//   resid_stack_kernel     a workgroup of 256 owns 32 x 8 cells of the grid (h fastest, as the planes).  A cell's world position
//                          (and its sin dec, cos dec for the tangent-plane images) is computed once; the images of the call
//                          come through LDS in batches of SK_BATCH records (WCS, plane offset, H, W, band), so any number of
//                          images fits; up to 8 channels accumulate in registers in one pass over the images, in the call's
//                          order; writes N, D, z, count per channel and the tile's z range per channel
//   stack_zrange_kernel    one workgroup per channel: cells with a z, z_max, z_min
//   peaks_count / peaks_scan / peaks_write   (celeste_resid.hip) over the channels' z planes
//   stack_finish_kernel    a candidate's record: the count at its cell and grid.pix_to_world(h + 1 + dh, w + 1 + dw)
// A gather: three 8-byte loads per (cell, image) at addresses that follow the projected tile -- neighbouring lanes read
// neighbouring pixels when the image is aligned with the grid, a rotated image spreads a wavefront over a few columns.  No
// atomic, no scatter; every number repeats bit for bit.  No expression here is contracted into an FMA (the numpy restatement
// repeats the sums and the projections).
//
// Culling is uniform over the workgroup: lanes project the tile's four corner cells into the images of a batch, one lane
// per image folds them into a flag in LDS, and all lanes read it.
#pragma once

// Mutation testing (tests/test_stack_mutants.py builds the library with -DCELESTE_STACK_MUTANT=k and checks that
// tests/test_gpu_stack.py notices; a macro of its own: CELESTE_RESID_MUTANT's numbers keep their meaning).  A mutant changes
// arithmetic, a comparison or an index inside the same plane; never a size, a launch, a barrier or a range check.  0 = the product;
//   1 = D weighted by s instead of s * s
//   2 = the projected coordinate truncated instead of rounded to nearest (the range check that follows is the product's)
//   3 = the gather reads the image's planes transposed: index qw + W qh (<= W - 1 + W (H - 1) = H W - 1)
//   4 = a pixel whose z is NaN is not skipped
//   5 = min_images compared with > instead of >=
//   6 = culling without its one-pixel margin
// Never defined in the shipped build.
#ifndef CELESTE_STACK_MUTANT
#define CELESTE_STACK_MUTANT 0
#endif

#define SK_TH 32                         // rows of a tile
#define SK_TW 8                          // columns of a tile
#define SK_BATCH 16                      // image records staged in LDS at a time
#define SK_MAXCH CELESTE_RESID_STACK_MAX_CHANNELS
#define SK_D2R (M_PI / 180.0)
#define SK_R2D (180.0 / M_PI)

// fwd: world -> pixel (AFFINE: J11, J12, J21, J22; TAN: cd^-1); inv: pixel -> world (AFFINE: J^-1; TAN: cd); both row-major
struct StackWcs {
    int32_t kind, pad;
    double fwd[4], inv[4], w0[2], p0[2], sin0, cos0;
};
struct StackGrid { int32_t H, W; StackWcs wcs; };
// an image of the call (13 doubles: staged word by word)
struct StackImg {
    int32_t kind, band, H, W;
    int64_t off;                         // its planes in the search's buffers
    double fwd[4], w0[2], p0[2], sin0, cos0;
};
static_assert(sizeof(StackImg) == 13 * sizeof(double), "StackImg is staged as 13 doubles");
struct StackTileRec { double z_max, z_min; int32_t n, pad; };

// (ra, dec) and, for the tangent-plane images, sin dec and cos dec
struct StackWorld { double w1, w2, sd, cd; };

__device__ __forceinline__ StackWorld stack_pix_to_world(const StackWcs &g, double c1, double c2) {
#pragma clang fp contract(off)
    StackWorld o;
    const double u = c1 - g.p0[0], v = c2 - g.p0[1];
    if (g.kind == CELESTE_RESID_WCS_TAN) {
        const double x = (g.inv[0] * u + g.inv[1] * v) * SK_D2R, y = (g.inv[2] * u + g.inv[3] * v) * SK_D2R;
        const double den = g.cos0 - y * g.sin0, num = g.sin0 + y * g.cos0;
        o.w1 = g.w0[0] + atan2(x, den) * SK_R2D;
        const double hyp = hypot(x, den);
        // num cos0 - hyp sin0 = y - sin0 x^2 / (hyp + den), without the cancellation
        o.w2 = g.w0[1] + atan2(y - g.sin0 * ((x * x) / (hyp + den)), num * g.sin0 + hyp * g.cos0) * SK_R2D;
    } else {
        o.w1 = (g.inv[0] * u + g.inv[1] * v) + g.w0[0];
        o.w2 = (g.inv[2] * u + g.inv[3] * v) + g.w0[1];
    }
    sincos(o.w2 * SK_D2R, &o.sd, &o.cd);
    return o;
}

// NaN behind the tangent plane
__device__ __forceinline__ void stack_world_to_pix(const StackImg &im, const StackWorld &p, double &pc1, double &pc2) {
#pragma clang fp contract(off)
    if (im.kind == CELESTE_RESID_WCS_TAN) {
        const double da = (p.w1 - im.w0[0]) * SK_D2R;
        double sa, ca;
        sincos(da, &sa, &ca);
        const double l = p.cd * sa;
        const double sh = sin(0.5 * da);
        // sin dec cos0 - cos dec sin0 cos da as sin(dec - dec0) + 2 cos dec sin0 sin^2(da / 2)
        const double m = sin((p.w2 - im.w0[1]) * SK_D2R) + (2.0 * (p.cd * im.sin0)) * (sh * sh);
        const double n = p.sd * im.sin0 + (p.cd * im.cos0) * ca;
        if (!(n > 0.0)) { pc1 = NAN; pc2 = NAN; return; }
        const double x = (l / n) * SK_R2D, y = (m / n) * SK_R2D;
        pc1 = im.p0[0] + (im.fwd[0] * x + im.fwd[1] * y);
        pc2 = im.p0[1] + (im.fwd[2] * x + im.fwd[3] * y);
    } else {
        const double d1 = p.w1 - im.w0[0], d2 = p.w2 - im.w0[1];
        pc1 = (im.fwd[0] * d1 + im.fwd[1] * d2) + im.p0[0];
        pc2 = (im.fwd[2] * d1 + im.fwd[3] * d2) + im.p0[1];
    }
}

// NCH: the channels held in registers (n_ch <= NCH; the weights of the others are zero)
template <int NCH>
__global__ void __launch_bounds__(256)
resid_stack_kernel(const StackGrid g, const StackImg *__restrict__ imgs, int n_img, const double *__restrict__ wts, int n_ch,
                   int min_images, int cull, const double *__restrict__ n_plane, const double *__restrict__ d_plane,
                   const double *__restrict__ z_plane, double *__restrict__ oN, double *__restrict__ oD, double *__restrict__ oZ,
                   int32_t *__restrict__ oC, StackTileRec *__restrict__ rec) {
    __shared__ StackImg simg[SK_BATCH];
    __shared__ double swt[SK_MAXCH * 5];
    __shared__ StackWorld corner[4];
    __shared__ double cp[SK_BATCH][4][2];
    __shared__ int skip[SK_BATCH];
    __shared__ double shz[SK_MAXCH][2][4];
    __shared__ int shn[SK_MAXCH][4];
    const int t = threadIdx.x;
    const int H = g.H, W = g.W;
    const int tiles_h = (H + SK_TH - 1) / SK_TH;
    const int tw_i = (int)(blockIdx.x / (unsigned)tiles_h), th_i = (int)(blockIdx.x - (unsigned)tw_i * (unsigned)tiles_h);
    const int h0 = th_i * SK_TH, w0 = tw_i * SK_TW;
    const int h = h0 + (t & (SK_TH - 1)), w = w0 + (t >> 5);
    const bool inb = h < H && w < W;
    if (t < SK_MAXCH * 5) swt[t] = t < n_ch * 5 ? wts[t] : 0.0;
    if (t < 4) {                                              // the tile's corner cells, inside the grid
        const int ch = (t & 1) ? min(h0 + SK_TH, H) - 1 : h0, cw = (t & 2) ? min(w0 + SK_TW, W) - 1 : w0;
        corner[t] = stack_pix_to_world(g.wcs, (double)(ch + 1), (double)(cw + 1));
    }
    const StackWorld me = stack_pix_to_world(g.wcs, (double)(min(h, H - 1) + 1), (double)(min(w, W - 1) + 1));
    double Ns[NCH], Ds[NCH];
    int cnt[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) { Ns[k] = 0.0; Ds[k] = 0.0; cnt[k] = 0; }
    for (int b0 = 0; b0 < n_img; b0 += SK_BATCH) {            // (uniform over the workgroup)
        const int nb = min(SK_BATCH, n_img - b0);
        __syncthreads();
        {
            const double *s = reinterpret_cast<const double *>(imgs + b0);
            double *d = reinterpret_cast<double *>(simg);
            if (t < nb * 13) d[t] = s[t];
        }
        __syncthreads();
        if (cull) {
            if (t < nb * 4) stack_world_to_pix(simg[t >> 2], corner[t & 3], cp[t >> 2][t & 3][0], cp[t >> 2][t & 3][1]);
            __syncthreads();
            if (t < nb) {
                const StackImg &im = simg[t];
                double lo1 = INFINITY, hi1 = -INFINITY, lo2 = INFINITY, hi2 = -INFINITY;
                bool front = true;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const double a = cp[t][c][0], b = cp[t][c][1];
                    front &= isfinite(a) && isfinite(b);
                    lo1 = fmin(lo1, a); hi1 = fmax(hi1, a); lo2 = fmin(lo2, b); hi2 = fmax(hi2, b);
                }
#if CELESTE_STACK_MUTANT == 6
                const double mg = 0.0;
#else
                const double mg = 1.0;
#endif
                const bool miss = hi1 + mg < 1.0 || lo1 - mg > (double)im.H || hi2 + mg < 1.0 || lo2 - mg > (double)im.W;
                skip[t] = front && im.kind == g.wcs.kind && miss;
            }
            __syncthreads();
        }
        for (int i = 0; i < nb; ++i) {
            if (cull && skip[i]) continue;                    // (LDS: the same for every lane)
            const StackImg &im = simg[i];
            double p1, p2;
            stack_world_to_pix(im, me, p1, p2);
#if CELESTE_STACK_MUTANT == 2
            const double r1 = trunc(p1), r2 = trunc(p2);
#else
            const double r1 = rint(p1), r2 = rint(p2);
#endif
            // the range check in double: NaN and anything an int cannot hold end here
            if (!(inb && r1 >= 1.0 && r1 <= (double)im.H && r2 >= 1.0 && r2 <= (double)im.W)) continue;
            const int qh = (int)r1 - 1, qw = (int)r2 - 1;
#if CELESTE_STACK_MUTANT == 3
            const int64_t gi = im.off + (int64_t)qw + (int64_t)im.W * qh;
#else
            const int64_t gi = im.off + (int64_t)qh + (int64_t)im.H * qw;
#endif
#if CELESTE_STACK_MUTANT != 4
            if (isnan(z_plane[gi])) continue;
#endif
            const double Nv = n_plane[gi], Dv = d_plane[gi];
#pragma unroll
            for (int k = 0; k < NCH; ++k) {
                const double s = swt[k * 5 + im.band - 1];
                if (s > 0.0) {
                    Ns[k] = __dadd_rn(Ns[k], __dmul_rn(s, Nv));
#if CELESTE_STACK_MUTANT == 1
                    Ds[k] = __dadd_rn(Ds[k], __dmul_rn(s, Dv));
#else
                    Ds[k] = __dadd_rn(Ds[k], __dmul_rn(__dmul_rn(s, s), Dv));
#endif
                    ++cnt[k];
                }
            }
        }
    }
    const int64_t HW = (int64_t)H * W, ci = (int64_t)h + (int64_t)H * w;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        if (k >= n_ch) break;                                 // (uniform)
#if CELESTE_STACK_MUTANT == 5
        const bool has = inb && cnt[k] > min_images && Ds[k] > 0.0;
#else
        const bool has = inb && cnt[k] >= min_images && Ds[k] > 0.0;
#endif
        const double z = has ? Ns[k] / sqrt(Ds[k]) : (double)NAN;
        if (inb) {
            oN[k * HW + ci] = Ns[k];
            oD[k * HW + ci] = Ds[k];
            oZ[k * HW + ci] = z;
            oC[k * HW + ci] = cnt[k];
        }
        const bool fin = has && !isnan(z);
        const double zmax = wave_max(fin ? z : -INFINITY), zmin = -wave_max(fin ? -z : -INFINITY);
        const unsigned long long bal = __ballot(fin);
        if ((t & 63) == 0) { shz[k][0][t >> 6] = zmax; shz[k][1][t >> 6] = zmin; shn[k][t >> 6] = __popcll(bal); }
    }
    __syncthreads();
    if (t < n_ch) {
        StackTileRec r;
        r.z_max = fmax(fmax(shz[t][0][0], shz[t][0][1]), fmax(shz[t][0][2], shz[t][0][3]));
        r.z_min = fmin(fmin(shz[t][1][0], shz[t][1][1]), fmin(shz[t][1][2], shz[t][1][3]));
        r.n = shn[t][0] + shn[t][1] + shn[t][2] + shn[t][3];
        r.pad = 0;
        rec[(int64_t)t * gridDim.x + blockIdx.x] = r;
    }
}

// one workgroup per channel over its n_tiles tile records
__global__ void __launch_bounds__(256)
stack_zrange_kernel(const StackTileRec *__restrict__ rec, int n_tiles, celeste_resid_stack_frame_t *__restrict__ frames) {
    __shared__ double shz[2][4];
    __shared__ long long shn[4];
    const int k = blockIdx.x, t = threadIdx.x;
    double zmax = -INFINITY, zmin = INFINITY;
    long long n = 0;
    for (int i = t; i < n_tiles; i += 256) {
        const StackTileRec r = rec[(int64_t)k * n_tiles + i];
        zmax = fmax(zmax, r.z_max); zmin = fmin(zmin, r.z_min); n += r.n;
    }
    zmax = wave_max(zmax);
    zmin = -wave_max(-zmin);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((t & 63) == 0) { shz[0][t >> 6] = zmax; shz[1][t >> 6] = zmin; shn[t >> 6] = n; }
    __syncthreads();
    if (t == 0) {
        celeste_resid_stack_frame_t f;
        f.channel = k; f.reserved = 0;
        f.n_cells = shn[0] + shn[1] + shn[2] + shn[3];
        zmax = fmax(fmax(shz[0][0], shz[0][1]), fmax(shz[0][2], shz[0][3]));
        zmin = fmin(fmin(shz[1][0], shz[1][1]), fmin(shz[1][2], shz[1][3]));
        f.z_max = zmax >= zmin ? zmax : (double)NAN;
        f.z_min = zmax >= zmin ? zmin : (double)NAN;
        frames[k] = f;
    }
}

// the stack's record of candidate i from the peak kernels' (image = channel; cov is not read)
__global__ void stack_finish_kernel(int64_t n, const celeste_resid_candidate_t *__restrict__ in, const StackGrid g,
                                    const int32_t *__restrict__ oC, celeste_resid_stack_candidate_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const celeste_resid_candidate_t c = in[i];
    celeste_resid_stack_candidate_t o;
    o.channel = c.image; o.h = c.h; o.w = c.w;
    o.n_images = oC[(int64_t)c.image * ((int64_t)g.H * g.W) + (int64_t)c.h + (int64_t)g.H * c.w];
    o.dh = c.dh; o.dw = c.dw; o.z = c.z; o.f = c.f; o.D = c.D;
    const StackWorld p = stack_pix_to_world(g.wcs, __dadd_rn((double)(c.h + 1), c.dh), __dadd_rn((double)(c.w + 1), c.dw));
    o.world[0] = p.w1; o.world[1] = p.w2;
    out[i] = o;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
static bool stack_wcs_ok(const celeste_resid_wcs_t &w) {
    if (w.kind != CELESTE_RESID_WCS_AFFINE && w.kind != CELESTE_RESID_WCS_TAN) return false;
    for (int k = 0; k < 2; ++k) if (!std::isfinite(w.world0[k]) || !std::isfinite(w.pix0[k])) return false;
    for (int k = 0; k < 4; ++k) if (!std::isfinite(w.m[k])) return false;
    const double det = w.kind == CELESTE_RESID_WCS_TAN ? w.m[0] * w.m[3] - w.m[1] * w.m[2] : w.m[0] * w.m[3] - w.m[2] * w.m[1];
    if (det == 0.0 || !std::isfinite(det)) return false;
    return w.kind != CELESTE_RESID_WCS_TAN || std::fabs(w.world0[1]) <= 90.0;
}

// the device's record of a checked WCS: the matrix, its inverse by the adjugate, sin0 and cos0 from the host's libm
static StackWcs stack_wcs_dev(const celeste_resid_wcs_t &w) {
    StackWcs d;
    d.kind = w.kind; d.pad = 0;
    for (int k = 0; k < 2; ++k) { d.w0[k] = w.world0[k]; d.p0[k] = w.pix0[k]; }
    // a = the given matrix, row-major (AFFINE is given by columns)
    double a[4];
    if (w.kind == CELESTE_RESID_WCS_TAN) { a[0] = w.m[0]; a[1] = w.m[1]; a[2] = w.m[2]; a[3] = w.m[3]; }
    else { a[0] = w.m[0]; a[1] = w.m[2]; a[2] = w.m[1]; a[3] = w.m[3]; }
    const double det = a[0] * a[3] - a[1] * a[2];
    const double ai[4] = {a[3] / det, -a[1] / det, -a[2] / det, a[0] / det};
    const bool tan = w.kind == CELESTE_RESID_WCS_TAN;        // TAN is given pixel -> world, AFFINE world -> pixel
    for (int k = 0; k < 4; ++k) { d.fwd[k] = tan ? ai[k] : a[k]; d.inv[k] = tan ? a[k] : ai[k]; }
    const double d0 = w.world0[1] * SK_D2R;
    d.sin0 = tan ? std::sin(d0) : 0.0; d.cos0 = tan ? std::cos(d0) : 1.0;
    return d;
}
