// celeste_synth.hip -- libceleste_synth.so: the reference's Synthetic.gen_images! on gfx950 (include/celeste_synth.h).
//
// Per call:
//   spline_prefilter_kernel  (elbo_kernels.h) conditions and prefilters every raw PSF stamp, as celeste_ctx_create does.
//   syn_tables_kernel        one wavefront per galaxy entry: its PSF (x) prototype component table (prep_visit_values of
//                            elbo_kernels.h), once, in HBM (14 K records of 64 bytes).
//   syn_pixel_kernel         one 256-thread workgroup per tile of 64 (h) x 32 (w) pixels.  A wavefront covers 64
//                            consecutive h of one column (planes are column-major: loads and stores coalesce) and 8 of
//                            the tile's columns; a lane keeps its 8 sums in registers.  The tile's entries -- a list the
//                            host builds in entry order, so every pixel adds its sources in catalog order and no atomics
//                            are needed -- are staged through LDS 64 headers at a time; box tests on the column are
//                            wave-uniform.  A galaxy's component table is copied into LDS once per tile.  Then
//                            lambda = sum * iota, written as fp64 and / or sampled (synth_sampler.h) and written as
//                            Float32: the fp64 plane exists in HBM only when the caller asks for it.  A tile without
//                            entries reads the sky, samples and stores.
//   syn_sample_kernel        celeste_synth_sample: one lane per element of a caller's fp64 array.
// The densities are the VI kernels' own (star_value, galaxy_value); their code is included, not copied.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "../elbo_kernels.h"
#include "../host_tables.h"
#include "../../../include/celeste_synth.h"
#include "synth_sampler.h"

#define SYN_TH 64          // tile height: one wavefront along h
#define SYN_TW 32          // tile width
#define SYN_WAVES 4
#define SYN_COLS (SYN_TW / SYN_WAVES)
#define SYN_CHUNK 64       // entry headers per LDS stage
#define SYN_NCMAX (14 * CELESTE_SYNTH_MAX_K)

struct SynImage {
    int32_t H, W, K;
    uint32_t stream;
    const float *sky;
    const float *iota;
    double *lam;       // or nullptr
    float *pix;        // or nullptr
};

struct SynEntry {      // 48 bytes
    int32_t h0, h1, w0, w1;     // 1-based, inclusive
    int32_t stamp;              // star: stamp index; galaxy: -1
    int32_t table;              // galaxy: index of its component table
    double m1, m2, flux;
};

struct SynGalaxy {
    int32_t image, pad;
    double shape[4];            // frac_dev, axis_ratio, angle, radius
};

struct SynTile {
    int32_t image, h_start, w_start;   // 0-based first pixel
    int32_t ent_begin, ent_count;      // the tile's slice of the entry list
};

struct SynArgs {
    const SynImage *images;
    const SynTile *tiles;
    const int32_t *tile_ent;
    const SynEntry *entries;
    const double *coefs;
    const Comp *tables;
    unsigned long long *n_capped;
    uint32_t k0, k1;
    int32_t expectation;
};

__global__ void __launch_bounds__(64) syn_tables_kernel(const SynGalaxy *gal, const SynImage *images, const double *psfs, Comp *tables) {
    __shared__ DevPatch P;
    __shared__ double vs[6];
    const int g = blockIdx.x, lane = threadIdx.x;
    const SynGalaxy G = gal[g];
    const int K = images[G.image].K;
    if (lane < 6 * CEL_MAXK) P.psf[lane] = lane < 6 * K ? psfs[(size_t)G.image * (6 * CEL_MAXK) + lane] : 0.0;
    if (lane < 4) { P.J[lane] = 0.0; vs[2 + lane] = G.shape[lane]; }
    if (lane < 2) { P.wc[lane] = 0.0; P.pc[lane] = 0.0; vs[lane] = 0.0; }
    __syncthreads();
    prep_visit_values<false>(lane, vs, P, 0, K, nullptr, tables + (size_t)g * SYN_NCMAX);
}

__global__ void __launch_bounds__(256) syn_pixel_kernel(SynArgs A, int tile0) {
    __shared__ SynEntry ent[SYN_CHUNK];
    __shared__ Comp tc[SYN_NCMAX];
    __shared__ double etab[64];
    exp_table_init(etab);
    const SynTile T = A.tiles[tile0 + blockIdx.x];
    const SynImage img = A.images[T.image];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int h = T.h_start + lane + 1;                 // 1-based
    const bool row_ok = h <= img.H;
    const int NC = 14 * img.K;
    double acc[SYN_COLS];
#pragma unroll
    for (int j = 0; j < SYN_COLS; ++j) {
        const int w = T.w_start + wv + SYN_WAVES * j + 1;
        acc[j] = (row_ok && w <= img.W) ? (double)img.sky[(size_t)(h - 1) + (size_t)img.H * (w - 1)] : 0.0;
    }
    const double hh = (double)h;
    for (int c0 = 0; c0 < T.ent_count; c0 += SYN_CHUNK) {
        const int nc = min(SYN_CHUNK, T.ent_count - c0);
        __syncthreads();
        if ((int)threadIdx.x < nc) ent[threadIdx.x] = A.entries[A.tile_ent[T.ent_begin + c0 + threadIdx.x]];
        __syncthreads();
        for (int e = 0; e < nc; ++e) {
            // the entry is the same for the whole workgroup: a galaxy's component table goes through LDS once per tile
            const int stamp = ent[e].stamp;
            if (stamp < 0) {
                __syncthreads();
                const double *src = reinterpret_cast<const double *>(A.tables + (size_t)ent[e].table * SYN_NCMAX);
                for (int k = threadIdx.x; k < NC * (int)(sizeof(Comp) / sizeof(double)); k += 256) reinterpret_cast<double *>(tc)[k] = src[k];
                __syncthreads();
            }
            const int h0 = ent[e].h0, h1 = ent[e].h1, w0 = ent[e].w0, w1 = ent[e].w1;
            const double m1 = ent[e].m1, m2 = ent[e].m2, flux = ent[e].flux;
            const double *coef = A.coefs + (size_t)(stamp < 0 ? 0 : stamp) * (CEL_COEF * CEL_COEF);
            if (row_ok && h >= h0 && h <= h1) {                                   // per lane; the barriers stay outside
#pragma unroll
                for (int j = 0; j < SYN_COLS; ++j) {
                    const int w = T.w_start + wv + SYN_WAVES * j + 1;             // wave-uniform
                    if (w < w0 || w > w1) continue;                               // (w1 <= W)
                    const double ww = (double)w;
                    const double f = stamp >= 0 ? star_value(coef, hh - m1 + 26.0, ww - m2 + 26.0)
                                                : galaxy_value(tc, NC, hh - m1, ww - m2, etab);
                    acc[j] += f * flux;
                }
            }
        }
    }
    if (!row_ok) return;
    const double iota = (double)img.iota[h - 1];
    unsigned long long ncap = 0;
    for (int j = 0; j < SYN_COLS; ++j) {
        const int w = T.w_start + wv + SYN_WAVES * j + 1;
        if (w > img.W) continue;
        const size_t q = (size_t)(h - 1) + (size_t)img.H * (w - 1);
        const double lam = acc[j] * iota;
        if (img.lam) img.lam[q] = lam;
        if (img.pix) {
            bool capped = false;
            img.pix[q] = A.expectation ? (float)lam : syn_poisson(lam, A.k0, A.k1, (uint32_t)q, img.stream, &capped);
            ncap += capped ? 1 : 0;
        }
    }
    if (ncap) atomicAdd(A.n_capped, ncap);     // an integer count; never reached on finite images (64 blocks)
}

__global__ void __launch_bounds__(256) syn_sample_kernel(const double *lam, float *pix, int64_t n, uint32_t k0, uint32_t k1,
                                                           uint32_t stream, uint32_t first_index, unsigned long long *n_capped) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    bool capped = false;
    pix[i] = syn_poisson(lam[i], k0, k1, first_index + (uint32_t)i, stream, &capped);
    if (capped) atomicAdd(n_capped, 1ull);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
#define SYN_HIP(expr) do { if ((expr) != hipSuccess) { (void)hipGetLastError(); return CELESTE_SYNTH_ERR_HIP; } } while (0)

static std::mutex g_mu;                 // one call at a time
static float g_last_ms[3] = {0, 0, 0};

// One stream per device, made on first use and kept for the life of the process (calls are serialised by g_mu): the HIP
// runtime has been seen writing into a stream object after hipStreamDestroy freed it (profiles/r08_stale_stream_write.md),
// so this library destroys none.
static hipStream_t g_streams[64] = {};

// the device buffers and the events of one call
struct SynCall {
    std::vector<void *> bufs;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    ~SynCall() {
        if (stream) (void)hipStreamSynchronize(stream);
        for (auto e : ev) if (e) (void)hipEventDestroy(e);
        for (void *p : bufs) (void)hipFree(p);
    }
    int open(int device) {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { (void)hipGetLastError(); return CELESTE_SYNTH_ERR_NO_DEVICE; }
        if (device >= count) return CELESTE_SYNTH_ERR_INVALID_ARG;
        SYN_HIP(hipSetDevice(device));
        if (!g_streams[device]) SYN_HIP(hipStreamCreateWithFlags(&g_streams[device], hipStreamNonBlocking));
        stream = g_streams[device];
        for (auto &e : ev) SYN_HIP(hipEventCreate(&e));
        return CELESTE_SYNTH_OK;
    }
    template <class T> int up(T **dst, const T *src, size_t n) {
        void *p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); return CELESTE_SYNTH_ERR_ALLOC; }
        bufs.push_back(p);
        if (src && n) SYN_HIP(hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyHostToDevice, stream));
        *dst = (T *)p;
        return CELESTE_SYNTH_OK;
    }
};

// the constants of this code object: galaxy prototypes, the exponential's table; once per device
static int syn_constants(int device) {
    static bool ready[64] = {};
    if (ready[device]) return CELESTE_SYNTH_OK;
    double eta[16], nu[16];
    galaxy_prototypes(eta, nu);
    SYN_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_eta), eta, sizeof eta));
    SYN_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_nu), nu, sizeof nu));
    hipLaunchKernelGGL(exp_table_kernel, dim3(1), dim3(64), 0, nullptr);
    SYN_HIP(hipGetLastError());
    SYN_HIP(hipStreamSynchronize(nullptr));
    ready[device] = true;
    return CELESTE_SYNTH_OK;
}

extern "C" int celeste_synth_version(void) { return CELESTE_SYNTH_ABI_VERSION; }

extern "C" const char *celeste_synth_strerror(int status) {
    switch (status) {
        case CELESTE_SYNTH_OK: return "ok";
        case CELESTE_SYNTH_ERR_INVALID_ARG: return "invalid argument";
        case CELESTE_SYNTH_ERR_NO_DEVICE: return "no HIP device (there is no CPU fallback)";
        case CELESTE_SYNTH_ERR_HIP: return "HIP runtime error";
        case CELESTE_SYNTH_ERR_ALLOC: return "allocation failed";
        default: return "unknown status";
    }
}

extern "C" int celeste_synth_last_ms(float ms[3]) {
    if (!ms) return CELESTE_SYNTH_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_mu);
    for (int i = 0; i < 3; ++i) ms[i] = g_last_ms[i];
    return CELESTE_SYNTH_OK;
}

extern "C" int celeste_synth_generate(int device, int32_t n_images, const celeste_synth_image_t *images, int64_t n_entries,
                                      const celeste_synth_entry_t *entries, int32_t n_stamps, const double *stamps, uint64_t seed,
                                      uint32_t flags, int32_t chunk_tiles, int64_t *n_capped) {
    // ---- arguments: everything is checked before the first HIP call
    if (device < 0 || device >= 64 || n_images <= 0 || !images || n_entries < 0 || (n_entries && !entries) || n_stamps < 0 || (n_stamps && !stamps) ||
        chunk_tiles < 0 || (flags & ~(uint32_t)CELESTE_SYNTH_FLAG_EXPECTATION))
        return CELESTE_SYNTH_ERR_INVALID_ARG;
    int64_t n_tiles = 0;
    std::vector<int64_t> tile_base((size_t)n_images + 1, 0);
    for (int n = 0; n < n_images; ++n) {
        const celeste_synth_image_t &im = images[n];
        if (im.H <= 0 || im.W <= 0 || (int64_t)im.H * im.W > 0x7fffffff || im.psf_K < 1 || im.psf_K > CELESTE_SYNTH_MAX_K || !im.sky ||
            !im.nelec_per_nmgy || !im.psf || (!im.lambda_out && !im.pixels_out))
            return CELESTE_SYNTH_ERR_INVALID_ARG;
        n_tiles += (int64_t)((im.H + SYN_TH - 1) / SYN_TH) * ((im.W + SYN_TW - 1) / SYN_TW);
        tile_base[n + 1] = n_tiles;
    }
    if (n_tiles > 0x7fffffff) return CELESTE_SYNTH_ERR_INVALID_ARG;
    std::vector<int32_t> tile_cnt((size_t)n_tiles + 1, 0);
    int64_t n_gal = 0, n_list = 0;
    for (int64_t e = 0; e < n_entries; ++e) {
        const celeste_synth_entry_t &E = entries[e];
        if (E.image < 0 || E.image >= n_images || E.source < 0) return CELESTE_SYNTH_ERR_INVALID_ARG;
        if (e && (E.image < entries[e - 1].image || (E.image == entries[e - 1].image && E.source <= entries[e - 1].source)))
            return CELESTE_SYNTH_ERR_INVALID_ARG;                                  // sorted by (image, source)
        const celeste_synth_image_t &im = images[E.image];
        if (E.h0 < 1 || E.h1 > im.H || E.h1 < E.h0 || E.w0 < 1 || E.w1 > im.W || E.w1 < E.w0) return CELESTE_SYNTH_ERR_INVALID_ARG;
        if (E.is_star) { if (E.stamp < 0 || E.stamp >= n_stamps) return CELESTE_SYNTH_ERR_INVALID_ARG; }
        else ++n_gal;
        const int ntw = (im.W + SYN_TW - 1) / SYN_TW;
        for (int th = (E.h0 - 1) / SYN_TH; th <= (E.h1 - 1) / SYN_TH; ++th)
            for (int tw = (E.w0 - 1) / SYN_TW; tw <= (E.w1 - 1) / SYN_TW; ++tw) {
                ++tile_cnt[(size_t)(tile_base[E.image] + (int64_t)th * ntw + tw)];
                ++n_list;
            }
    }
    if (n_list > 0x7fffffff || n_entries > 0x7fffffff) return CELESTE_SYNTH_ERR_INVALID_ARG;
    // ---- the tables: tiles with their entry lists (in entry order), compact entries, galaxies
    std::vector<SynTile> tiles((size_t)n_tiles);
    {
        int32_t at = 0;
        for (int n = 0; n < n_images; ++n) {
            const int ntw = (images[n].W + SYN_TW - 1) / SYN_TW;
            for (int64_t t = tile_base[n]; t < tile_base[n + 1]; ++t) {
                const int64_t l = t - tile_base[n];
                SynTile &T = tiles[(size_t)t];
                T.image = n; T.h_start = (int32_t)(l / ntw) * SYN_TH; T.w_start = (int32_t)(l % ntw) * SYN_TW;
                T.ent_begin = at; T.ent_count = 0;
                at += tile_cnt[(size_t)t];
            }
        }
    }
    std::vector<int32_t> tile_ent((size_t)n_list);
    std::vector<SynEntry> ents((size_t)n_entries);
    std::vector<SynGalaxy> gals((size_t)n_gal);
    {
        int32_t g = 0;
        for (int64_t e = 0; e < n_entries; ++e) {
            const celeste_synth_entry_t &E = entries[e];
            SynEntry &D = ents[(size_t)e];
            D.h0 = E.h0; D.h1 = E.h1; D.w0 = E.w0; D.w1 = E.w1; D.m1 = E.m[0]; D.m2 = E.m[1]; D.flux = E.flux;
            if (E.is_star) { D.stamp = E.stamp; D.table = -1; }
            else {
                D.stamp = -1; D.table = g;
                SynGalaxy &G = gals[(size_t)g++];
                G.image = E.image; G.pad = 0;
                G.shape[0] = E.gal_frac_dev; G.shape[1] = E.gal_axis_ratio; G.shape[2] = E.gal_angle; G.shape[3] = E.gal_radius_px;
            }
            const int ntw = (images[E.image].W + SYN_TW - 1) / SYN_TW;
            for (int th = (E.h0 - 1) / SYN_TH; th <= (E.h1 - 1) / SYN_TH; ++th)
                for (int tw = (E.w0 - 1) / SYN_TW; tw <= (E.w1 - 1) / SYN_TW; ++tw) {
                    SynTile &T = tiles[(size_t)(tile_base[E.image] + (int64_t)th * ntw + tw)];
                    tile_ent[(size_t)T.ent_begin + T.ent_count++] = (int32_t)e;
                }
        }
    }
    std::vector<double> psfs((size_t)n_images * 6 * CEL_MAXK, 0.0);
    for (int n = 0; n < n_images; ++n) memcpy(&psfs[(size_t)n * 6 * CEL_MAXK], images[n].psf, sizeof(double) * 6 * images[n].psf_K);

    // ---- the device
    std::lock_guard<std::mutex> lk(g_mu);
    SynCall call;
    int st = call.open(device);
    if (st) return st;
    if ((st = syn_constants(device))) return st;
    std::vector<SynImage> dimgs((size_t)n_images);
    for (int n = 0; n < n_images; ++n) {
        const celeste_synth_image_t &im = images[n];
        const size_t np = (size_t)im.H * im.W;
        SynImage &D = dimgs[(size_t)n];
        D.H = im.H; D.W = im.W; D.K = im.psf_K; D.stream = im.stream; D.lam = nullptr; D.pix = nullptr;
        float *sky, *iota;
        if ((st = call.up(&sky, im.sky, np)) || (st = call.up(&iota, im.nelec_per_nmgy, (size_t)im.H))) return st;
        D.sky = sky; D.iota = iota;
        if (im.lambda_out && (st = call.up<double>(&D.lam, nullptr, np))) return st;
        if (im.pixels_out && (st = call.up<float>(&D.pix, nullptr, np))) return st;
    }
    SynArgs A;
    memset(&A, 0, sizeof A);
    SynImage *d_images; SynTile *d_tiles; int32_t *d_tile_ent; SynEntry *d_ents; SynGalaxy *d_gals; double *d_psfs, *d_stamps, *d_coefs;
    float *d_coefs_f; Comp *d_tables; unsigned long long *d_cap;
    if ((st = call.up(&d_images, dimgs.data(), dimgs.size())) || (st = call.up(&d_tiles, tiles.data(), tiles.size())) ||
        (st = call.up(&d_tile_ent, tile_ent.data(), tile_ent.size())) || (st = call.up(&d_ents, ents.data(), ents.size())) ||
        (st = call.up(&d_gals, gals.data(), gals.size())) || (st = call.up(&d_psfs, psfs.data(), psfs.size())) ||
        (st = call.up(&d_stamps, stamps, (size_t)n_stamps * CEL_STAMP * CEL_STAMP)) ||
        (st = call.up<double>(&d_coefs, nullptr, (size_t)n_stamps * CEL_COEF * CEL_COEF)) ||
        (st = call.up<float>(&d_coefs_f, nullptr, (size_t)n_stamps * CEL_COEF * CEL_COEF)) ||
        (st = call.up<Comp>(&d_tables, nullptr, (size_t)n_gal * SYN_NCMAX)) || (st = call.up<unsigned long long>(&d_cap, nullptr, 1)))
        return st;
    SYN_HIP(hipMemsetAsync(d_cap, 0, sizeof(unsigned long long), call.stream));
    A.images = d_images; A.tiles = d_tiles; A.tile_ent = d_tile_ent; A.entries = d_ents; A.coefs = d_coefs; A.tables = d_tables;
    A.n_capped = d_cap; A.k0 = (uint32_t)seed; A.k1 = (uint32_t)(seed >> 32);
    A.expectation = (flags & CELESTE_SYNTH_FLAG_EXPECTATION) ? 1 : 0;
    SYN_HIP(hipEventRecord(call.ev[0], call.stream));
    if (n_stamps > 0) {
        hipLaunchKernelGGL(spline_prefilter_kernel, dim3((unsigned)n_stamps), dim3(64), 0, call.stream, d_stamps, d_coefs, d_coefs_f);
        SYN_HIP(hipGetLastError());
    }
    SYN_HIP(hipEventRecord(call.ev[1], call.stream));
    if (n_gal > 0) {
        hipLaunchKernelGGL(syn_tables_kernel, dim3((unsigned)n_gal), dim3(64), 0, call.stream, d_gals, d_images, d_psfs, d_tables);
        SYN_HIP(hipGetLastError());
    }
    SYN_HIP(hipEventRecord(call.ev[2], call.stream));
    const int64_t per = chunk_tiles > 0 ? chunk_tiles : n_tiles;
    for (int64_t t0 = 0; t0 < n_tiles; t0 += per) {
        hipLaunchKernelGGL(syn_pixel_kernel, dim3((unsigned)std::min(per, n_tiles - t0)), dim3(256), 0, call.stream, A, (int)t0);
        SYN_HIP(hipGetLastError());
    }
    SYN_HIP(hipEventRecord(call.ev[3], call.stream));
    for (int n = 0; n < n_images; ++n) {
        const celeste_synth_image_t &im = images[n];
        const size_t np = (size_t)im.H * im.W;
        if (im.lambda_out) SYN_HIP(hipMemcpyAsync(im.lambda_out, dimgs[(size_t)n].lam, np * sizeof(double), hipMemcpyDeviceToHost, call.stream));
        if (im.pixels_out) SYN_HIP(hipMemcpyAsync(im.pixels_out, dimgs[(size_t)n].pix, np * sizeof(float), hipMemcpyDeviceToHost, call.stream));
    }
    unsigned long long cap = 0;
    SYN_HIP(hipMemcpyAsync(&cap, d_cap, sizeof cap, hipMemcpyDeviceToHost, call.stream));
    SYN_HIP(hipStreamSynchronize(call.stream));
    if (n_capped) *n_capped = (int64_t)cap;
    for (int i = 0; i < 3; ++i) (void)hipEventElapsedTime(&g_last_ms[i], call.ev[i], call.ev[i + 1]);
    return CELESTE_SYNTH_OK;
}

extern "C" int celeste_synth_sample(int device, int64_t n, const double *lambda, uint64_t seed, uint32_t stream, uint32_t first_index,
                                    float *pixels, int64_t *n_capped) {
    if (device < 0 || device >= 64 || n < 0 || (n && (!lambda || !pixels)) || n > 0x7fffffff || (uint64_t)first_index + (uint64_t)n > 0x100000000ull)
        return CELESTE_SYNTH_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_mu);
    SynCall call;
    int st = call.open(device);
    if (st) return st;
    double *d_lam; float *d_pix; unsigned long long *d_cap;
    if ((st = call.up(&d_lam, lambda, (size_t)n)) || (st = call.up<float>(&d_pix, nullptr, (size_t)n)) ||
        (st = call.up<unsigned long long>(&d_cap, nullptr, 1)))
        return st;
    SYN_HIP(hipMemsetAsync(d_cap, 0, sizeof(unsigned long long), call.stream));
    SYN_HIP(hipEventRecord(call.ev[2], call.stream));
    if (n > 0) {
        hipLaunchKernelGGL(syn_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, call.stream, d_lam, d_pix, n,
                           (uint32_t)seed, (uint32_t)(seed >> 32), stream, first_index, d_cap);
        SYN_HIP(hipGetLastError());
    }
    SYN_HIP(hipEventRecord(call.ev[3], call.stream));
    unsigned long long cap = 0;
    if (n > 0) SYN_HIP(hipMemcpyAsync(pixels, d_pix, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, call.stream));
    SYN_HIP(hipMemcpyAsync(&cap, d_cap, sizeof cap, hipMemcpyDeviceToHost, call.stream));
    SYN_HIP(hipStreamSynchronize(call.stream));
    if (n_capped) *n_capped = (int64_t)cap;
    g_last_ms[0] = g_last_ms[1] = 0.0f;
    (void)hipEventElapsedTime(&g_last_ms[2], call.ev[2], call.ev[3]);
    return CELESTE_SYNTH_OK;
}
