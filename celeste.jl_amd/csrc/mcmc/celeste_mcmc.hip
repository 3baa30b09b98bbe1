// celeste_mcmc.hip -- libceleste_mcmc.so: the reference's MCMC method of infer_box on gfx950 (include/celeste_mcmc.h).
//
// Per call:
//   mc_setup_kernel   one wavefront per (target, non-empty patch of the target): the data of patch_to_image
//                     (mcmc_misc.jl:390-419: pixels rounded half to even, NaN or inactive -> NaN), the patch's
//                     sum of lgamma(x + 1) (compute_lgamma_sum, mcmc_functions.jl:437-451) and the background of
//                     render_patch_nmgy (mcmc_misc.jl:284-304: the sky plane plus every neighbour's light at its catalog
//                     point parameters, rendered through the TARGET's patch, accumulated in Float32 in neighbour order).
//   mc_ais_kernel     one wavefront per (target, model, AIS run): a prior draw, then one component-wise slice transition
//                     per temperature (ais.jl:17-65), over several launches of temps_per_launch temperatures each.
//   mc_chain_kernel   one wavefront per (target, model, chain): num_chain_samples slice transitions at t = 1, starting
//                     from AIS run 1's final state (mcmc_infer.jl:47-52), over launches of samples_per_launch samples.
// The likelihood of a point is a wave-wide sum over the target's patches and pixels (make_star_loglike /
// make_gal_loglike, mcmc_functions.jl:109-318) on the densities of the VI kernels (star_value, galaxy_value,
// prep_visit_values of elbo_kernels.h), folded in a fixed order (no atomics).  Every lane of a wavefront runs the same
// control flow and draws the same random numbers, so the sampler's state is wave-uniform.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../elbo_kernels.h"
#include "../host_tables.h"
#include "../../../include/celeste_mcmc.h"

// Mutation testing (tests/test_satellite_mutants.py builds this library with -DCELESTE_MCMC_MUTANT=k and checks that
// tests/test_gpu_mcmc.py notices).  A mutant changes arithmetic, or an index clamped into the same array; never a size, a launch,
// a barrier or a loop.  0 = the product;
//   1 = srcf is kept in double: no Float32 rounding of the source's light
//   2 = iota indexed by column, clamped to its H entries (img.iota[min(P.off_w + w2, img.H - 1)])
//   3 = a NaN pixel still subtracts its rate
//   4 = lgs is not subtracted
//   5 = ang is accepted up to 2 * M_PI
//   6 = llscale uses log(s) for log(sc * s)
// Never defined in the shipped build.
#ifndef CELESTE_MCMC_MUTANT
#define CELESTE_MCMC_MUTANT 0
#endif

#define MC_D CELESTE_MCMC_D
#define MC_STEP_OUT 10        // max_steps_out (slicesample.jl:24)
#define MC_ACCEPT_MAX 1000    // acceptable's loop guard (slicesample.jl:58-62)
#define MC_SHRINK_DEFAULT 10000

// ---------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
// ---------------------------------------------------------------------------------------------
struct U4 { uint32_t x[4]; };
__host__ __device__ inline U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c.x[0], p1 = (uint64_t)0xCD9E8D57u * c.x[2];
        U4 o;
        o.x[0] = (uint32_t)(p1 >> 32) ^ c.x[1] ^ k0;
        o.x[1] = (uint32_t)p1;
        o.x[2] = (uint32_t)(p0 >> 32) ^ c.x[3] ^ k1;
        o.x[3] = (uint32_t)p0;
        c = o;
    }
    return c;
}

// Draw protocol: stream (source s, id), draw n uses the block philox({s, id, n_lo, n_hi}, seed);
// every draw below takes ONE block and advances n by one.
//   uniform      (((x0 << 32) | x1) >> 11 + 0.5) * 2^-53, in (0, 1)
//   exponential  -log(uniform)
//   normal       Box-Muller: sqrt(-2 log u1) cos(2 pi u2), u1 from (x0, x1), u2 from (x2, x3)
//   categorical  the first k with u < p_0 + ... + p_k (the last one if rounding leaves none)
//   permutation  Fisher-Yates from the identity: for i = D-1 .. 1, j = floor(u (i + 1)), swap(perm[i], perm[j])
// id = model + 2 * (kind + 2 * index), kind 0 = AIS run `index`, 1 = chain `index`.
struct Rng {
    uint32_t s, id, k0, k1;
    uint64_t n;
    __device__ U4 block() {
        U4 c; c.x[0] = s; c.x[1] = id; c.x[2] = (uint32_t)n; c.x[3] = (uint32_t)(n >> 32);
        ++n;
        return philox4x32_10(c, k0, k1);
    }
    __device__ static double u53(uint32_t a, uint32_t b) {
        return ((double)((((uint64_t)a << 32) | b) >> 11) + 0.5) * 0x1p-53;
    }
    __device__ double uniform() { const U4 b = block(); return u53(b.x[0], b.x[1]); }
    __device__ double exponential() { return -log(uniform()); }
    __device__ double normal() {
        const U4 b = block();
        return sqrt(-2.0 * log(u53(b.x[0], b.x[1]))) * cos(2.0 * M_PI * u53(b.x[2], b.x[3]));
    }
};

// ---------------------------------------------------------------------------------------------
// tables
// ---------------------------------------------------------------------------------------------
struct McPrior {
    PriorDev pd;               // the prior with the inverse colour covariances and their log-determinants
    double chol[2][8][16];     // lower Cholesky factors of the colour covariances, column-major (prior draws)
};

struct McArgs {
    const DevImage *images;
    const DevPatch *patches;
    const double *coefs;
    const McPrior *prior;
    const celeste_mcmc_source_t *sources;
    const int32_t *targets;     // [n_t] source ids
    const double *box;          // [n_t][4] ra_lo, ra_hi, dec_lo, dec_hi
    const int32_t *mv_off;      // [n_t + 1] the target's patches in mv_*
    const int32_t *mv_patch;    // patch table index
    const int32_t *mv_img;      // image
    const int64_t *mv_pix;      // first pixel in the arena
    const uint8_t *bitmaps;     // explicit active-pixel bitmaps (DevPatch.bitmap_off)
    const int64_t *nbr_off;
    const int32_t *nbr_idx;
    double *data;               // rounded data, NaN where the pixel does not count
    double *bg;                 // Float64 background
    float *bgf;                 // its Float32 accumulator
    double *lg;                 // per patch: sum of lgamma(x + 1)
    int K, NC;
};

// ---------------------------------------------------------------------------------------------
// mc_setup_kernel
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) mc_setup_kernel(McArgs A) {
    __shared__ Comp tc[14 * CEL_MAXK];
    __shared__ double etab[64];
    exp_table_init(etab);
    const int v = blockIdx.x, lane = threadIdx.x;
    // the target of this patch: mv_off is short, a linear search is cheap next to the pixel loops
    int ti = 0;
    while (A.mv_off[ti + 1] <= v) ++ti;
    const DevPatch &P = A.patches[A.mv_patch[v]];
    const DevImage &img = A.images[A.mv_img[v]];
    const int b = img.band - 1, npx = P.H2 * P.W2;
    const int64_t po = A.mv_pix[v];
    double s = 0.0;
    for (int idx = lane; idx < npx; idx += 64) {
        const int w2 = idx / P.H2, h2 = idx - w2 * P.H2;
        const size_t q = (size_t)(P.off_h + h2) + (size_t)img.H * (P.off_w + w2);
        const float x = img.pixels[q];
        bool valid = !isnan(x);
        if (valid && P.bitmap_off >= 0) valid = A.bitmaps[P.bitmap_off + h2 + (int64_t)P.H2 * w2] != 0;   // active_pixel_bitmap
        double xr = valid ? rint((double)x) : __builtin_nan("");
        if (valid) s += lgamma(xr + 1.0);
        A.data[po + idx] = xr;
        A.bgf[po + idx] = img.sky[q];
    }
    s = wave_sum(s);
    if (lane == 0) A.lg[v] = s;
    const int src = A.targets[ti];
    const double *coef = A.coefs + (size_t)P.stamp * (CEL_COEF * CEL_COEF);
    for (int64_t e = A.nbr_off[src]; e < A.nbr_off[src + 1]; ++e) {
        const celeste_mcmc_source_t &n = A.sources[A.nbr_idx[e]];
        double vs[6] = {n.pos[0], n.pos[1], n.gal_frac_dev, n.gal_axis_ratio, n.gal_angle, n.gal_radius_px};
        double m1, m2;
        world_to_pix(vs, P, m1, m2);
        const bool star = n.is_star != 0;
        const double flux = star ? n.star_fluxes[b] : n.gal_fluxes[b];
        __syncthreads();
        if (!star) prep_visit_values<false>(lane, vs, P, b, A.K, nullptr, tc);
        __syncthreads();
        const double sh0 = 26.0 - m1, sw0 = 26.0 - m2;
        for (int idx = lane; idx < npx; idx += 64) {
            const int w2 = idx / P.H2, h2 = idx - w2 * P.H2;
            const double hh = (double)(P.off_h + h2 + 1), ww = (double)(P.off_w + w2 + 1);
            const double f = star ? star_value(coef, hh + sh0, ww + sw0) : galaxy_value(tc, A.NC, hh - m1, ww - m2, etab);
            A.bgf[po + idx] = (float)((double)A.bgf[po + idx] + f * flux);     // pixels[h2, w2] += v * flux, Float32
        }
    }
    for (int idx = lane; idx < npx; idx += 64) A.bg[po + idx] = (double)A.bgf[po + idx];
}

// ---------------------------------------------------------------------------------------------
// densities, likelihood, prior (one wavefront, wave-uniform results)
// ---------------------------------------------------------------------------------------------
__device__ inline void mc_position(const double *box, const double *th, double &ra, double &dec) {
    ra = (box[1] - box[0]) * th[5] + box[0];      // uniform_to_deg (mcmc_functions.jl:350-354)
    dec = (box[3] - box[2]) * th[6] + box[2];
}

// make_star_loglike / make_gal_loglike for target ti; th is wave-uniform
__device__ double mc_loglike(const McArgs &A, int ti, int model, const double *th, Comp *tc, const double *etab, int lane) {
    double ra, dec;
    mc_position(A.box + 4 * ti, th, ra, dec);
    double vs[6] = {ra, dec, 0.0, 0.0, 0.0, 0.0};
    if (model == 1) { vs[2] = th[7]; vs[3] = th[8]; vs[4] = th[9]; vs[5] = th[10]; }
    double acc = 0.0, lgs = 0.0;
    bool inf = false;
    for (int v = A.mv_off[ti]; v < A.mv_off[ti + 1]; ++v) {
        const DevPatch &P = A.patches[A.mv_patch[v]];
        const DevImage &img = A.images[A.mv_img[v]];
        const int b = img.band - 1, npx = P.H2 * P.W2;
        const double flux = exp(th[b]);
        if (isinf(flux)) return -INFINITY;
        double m1, m2;
        world_to_pix(vs, P, m1, m2);
        if (model == 1) {
            __syncthreads();
            prep_visit_values<false>(lane, vs, P, b, A.K, nullptr, tc);
            __syncthreads();
        }
        const double *coef = A.coefs + (size_t)P.stamp * (CEL_COEF * CEL_COEF);
        const double sh0 = 26.0 - m1, sw0 = 26.0 - m2;
        const int64_t po = A.mv_pix[v];
        for (int idx = lane; idx < npx; idx += 64) {
            const int w2 = idx / P.H2, h2 = idx - w2 * P.H2;
            const double hh = (double)(P.off_h + h2 + 1), ww = (double)(P.off_w + w2 + 1);
            const double f = model == 0 ? star_value(coef, hh + sh0, ww + sw0) : galaxy_value(tc, A.NC, hh - m1, ww - m2, etab);
#if CELESTE_MCMC_MUTANT == 1
            const double srcf = f * flux;
#else
            const float srcf = (float)(f * flux);                                           // src_pixels::Float32
#endif
#if CELESTE_MCMC_MUTANT == 2
            const double rate = ((double)srcf + A.bg[po + idx]) * (double)img.iota[min(P.off_w + w2, img.H - 1)];
#else
            const double rate = ((double)srcf + A.bg[po + idx]) * (double)img.iota[P.off_h + h2];
#endif
            inf |= isinf(rate);
            const double x = A.data[po + idx];
#if CELESTE_MCMC_MUTANT == 3
            acc += isnan(x) ? -rate : x * log(rate) - rate;
#else
            if (!isnan(x)) acc += x * log(rate) - rate;
#endif
        }
        lgs += A.lg[v];
    }
    if (__any(inf)) return -INFINITY;
#if CELESTE_MCMC_MUTANT == 4
    return wave_sum(acc);
#else
    return wave_sum(acc) - lgs;
#endif
}

__device__ inline double mc_logsumexp8(const double *x) {
    double m = x[0];
    for (int k = 1; k < 8; ++k) m = fmax(m, x[k]);
    if (isinf(m)) return m;
    double s = 0.0;
    for (int k = 0; k < 8; ++k) s += exp(x[k] - m);
    return m + log(s);
}

// logflux_logprior (mcmc_functions.jl:576-596)
__device__ double mc_logflux_prior(const McPrior &pr, int type, const double *th) {
    const celeste_prior_t &p = pr.pd.p;
    const double lnr = th[2];
    const double col[4] = {th[1] - th[0], th[2] - th[1], th[3] - th[2], th[4] - th[3]};
    const double sd = sqrt(p.flux_var[type]);
    const double zr = (lnr - p.flux_mean[type]) / sd;
    const double llr = -0.5 * zr * zr - log(sd) - 0.5 * log(2.0 * M_PI);
    double llk[8];
    for (int k = 0; k < 8; ++k) {
        const double *mu = p.color_mean[type][k], *iv = pr.pd.inv_cov[type][k];
        double d[4], q = 0.0;
        for (int i = 0; i < 4; ++i) d[i] = col[i] - mu[i];
        for (int j = 0; j < 4; ++j) for (int i = 0; i < 4; ++i) q += d[i] * iv[i + 4 * j] * d[j];
        llk[k] = -0.5 * (4.0 * log(2.0 * M_PI) + pr.pd.logdet[type][k] + q) + log(p.k[type][k]);
    }
    return llr + mc_logsumexp8(llk);
}

__device__ inline bool mc_inrange(double v, double a, double b) { return !(v <= a || v >= b); }   // mcmc_misc.jl:23-28

// logprior of make_star_inference_functions / make_gal_inference_functions (mcmc_functions.jl:1-104)
__device__ double mc_logprior(const McPrior &pr, int model, const double *th, const double *box) {
    double ra, dec;
    mc_position(box, th, ra, dec);
    double pos;
    if (!mc_inrange(ra, box[0], box[1]) || !mc_inrange(dec, box[2], box[3])) pos = -INFINITY;
    else pos = log(1.0 / (box[1] - box[0])) + log(1.0 / (box[3] - box[2]));
    if (model == 0) return mc_logflux_prior(pr, 0, th) + pos;
    // make_gal_logprior (:372-411)
    const double dev = th[7], ab = th[8], ang = th[9], sc = th[10];
    double g;
#if CELESTE_MCMC_MUTANT == 5
    if (!mc_inrange(dev, 0.0, 1.0) || !mc_inrange(ab, 0.0, 1.0) || !mc_inrange(ang, 0.0, 2 * M_PI) || !mc_inrange(sc, 1e-5, INFINITY))
#else
    if (!mc_inrange(dev, 0.0, 1.0) || !mc_inrange(ab, 0.0, 1.0) || !mc_inrange(ang, 0.0, M_PI) || !mc_inrange(sc, 1e-5, INFINITY))
#endif
        g = -INFINITY;
    else {
        const double mu = pr.pd.p.gal_radius_px_mean, s = sqrt(pr.pd.p.gal_radius_px_var);
        const double z = (log(sc) - mu) / s;
#if CELESTE_MCMC_MUTANT == 6
        const double llscale = -0.5 * z * z - log(s) - 0.5 * log(2.0 * M_PI);
#else
        const double llscale = -0.5 * z * z - log(sc * s) - 0.5 * log(2.0 * M_PI);     // LogNormal(mean, sqrt(var))
#endif
        g = mc_logflux_prior(pr, 1, th) + (-log(M_PI)) + llscale;
    }
    return g + pos;
}

// prior draws: sample_logfluxes (:615-631), u ~ U[0, 1]^2, sample_galaxy_shape (:413-420)
__device__ void mc_prior_draw(const McPrior &pr, int model, Rng &rng, double *th) {
    const celeste_prior_t &p = pr.pd.p;
    const double lnr = p.flux_mean[model] + sqrt(p.flux_var[model]) * rng.normal();
    const double u = rng.uniform();
    int k = 7;
    double cum = 0.0;
    for (int j = 0; j < 8; ++j) { cum += p.k[model][j]; if (u < cum) { k = j; break; } }
    double z[4], c[4];
    for (int i = 0; i < 4; ++i) z[i] = rng.normal();
    const double *L = pr.chol[model][k];
    for (int i = 0; i < 4; ++i) {
        double s = p.color_mean[model][k][i];
        for (int j = 0; j <= i; ++j) s += L[i + 4 * j] * z[j];
        c[i] = s;
    }
    // log.(colors_to_fluxes(lnr, c)), formed in log space
    th[2] = lnr; th[1] = lnr - c[1]; th[0] = th[1] - c[0]; th[3] = lnr + c[2]; th[4] = th[3] + c[3];
    th[5] = rng.uniform(); th[6] = rng.uniform();
    if (model == 1) {
        th[7] = rng.uniform(); th[8] = rng.uniform(); th[9] = rng.uniform() * M_PI;
        th[10] = exp(p.gal_radius_px_mean + sqrt(p.gal_radius_px_var) * rng.normal());
    } else {
        th[7] = th[8] = th[9] = th[10] = 0.0;
    }
}

// ---------------------------------------------------------------------------------------------
// the slice sampler (slicesample.jl:20-205), one wavefront
// ---------------------------------------------------------------------------------------------
struct McState {
    double th[MC_D];
    double lp, ll, w;   // current point's log-prior and log-likelihood (ll is not evaluated when lp < -1e100), AIS weight
    uint64_t n;         // draws taken from the stream
    int64_t evals;
    int32_t status, pad;
};

__device__ inline double mc_post(double lp, double ll) { return lp < -1e100 ? lp : ll + lp; }   // logpost (:37-42)
// lnpdf_t (ais.jl:31-39): t * logpost + (1 - t) * logprior, the endpoints special-cased
__device__ inline double mc_val_t(double lp, double ll, double t) {
    if (t == 0.0) return lp;
    const double post = mc_post(lp, ll);
    if (t == 1.0) return post;
    return t * post + (1.0 - t) * lp;
}

struct McWave {
    const McArgs &A;
    int ti, model, D, lane, max_shrink;
    Comp *tc;
    const double *etab;
    double *th;        // LDS, wave-uniform
    int64_t evals;
    // the tempered density at th + z e_d; also returns the point's (lp, ll)
    __device__ double eval(int d, double z, double t, double &lp, double &ll) {
        __syncthreads();
        const double x0 = th[d];
        __syncthreads();
        if (lane == 0) th[d] = x0 + z;
        __syncthreads();
        lp = mc_logprior(A.prior[0], model, th, A.box + 4 * ti);
        ll = 0.0;
        if (!(lp < -1e100)) { ll = mc_loglike(A, ti, model, th, tc, etab, lane); ++evals; }
        __syncthreads();
        if (lane == 0) th[d] = x0;
        __syncthreads();
        return mc_val_t(lp, ll, t);
    }
    __device__ double f(int d, double z, double t) { double a, b; return eval(d, z, t, a, b); }

    // direction_slice along coordinate d from the current point (value f0 = lnpdf_t there); returns a status
    __device__ int direction_slice(int d, double t, Rng &rng, double &lp, double &ll) {
        const double sigma = 1.0;
        const double f0 = mc_val_t(lp, ll, t);          // dir_logprob(0): the current point's value, not re-evaluated
        double upper = sigma * rng.uniform();
        double lower = upper - sigma;
        const double llh_s = f0 - rng.exponential();
        // doubling step-out; the side that did not move keeps its value (the reference re-evaluates both)
        double fl = f(d, lower, t), fu = f(d, upper, t);
        int steps = 0;
        while ((fl > llh_s || fu > llh_s) && steps < MC_STEP_OUT) {
            if (rng.uniform() < 0.5) { lower -= (upper - lower); ++steps; if (steps < MC_STEP_OUT) fl = f(d, lower, t); }
            else { upper += (upper - lower); ++steps; if (steps < MC_STEP_OUT) fu = f(d, upper, t); }
        }
        const double start_lower = lower, start_upper = upper;
        for (int it = 0; it < max_shrink; ++it) {
            const double z = (upper - lower) * rng.uniform() + lower;
            double zlp, zll;
            const double fz = eval(d, z, t, zlp, zll);
            if (isnan(fz)) return CELESTE_MCMC_CHAIN_NAN;
            bool ok = llh_s < fz;
            if (ok) {
                // acceptable (slicesample.jl:40-68)
                const double starting_width = start_upper - start_lower;
                double Lt = start_lower, Ut = start_upper;
                int iter = 0;
                while ((Ut - Lt) > 1.1 * sigma && (Ut - Lt) < 1.1 * starting_width) {
                    const double middle = 0.5 * (Lt + Ut);
                    const bool splits = (middle > 0 && z >= middle) || (middle <= 0 && z < middle);
                    if (z < middle) Ut = middle; else Lt = middle;
                    if (splits && llh_s >= f(d, Ut, t) && llh_s >= f(d, Lt, t)) { ok = false; break; }
                    if (iter > MC_ACCEPT_MAX) return CELESTE_MCMC_CHAIN_ACCEPT_LOOP;
                    ++iter;
                }
            }
            if (ok) {
                __syncthreads();
                const double x0 = th[d];
                __syncthreads();
                if (lane == 0) th[d] = x0 + z;
                __syncthreads();
                lp = zlp; ll = zll;
                return CELESTE_MCMC_CHAIN_OK;
            }
            if (z < 0) lower = z;
            else if (z > 0) upper = z;
            else return CELESTE_MCMC_CHAIN_SHRANK_TO_ZERO;
        }
        return CELESTE_MCMC_CHAIN_SHRINK_CAP;
    }

    // slicesample, compwise: the dimensions in a random order (shuffle(1:dims))
    __device__ int transition(double t, Rng &rng, double &lp, double &ll) {
        int perm[MC_D];
        for (int i = 0; i < D; ++i) perm[i] = i;
        for (int i = D - 1; i >= 1; --i) {
            const int j = min((int)(rng.uniform() * (i + 1)), i);
            const int x = perm[i]; perm[i] = perm[j]; perm[j] = x;
        }
        for (int q = 0; q < D; ++q) {
            const int st = direction_slice(perm[q], t, rng, lp, ll);
            if (st) return st;
        }
        return CELESTE_MCMC_CHAIN_OK;
    }
};

__device__ inline Rng mc_rng(uint64_t seed, int src, int model, int kind, int index, uint64_t n) {
    Rng r;
    r.s = (uint32_t)src; r.id = (uint32_t)(model + 2 * (kind + 2 * index));
    r.k0 = (uint32_t)seed; r.k1 = (uint32_t)(seed >> 32); r.n = n;
    return r;
}

// AIS (ais.jl:17-65) over schedule indices [i0, i1): wave g = (ti * 2 + model) * R + run
__global__ void __launch_bounds__(64) mc_ais_kernel(McArgs A, McState *st, const double *sched, int R, int i0, int i1,
                                                      uint64_t seed, int max_shrink) {
    __shared__ Comp tc[14 * CEL_MAXK];
    __shared__ double etab[64];
    __shared__ double th[MC_D];
    exp_table_init(etab);
    const int g = blockIdx.x, lane = threadIdx.x;
    const int run = g % R, model = (g / R) & 1, ti = g / (2 * R);
    McState &S = st[g];
    if (S.status) return;
    Rng rng = mc_rng(seed, A.targets[ti], model, 0, run, S.n);
    McWave W{A, ti, model, model ? MC_D : 7, lane, max_shrink, tc, etab, th, S.evals};
    double lp = S.lp, ll = S.ll, w = S.w;
    if (i0 == 1) {
        double t0[MC_D];
        mc_prior_draw(A.prior[0], model, rng, t0);
        if (lane == 0) for (int i = 0; i < MC_D; ++i) th[i] = t0[i];
        __syncthreads();
        lp = mc_logprior(A.prior[0], model, th, A.box + 4 * ti);
        ll = 0.0;
        if (!(lp < -1e100)) { ll = mc_loglike(A, ti, model, th, tc, etab, lane); ++W.evals; }
        w = 0.0;
    } else {
        if (lane < MC_D) th[lane] = S.th[lane];
        __syncthreads();
    }
    int status = 0;
    for (int i = i0; i < i1 && !status; ++i) {
        const double tprev = sched[i - 1], tcurr = sched[i];
        status = W.transition(tcurr, rng, lp, ll);
        if (!status) w += mc_val_t(lp, ll, tcurr) - mc_val_t(lp, ll, tprev);   // llcurr - llprev, no evaluation
    }
    __syncthreads();
    if (lane == 0) {
        for (int i = 0; i < MC_D; ++i) S.th[i] = th[i];
        S.lp = lp; S.ll = ll; S.w = w; S.n = rng.n; S.evals = W.evals; S.status = status;
    }
}

// chains (slicesample_chain, slicesample.jl:210-235) over samples [s0, s1): wave g = (ti * 2 + model) * R + chain
__global__ void __launch_bounds__(64) mc_chain_kernel(McArgs A, McState *st, const McState *ais, int R, int L, int s0, int s1,
                                                        uint64_t seed, int max_shrink, double *samples, double *sample_lp) {
    __shared__ Comp tc[14 * CEL_MAXK];
    __shared__ double etab[64];
    __shared__ double th[MC_D];
    exp_table_init(etab);
    const int g = blockIdx.x, lane = threadIdx.x;
    const int c = g % R, model = (g / R) & 1, ti = g / (2 * R);
    McState &S = st[g];
    // every chain starts from AIS run 1's final state (mcmc_infer.jl:47-52)
    const McState &from = s0 == 0 ? ais[(size_t)(ti * 2 + model) * R] : S;
    const int status0 = from.status;
    if (s0 == 0 && lane == 0 && status0) S.status = status0;
    if (status0) return;
    Rng rng = mc_rng(seed, A.targets[ti], model, 1, c, s0 == 0 ? 0 : S.n);
    McWave W{A, ti, model, model ? MC_D : 7, lane, max_shrink, tc, etab, th, s0 == 0 ? 0 : S.evals};
    if (lane < MC_D) th[lane] = from.th[lane];
    double lp = from.lp, ll = from.ll;
    __syncthreads();
    int status = 0;
    for (int s = s0; s < s1 && !status; ++s) {
        status = W.transition(1.0, rng, lp, ll);
        if (status) break;
        const size_t k = ((size_t)(ti * 2 + model) * R + c) * L + s;
        if (lane < MC_D) samples[k * MC_D + lane] = th[lane];
        if (lane == 0) sample_lp[k] = mc_post(lp, ll);
    }
    __syncthreads();
    if (lane == 0) {
        for (int i = 0; i < MC_D; ++i) S.th[i] = th[i];
        S.lp = lp; S.ll = ll; S.n = rng.n; S.evals = W.evals; S.status = status;
    }
}

// celeste_mcmc_loglike: one wavefront per point
__global__ void __launch_bounds__(64) mc_loglike_kernel(McArgs A, int model, const int32_t *which, const double *theta,
                                                          double *ll, double *lp) {
    __shared__ Comp tc[14 * CEL_MAXK];
    __shared__ double etab[64];
    __shared__ double th[MC_D];
    exp_table_init(etab);
    const int k = blockIdx.x, lane = threadIdx.x, ti = which[k];
    if (lane < MC_D) th[lane] = theta[(size_t)k * MC_D + lane];
    __syncthreads();
    const double l = mc_loglike(A, ti, model, th, tc, etab, lane);
    const double p = mc_logprior(A.prior[0], model, th, A.box + 4 * ti);
    if (lane == 0) { ll[k] = l; lp[k] = p; }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct celeste_mcmc_ctx {
    int device = 0, N = 0, S = 0, K = 0;
    std::vector<void *> allocs;
    DevImage *d_images = nullptr;
    DevPatch *d_patches = nullptr;
    uint8_t *d_bitmaps = nullptr;
    double *d_coefs = nullptr;
    McPrior *d_prior = nullptr;
    int64_t *d_nbr_off = nullptr;
    int32_t *d_nbr_idx = nullptr;
    std::vector<int64_t> h_nbr_off;
    std::vector<int32_t> h_pidx;          // [s * N + n] -> patch table index, -1: empty
    std::vector<DevPatch> h_patches;
    std::vector<int32_t> h_band;
    hipStream_t stream = nullptr;
    float last_ms[3] = {0, 0, 0};
};

#define MC_HIP(expr) do { if ((expr) != hipSuccess) { (void)hipGetLastError(); return CELESTE_MCMC_ERR_HIP; } } while (0)

template <class T>
static int mc_upload(celeste_mcmc_ctx *c, T **dst, const T *src, size_t n) {
    void *p = nullptr;
    MC_HIP(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
    c->allocs.push_back(p);
    if (src && n) MC_HIP(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
    *dst = (T *)p;
    return CELESTE_MCMC_OK;
}

// lower Cholesky factor of a 4 x 4 column-major covariance
static void chol4(const double *S, double *L) {
    for (int i = 0; i < 16; ++i) L[i] = 0.0;
    for (int j = 0; j < 4; ++j) {
        double d = S[j + 4 * j];
        for (int k = 0; k < j; ++k) d -= L[j + 4 * k] * L[j + 4 * k];
        L[j + 4 * j] = std::sqrt(d);
        for (int i = j + 1; i < 4; ++i) {
            double s = S[i + 4 * j];
            for (int k = 0; k < j; ++k) s -= L[i + 4 * k] * L[j + 4 * k];
            L[i + 4 * j] = s / L[j + 4 * j];
        }
    }
}

extern "C" int celeste_mcmc_version(void) { return CELESTE_MCMC_ABI_VERSION; }

extern "C" const char *celeste_mcmc_strerror(int status) {
    switch (status) {
        case CELESTE_MCMC_OK: return "ok";
        case CELESTE_MCMC_ERR_INVALID_ARG: return "invalid argument";
        case CELESTE_MCMC_ERR_NO_DEVICE: return "no HIP device (there is no CPU fallback)";
        case CELESTE_MCMC_ERR_HIP: return "HIP runtime error";
        case CELESTE_MCMC_ERR_ALLOC: return "allocation failed";
        default: return "unknown status";
    }
}

extern "C" void celeste_mcmc_ctx_destroy(celeste_mcmc_ctx_t *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    for (void *p : c->allocs) (void)hipFree(p);
    delete c;
}

extern "C" int celeste_mcmc_ctx_create(const celeste_problem_t *pr, int device, celeste_mcmc_ctx_t **out) {
    if (!pr || !out) return CELESTE_MCMC_ERR_INVALID_ARG;
    *out = nullptr;
    if (pr->n_images <= 0 || pr->n_sources <= 0 || !pr->images || !pr->patches || pr->psf_K <= 0 || pr->psf_K > CEL_MAXK ||
        pr->n_stamps <= 0 || !pr->stamps)
        return CELESTE_MCMC_ERR_INVALID_ARG;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { (void)hipGetLastError(); return CELESTE_MCMC_ERR_NO_DEVICE; }
    if (device < 0 || device >= count) return CELESTE_MCMC_ERR_INVALID_ARG;
    MC_HIP(hipSetDevice(device));
    celeste_mcmc_ctx *c = new (std::nothrow) celeste_mcmc_ctx();
    if (!c) return CELESTE_MCMC_ERR_ALLOC;
    c->device = device; c->N = pr->n_images; c->S = pr->n_sources; c->K = pr->psf_K;
#define MC_TRY(expr) do { int s__ = (expr); if (s__) { celeste_mcmc_ctx_destroy(c); return s__; } } while (0)
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { c->stream = nullptr; MC_TRY(CELESTE_MCMC_ERR_HIP); }
    // image planes (pixels, sky, iota); log_iota is not used here
    std::vector<DevImage> imgs(c->N);
    for (int n = 0; n < c->N; ++n) {
        const celeste_image_t &im = pr->images[n];
        if (im.H <= 0 || im.W <= 0 || im.band < 1 || im.band > 5 || !im.pixels || !im.sky || !im.nelec_per_nmgy)
            MC_TRY(CELESTE_MCMC_ERR_INVALID_ARG);
        float *px, *sky, *iota;
        const size_t np = (size_t)im.H * im.W;
        MC_TRY(mc_upload(c, &px, im.pixels, np));
        MC_TRY(mc_upload(c, &sky, im.sky, np));
        MC_TRY(mc_upload(c, &iota, im.nelec_per_nmgy, (size_t)im.H));
        DevImage d; memset(&d, 0, sizeof d);
        d.H = im.H; d.W = im.W; d.band = im.band; d.pixels = px; d.sky = sky; d.iota = iota; d.log_iota = nullptr;
        imgs[n] = d;
    }
    MC_TRY(mc_upload(c, &c->d_images, imgs.data(), imgs.size()));
    // patches: the non-empty ones, indexed through h_pidx; explicit bitmaps are stored as a byte pool
    const bool sparse = pr->n_patch_entries > 0;
    const size_t n_entries = sparse ? (size_t)pr->n_patch_entries : (size_t)c->S * c->N;
    c->h_pidx.assign((size_t)c->S * c->N, -1);
    std::vector<uint8_t> pool;
    for (size_t k = 0; k < n_entries; ++k) {
        size_t q = k;
        if (sparse) {
            if (!pr->patch_source || !pr->patch_image) MC_TRY(CELESTE_MCMC_ERR_INVALID_ARG);
            const int32_t s = pr->patch_source[k], n = pr->patch_image[k];
            if (s < 0 || s >= c->S || n < 0 || n >= c->N) MC_TRY(CELESTE_MCMC_ERR_INVALID_ARG);
            q = (size_t)s * c->N + n;
        }
        const celeste_patch_t &p = pr->patches[k];
        const celeste_image_t &im = pr->images[q % c->N];
        if (p.H2 <= 0 || p.W2 <= 0) continue;
        if (p.off_h < 0 || p.off_w < 0 || p.off_h + p.H2 > im.H || p.off_w + p.W2 > im.W || p.stamp < 0 || p.stamp >= pr->n_stamps ||
            !p.psf)
            MC_TRY(CELESTE_MCMC_ERR_INVALID_ARG);
        DevPatch d; memset(&d, 0, sizeof d);
        d.off_h = p.off_h; d.off_w = p.off_w; d.H2 = p.H2; d.W2 = p.W2; d.stamp = p.stamp; d.bitmap_off = -1;
        if (p.bitmap) { d.bitmap_off = (int64_t)pool.size(); pool.insert(pool.end(), p.bitmap, p.bitmap + (size_t)p.H2 * p.W2); }
        memcpy(d.J, p.wcs_jacobian, sizeof d.J);
        memcpy(d.wc, p.world_center, sizeof d.wc);
        memcpy(d.pc, p.pixel_center, sizeof d.pc);
        memcpy(d.psf, p.psf, sizeof(double) * 6 * c->K);
        c->h_pidx[q] = (int32_t)c->h_patches.size();
        c->h_patches.push_back(d);
    }
    MC_TRY(mc_upload(c, &c->d_patches, c->h_patches.data(), c->h_patches.size()));
    MC_TRY(mc_upload(c, &c->d_bitmaps, pool.data(), pool.size()));
    // spline coefficients: spline_prefilter_kernel of the VI library
    {
        double *d_stamps = nullptr;
        float *d_coefs_f = nullptr;
        MC_TRY(mc_upload(c, &d_stamps, pr->stamps, (size_t)pr->n_stamps * CEL_STAMP * CEL_STAMP));
        MC_TRY(mc_upload<double>(c, &c->d_coefs, nullptr, (size_t)pr->n_stamps * CEL_COEF * CEL_COEF));
        MC_TRY(mc_upload<float>(c, &d_coefs_f, nullptr, (size_t)pr->n_stamps * CEL_COEF * CEL_COEF));
        hipLaunchKernelGGL(spline_prefilter_kernel, dim3((unsigned)pr->n_stamps), dim3(64), 0, c->stream, d_stamps, c->d_coefs, d_coefs_f);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) MC_TRY(CELESTE_MCMC_ERR_HIP);
    }
    // neighbours
    c->h_nbr_off.assign((size_t)c->S + 1, 0);
    std::vector<int32_t> nidx;
    if (pr->nbr_offsets) {
        for (int s = 0; s <= c->S; ++s) c->h_nbr_off[s] = pr->nbr_offsets[s];
        for (int64_t e = 0; e < c->h_nbr_off[c->S]; ++e) {
            const int32_t v = pr->nbr_index[e];
            if (v < 0 || v >= c->S) MC_TRY(CELESTE_MCMC_ERR_INVALID_ARG);
            nidx.push_back(v);
        }
    }
    MC_TRY(mc_upload(c, &c->d_nbr_off, c->h_nbr_off.data(), c->h_nbr_off.size()));
    MC_TRY(mc_upload(c, &c->d_nbr_idx, nidx.data(), nidx.size()));
    // prior
    {
        McPrior mp;
        memset(&mp, 0, sizeof mp);
        mp.pd.p = pr->prior ? *pr->prior : DEFAULT_PRIOR;
        for (int i = 0; i < 2; ++i)
            for (int d = 0; d < 8; ++d) {
                inv4_logdet(mp.pd.p.color_cov[i][d], mp.pd.inv_cov[i][d], &mp.pd.logdet[i][d]);
                chol4(mp.pd.p.color_cov[i][d], mp.chol[i][d]);
            }
        MC_TRY(mc_upload(c, &c->d_prior, &mp, 1));
    }
    // library constants of this code object: galaxy prototypes, the exponential's table
    {
        static std::mutex mu;
        static bool ready[64] = {};
        std::lock_guard<std::mutex> lk(mu);
        if (device >= 64 || !ready[device]) {
            double eta[16], nu[16];
            galaxy_prototypes(eta, nu);
            if (hipMemcpyToSymbol(HIP_SYMBOL(c_eta), eta, sizeof eta) != hipSuccess ||
                hipMemcpyToSymbol(HIP_SYMBOL(c_nu), nu, sizeof nu) != hipSuccess)
                MC_TRY(CELESTE_MCMC_ERR_HIP);
            hipLaunchKernelGGL(exp_table_kernel, dim3(1), dim3(64), 0, nullptr);
            if (hipStreamSynchronize(nullptr) != hipSuccess) MC_TRY(CELESTE_MCMC_ERR_HIP);
            if (device < 64) ready[device] = true;
        }
    }
    *out = c;
    return CELESTE_MCMC_OK;
#undef MC_TRY
}

// the per-call tables of a list of targets: patches, pixel arena, setup launch.  Owns its device buffers.
struct McCall {
    celeste_mcmc_ctx *c;
    std::vector<void *> bufs;
    McArgs A;
    int n_mv = 0;
    ~McCall() { for (void *p : bufs) (void)hipFree(p); }
    template <class T> int up(T **dst, std::nullptr_t, size_t n) { return up(dst, (const T *)nullptr, n); }
    template <class T, class U> int up(T **dst, const U *src, size_t n) {
        static_assert(sizeof(T) == sizeof(U), "element size");
        void *p = nullptr;
        MC_HIP(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
        bufs.push_back(p);
        if (src && n) MC_HIP(hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
        *dst = (T *)p;
        return CELESTE_MCMC_OK;
    }
    int setup(const celeste_mcmc_source_t *sources, int n_t, const int32_t *targets, const double *box) {
        std::vector<int32_t> off(1, 0), mvp, mvi;
        std::vector<int64_t> pix;
        int64_t P = 0;
        for (int ti = 0; ti < n_t; ++ti) {
            const int s = targets[ti];
            if (s < 0 || s >= c->S) return CELESTE_MCMC_ERR_INVALID_ARG;
            for (int n = 0; n < c->N; ++n) {
                const int32_t q = c->h_pidx[(size_t)s * c->N + n];
                if (q < 0) continue;
                mvp.push_back(q); mvi.push_back(n); pix.push_back(P);
                P += (int64_t)c->h_patches[q].H2 * c->h_patches[q].W2;
            }
            off.push_back((int32_t)mvp.size());
        }
        for (int ti = 0; ti < n_t; ++ti)
            if (!(box[4 * ti] < box[4 * ti + 1]) || !(box[4 * ti + 2] < box[4 * ti + 3])) return CELESTE_MCMC_ERR_INVALID_ARG;
        n_mv = (int)mvp.size();
        memset(&A, 0, sizeof A);
        A.images = c->d_images; A.patches = c->d_patches; A.coefs = c->d_coefs; A.prior = c->d_prior;
        A.bitmaps = c->d_bitmaps; A.nbr_off = c->d_nbr_off; A.nbr_idx = c->d_nbr_idx; A.K = c->K; A.NC = 14 * c->K;
        int st;
        if ((st = up(&A.sources, sources, (size_t)c->S)) || (st = up(&A.targets, targets, (size_t)n_t)) ||
            (st = up(&A.box, box, (size_t)4 * n_t)) || (st = up(&A.mv_off, off.data(), off.size())) ||
            (st = up(&A.mv_patch, mvp.data(), mvp.size())) || (st = up(&A.mv_img, mvi.data(), mvi.size())) ||
            (st = up(&A.mv_pix, pix.data(), pix.size())) || (st = up<double>(&A.data, nullptr, (size_t)P)) ||
            (st = up<double>(&A.bg, nullptr, (size_t)P)) || (st = up<float>(&A.bgf, nullptr, (size_t)P)) ||
            (st = up<double>(&A.lg, nullptr, (size_t)n_mv)))
            return st;
        if (n_mv > 0) {
            hipLaunchKernelGGL(mc_setup_kernel, dim3((unsigned)n_mv), dim3(64), 0, c->stream, A);
            MC_HIP(hipGetLastError());
        }
        MC_HIP(hipStreamSynchronize(c->stream));   // (the host arrays above are pageable and go out of scope)
        return CELESTE_MCMC_OK;
    }
};

extern "C" int celeste_mcmc_loglike(celeste_mcmc_ctx_t *c, const celeste_mcmc_source_t *sources, int32_t n_targets,
                                    const int32_t *targets, const double *pos_box, int32_t model, int32_t n, const int32_t *which,
                                    const double *theta, double *ll, double *lp) {
    if (!c || !sources || n_targets <= 0 || !targets || !pos_box || (model != 0 && model != 1) || n < 0 || (n && (!which || !theta || !ll || !lp)))
        return CELESTE_MCMC_ERR_INVALID_ARG;
    for (int k = 0; k < n; ++k) if (which[k] < 0 || which[k] >= n_targets) return CELESTE_MCMC_ERR_INVALID_ARG;
    MC_HIP(hipSetDevice(c->device));
    McCall call{c};
    int st = call.setup(sources, n_targets, targets, pos_box);
    if (st || n == 0) return st;
    int32_t *d_which; double *d_th, *d_ll, *d_lp;
    if ((st = call.up(&d_which, which, (size_t)n)) || (st = call.up(&d_th, theta, (size_t)n * MC_D)) ||
        (st = call.up<double>(&d_ll, nullptr, (size_t)n)) || (st = call.up<double>(&d_lp, nullptr, (size_t)n)))
        return st;
    hipLaunchKernelGGL(mc_loglike_kernel, dim3((unsigned)n), dim3(64), 0, c->stream, call.A, (int)model, d_which, d_th, d_ll, d_lp);
    MC_HIP(hipGetLastError());
    MC_HIP(hipMemcpyAsync(ll, d_ll, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    MC_HIP(hipMemcpyAsync(lp, d_lp, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    MC_HIP(hipStreamSynchronize(c->stream));
    return CELESTE_MCMC_OK;
}

// sigmoid_schedule(T; rad = 4) (ais.jl:99-107), t = linspace(-rad, rad, T) as numpy forms it
static std::vector<double> sigmoid_schedule(int T, double rad) {
    if (T == 1) return {0.0, 1.0};
    std::vector<double> s(T);
    const double step = (2.0 * rad) / (T - 1);
    for (int i = 0; i < T; ++i) {
        const double t = i == T - 1 ? rad : i * step - rad;
        s[i] = 1.0 / (1.0 + std::exp(-t));
    }
    const double lo = *std::min_element(s.begin(), s.end()), hi = *std::max_element(s.begin(), s.end());
    for (double &x : s) x = (x - lo) / (hi - lo);
    return s;
}

extern "C" int celeste_mcmc_ais(celeste_mcmc_ctx_t *c, const celeste_mcmc_config_t *cfg, const celeste_mcmc_source_t *sources,
                                int32_t n_targets, const int32_t *targets, const double *pos_box, double *ais_state,
                                double *ais_weight, double *samples, double *sample_lp, int64_t *evals, int32_t *status) {
    if (!c || !cfg || !sources || n_targets <= 0 || !targets || !pos_box || !ais_state || !ais_weight || !samples || !sample_lp ||
        !evals || !status || cfg->num_temperatures < 1 || cfg->num_ais_runs < 1 || cfg->num_chain_samples < 0)
        return CELESTE_MCMC_ERR_INVALID_ARG;
    if ((int64_t)n_targets * 2 * cfg->num_ais_runs > 0x7fffffff) return CELESTE_MCMC_ERR_INVALID_ARG;
    MC_HIP(hipSetDevice(c->device));
    const int R = cfg->num_ais_runs, L = cfg->num_chain_samples, G = n_targets * 2 * R;
    const int max_shrink = cfg->max_shrink > 0 ? cfg->max_shrink : MC_SHRINK_DEFAULT;
    const int tpl = cfg->temps_per_launch > 0 ? cfg->temps_per_launch : 10;
    const int spl = cfg->samples_per_launch > 0 ? cfg->samples_per_launch : 5;
    const std::vector<double> sched = sigmoid_schedule(cfg->num_temperatures, 4.0);
    const int T = (int)sched.size();
    hipEvent_t ev[4];
    for (auto &e : ev) MC_HIP(hipEventCreate(&e));
    struct EvGuard { hipEvent_t *e; ~EvGuard() { for (int i = 0; i < 4; ++i) (void)hipEventDestroy(e[i]); } } eg{ev};
    MC_HIP(hipEventRecord(ev[0], c->stream));
    McCall call{c};
    int st = call.setup(sources, n_targets, targets, pos_box);
    if (st) return st;
    MC_HIP(hipEventRecord(ev[1], c->stream));
    McState *d_ais, *d_chain;
    double *d_sched, *d_samples, *d_slp;
    if ((st = call.up<McState>(&d_ais, nullptr, (size_t)G)) || (st = call.up<McState>(&d_chain, nullptr, (size_t)G)) ||
        (st = call.up(&d_sched, sched.data(), sched.size())) ||
        (st = call.up<double>(&d_samples, nullptr, (size_t)G * std::max(L, 1) * MC_D)) ||
        (st = call.up<double>(&d_slp, nullptr, (size_t)G * std::max(L, 1))))
        return st;
    MC_HIP(hipMemsetAsync(d_ais, 0, sizeof(McState) * G, c->stream));
    MC_HIP(hipMemsetAsync(d_chain, 0, sizeof(McState) * G, c->stream));
    MC_HIP(hipMemsetAsync(d_samples, 0xff, sizeof(double) * G * std::max(L, 1) * MC_D, c->stream));   // NaN where a chain stopped
    MC_HIP(hipMemsetAsync(d_slp, 0xff, sizeof(double) * G * std::max(L, 1), c->stream));
    // AIS: schedule indices 1 .. T-1 in launches of tpl temperatures (state in HBM between launches)
    for (int i0 = 1; i0 < T; i0 += tpl) {
        hipLaunchKernelGGL(mc_ais_kernel, dim3((unsigned)G), dim3(64), 0, c->stream, call.A, d_ais, d_sched, R, i0,
                           std::min(T, i0 + tpl), (uint64_t)cfg->seed, max_shrink);
        MC_HIP(hipGetLastError());
        MC_HIP(hipStreamSynchronize(c->stream));
    }
    MC_HIP(hipEventRecord(ev[2], c->stream));
    if (L == 0) {
        // no chain samples: the chains' state only carries AIS run 1's status
        hipLaunchKernelGGL(mc_chain_kernel, dim3((unsigned)G), dim3(64), 0, c->stream, call.A, d_chain, d_ais, R, 1, 0, 0,
                           (uint64_t)cfg->seed, max_shrink, d_samples, d_slp);
        MC_HIP(hipGetLastError());
    }
    for (int s0 = 0; s0 < L; s0 += spl) {
        hipLaunchKernelGGL(mc_chain_kernel, dim3((unsigned)G), dim3(64), 0, c->stream, call.A, d_chain, d_ais, R, L, s0,
                           std::min(L, s0 + spl), (uint64_t)cfg->seed, max_shrink, d_samples, d_slp);
        MC_HIP(hipGetLastError());
        MC_HIP(hipStreamSynchronize(c->stream));
    }
    MC_HIP(hipEventRecord(ev[3], c->stream));
    std::vector<McState> ha(G), hc(G);
    MC_HIP(hipMemcpyAsync(ha.data(), d_ais, sizeof(McState) * G, hipMemcpyDeviceToHost, c->stream));
    MC_HIP(hipMemcpyAsync(hc.data(), d_chain, sizeof(McState) * G, hipMemcpyDeviceToHost, c->stream));
    if (L > 0) {
        MC_HIP(hipMemcpyAsync(samples, d_samples, sizeof(double) * G * L * MC_D, hipMemcpyDeviceToHost, c->stream));
        MC_HIP(hipMemcpyAsync(sample_lp, d_slp, sizeof(double) * G * L, hipMemcpyDeviceToHost, c->stream));
    }
    MC_HIP(hipStreamSynchronize(c->stream));
    for (int g = 0; g < G; ++g) {
        const int tm = g / R, r = g % R;
        for (int i = 0; i < MC_D; ++i) ais_state[(size_t)g * MC_D + i] = ha[g].th[i];
        ais_weight[g] = ha[g].w;
        evals[(size_t)tm * 2 * R + r] = ha[g].evals;
        evals[(size_t)tm * 2 * R + R + r] = hc[g].evals;
        status[(size_t)tm * 2 * R + r] = ha[g].status;
        status[(size_t)tm * 2 * R + R + r] = hc[g].status;
    }
    (void)hipEventElapsedTime(&c->last_ms[0], ev[0], ev[1]);
    (void)hipEventElapsedTime(&c->last_ms[1], ev[1], ev[2]);
    (void)hipEventElapsedTime(&c->last_ms[2], ev[2], ev[3]);
    return CELESTE_MCMC_OK;
}

extern "C" int celeste_mcmc_last_ms(celeste_mcmc_ctx_t *c, float ms[3]) {
    if (!c || !ms) return CELESTE_MCMC_ERR_INVALID_ARG;
    for (int i = 0; i < 3; ++i) ms[i] = c->last_ms[i];
    return CELESTE_MCMC_OK;
}
