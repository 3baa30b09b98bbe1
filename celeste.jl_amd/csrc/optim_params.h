// optim_params.h -- the optimiser's parameter space: the 41 free parameters of a source, its state and settings, the box and
// simplex transforms between free and bound space (ElboMaximize.elbo_constraints, ConstraintTransforms.enforce!, to_free!,
// to_bound!) and the start of maximize! for one target.  No solver: optim_kernels.h includes this under its switches and adds
// the Newton step; eval_fused.h (FusedArgs carries an OptParams) and the blend library's kernels include it alone.
#pragma once
#include <hip/hip_runtime.h>
#include "elbo_device.h"
#include "../../include/celeste_mi355x.h"

#define NF 41

struct OptState {                 // per target slot
    double x[NF], xt[NF], g[NF];
    double f, delta, m;
    double pos0[2];               // centre of the position box (ElboMaximize.jl:70-73)
    int32_t iter, done, interior, evals, status, pad;
};

struct OptParams {
    double loc_width, loc_scale, xtol_abs, ftol_rel, gtol, initial_delta, delta_hat;
    int32_t max_iters, solver;    // 0: tridiagonal-space solve (default), 1: eigen-decomposition always
    int32_t secular_iters, pad;   // cap of the Newton iterations on lambda (20: to convergence; Optim.jl stops after 5)
};

template <class OP>   // OptParams in any address space (the fused kernel reads it in the kernel-argument segment)
__device__ __forceinline__ void box_bounds(int i, const double *pos0, const OP &op, double &lo, double &hi,
                                           double &scale) {
    scale = 1.0;
    if (i < 2) { lo = pos0[i] - op.loc_width; hi = pos0[i] + op.loc_width; scale = op.loc_scale; }
    else if (i < 4) { lo = 1e-2; hi = 0.99; }
    else if (i == 4) { lo = -10.0; hi = 10.0; }
    else if (i == 5) { lo = 0.10; hi = 70.0; }
    else if (i < 8) { lo = -1.0; hi = 10.0; }
    else if (i < 10) { lo = 1e-4; hi = 0.10; }
    else if (i < 18) { lo = -10.0; hi = 10.0; }
    else { lo = 1e-4; hi = 1.0; }
}
__device__ __constant__ double c_simplex_lo[3] = {0.005, 0.01 / 8, 0.01 / 8};
__device__ __constant__ int c_simplex_n[3] = {2, 8, 8};
__device__ __constant__ int c_simplex_b0[3] = {26, 28, 36};
__device__ __constant__ int c_simplex_f0[3] = {26, 27, 34};

// to_bound! for one group of the simplex constraints: free x[f0..f0+n-2] -> p[0..n-1] (softmax with the last
// logit fixed at 0), bound = (1 - n lo) p + lo
__device__ inline void simplex_probs(const double *x, int g, double *p) {
    const int n = c_simplex_n[g], f0 = c_simplex_f0[g];
    double m = x[f0];
    for (int i = 1; i < n - 1; ++i) m = fmax(m, x[f0 + i]);
    const double exp_neg_m = exp(-m);
    double sum = exp_neg_m;
    for (int i = 0; i < n - 1; ++i) { p[i] = exp(x[f0 + i] - m); sum += p[i]; }
    for (int i = 0; i < n - 1; ++i) p[i] = p[i] / sum;
    p[n - 1] = (1.0 / sum) * exp_neg_m;
}

// serial to_bound (used by one thread per target): x (41) -> vs (44)
// The same by eight lanes per group (lane = entry i of group g; the three groups side by side): the exponentials -- the
// expensive part, eight library calls in a row on one lane above -- in parallel, the sum by one lane in simplex_probs's order,
// the divisions in parallel: the same operations on the same operands, so the same bits.  x: LDS; ebuf[3][8], sbuf[3]: LDS
// scratch of the calling wavefront.  Returns p[i] of group g (lanes i >= n: nothing meaningful).
__device__ __forceinline__ double simplex_prob_lane(const double *x, int g, int i, double *ebuf, double *sbuf) {
    const int n = c_simplex_n[g], f0 = c_simplex_f0[g];
    double m = x[f0];
    for (int k = 1; k < n - 1; ++k) m = fmax(m, x[f0 + k]);
    const double e = i < n - 1 ? exp(x[f0 + i] - m) : exp(-m);    // (i = n - 1: the last entry's exp(-m))
    if (i < n) ebuf[8 * g + i] = e;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (i == 0) {
        double sum = ebuf[8 * g + n - 1];
        for (int k = 0; k < n - 1; ++k) sum += ebuf[8 * g + k];
        sbuf[g] = sum;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const double sum = sbuf[g];
    return i < n - 1 ? e / sum : (1.0 / sum) * e;
}

template <class OP>
__device__ inline void to_bound_dev(const double *x, const double *pos0, const OP &op, double *vs) {
    for (int i = 0; i < 26; ++i) {
        double lo, hi, sc;
        box_bounds(i, pos0, op, lo, hi, sc);
        vs[i] = (1.0 / (1.0 + exp(-x[i] / sc))) * (hi - lo) + lo;
    }
    for (int g = 0; g < 3; ++g) {
        double p[8];
        simplex_probs(x, g, p);
        const int n = c_simplex_n[g];
        const double lo = c_simplex_lo[g];
        for (int i = 0; i < n; ++i) vs[c_simplex_b0[g] + i] = (1 - n * lo) * p[i] + lo;
    }
}

// enforce! + to_free! + first trial point; one thread per target
// One thread: the start of maximize! for one target -- vs: its 44 parameters (enforced in place, then set to the first
// evaluation point), S: its optimiser state, pos: the centre of its position box (nullptr: its current position)
template <class OP>
__device__ inline void optim_init_values(double *__restrict__ vs, const OP &op, const double *__restrict__ pos, OptState &S) {
    // the position box stays where the first ElboConfig put it (ParallelRun.jl:96-100); default: current position
    S.pos0[0] = pos ? pos[0] : vs[0];
    S.pos0[1] = pos ? pos[1] : vs[1];
    for (int i = 0; i < 26; ++i) {
        double lo, hi, sc;
        box_bounds(i, S.pos0, op, lo, hi, sc);
        double b = vs[i];
        if (!(lo < b && b < hi)) b = fmax(fmin(b, nextafter(hi, -INFINITY)), nextafter(lo, INFINITY));
        vs[i] = b;
        S.x[i] = -log(1.0 / ((b - lo) / (hi - lo)) - 1.0) * sc;
    }
    for (int g = 0; g < 3; ++g) {
        const int n = c_simplex_n[g], b0 = c_simplex_b0[g], f0 = c_simplex_f0[g];
        const double lo = c_simplex_lo[g];
        double sum = 0;
        for (int i = 0; i < n; ++i) {
            double b = vs[b0 + i];
            if (!(lo < b && b < 1.0)) b = fmax(fmin(b, nextafter(1.0, -INFINITY)), nextafter(lo, INFINITY));
            vs[b0 + i] = b; sum += b;
        }
        if (!(fabs(sum - 1.0) <= 1.4901161193847656e-08 * fmax(fabs(sum), 1.0))) {
            const double rescale = (1 - n * lo) / (sum - n * lo);
            for (int i = 0; i < n; ++i) vs[b0 + i] = nextafter(lo, INFINITY) + rescale * (vs[b0 + i] - lo);
        }
        const double log_last = log((vs[b0 + n - 1] - lo) / (1 - n * lo));
        for (int i = 0; i < n - 1; ++i) S.x[f0 + i] = log((vs[b0 + i] - lo) / (1 - n * lo)) - log_last;
    }
    for (int i = 0; i < NF; ++i) S.xt[i] = S.x[i];
    S.f = 0; S.delta = op.initial_delta; S.m = 0; S.iter = -1; S.done = 0; S.interior = 0; S.evals = 0; S.status = 0;
    to_bound_dev(S.xt, S.pos0, op, vs);  // the evaluation point, as evaluate! does (ElboMaximize.jl:163-166)
}

__global__ void optim_init_kernel(double *__restrict__ vp, const int32_t *__restrict__ targets, int n_targets,
                                  OptParams op, OptState *__restrict__ st, int32_t *__restrict__ active,
                                  const double *__restrict__ pos_centers) {
    const int ti = blockIdx.x * blockDim.x + threadIdx.x;
    if (ti >= n_targets) return;
    optim_init_values(vp + (size_t)targets[ti] * CEL_P, op, pos_centers ? pos_centers + 2 * ti : nullptr, st[ti]);
    active[ti] = ti;
}
