// synth_sampler.h -- the Poisson sampler of libceleste_synth.so and its random numbers (include/celeste_synth.h states the
// protocol).  Plain C++ with no HIP dependency beyond the function attributes, so that a host compiler
// can build the same text.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SYN_HD __host__ __device__ inline
#else
#define SYN_HD inline
#endif

#define SYN_TAG 0x53594E54u   // CELESTE_SYNTH_PHILOX_TAG
#define SYN_MAX_BLOCKS 64     // CELESTE_SYNTH_MAX_BLOCKS

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
struct SynU4 { uint32_t x[4]; };
SYN_HD SynU4 syn_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    SynU4 c = {{c0, c1, c2, c3}};
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c.x[0], p1 = (uint64_t)0xCD9E8D57u * c.x[2];
        SynU4 o;
        o.x[0] = (uint32_t)(p1 >> 32) ^ c.x[1] ^ k0;
        o.x[1] = (uint32_t)p1;
        o.x[2] = (uint32_t)(p0 >> 32) ^ c.x[3] ^ k1;
        o.x[3] = (uint32_t)p0;
        c = o;
    }
    return c;
}
SYN_HD double syn_u53(uint32_t a, uint32_t b) { return ((double)((((uint64_t)a << 32) | b) >> 11) + 0.5) * 0x1p-53; }

// One pixel: Poisson(lam) from the stream (seed, stream id, pixel index).  *capped is set when block SYN_MAX_BLOCKS would
// be needed (the result is NaN then).  Every operation is rounded once, in the order written: no contraction.
SYN_HD float syn_poisson(double lam, uint32_t k0, uint32_t k1, uint32_t index, uint32_t stream, bool *capped) {
#pragma clang fp contract(off)
    if (!(fabs(lam) < INFINITY)) return __builtin_nanf("");   // NaN, +-inf
    if (lam <= 0.0) return 0.0f;
    if (lam < 10.0) {
        const double L = exp(-lam);
        double p = 1.0, k = 0.0;
        for (uint32_t n = 0; n < SYN_MAX_BLOCKS; ++n) {
            const SynU4 r = syn_philox(index, stream, n, SYN_TAG, k0, k1);
            p *= syn_u53(r.x[0], r.x[1]);
            if (p <= L) return (float)k;
            k += 1.0;
            p *= syn_u53(r.x[2], r.x[3]);
            if (p <= L) return (float)k;
            k += 1.0;
        }
    } else {
        const double slam = sqrt(lam), loglam = log(lam);
        const double b = 0.931 + 2.53 * slam;
        const double a = -0.059 + 0.02483 * b;
        const double linv = log(1.1239 + 1.1328 / (b - 3.4));
        const double vr = 0.9277 - 3.6224 / (b - 2.0);
        for (uint32_t n = 0; n < SYN_MAX_BLOCKS; ++n) {
            const SynU4 r = syn_philox(index, stream, n, SYN_TAG, k0, k1);
            const double U = syn_u53(r.x[0], r.x[1]) - 0.5, V = syn_u53(r.x[2], r.x[3]);
            const double us = 0.5 - fabs(U);
            const double k = floor((2.0 * a / us + b) * U + lam + 0.43);
            if (us >= 0.07 && V <= vr) return (float)k;
            if (k < 0.0 || (us < 0.013 && V > us)) continue;
            if (log(V) + linv - log(a / (us * us) + b) <= -lam + k * loglam - lgamma(k + 1.0)) return (float)k;
        }
    }
    *capped = true;
    return __builtin_nanf("");
}
