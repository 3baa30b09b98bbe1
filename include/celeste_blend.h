/* celeste_blend.h -- C ABI of libceleste_blend.so: joint optimisation of blended sources on an AMD Instinct MI355X (gfx950).
 *
 * The reference's maximize! with several active sources (src/deterministic_vi/ElboMaximize.jl:38-93, 228-242): ONE Newton
 * trust-region over the free parameters of every active source of an ElboArgs.  Here a "blend" is such a set of active
 * sources; a call optimises many blends at once, each on its own.
 *
 * A blend of Sa members has n = 41 Sa free parameters, in member order, parameter index fastest.  Its objective is the
 * multi-active elbo() of celeste_elbo_eval_multi: every pixel of the union of the members' patches counted once, the KL
 * of every member when include_kl is set.  Its free-space Hessian is exact: H_ab = J_a' h_ab J_b for a != b, and the
 * diagonal blocks with their second-order transform terms (the reference's propagate_derivatives!
 * scrambles the Hessian for Sa > 1; this library does not reproduce that).
 *
 * Blends of one call: blend b is blend_sources[blend_offsets[b] .. blend_offsets[b + 1]).  A call is refused with
 * CELESTE_ERR_INVALID_ARG, nothing modified, when a source repeats (within a blend or across blends), a blend is empty or
 * has more than CELESTE_BLEND_SA_MAX members, or a member of one blend is a neighbour of a member of another (either
 * direction of the problem's neighbour lists).  Every non-member, the members of other blends included, is frozen.
 *
 * Status codes, flags, celeste_problem_t and celeste_optim_config_t are those of celeste_mi355x.h.  Thread safety: one
 * call at a time per context.  Without a HIP device every entry point returns CELESTE_ERR_NO_DEVICE -- there is no CPU
 * path. */
#ifndef CELESTE_BLEND_H
#define CELESTE_BLEND_H

#include <stdint.h>
#include "celeste_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CELESTE_BLEND_ABI_VERSION 100
#define CELESTE_BLEND_SA_MAX 4          /* members per blend: up to 4 x 41 = 164 free parameters */

typedef struct celeste_blend_ctx celeste_blend_ctx_t;

int celeste_blend_version(void);
const char *celeste_blend_strerror(int status);
int celeste_blend_ctx_create(const celeste_problem_t *problem, int device, celeste_blend_ctx_t **out);
void celeste_blend_ctx_destroy(celeste_blend_ctx_t *ctx);

/* elbo() with active_sources = each blend, for n_blends blends in one launch set.  vp: n_sources x 44 host doubles.
 * Per blend b of Sa_b members the outputs follow each other in blend order, each in the layout of
 * celeste_elbo_eval_multi: v[b]; d: 44 x Sa_b (column a = member a); h: (44 Sa_b) x (44 Sa_b) column-major with the cross
 * blocks, exactly symmetric; counters[2 b], counters[2 b + 1]: active and inactive pixels; status[b].  d and h may be NULL
 * when the flags do not ask for them.  Returns the first non-OK status of a blend; the other blends' outputs are valid. */
int celeste_blend_eval(celeste_blend_ctx_t *ctx, const double *vp, int32_t n_blends, const int64_t *blend_offsets,
                       const int32_t *blend_sources, uint32_t flags, double *v, double *d, double *h, int64_t *counters,
                       int32_t *status);

/* maximize! for every blend: enforce! / to_free! per member (the position box of member k, k indexing blend_sources,
 * centred on pos_centers[2 k ..], NULL = its current position), then Newton trust-region iterations over the blend's
 * 41 Sa free parameters with the rules of celeste_maximize_batch, then to_bound!.  vp (n_sources x 44, host) is updated
 * in place for blend members only.  vp_neighbors (n_sources x 44, may be NULL = vp) holds every non-member.  Per-blend
 * outputs (may be NULL): iterations, f_evals, elbo (the final value), status.  A blend whose ELBO turns non-finite stops
 * with its status set and keeps its input rows; the others finish normally; the return value is the first such status.
 * A blend's result depends on its own inputs only: not on the other blends of the call or their order. */
int celeste_blend_maximize(celeste_blend_ctx_t *ctx, double *vp, const double *vp_neighbors, const double *pos_centers,
                           int32_t n_blends, const int64_t *blend_offsets, const int32_t *blend_sources,
                           const celeste_optim_config_t *cfg, int32_t *iterations, int32_t *f_evals, double *elbo,
                           int32_t *status);

/* The blends' trust-region sub-problem on its own (test entry): problem k minimises g'p + p'Hp/2 subject to |p| <= delta
 * in dimension dims[k] (1 ... 41 CELESTE_BLEND_SA_MAX).  H: the n_k x n_k matrices one after another (symmetric); g, p:
 * the n_k vectors one after another; delta, m (may be NULL: model value), interior (may be NULL: 1 = plain Newton step):
 * one per problem.  solver must be 0 (eigen-decomposition); secular_iters as in celeste_tr_solve_batch (0 = to
 * convergence).  Host pointers. */
int celeste_blend_tr_solve_batch(int device, int32_t n, const int32_t *dims, const double *H, const double *g,
                                 const double *delta, int32_t solver, int32_t secular_iters, double *p, double *m,
                                 int32_t *interior);

/* Device time of the last celeste_blend_maximize: ms[0] its evaluation launches (multi-active evaluation and cross
 * blocks), ms[1] its step launches, both summed over its iterations; ms[2] the number of iterations (launch sets). */
int celeste_blend_last_ms(celeste_blend_ctx_t *ctx, float ms[3]);

#ifdef __cplusplus
}
#endif
#endif /* CELESTE_BLEND_H */
