/* celeste_targets.h -- prepared target lists of libceleste_mi355x.so.  Part of celeste_mi355x.h, which includes it behind
 * the types it needs: include that header, not this one. */
#ifndef CELESTE_TARGETS_H
#define CELESTE_TARGETS_H

/* A prepared target list.  The work list of a sweep, its record offsets and visit items, the target marks and the choice
 * of per-image tables to fill and neighbour light to render depend on the context and the target list, not on d_vp.  A
 * caller that evaluates one target list again and again (a rank draining its shard) has them made once:
 * celeste_targets_create[_device] copies the list (the caller's array may change afterwards), synchronises and is off
 * the hot path; celeste_elbo_eval_targets_device is then celeste_elbo_eval_batch_device over that list, in four launches
 * instead of eight, with bit-identical results.  A list
 * belongs to the context it was created on (another context: CELESTE_ERR_INVALID_ARG); celeste_ctx_destroy frees the lists
 * still alive, after which their handles are dangling.
 * Lists are made for the context's 256-pixel fp64 chunks: a call with CELESTE_FLAG_FP32 or CELESTE_FLAG_SPLIT, and a
 * Hessian batch small enough for the one-launch evaluation (<= 32 targets), runs celeste_elbo_eval_batch_device on the
 * list's targets instead -- same results, nothing saved.  CELESTE_NO_PREPARED=1 in the environment does so for every call.
 * A list also holds the set of neighbour pixels its targets gather, each once (4 bytes per pixel of device memory: 8 MB for
 * 2000 targets of a single field, 138 MB for 30 000 targets of a 4 x 4 grid of fields; CELESTE_ERR_ALLOC if it does not
 * fit), so that a sweep renders a neighbour wanted by several targets once; CELESTE_NO_VALUE_UNION=1 in the environment
 * renders it once per target as celeste_elbo_eval_batch_device does -- same results.
 * A list holds one 64-byte descriptor per work item of its pixel launch (1.1 MB for the 2000 targets above), from which a
 * workgroup starts the item without looking it up; CELESTE_NO_SEQUENCES=1 in the environment launches the pixel kernel over
 * the work list as celeste_elbo_eval_batch_device does -- same results. */
typedef struct celeste_targets celeste_targets_t;
int celeste_targets_create(celeste_ctx_t *ctx, int32_t n_targets, const int32_t *targets, celeste_targets_t **out);
int celeste_targets_create_device(celeste_ctx_t *ctx, int32_t n_targets, const int32_t *d_targets, void *stream,
                                  celeste_targets_t **out);
void celeste_targets_destroy(celeste_targets_t *targets);
int celeste_elbo_eval_targets_device(celeste_ctx_t *ctx, const celeste_targets_t *targets, const double *d_vp, uint32_t flags,
                                     double *d_v, double *d_d, double *d_h, int64_t *d_counters, int32_t *d_status,
                                     void *stream);

#endif
