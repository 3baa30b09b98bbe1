// eval_fused.h -- what the evaluation launcher (engine_eval.h: launch_eval) needs of the fused kernels: the queue constants
// and FusedArgs, fused_setup_kernel, drain_stores and eval_fused_kernel.  fused_kernels.h includes it at its head and adds
// the persistent optimiser launch (optim_fused_kernel) on top; the blend library compiles this header and not that one.
#pragma once
#include "elbo_kernels.h"
#include "optim_params.h"

#define FQ_EMPTY (-1)      // queue slot not written yet (the array is memset to 0xFF before every launch)
#define FQ_EXIT (-2)
#define FQ_DIRECT0 (-3)    // item <= FQ_DIRECT0: target ti = FQ_DIRECT0 - item has no pixel to visit -- straight to its step
#define FUSED_NT 256
#ifndef FUSED_GATED
#define FUSED_GATED 1      // 1: a wavefront forms its pixels' record entries before it waits for its turn to add them (pixel_iter)
#endif
#define FUSED_WAVES (FUSED_NT / 64)

// q_ctl words
#define FQC_HEAD 0         // next ticket
#define FQC_TAIL 1         // next free queue position
#define FQC_LIVE 2         // targets still running
#define FQC_ABORT 3        // 0, or why the launch gave up: 1 wait timed out, 2 queue capacity exceeded
#define FQC_WORDS 8

struct FusedArgs {
    // the context's tables (immutable during the launch)
    const DevImage *images; const DevPatch *patches; const double *coefs; const uint8_t *bitmaps;
    const int64_t *nbr_off; const int32_t *nbr_idx; const int64_t *val_off; const double2 *val;
    const int64_t *nv_base; const int32_t *nbr_vis; const int2 *items; const SrcGeo *geo; const PriorDev *prior;
    const int32_t *vis_off; const int32_t *vis_img; const double *lg_sum; const int32_t *rec_off;
    int N, NC, K, M, CH, chunk_px;
    // the batch
    const int32_t *targets; int n_targets;
    double *vp;                    // n_sources x 44: the targets' rows move, every other row is frozen
    double *acc;                   // chunk records, 68 doubles each
    const int4 *chunk_desc;        // per record, two entries: {ti, j, chunk, target} {visit, image, 0, 0}
    const int2 *tgt_rec;           // per target: {first record, number of records}
    OptState *st; double *Hstate; double *Tstate; OptParams op; uint32_t flags;   // Tstate: TRI_STATE doubles per target (optim_step_target)
    double *Spec;                  // 2 x SPEC_STATE doubles per target: the quarter-radius step computed ahead (fused_speculate); nullptr: off
    // the queue
    int32_t *q_items; int32_t *q_ctl; int32_t *arrivals; int q_cap;
    long long timeout_ticks;       // wall_clock64 ticks (100 MHz) a workgroup waits for its ticket before it gives up
    // joint mode (optim_fused_kernel<true>): `targets` lists the entries of the schedule (sources repeat)
    int j_R;                       // number of chunk records = first START item; START e = j_R + e
    int j_gshift;                  // RENDER (e, g) = j_R + n_targets + (e << j_gshift | g)
    int32_t *j_dep;                // per entry: predecessors still running
    const int32_t *j_succ_off; const int32_t *j_succ;   // per entry: the entries that wait for it
    const int32_t *j_vitem_off; const int4 *j_vitems;   // per source: its value-kernel items (celeste_ctx_create)
    int32_t *j_render_arr;         // per entry: render groups done
    double *j_saved;               // per entry: the source's row before the entry
    const double *j_pos;           // per entry: centre of the position box (nullptr: the position at its start)
    SrcImg *j_srcimg; Comp *j_comps; SrcGeo *j_geo;     // the context's per-visit / per-source tables, refreshed in flight
};
// How the phases of the persistent kernel see the launch's arguments: in place, in the kernel-argument segment (constant
// address space: scalar loads through the scalar cache).  Passed as `const FusedArgs &` they were a copy on the kernel's
// stack -- 464 B of scratch per lane, every field a flat load from it in front of the access it serves.
typedef const __attribute__((address_space(4))) FusedArgs &FusedArgsK;
// (handed down as a plain pointer and made wave-uniform again inside every phase: a pointer that arrives as a function
// argument is a per-lane value to the compiler, and the loads through it would be vector loads)
__device__ __forceinline__ FusedArgsK fused_args(const FusedArgs *p) {
    const unsigned long long b = (unsigned long long)(size_t)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    return *(const __attribute__((address_space(4))) FusedArgs *)(size_t)(((unsigned long long)hi << 32) | lo);
}


// per batch, once: the targets' record ranges, the description of every record, the first round of queue items
// (q_items == nullptr: no queue -- eval_fused_kernel)
__global__ void fused_setup_kernel(const int32_t *__restrict__ targets, int n_targets, const DevPatch *__restrict__ patches,
                                   const int32_t *__restrict__ vis_off, const int2 *__restrict__ items, int N, int M,
                                   int chunk_px, const int32_t *__restrict__ rec_off, int4 *__restrict__ chunk_desc,
                                   int2 *__restrict__ tgt_rec, int32_t *__restrict__ q_items, int32_t *__restrict__ q_ctl,
                                   const int32_t *__restrict__ j_dep = nullptr, int j_R = 0) {
    const int ti = blockIdx.x * blockDim.x + threadIdx.x;
    if (ti >= n_targets) return;
    const int t = targets[ti];
    int first;
    const int n_rec = describe_target_records(ti, t, patches, items, N, M, chunk_px, rec_off, chunk_desc, first);
    tgt_rec[ti] = make_int2(first < 0 ? 0 : first, n_rec);
    if (!q_items) return;
    if (j_dep) {     // joint mode: the entries without predecessors start
        if (j_dep[ti] == 0) q_items[atomicAdd(&q_ctl[FQC_TAIL], 1)] = j_R + ti;
        if (ti == 0) q_ctl[FQC_LIVE] = n_targets;
        return;
    }
    const int cnt = n_rec > 0 ? n_rec : 1;
    const int base = atomicAdd(&q_ctl[FQC_TAIL], cnt);
    if (n_rec > 0) for (int i = 0; i < n_rec; ++i) q_items[base + i] = first + i;
    else q_items[base] = FQ_DIRECT0 - ti;
    if (ti == 0) q_ctl[FQC_LIVE] = n_targets;
}

__device__ __forceinline__ void drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// ---------------------------------------------------------------------------------------------------------
// eval_fused_kernel: one elbo() sweep of a SMALL batch (a rank's shard at N >= 4, a single call) with the fused kernel's
// chunk evaluation -- one workgroup per chunk record, its four 64-pixel iterations on four wavefronts adding in
// iteration order -- and the lift done by whichever workgroup completes a target (arrival counter), instead of
// pixel_kernel (one wavefront per record, four iterations in a row: the critical path of a batch that cannot fill the
// chip) followed by a lift launch.  Records and results are bit-identical to that pair's.  No queue and no waiting:
// every workgroup does its record, and at most one lift.  The per-image tables come from prep_kernel (HBM).
// ---------------------------------------------------------------------------------------------------------
struct EvalFusedShared {
    Comp tc[14 * CEL_MAXK];
    double tcx[COMPX * 14 * CEL_MAXK];
    double etab[64];
    double sacc[ACC_N * ACC_SLOTS];
    int turn, last;
    LiftShared lift;
};

__global__ void __launch_bounds__(FUSED_NT, 2)
eval_fused_kernel(const FusedArgs A, const SrcImg *__restrict__ srcimg, const Comp *__restrict__ comps,
                  const int32_t *__restrict__ n_records, int rec_bound, double *__restrict__ out_v, double *__restrict__ out_d,
                  double *__restrict__ out_h, int64_t *__restrict__ out_cnt, int32_t *__restrict__ out_status) {
    __shared__ EvalFusedShared F;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int item = blockIdx.x;
    if (item >= rec_bound) {
        // the last n_targets blocks: targets that visit no pixel at all (off every image) have no record to complete them
        const int te = item - rec_bound;
        if (A.tgt_rec[te].y > 0) return;
        const size_t HSe = (A.flags & CELESTE_FLAG_PACKED_HESS) ? CELESTE_HP : (size_t)CEL_P * CEL_P;
        lift_target<false, true>(F.lift, tid, te, A.targets[te], A.vp, A.images, A.patches, A.geo, A.nbr_off, A.nbr_idx, A.acc,
                                 A.prior, A.vis_off, A.vis_img, A.N, A.M, A.CH, A.chunk_px, A.flags, out_v + te,
                                 out_d + (size_t)te * CEL_P, out_h + (size_t)te * HSe, out_cnt ? out_cnt + 2 * (size_t)te : nullptr,
                                 out_status + te, A.lg_sum, A.rec_off);
        return;
    }
    if (item >= *n_records) return;              // rec_bound is the host's bound on the number of records
    const int4 d0 = A.chunk_desc[2 * item], d1 = A.chunk_desc[2 * item + 1];
    const int ti = d0.x, j = d0.y, ch = d0.z, t = d0.w, v = d1.x, n = d1.y;
    const DevPatch &P = A.patches[v];
    const int npx = P.H2 * P.W2;
    const int p0 = ch * A.chunk_px, p1 = min(npx, p0 + A.chunk_px);
    {
        const double *src = reinterpret_cast<const double *>(comps + (size_t)v * A.NC);
        double *dst = reinterpret_cast<double *>(F.tc);
        for (int i = tid; i < A.NC * 8; i += FUSED_NT) dst[i] = src[i];
        if (wave == 2) F.etab[lane] = g_exp2_table[lane];
        for (int i = tid; i < ACC_N * ACC_SLOTS; i += FUSED_NT) F.sacc[i] = 0.0;
        if (tid == 0) F.turn = 0;
        __syncthreads();
        if (tid < A.NC) comp_extra(F.tc[tid], F.tcx + COMPX * tid);
        __syncthreads();
    }
    const int base = p0 + 64 * wave;
    if (base < p1) {
        PixWork<double> W;
        W.img = &A.images[n]; W.P = &P; W.patches = A.patches; W.bitmaps = A.bitmaps; W.nbr_idx = A.nbr_idx;
        W.nb0 = A.nbr_off[t]; W.nb1 = A.nbr_off[t + 1];
        W.nv = A.nbr_vis ? A.nbr_vis + A.nv_base[t] + (int64_t)j * (W.nb1 - W.nb0) : nullptr;
        W.val_off = A.val_off; W.val = A.val; W.active_rank = nullptr; W.my_rank = 0;
        W.N = A.N; W.n = n; W.NC = A.NC; W.v = v;
        W.si = srcimg[v];
        W.tc = F.tc; W.tcx = F.tcx; W.tcr = reinterpret_cast<const CompR<double> *>(F.tc);
        W.etab = F.etab;
        W.tcoef = A.coefs + (size_t)(CELESTE_MUTANT == 3 ? 0 : P.stamp) * (CEL_COEF * CEL_COEF);
        W.tile_off = nullptr; W.rec = nullptr;
        double a[3] = {0.0, 0.0, 0.0};
        volatile int *turn = &F.turn;
        pixel_iter<2, double, false, FUSED_GATED != 0>(W, base, p1, lane, F.sacc + (lane & (ACC_SLOTS - 1)), a, [&]() {
            while (*turn != wave) __builtin_amdgcn_s_sleep(1);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        });
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane == 0) *turn = wave + 1;
    }
    __syncthreads();
    if (wave == 0) {
        double *out = A.acc + (size_t)item * ACC_N;
        fold_record_slots<2>(F.sacc, lane, [&](int e, double s) { stc<true>(out + e, s); });
        drain_stores();
        if (lane == 0) {
            const int before = __hip_atomic_fetch_add(&A.arrivals[ti], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            F.last = before == A.tgt_rec[ti].y - 1;
            if (F.last) stc<true>(&A.arrivals[ti], 0);        // re-armed for the next launch
        }
    }
    __syncthreads();
    if (!F.last) return;
    const size_t HS = (A.flags & CELESTE_FLAG_PACKED_HESS) ? CELESTE_HP : (size_t)CEL_P * CEL_P;
    lift_target<false, true>(F.lift, tid, ti, t, A.vp, A.images, A.patches, A.geo, A.nbr_off, A.nbr_idx, A.acc, A.prior, A.vis_off,
                             A.vis_img, A.N, A.M, A.CH, A.chunk_px, A.flags, out_v + ti, out_d + (size_t)ti * CEL_P,
                             out_h + (size_t)ti * HS, out_cnt ? out_cnt + 2 * (size_t)ti : nullptr, out_status + ti, A.lg_sum,
                             A.rec_off);
}
