// celeste_blend.hip -- libceleste_blend.so: maximize! with several active sources (include/celeste_blend.h).
//
// The engine's context and its evaluation launcher (engine_eval.h: launch_eval, launch_cross, optim_config) are compiled into
// this library, unchanged -- not the engine's host ABI, its optimiser or its device groups, so no RCCL; the context with its
// device buffers is engine_client.h's; this file adds the blend driver and four kernels of its own.  Per Newton iteration, for every live blend of the call at once:
//   launch_eval (MULTI)        the members of all live blends as one target list; every member's pixel sums with the
//                              multi-active rule "an earlier active source visits this pixel" (elbo_kernels.h).  The
//                              refusal rule (no member is a neighbour of a member of another blend) means a member's
//                              neighbour list holds members of its own blend only, so that rule compares members of the
//                              same blend and nothing else.  Every source's light is rendered from the call's table, in
//                              which non-members sit at vp_neighbors and members at their current trial point.
//   cross_kernel + cross_lift  the cross blocks of all overlapping member pairs of all live blends, one launch each
//   blend_step_kernel          one 256-thread workgroup per live blend: the chain rule to free space with cross blocks,
//                              the trust-region sub-problem in dimension 41 Sa (cyclic Jacobi in round-robin order, as the
//                              host restatement's solver), accept / reject, the radius update and the stopping rules of
//                              celeste_maximize_batch, and the next trial point written into the table.
// The (44 Sa)^2 blocks and the (41 Sa)^2 free Hessians stay in HBM; the host waits once per iteration for the blends'
// phases.  No floating-point atomics: every sum runs in a fixed order.
#include "../engine_eval.h"
#include "../engine_client.h"
#include "../../../include/celeste_blend.h"

#define BL_SA_MAX CELESTE_BLEND_SA_MAX
#define BL_NMAX (NF * BL_SA_MAX)
#define BL_NT 256
#define BL_JN (CEL_P * NF)           // one member's Jacobian d bound / d free, 44 x 41 column-major

enum { BL_INIT = 0, BL_TRIAL = 1, BL_DONE = 2 };

struct BlendState {
    double f, delta, m, pad0;
    int32_t it, evals, phase, status, interior, cur;   // cur: which of the two gradient / Hessian slots holds the point x
};

struct BlendDesc {      // a live blend of one step launch
    int32_t blend;      // index in the call
    int32_t sa;         // members
    int32_t t0;         // first member's position in this launch's target list
    int32_t k0, nk;     // its overlapping member pairs in this launch's pair list
    int32_t m0;         // first member's index in the call's member list
};

struct BlendPair { int32_t ia, ib; };   // members (in the blend) of a pair: the cross record is d2 / d theta_ia d theta_ib

struct BlLds {
    double red[BL_NT];
    double cs[BL_NMAX / 2 + 1], sn[BL_NMAX / 2 + 1];
    int32_t pp[BL_NMAX / 2 + 1], qq[BL_NMAX / 2 + 1];
    double w[BL_NMAX], qg[BL_NMAX], c[BL_NMAX], s[BL_NMAX];
    int32_t perm[BL_NMAX];
    double scal[4];
    int32_t iscal[4];
};

// fixed-order workgroup sum (every thread gets the total)
__device__ double bl_block_sum(double v, double *red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = BL_NT / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// Trust-region sub-problem min g's + s'As/2, |s| <= delta, in dimension n <= BL_NMAX, by one workgroup.  A (n x n,
// column-major, HBM) is destroyed; V (n x n, HBM) receives the eigenvectors.  The eigen-decomposition is cyclic Jacobi with
// the round-robin ordering (n/2 disjoint rotations per round, all applied at once), to the restatement's threshold
// off(A)^2 <= 1e-30 |A|^2; the rules on the eigenbasis are celeste_tr_solve_batch's (Optim.jl's solve_tr_subproblem!).
// Result in L.s, L.scal[0] (model value), L.iscal[0] (interior).
__device__ void bl_tr_solve(int n, double *__restrict__ A, double *__restrict__ V, const double *g, double delta,
                            int secular_iters, BlLds &L) {
    const int t = threadIdx.x;
    for (int idx = t; idx < n * n; idx += BL_NT) V[idx] = (idx % n == idx / n) ? 1.0 : 0.0;
    const int mm = n + (n & 1);      // players of the round-robin; index n of an odd n is a dummy
    const int half = mm / 2;
    __syncthreads();
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0, dg = 0;
        for (int idx = t; idx < n * n; idx += BL_NT) {
            const int i = idx % n, j = idx / n;
            const double a = A[idx];
            if (i == j) dg += a * a;
            else if (i < j) off += a * a;
        }
        off = bl_block_sum(off, L.red);
        dg = bl_block_sum(dg, L.red);
        if (off <= 1e-30 * (dg + off) || off == 0) break;
        for (int r = 0; r < mm - 1; ++r) {
            for (int k = t; k < half; k += BL_NT) {
                int p = k == 0 ? r : (r + k) % (mm - 1);
                int q = k == 0 ? mm - 1 : (r - k + (mm - 1)) % (mm - 1);
                if (p > q) { const int u = p; p = q; q = u; }
                double c = 1.0, s = 0.0;
                if (q < n) {
                    const double apq = A[p + (size_t)n * q];
                    if (apq != 0) {
                        const double theta = (A[q + (size_t)n * q] - A[p + (size_t)n * p]) / (2 * apq);
                        const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1));
                        c = 1 / sqrt(tt * tt + 1);
                        s = tt * c;
                    }
                }
                L.pp[k] = p; L.qq[k] = q; L.cs[k] = c; L.sn[k] = s;
            }
            __syncthreads();
            for (int idx = t; idx < half * n; idx += BL_NT) {      // rows p, q
                const int k = idx / n, j = idx % n;
                const int p = L.pp[k], q = L.qq[k];
                const double s = L.sn[k];
                if (q >= n || s == 0) continue;
                const double c = L.cs[k];
                const double ap = A[p + (size_t)n * j], aq = A[q + (size_t)n * j];
                A[p + (size_t)n * j] = c * ap - s * aq;
                A[q + (size_t)n * j] = s * ap + c * aq;
            }
            __syncthreads();
            for (int idx = t; idx < half * n; idx += BL_NT) {      // columns p, q (and the eigenvectors)
                const int k = idx / n, i = idx % n;
                const int p = L.pp[k], q = L.qq[k];
                const double s = L.sn[k];
                if (q >= n || s == 0) continue;
                const double c = L.cs[k];
                const double ap = A[i + (size_t)n * p], aq = A[i + (size_t)n * q];
                A[i + (size_t)n * p] = c * ap - s * aq;
                A[i + (size_t)n * q] = s * ap + c * aq;
                const double vp = V[i + (size_t)n * p], vq = V[i + (size_t)n * q];
                V[i + (size_t)n * p] = c * vp - s * vq;
                V[i + (size_t)n * q] = s * vp + c * vq;
            }
            __syncthreads();
        }
    }
    // eigenvalues in ascending order (ties by index), Q'g
    for (int i = t; i < n; i += BL_NT) L.perm[i] = i;
    __syncthreads();
    for (int i = t; i < n; i += BL_NT) {
        const double wi = A[i + (size_t)n * i];
        int r = 0;
        for (int j = 0; j < n; ++j) {
            const double wj = A[j + (size_t)n * j];
            r += (wj < wi) || (wj == wi && j < i);
        }
        L.perm[r] = i;
    }
    __syncthreads();
    for (int r = t; r < n; r += BL_NT) {
        const int i = L.perm[r];
        L.w[r] = A[i + (size_t)n * i];
        double q = 0;
        for (int k = 0; k < n; ++k) q += V[k + (size_t)n * i] * g[k];
        L.qg[r] = q;
    }
    __syncthreads();
    if (t == 0) {
        const double *w = L.w, *qg = L.qg;
        double *c = L.c;
        const double wmin = w[0], wmax = w[n - 1], d2 = delta * delta;
        int interior = 0;
        if (wmin >= 1e-8) {
            double p2 = 0;
            for (int i = 0; i < n; ++i) p2 += (qg[i] / w[i]) * (qg[i] / w[i]);
            if (p2 <= d2) interior = 1;
        }
        if (interior) {
            for (int i = 0; i < n; ++i) c[i] = -qg[i] / w[i];
        } else {
            const double lambda_lb = -wmin + fmax(1e-8, 1e-8 * (wmax - wmin));
            double lambda = lambda_lb;
            int hard = 0;
            if (wmin < 0) {
                int cand = 1, idx = 0;
                while (idx < n && fabs(w[0] - w[idx]) <= 1e-10) {
                    if (fabs(qg[idx]) > 1e-10) { cand = 0; break; }
                    ++idx;
                }
                if (cand) {
                    double p2 = 0;
                    for (int i = idx; i < n; ++i) p2 += (qg[i] / (w[i] + lambda)) * (qg[i] / (w[i] + lambda));
                    if (p2 <= d2) {   // N&W (4.45): to the boundary along the lowest eigenvector
                        hard = 1;
                        for (int i = 0; i < n; ++i) c[i] = i < idx ? 0.0 : -qg[i] / (w[i] + lambda);
                        c[0] = sqrt(d2 - p2);
                    }
                }
            }
            if (!hard) {
                for (int it = 0; it < secular_iters; ++it) {
                    double q2 = 0, q3 = 0;
                    for (int i = 0; i < n; ++i) {
                        c[i] = -qg[i] / (w[i] + lambda);
                        q2 += c[i] * c[i];
                        q3 += c[i] * c[i] / (w[i] + lambda);
                    }
                    const double prev = lambda;
                    lambda += q2 * (sqrt(q2) - delta) / (delta * q3);
                    if (lambda < lambda_lb) lambda = 0.5 * (prev - lambda_lb) + lambda_lb;
                    if (fabs(lambda - prev) < 1e-10 || lambda <= prev) break;
                }
            }
        }
        double m = 0;
        for (int i = 0; i < n; ++i) m += qg[i] * c[i] + 0.5 * w[i] * c[i] * c[i];
        L.scal[0] = m;
        L.iscal[0] = interior;
    }
    __syncthreads();
    for (int k = t; k < n; k += BL_NT) {
        double s = 0;
        for (int r = 0; r < n; ++r) s += V[k + (size_t)n * L.perm[r]] * L.c[r];
        L.s[k] = s;
    }
    __syncthreads();
}

// the test entry: one workgroup per problem
__global__ __launch_bounds__(BL_NT) void blend_tr_kernel(const int32_t *__restrict__ dims, const int64_t *__restrict__ moff,
                                                          const int64_t *__restrict__ voff, const double *__restrict__ H,
                                                          const double *__restrict__ g, const double *__restrict__ delta,
                                                          int secular_iters, double *__restrict__ A, double *__restrict__ V,
                                                          double *__restrict__ p, double *__restrict__ m,
                                                          int32_t *__restrict__ interior) {
    __shared__ BlLds L;
    const int k = blockIdx.x, n = dims[k];
    for (int idx = threadIdx.x; idx < n * n; idx += BL_NT) A[moff[k] + idx] = H[moff[k] + idx];
    __syncthreads();
    bl_tr_solve(n, A + moff[k], V + moff[k], g + voff[k], delta[k], secular_iters, L);
    for (int i = threadIdx.x; i < n; i += BL_NT) p[voff[k] + i] = L.s[i];
    if (threadIdx.x == 0) { m[k] = L.scal[0]; interior[k] = L.iscal[0]; }
}

// enforce! + to_free! of every member (one thread each) and its first evaluation point in the table
__global__ void blend_init_kernel(double *__restrict__ table, const int32_t *__restrict__ members, int n_members,
                                  const int32_t *__restrict__ member_blend, const int32_t *__restrict__ member_slot,
                                  const double *__restrict__ pos_centers, OptParams op, double *__restrict__ X,
                                  double *__restrict__ pos0) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_members) return;
    OptState S;
    optim_init_values(table + (size_t)members[k] * CEL_P, op, pos_centers ? pos_centers + 2 * k : nullptr, S);
    double *x = X + (size_t)member_blend[k] * 2 * BL_NMAX + NF * member_slot[k];
    for (int i = 0; i < NF; ++i) x[i] = S.x[i];
    pos0[2 * k] = S.pos0[0];
    pos0[2 * k + 1] = S.pos0[1];
}

// One member at free point x: its Jacobian J (44 x 41, column-major) and the second-order term sum_a d_a d2 bound_a /
// dx_i dx_j added into its diagonal block Hd (leading dimension ldh) -- the restatement's to_bound! with derivatives.
__device__ void bl_member_jacobian(const double *x, const double *pos0, const OptParams &op, const double *d,
                                   double *__restrict__ J, double *__restrict__ Hd, int ldh) {
    for (int i = 0; i < 26; ++i) {
        double lo, hi, sc;
        box_bounds(i, pos0, op, lo, hi, sc);
        const double s = 1.0 / (1.0 + exp(-x[i] / sc));
        const double w = hi - lo;
        J[i + CEL_P * i] = w * s * (1 - s) / sc;
        Hd[i + (size_t)ldh * i] += d[i] * w * s * (1 - s) * (1 - 2 * s) / (sc * sc);
    }
    for (int g = 0; g < 3; ++g) {
        const int n = c_simplex_n[g], b0 = c_simplex_b0[g], f0 = c_simplex_f0[g];
        const double sc = 1 - n * c_simplex_lo[g];
        double p[8];
        simplex_probs(x, g, p);
        for (int a = 0; a < n; ++a)
            for (int j = 0; j < n - 1; ++j) {
                J[(b0 + a) + CEL_P * (f0 + j)] = sc * (p[a] * ((a == j) - p[j]));
                for (int k = 0; k < n - 1; ++k) {
                    const double d2 = p[a] * (((a == j) - p[j]) * ((a == k) - p[k]) - p[j] * ((j == k) - p[k]));
                    Hd[(f0 + j) + (size_t)ldh * (f0 + k)] += d[b0 + a] * sc * d2;
                }
            }
    }
}

// Free-space gradient and Hessian of the blend's objective -elbo at the evaluated point xe (all members):
//   g_a = -J_a' d_a,  H_ab = -(J_a' h_ab J_b + [a == b] sum d_a d2 bound_a), then symmetrised.
__device__ void bl_free_derivs(int sa, const double *xe, const double *pos0, const OptParams &op, const double *ev_d,
                               const double *ev_h, const double *ev_x, const int (&pidx)[BL_SA_MAX][BL_SA_MAX],
                               double *__restrict__ J, double *__restrict__ W, double *__restrict__ g, double *__restrict__ H) {
    const int t = threadIdx.x, n = NF * sa;
    for (int idx = t; idx < sa * BL_JN; idx += BL_NT) J[idx] = 0;
    for (int idx = t; idx < n * n; idx += BL_NT) H[idx] = 0;
    __syncthreads();
    if (t < sa)
        bl_member_jacobian(xe + NF * t, pos0 + 2 * t, op, ev_d + (size_t)CEL_P * t, J + (size_t)BL_JN * t,
                           H + NF * t + (size_t)n * NF * t, n);
    __syncthreads();
    for (int idx = t; idx < n; idx += BL_NT) {
        const int a = idx / NF, i = idx % NF;
        const double *Ja = J + (size_t)BL_JN * a, *da = ev_d + (size_t)CEL_P * a;
        double s = 0;
        for (int al = 0; al < CEL_P; ++al) s += Ja[al + CEL_P * i] * da[al];
        g[idx] = -s;
    }
    for (int a = 0; a < sa; ++a)
        for (int b = 0; b < sa; ++b) {
            const int k = pidx[a][b];
            if (a != b && k == 0) continue;           // no common pixels: a zero block
            const double *Jb = J + (size_t)BL_JN * b;
            // W = h_ab J_b (44 x 41)
            for (int idx = t; idx < BL_JN; idx += BL_NT) {
                const int al = idx % CEL_P, j = idx / CEL_P;
                double s = 0;
                if (a == b) {
                    const double *h = ev_h + (size_t)CEL_P * CEL_P * a;
                    for (int be = 0; be < CEL_P; ++be) s += h[al + CEL_P * be] * Jb[be + CEL_P * j];
                } else if (al < LIFT_NP) {
                    const double *x = ev_x + (size_t)LIFT_NP * LIFT_NP * (k > 0 ? k - 1 : -k - 1);
                    for (int be = 0; be < LIFT_NP; ++be)
                        s += (k > 0 ? x[al + LIFT_NP * be] : x[be + LIFT_NP * al]) * Jb[be + CEL_P * j];
                }
                W[idx] = s;
            }
            __syncthreads();
            const double *Ja = J + (size_t)BL_JN * a;
            for (int idx = t; idx < NF * NF; idx += BL_NT) {
                const int i = idx % NF, j = idx / NF;
                double s = 0;
                for (int al = 0; al < CEL_P; ++al) s += Ja[al + CEL_P * i] * W[al + CEL_P * j];
                H[(NF * a + i) + (size_t)n * (NF * b + j)] += s;
            }
            __syncthreads();
        }
    for (int idx = t; idx < n * n; idx += BL_NT) {
        const int i = idx % n, j = idx / n;
        if (i > j) {
            const double s = 0.5 * (H[i + (size_t)n * j] + H[j + (size_t)n * i]);
            H[i + (size_t)n * j] = -s;
            H[j + (size_t)n * i] = -s;
        } else if (i == j) {
            H[idx] = -H[idx];
        }
    }
    __syncthreads();
}

// One Newton trust-region step of every live blend (one workgroup each); see the file comment.
__global__ __launch_bounds__(BL_NT) void blend_step_kernel(
        double *__restrict__ table, const BlendDesc *__restrict__ desc, const int32_t *__restrict__ members,
        const double *__restrict__ pos0, const double *__restrict__ orig, const double *__restrict__ ev_v,
        const double *__restrict__ ev_d, const double *__restrict__ ev_h, const int32_t *__restrict__ ev_st,
        const BlendPair *__restrict__ pairs, const double *__restrict__ ev_x, BlendState *__restrict__ state,
        double *__restrict__ X, double *__restrict__ G, double *__restrict__ Hm, double *__restrict__ A,
        double *__restrict__ V, double *__restrict__ J, double *__restrict__ W, OptParams op) {
    __shared__ BlLds L;
    __shared__ int pidx_s[BL_SA_MAX][BL_SA_MAX];
    __shared__ int s_decision, s_accept;
    const int t = threadIdx.x, slot = blockIdx.x;
    const BlendDesc D = desc[slot];
    const int sa = D.sa, n = NF * sa, b = D.blend;
    BlendState &S = state[b];
    if (S.phase == BL_DONE) return;                 // (uniform: not expected, the host launches live blends only)
    double *x = X + (size_t)b * 2 * BL_NMAX, *xt = x + BL_NMAX;
    const size_t NN = (size_t)BL_NMAX * BL_NMAX;
    double *Aw = A + NN * slot, *Vw = V + NN * slot, *Jw = J + (size_t)BL_SA_MAX * BL_JN * slot, *Ww = W + (size_t)BL_JN * slot;
    const double *pz = pos0 + 2 * D.m0;
    // pair lookup: pidx[a][b] = k + 1 when pair k's record is d2 / d theta_a d theta_b, -(k + 1) when transposed, 0: none
    if (t < BL_SA_MAX * BL_SA_MAX) pidx_s[t / BL_SA_MAX][t % BL_SA_MAX] = 0;
    __syncthreads();
    if (t < D.nk) {
        const BlendPair pr = pairs[D.k0 + t];
        pidx_s[pr.ia][pr.ib] = t + 1;
        pidx_s[pr.ib][pr.ia] = -(t + 1);
    }
    // the evaluation's status: the first failing member, then non-finite cross blocks
    int bad = 0;
    for (int a = 0; a < sa; ++a) if (!bad && ev_st[D.t0 + a] != CELESTE_OK) bad = ev_st[D.t0 + a];
    const double *exs = ev_x + (size_t)LIFT_NP * LIFT_NP * D.k0;
    int nonfinite = 0;
    for (int idx = t; idx < D.nk * LIFT_NP * LIFT_NP; idx += BL_NT) nonfinite |= !isfinite(exs[idx]);
    nonfinite = __syncthreads_or(nonfinite);
    if (!bad && nonfinite) bad = CELESTE_ERR_NONFINITE_RESULT;
    int pidx[BL_SA_MAX][BL_SA_MAX];
    for (int a = 0; a < BL_SA_MAX; ++a) for (int c = 0; c < BL_SA_MAX; ++c) pidx[a][c] = pidx_s[a][c];
    const int phase = S.phase;
    const int newslot = phase == BL_INIT ? S.cur : S.cur ^ 1;
    double *gN = G + ((size_t)b * 2 + newslot) * BL_NMAX, *HN = Hm + ((size_t)b * 2 + newslot) * NN;
    if (!bad) {
        bl_free_derivs(sa, phase == BL_INIT ? x : xt, pz, op, ev_d + (size_t)CEL_P * D.t0, ev_h + (size_t)CEL_P * CEL_P * D.t0,
                       exs, pidx, Jw, Ww, gN, HN);
    }
    // decisions (thread 0): 0 = stop, 1 = solve a new sub-problem
    if (t == 0) {
        int decision = 0, accept = 0;
        if (bad) {
            S.status = bad;
        } else {
            double v = 0;
            for (int a = 0; a < sa; ++a) v += ev_v[D.t0 + a];
            const double fe = -v;
            if (phase == BL_INIT) {
                S.f = fe;
                double gmax0 = 0;
                for (int i = 0; i < n; ++i) gmax0 = fmax(gmax0, fabs(gN[i]));
                decision = !(gmax0 <= op.gtol) && S.it < op.max_iters;
            } else {
                const double m = S.m;
                double rho;
                if (fabs(m) <= 2.220446049250313e-16) rho = 1.0;
                else if (m > 0) rho = 0.25 - 1.0;
                else rho = (S.f - fe) / (0 - m);
                if (rho < 0.25) S.delta *= 0.25;
                else if (rho > 0.75 && !S.interior) S.delta = fmin(2 * S.delta, op.delta_hat);
                bool conv = false;
                if (rho > 0.1) {
                    accept = 1;
                    double dx = 0, gmax = 0;
                    for (int i = 0; i < n; ++i) { dx = fmax(dx, fabs(xt[i] - x[i])); gmax = fmax(gmax, fabs(gN[i])); }
                    const double df = fabs(fe - S.f);
                    S.f = fe;
                    S.cur ^= 1;
                    conv = dx <= op.xtol_abs || df <= op.ftol_rel * fabs(fe) || gmax <= op.gtol;
                }
                decision = !conv && S.it < op.max_iters;
            }
        }
        s_decision = decision;
        s_accept = accept;
    }
    __syncthreads();
    if (s_accept)
        for (int i = t; i < n; i += BL_NT) x[i] = xt[i];
    __syncthreads();
    if (bad) {                                       // the input rows stay
        for (int idx = t; idx < sa * CEL_P; idx += BL_NT)
            table[(size_t)members[D.m0 + idx / CEL_P] * CEL_P + idx % CEL_P] = orig[(size_t)D.m0 * CEL_P + idx];
        if (t == 0) S.phase = BL_DONE;
        return;
    }
    if (!s_decision) {                               // converged or out of iterations: to_bound! at x
        if (t < sa) to_bound_dev(x + NF * t, pz + 2 * t, op, table + (size_t)members[D.m0 + t] * CEL_P);
        if (t == 0) { S.phase = BL_DONE; S.status = CELESTE_OK; }
        return;
    }
    // the sub-problem at x, the trial point xt = x + s
    const int cur = S.cur;
    const double *gC = G + ((size_t)b * 2 + cur) * BL_NMAX, *HC = Hm + ((size_t)b * 2 + cur) * NN;
    for (int idx = t; idx < n * n; idx += BL_NT) Aw[idx] = HC[idx];
    __syncthreads();
    bl_tr_solve(n, Aw, Vw, gC, S.delta, op.secular_iters, L);
    for (int i = t; i < n; i += BL_NT) xt[i] = x[i] + L.s[i];
    __syncthreads();
    if (t < sa) to_bound_dev(xt + NF * t, pz + 2 * t, op, table + (size_t)members[D.m0 + t] * CEL_P);
    if (t == 0) {
        S.m = L.scal[0];
        S.interior = L.iscal[0];
        S.it += 1;
        S.evals += 1;
        S.phase = BL_TRIAL;
    }
}

// celeste_blend_eval: one workgroup per blend assembles the (44 Sa)^2 Hessian, the value, the counters and the status
__global__ __launch_bounds__(BL_NT) void blend_assemble_kernel(
        const BlendDesc *__restrict__ desc, const int64_t *__restrict__ hoff, const BlendPair *__restrict__ pairs,
        const double *__restrict__ ev_v, const double *__restrict__ ev_h, const int64_t *__restrict__ ev_cnt,
        const int32_t *__restrict__ ev_st, const double *__restrict__ ev_x, int want_hess, double *__restrict__ v,
        double *__restrict__ h, int64_t *__restrict__ counters, int32_t *__restrict__ status) {
    const int t = threadIdx.x;
    const BlendDesc D = desc[blockIdx.x];
    const int sa = D.sa, PT = CEL_P * sa;
    int nonfinite = 0;
    if (want_hess) {
        double *hb = h + hoff[blockIdx.x];
        for (int idx = t; idx < PT * PT; idx += BL_NT) {
            const int r = idx % PT, c = idx / PT, a = r / CEL_P, bb = c / CEL_P, i = r % CEL_P, j = c % CEL_P;
            double x = 0;
            if (a == bb) {
                x = ev_h[(size_t)CEL_P * CEL_P * (D.t0 + a) + i + CEL_P * j];
            } else if (i < LIFT_NP && j < LIFT_NP) {
                for (int k = 0; k < D.nk; ++k) {
                    const BlendPair pr = pairs[D.k0 + k];
                    const double *xr = ev_x + (size_t)LIFT_NP * LIFT_NP * (D.k0 + k);
                    if (pr.ia == a && pr.ib == bb) { x = xr[i + LIFT_NP * j]; nonfinite |= !isfinite(x); }
                    else if (pr.ia == bb && pr.ib == a) { x = xr[j + LIFT_NP * i]; nonfinite |= !isfinite(x); }
                }
            }
            hb[idx] = x;
        }
    }
    nonfinite = __syncthreads_or(nonfinite);
    if (t == 0) {
        double vs = 0;
        int64_t na = 0, ni = 0;
        int st = CELESTE_OK;
        for (int a = 0; a < sa; ++a) {
            vs += ev_v[D.t0 + a];
            na += ev_cnt[2 * (D.t0 + a)];
            ni += ev_cnt[2 * (D.t0 + a) + 1];
            if (ev_st[D.t0 + a] != CELESTE_OK && st == CELESTE_OK) st = ev_st[D.t0 + a];
        }
        if (nonfinite && st == CELESTE_OK) st = CELESTE_ERR_NONFINITE_RESULT;
        v[blockIdx.x] = vs;
        counters[2 * blockIdx.x] = na;
        counters[2 * blockIdx.x + 1] = ni;
        status[blockIdx.x] = st;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
// last_ms of the last celeste_blend_maximize: evaluation launches, step launches (device time, summed over iterations), iterations
struct celeste_blend_ctx : ClientCtx<32, 3, 3> {
    // host staging of one evaluation launch set: kept here, not on the stack, so that it outlives the asynchronous copies
    // (the next launch set is built only after the stream has been waited for)
    std::vector<int32_t> tg, psa, psb;
    std::vector<BlendDesc> desc;
    std::vector<BlendPair> pairs;
};

extern "C" int celeste_blend_version(void) { return CELESTE_BLEND_ABI_VERSION; }

extern "C" const char *celeste_blend_strerror(int status) { return celeste_strerror(status); }

extern "C" int celeste_blend_ctx_create(const celeste_problem_t *problem, int device, celeste_blend_ctx_t **out) try {
    return client_create(problem, device, out);
} ABI_CATCH

extern "C" void celeste_blend_ctx_destroy(celeste_blend_ctx_t *b) { client_destroy(b); }

// The blends of a call, checked: members in call order, the blend and the slot of each, the overlapping pairs of each blend.
struct BlendPlan {
    int B = 0, M = 0;
    std::vector<int32_t> sa, m0, member_blend, member_slot, rank;
    std::vector<std::vector<BlendPair>> pairs;     // per blend
    std::vector<std::vector<int32_t>> pair_src;    // per blend: (source a, source b) of each pair, in the cross kernels' order
};

static int bl_plan(const celeste_ctx_t *c, int32_t n_blends, const int64_t *off, const int32_t *src, bool want_pairs,
                   BlendPlan &P) {
    if (n_blends < 0 || (n_blends > 0 && (!off || !src)) || (n_blends > 0 && off[0] != 0)) return CELESTE_ERR_INVALID_ARG;
    P.B = n_blends;
    P.rank.assign((size_t)c->S, -1);
    std::vector<int32_t> owner((size_t)c->S, -1);
    for (int b = 0; b < n_blends; ++b) {
        const int64_t k = off[b + 1] - off[b];
        if (k < 1 || k > BL_SA_MAX) return CELESTE_ERR_INVALID_ARG;
        P.sa.push_back((int32_t)k);
        P.m0.push_back((int32_t)off[b]);
        for (int64_t a = 0; a < k; ++a) {
            const int32_t s = src[off[b] + a];
            if (s < 0 || s >= c->S || owner[s] >= 0) return CELESTE_ERR_INVALID_ARG;   // out of range, or a repeat
            owner[s] = b;
            P.rank[s] = (int32_t)a;
            P.member_blend.push_back(b);
            P.member_slot.push_back((int32_t)a);
        }
    }
    P.M = n_blends > 0 ? (int)off[n_blends] : 0;
    // no member may neighbour a member of another blend (either direction: every member's list is scanned)
    for (int k = 0; k < P.M; ++k) {
        const int s = src[k];
        for (int64_t q = c->h_nbr_off[s]; q < c->h_nbr_off[s + 1]; ++q) {
            const int o = owner[c->h_nbr_idx[q]];
            if (o >= 0 && o != P.member_blend[k]) return CELESTE_ERR_INVALID_ARG;
        }
    }
    P.pairs.assign(n_blends, {});
    P.pair_src.assign(n_blends, {});
    if (want_pairs)    // pairs of members that light common pixels; the first of a pair lists the second (eval_multi's rule)
        for (int b = 0; b < n_blends; ++b)
            for (int ia = 0; ia < P.sa[b]; ++ia)
                for (int ib = ia + 1; ib < P.sa[b]; ++ib) {
                    const int sA = src[P.m0[b] + ia], sB = src[P.m0[b] + ib];
                    if (nbr_lists(c, sA, sB)) { P.pairs[b].push_back({ia, ib}); P.pair_src[b].push_back(sA); P.pair_src[b].push_back(sB); }
                    else if (nbr_lists(c, sB, sA)) { P.pairs[b].push_back({ib, ia}); P.pair_src[b].push_back(sB); P.pair_src[b].push_back(sA); }
                }
    return CELESTE_OK;
}

// The launch set of one evaluation of the blends `live`: target list, descriptors, pairs; the multi-active evaluation and
// the cross blocks.  Outputs in the buffers 0..8 of the context.
struct BlEvalOut {
    double *v, *d, *h, *x;
    int64_t *cnt;
    int32_t *st;
    BlendDesc *desc;
    BlendPair *pairs;
    int nt, np;
};

static int bl_eval_launch(celeste_blend_ctx_t *bc, const double *d_table, const int32_t *d_rank, const BlendPlan &P,
                          const int32_t *src, const std::vector<int32_t> &live, uint32_t flags, BlEvalOut &o) {
    celeste_ctx_t *c = bc->c;
    const bool want_hess = (flags & CELESTE_FLAG_HESS) != 0;
    std::vector<int32_t> &tg = bc->tg, &psa = bc->psa, &psb = bc->psb;
    std::vector<BlendDesc> &desc = bc->desc;
    std::vector<BlendPair> &pairs = bc->pairs;
    tg.clear(); psa.clear(); psb.clear(); desc.clear(); pairs.clear();
    for (int b : live) {
        BlendDesc D;
        D.blend = b; D.sa = P.sa[b]; D.t0 = (int32_t)tg.size(); D.m0 = P.m0[b];
        D.k0 = (int32_t)pairs.size(); D.nk = want_hess ? (int32_t)P.pairs[b].size() : 0;
        for (int a = 0; a < P.sa[b]; ++a) tg.push_back(src[P.m0[b] + a]);
        if (want_hess)
            for (size_t k = 0; k < P.pairs[b].size(); ++k) {
                pairs.push_back(P.pairs[b][k]);
                psa.push_back(P.pair_src[b][2 * k]);
                psb.push_back(P.pair_src[b][2 * k + 1]);
            }
        desc.push_back(D);
    }
    const size_t nt = tg.size(), np = pairs.size();
    o.nt = (int)nt; o.np = (int)np;
    int32_t *d_t = nullptr, *d_pa = nullptr, *d_pb = nullptr;
    double *d_rec = nullptr;
    if (client_get(bc, 0, nt * sizeof(int32_t), &d_t) != hipSuccess || client_get(bc, 1, nt * sizeof(double), &o.v) != hipSuccess ||
        client_get(bc, 2, nt * CEL_P * sizeof(double), &o.d) != hipSuccess ||
        client_get(bc, 3, (want_hess ? nt : 1) * CEL_P * CEL_P * sizeof(double), &o.h) != hipSuccess ||
        client_get(bc, 4, nt * 2 * sizeof(int64_t), &o.cnt) != hipSuccess || client_get(bc, 5, nt * sizeof(int32_t), &o.st) != hipSuccess ||
        client_get(bc, 6, desc.size() * sizeof(BlendDesc), &o.desc) != hipSuccess ||
        client_get(bc, 7, std::max<size_t>(np, 1) * sizeof(BlendPair), &o.pairs) != hipSuccess ||
        client_get(bc, 8, std::max<size_t>(np, 1) * LIFT_NP * LIFT_NP * sizeof(double), &o.x) != hipSuccess)
        return CELESTE_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(d_t, tg.data(), nt * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(o.desc, desc.data(), desc.size() * sizeof(BlendDesc), hipMemcpyHostToDevice, c->stream));
    const int rc = launch_eval(c, d_table, (int32_t)nt, d_t, flags, o.v, o.d, want_hess ? o.h : nullptr, o.cnt, o.st, c->stream,
                               true, d_rank);
    if (rc != CELESTE_OK) return rc;
    if (np > 0) {
        if (client_get(bc, 9, np * sizeof(int32_t), &d_pa) != hipSuccess || client_get(bc, 10, np * sizeof(int32_t), &d_pb) != hipSuccess ||
            client_get(bc, 11, np * c->N * ZV * ZV * sizeof(double), &d_rec) != hipSuccess)
            return CELESTE_ERR_HIP;
        HIP_TRY(hipMemcpyAsync(o.pairs, pairs.data(), np * sizeof(BlendPair), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_pa, psa.data(), np * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_pb, psb.data(), np * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        launch_cross(c, d_table, np, d_pa, d_pb, d_rec, o.x, c->stream);
        HIP_TRY(hipGetLastError());
    }
    return CELESTE_OK;
}

static int bl_upload_rank(celeste_blend_ctx_t *bc, const BlendPlan &P, int32_t **d_rank) {
    celeste_ctx_t *c = bc->c;
    if (client_get(bc, 12, (size_t)c->S * sizeof(int32_t), d_rank) != hipSuccess) return CELESTE_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(*d_rank, P.rank.data(), (size_t)c->S * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    return CELESTE_OK;
}

extern "C" int celeste_blend_eval(celeste_blend_ctx_t *bc, const double *vp, int32_t n_blends, const int64_t *blend_offsets,
                                  const int32_t *blend_sources, uint32_t flags, double *v, double *d, double *h,
                                  int64_t *counters, int32_t *status) try {
    if (!bc || !bc->c || !vp || (flags & (CELESTE_FLAG_SPLIT | CELESTE_FLAG_PACKED_HESS | CELESTE_FLAG_FP32)))
        return CELESTE_ERR_INVALID_ARG;
    celeste_ctx_t *c = bc->c;
    const bool want_hess = (flags & CELESTE_FLAG_HESS) != 0;
    const bool want_grad = want_hess || (flags & CELESTE_FLAG_GRAD) != 0;
    if (n_blends > 0 && (!v || !counters || !status || (want_grad && !d) || (want_hess && !h))) return CELESTE_ERR_INVALID_ARG;
    BlendPlan P;
    int rc = bl_plan(c, n_blends, blend_offsets, blend_sources, want_hess, P);
    if (rc != CELESTE_OK || n_blends == 0) return rc;
    HIP_TRY(hipSetDevice(c->device));
    double *d_table = nullptr, *d_vo = nullptr, *d_ho = nullptr;
    int64_t *d_hoff = nullptr, *d_co = nullptr;
    int32_t *d_rank = nullptr, *d_so = nullptr;
    std::vector<int64_t> hoff(n_blends + 1, 0);
    for (int b = 0; b < n_blends; ++b) hoff[b + 1] = hoff[b] + (int64_t)CEL_P * P.sa[b] * CEL_P * P.sa[b];
    if (client_get(bc, 13, (size_t)c->S * CEL_P * sizeof(double), &d_table) != hipSuccess ||
        client_get(bc, 14, n_blends * sizeof(double), &d_vo) != hipSuccess ||
        client_get(bc, 15, (want_hess ? hoff[n_blends] : 1) * sizeof(double), &d_ho) != hipSuccess ||
        client_get(bc, 16, (n_blends + 1) * sizeof(int64_t), &d_hoff) != hipSuccess ||
        client_get(bc, 17, 2 * n_blends * sizeof(int64_t), &d_co) != hipSuccess ||
        client_get(bc, 18, n_blends * sizeof(int32_t), &d_so) != hipSuccess)
        return CELESTE_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(d_table, vp, (size_t)c->S * CEL_P * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_hoff, hoff.data(), (n_blends + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    if ((rc = bl_upload_rank(bc, P, &d_rank)) != CELESTE_OK) return rc;
    std::vector<int32_t> live(n_blends);
    for (int b = 0; b < n_blends; ++b) live[b] = b;
    BlEvalOut o;
    if ((rc = bl_eval_launch(bc, d_table, d_rank, P, blend_sources, live, flags, o)) != CELESTE_OK) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    hipLaunchKernelGGL(blend_assemble_kernel, dim3((unsigned)n_blends), dim3(BL_NT), 0, c->stream, o.desc, d_hoff, o.pairs,
                       o.v, o.h, o.cnt, o.st, o.x, (int)want_hess, d_vo, d_ho, d_co, d_so);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(v, d_vo, n_blends * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(counters, d_co, 2 * n_blends * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(status, d_so, n_blends * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (want_grad) HIP_TRY(hipMemcpyAsync(d, o.d, (size_t)P.M * CEL_P * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (want_hess) HIP_TRY(hipMemcpyAsync(h, d_ho, hoff[n_blends] * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return client_first_status(status, n_blends);
} ABI_CATCH

extern "C" int celeste_blend_maximize(celeste_blend_ctx_t *bc, double *vp, const double *vp_neighbors,
                                      const double *pos_centers, int32_t n_blends, const int64_t *blend_offsets,
                                      const int32_t *blend_sources, const celeste_optim_config_t *cfg, int32_t *iterations,
                                      int32_t *f_evals, double *elbo, int32_t *status) try {
    if (!bc || !bc->c || !vp) return CELESTE_ERR_INVALID_ARG;
    celeste_ctx_t *c = bc->c;
    OptParams op;
    uint32_t flags = 0;
    int rc = optim_config(cfg, &op, &flags);
    if (rc != CELESTE_OK) return rc;
    BlendPlan P;
    if ((rc = bl_plan(c, n_blends, blend_offsets, blend_sources, true, P)) != CELESTE_OK || n_blends == 0) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const int B = n_blends, M = P.M;
    const size_t NN = (size_t)BL_NMAX * BL_NMAX;
    // the call's table: non-members at vp_neighbors, members at vp; the members' input rows for the blends that fail
    std::vector<double> tbl(vp_neighbors ? vp_neighbors : vp, (vp_neighbors ? vp_neighbors : vp) + (size_t)c->S * CEL_P);
    std::vector<double> orig((size_t)M * CEL_P);
    for (int k = 0; k < M; ++k) {
        const int s = blend_sources[k];
        memcpy(&tbl[(size_t)s * CEL_P], vp + (size_t)s * CEL_P, CEL_P * sizeof(double));
        memcpy(&orig[(size_t)k * CEL_P], vp + (size_t)s * CEL_P, CEL_P * sizeof(double));
    }
    std::vector<BlendState> hs(B);
    for (auto &s : hs) {
        memset(&s, 0, sizeof s);
        s.delta = op.initial_delta;
        s.evals = 1;
        s.phase = BL_INIT;
    }
    double *d_table = nullptr, *d_orig = nullptr, *d_pos = nullptr, *d_pos0 = nullptr, *d_X = nullptr, *d_G = nullptr,
           *d_H = nullptr, *d_A = nullptr, *d_V = nullptr, *d_J = nullptr, *d_W = nullptr;
    int32_t *d_members = nullptr, *d_mb = nullptr, *d_ms = nullptr, *d_rank = nullptr;
    BlendState *d_state = nullptr;
    if (client_get(bc, 13, (size_t)c->S * CEL_P * sizeof(double), &d_table) != hipSuccess ||
        client_get(bc, 19, (size_t)M * CEL_P * sizeof(double), &d_orig) != hipSuccess ||
        client_get(bc, 20, (size_t)M * 2 * sizeof(double), &d_pos) != hipSuccess ||
        client_get(bc, 21, (size_t)M * 2 * sizeof(double), &d_pos0) != hipSuccess ||
        client_get(bc, 22, (size_t)B * 2 * BL_NMAX * sizeof(double), &d_X) != hipSuccess ||
        client_get(bc, 23, (size_t)B * 2 * BL_NMAX * sizeof(double), &d_G) != hipSuccess ||
        client_get(bc, 24, (size_t)B * 2 * NN * sizeof(double), &d_H) != hipSuccess ||
        client_get(bc, 25, (size_t)B * NN * sizeof(double), &d_A) != hipSuccess ||
        client_get(bc, 26, (size_t)B * NN * sizeof(double), &d_V) != hipSuccess ||
        client_get(bc, 27, (size_t)B * BL_SA_MAX * BL_JN * sizeof(double), &d_J) != hipSuccess ||
        client_get(bc, 28, (size_t)B * BL_JN * sizeof(double), &d_W) != hipSuccess ||
        client_get(bc, 29, (size_t)M * 3 * sizeof(int32_t), &d_members) != hipSuccess ||
        client_get(bc, 30, (size_t)B * sizeof(BlendState), &d_state) != hipSuccess)
        return CELESTE_ERR_HIP;
    d_mb = d_members + M;
    d_ms = d_members + 2 * M;
    HIP_TRY(hipMemcpyAsync(d_table, tbl.data(), tbl.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_orig, orig.data(), orig.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_members, blend_sources, (size_t)M * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_mb, P.member_blend.data(), (size_t)M * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_ms, P.member_slot.data(), (size_t)M * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_state, hs.data(), (size_t)B * sizeof(BlendState), hipMemcpyHostToDevice, c->stream));
    if (pos_centers) HIP_TRY(hipMemcpyAsync(d_pos, pos_centers, (size_t)M * 2 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if ((rc = bl_upload_rank(bc, P, &d_rank)) != CELESTE_OK) return rc;
    hipLaunchKernelGGL(blend_init_kernel, dim3((unsigned)((M + 63) / 64)), dim3(64), 0, c->stream, d_table, d_members, M, d_mb,
                       d_ms, pos_centers ? d_pos : nullptr, op, d_X, d_pos0);
    HIP_TRY(hipGetLastError());
    std::vector<int32_t> live(B);
    for (int b = 0; b < B; ++b) live[b] = b;
    bc->last_ms[0] = bc->last_ms[1] = bc->last_ms[2] = 0;
    for (int round = 0; !live.empty() && round <= op.max_iters + 1; ++round) {
        BlEvalOut o;
        if (hipEventRecord(bc->ev[0], c->stream) != hipSuccess) { rc = CELESTE_ERR_HIP; break; }
        if ((rc = bl_eval_launch(bc, d_table, d_rank, P, blend_sources, live, flags, o)) != CELESTE_OK) break;
        if (hipEventRecord(bc->ev[1], c->stream) != hipSuccess) { rc = CELESTE_ERR_HIP; break; }
        hipLaunchKernelGGL(blend_step_kernel, dim3((unsigned)live.size()), dim3(BL_NT), 0, c->stream, d_table, o.desc, d_members,
                           d_pos0, d_orig, o.v, o.d, o.h, o.st, o.pairs, o.x, d_state, d_X, d_G, d_H, d_A, d_V, d_J, d_W, op);
        if (hipGetLastError() != hipSuccess || hipEventRecord(bc->ev[2], c->stream) != hipSuccess) { rc = CELESTE_ERR_HIP; break; }
        if (hipMemcpyAsync(hs.data(), d_state, (size_t)B * sizeof(BlendState), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) { rc = CELESTE_ERR_HIP; break; }
        float me = 0, ms = 0;
        if (hipEventElapsedTime(&me, bc->ev[0], bc->ev[1]) == hipSuccess && hipEventElapsedTime(&ms, bc->ev[1], bc->ev[2]) == hipSuccess) {
            bc->last_ms[0] += me;
            bc->last_ms[1] += ms;
        }
        bc->last_ms[2] += 1;
        std::vector<int32_t> next;
        for (int b : live) if (hs[b].phase != BL_DONE) next.push_back(b);
        live.swap(next);
    }
    if (rc == CELESTE_OK && !live.empty()) rc = CELESTE_ERR_HIP;   // (cannot happen: every blend stops within max_iters + 1)
    if (rc != CELESTE_OK) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    HIP_TRY(hipMemcpyAsync(tbl.data(), d_table, tbl.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int first = CELESTE_OK;
    for (int b = 0; b < B; ++b) {
        for (int a = 0; a < P.sa[b]; ++a) {
            const int s = blend_sources[P.m0[b] + a];
            memcpy(vp + (size_t)s * CEL_P, &tbl[(size_t)s * CEL_P], CEL_P * sizeof(double));
        }
        if (iterations) iterations[b] = hs[b].it;
        if (f_evals) f_evals[b] = hs[b].evals;
        if (elbo) elbo[b] = hs[b].status == CELESTE_OK ? -hs[b].f : NAN;
        if (status) status[b] = hs[b].status;
        if (hs[b].status != CELESTE_OK && first == CELESTE_OK) first = hs[b].status;
    }
    return first;
} ABI_CATCH

extern "C" int celeste_blend_last_ms(celeste_blend_ctx_t *bc, float ms[3]) { return client_last_ms(bc, ms); }

extern "C" int celeste_blend_tr_solve_batch(int device, int32_t n, const int32_t *dims, const double *H, const double *g,
                                            const double *delta, int32_t solver, int32_t secular_iters, double *p, double *m,
                                            int32_t *interior) try {
    if (n < 0 || solver != 0 || secular_iters < 0 || (n > 0 && (!dims || !H || !g || !delta || !p))) return CELESTE_ERR_INVALID_ARG;
    if (n == 0) return CELESTE_OK;
    std::vector<int64_t> moff(n + 1, 0), voff(n + 1, 0);
    for (int k = 0; k < n; ++k) {
        if (dims[k] < 1 || dims[k] > BL_NMAX) return CELESTE_ERR_INVALID_ARG;
        moff[k + 1] = moff[k] + (int64_t)dims[k] * dims[k];
        voff[k + 1] = voff[k] + dims[k];
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return CELESTE_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return CELESTE_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(device));
    const size_t MN = (size_t)moff[n], VN = (size_t)voff[n];
    double *d_H = nullptr, *d_A = nullptr, *d_V = nullptr, *d_g = nullptr, *d_delta = nullptr, *d_p = nullptr, *d_m = nullptr;
    int32_t *d_dims = nullptr, *d_int = nullptr;
    int64_t *d_off = nullptr;
    int rc = CELESTE_OK;
    std::vector<double> hm(n);
    std::vector<int32_t> hi(n);
#define TR_TRY(expr) do { if ((expr) != hipSuccess) { rc = CELESTE_ERR_HIP; goto done; } } while (0)
    TR_TRY(hipMalloc(&d_H, MN * sizeof(double)));
    TR_TRY(hipMalloc(&d_A, MN * sizeof(double)));
    TR_TRY(hipMalloc(&d_V, MN * sizeof(double)));
    TR_TRY(hipMalloc(&d_g, VN * sizeof(double)));
    TR_TRY(hipMalloc(&d_p, VN * sizeof(double)));
    TR_TRY(hipMalloc(&d_delta, n * sizeof(double)));
    TR_TRY(hipMalloc(&d_m, n * sizeof(double)));
    TR_TRY(hipMalloc(&d_dims, n * sizeof(int32_t)));
    TR_TRY(hipMalloc(&d_int, n * sizeof(int32_t)));
    TR_TRY(hipMalloc(&d_off, 2 * (n + 1) * sizeof(int64_t)));
    TR_TRY(hipMemcpy(d_H, H, MN * sizeof(double), hipMemcpyHostToDevice));
    TR_TRY(hipMemcpy(d_g, g, VN * sizeof(double), hipMemcpyHostToDevice));
    TR_TRY(hipMemcpy(d_delta, delta, n * sizeof(double), hipMemcpyHostToDevice));
    TR_TRY(hipMemcpy(d_dims, dims, n * sizeof(int32_t), hipMemcpyHostToDevice));
    TR_TRY(hipMemcpy(d_off, moff.data(), (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    TR_TRY(hipMemcpy(d_off + n + 1, voff.data(), (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(blend_tr_kernel, dim3((unsigned)n), dim3(BL_NT), 0, 0, d_dims, d_off, d_off + n + 1, d_H, d_g, d_delta,
                       secular_iters > 0 ? secular_iters : 20, d_A, d_V, d_p, d_m, d_int);
    TR_TRY(hipGetLastError());
    TR_TRY(hipMemcpy(p, d_p, VN * sizeof(double), hipMemcpyDeviceToHost));
    TR_TRY(hipMemcpy(hm.data(), d_m, n * sizeof(double), hipMemcpyDeviceToHost));
    TR_TRY(hipMemcpy(hi.data(), d_int, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (m) memcpy(m, hm.data(), n * sizeof(double));
    if (interior) memcpy(interior, hi.data(), n * sizeof(int32_t));
done:
#undef TR_TRY
    (void)hipDeviceSynchronize();
    for (void *q : {(void *)d_H, (void *)d_A, (void *)d_V, (void *)d_g, (void *)d_p, (void *)d_delta, (void *)d_m, (void *)d_dims,
                    (void *)d_int, (void *)d_off})
        if (q) (void)hipFree(q);
    return rc;
} ABI_CATCH
