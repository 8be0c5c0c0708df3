// hns_rnn_train.hip — the head and the loss of a recurrent MAPPO update over the GRU op's output, forward and backward.
//
// A recurrent minibatch is B segments x L steps x A agents.  Row (b, t, a) — row index (b L + t) A + a, the order of the encoder op's
// [B L A, 128] features — reads y[b, a, t, :] (hns_gru_forward's output, read as it lies through three strides) and its per-row data at
// env-step e = segment[b] L + t of the rollout's contiguous [N T, A(, 4)] arrays.  The encoder and the GRU run through their own entries; these
// kernels are what remained in torch: fc_mean / v_out, the distribution, the loss, and their backward pass down to dy.
//
// Mapping (both networks): a workgroup is 256 threads = 32 row groups of 8 lanes; lane g of a group holds the row's features 4 g + 32 i + u
// (i, u in [0, 4): four float4 loads, 128 contiguous bytes per group and load).  A TRIP of a workgroup is 32 consecutive rows (kRtRows); the
// grid is G = min(ceil(rows / 32), 512) workgroups (kRtMaxGroups) and workgroup w takes trips w, w + G, w + 2 G, ...  The head's 128-wide dot
// products are 16 fmaf per lane (feature order i, u) and the butterfly s += s[lane ^ 1], [lane ^ 2], [lane ^ 4]; no MFMA.
//
//   hns_rnn_actor_rows_kernel    : per row mu, logp (fp64), the ratio, the clipped surrogate and its backward weight (hns_actor_train_grad's
//                                  statements), dy, log_probs; the ratio of every row goes to the workspace, column-major [L A][B] (-1 marks a row that is left out)
//   hns_rnn_ess_kernel           : one 256-thread workgroup per (step, agent) column c: M = the column's largest ratio, thread i adds exp(r - M) and
//                                  exp(2 (r - M)) of segments i, i + 256, ..., thread 0 adds the 256 sums in index order -> col[c] = exp(2 lse(r) - lse(2 r))
//   hns_rnn_actor_final_kernel   : element e of [d fc_mean.weight (512), d fc_mean.bias (4), d log_std (4), the loss sum] adds the G workgroup
//                                  partials in index order (fp64), rounds once; d log_std takes -entropy_coef once; ess = sum_c col[c] / (L A) / B
//   hns_rnn_critic_values_kernel : per row v and the five fp64 terms of hns_critic_train_grad's loss launch; v goes to the workspace
//   hns_rnn_critic_decide_kernel : the G partials of each of the five sums in index order; value_loss, explained_var and the branch weights by
//                                  ct_loss_decide's rule (1 / 0, 0 / 1, or 0.5 / 0.5 at an exact tie)
//   hns_rnn_critic_grad_kernel   : per row dv from the branch weights, dy, and the head's gradient partials (y is read a second time)
//   hns_rnn_critic_final_kernel  : element e of [d v_out.weight (128), d v_out.bias] adds the G partials in index order, rounds once
//
// The global forms (one rank's part of an update over the union of W ranks' minibatches) are the same row kernels with other
// scalars — inv_n = f32(1 / global_rows), n = global_rows, entropy_coef entropy_share — and two small kernels:
//   hns_rnn_critic_sums_kernel          : hns_rnn_critic_head_sums' second launch: the G partials of the five sums in the decide kernel's order,
//                                         written as they are (fp64) for the caller's all-reduce
//   hns_rnn_critic_decide_global_kernel : the decide kernel's rule (rt_decide, shared) on the union's sums and row count given by the caller
// hns_rnn_critic_head_grad_global runs the values kernel again for v (its own workspace: the call stands alone), so y is read twice as in the
// local entry.  With one rank every output has the local entries' bits.
//
// One head per agent (hns_rnn_actor_head_grad_agents): head_w [A, 4, 128], head_b [A, 4], log_std [A, 4], the row's agent
// selects the slices.
//   hns_rnn_actor_rows_agents_kernel  : the rows kernel's body (hns_rnn_bodies.inc, shared as text) on A gpa workgroups, gpa = min(ceil(B L / 32),
//                                       floor(512 / A)); workgroup w belongs to agent w / gpa and takes trips w % gpa, w % gpa + gpa, ... of that
//                                       agent's B L positions (b, t), 32 to a trip — the per-row arithmetic is the shared kernel's
//   hns_rnn_ess_kernel                : unchanged (its columns are per agent already)
//   hns_rnn_actor_final_agents_kernel : agent a's slice of the stacked gradients from its gpa partials in index order; d log_std[a] takes
//                                       -entropy_coef / A once; the loss sum adds all A gpa partials in workgroup order (agent-major);
//                                       entropy = the agents' entropies (four terms in index order each) added in agent order, over A
// hns_rnn_actor_head_grad_agents_global is these launches with the global forms' scalars: inv_n = f32(1 / global_rows),
// n = global_rows, and entropy_coef entropy_share where the final kernel takes entropy_coef, so d log_std[a] takes -(entropy_coef entropy_share) / A.
//
// Order of every sum.  A lane adds its rows' contributions trip after trip (the head-gradient products in fp32, the loss terms in fp64: a lane
// sees ceil(trips / G) rows); the workgroup's partial is the 32 row groups added in index order in fp64; the partials are added in workgroup
// order in fp64 and rounded once to fp32.  G and the trips are functions of the shape alone: the same inputs give the same bits.  No atomics.
//
// A segment id outside [0, num_segments) makes its L A rows DEAD: their per-row data is not read (the id never enters an address), their dy
// rows are zeros, they add nothing to any sum; n stays B L A.  y and dy are addressed by b, never by the id.
#include <hip/hip_runtime.h>

#include <string>

#include "hns_device.h"
#include "hns_host.h"
#include "../../include/hns.h"

static_assert(sizeof(hns_rnn_rows) == 72, "hns_rnn_rows: abi.HnsRnnRows mirrors this layout");

namespace hns {

typedef float rt_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kRtThreads = 256;
constexpr int kRtRows = 32;                                     // rows of a trip: 8 lanes each
constexpr int kRtMaxGroups = 512;                               // two workgroups per CU
constexpr int kRtE = HNS_GRU_HIDDEN;
constexpr int kRtAct = 4;
constexpr int kRtActorSlots = 528;                              // fp64 per workgroup: d W [4][128], d b [4], d log_std [4], the loss sum (521 used)
constexpr int kRtActorUsed = 521;
constexpr int kRtCriticSlots = 136;                             // d W [128], d b (129 used)
constexpr int kRtCriticUsed = 129;
constexpr int kRtSumSlots = 8;                                  // the critic's five sums (5 used)
constexpr int kRtFinalElems = 8;                                // elements of a final-sum workgroup: their G partials staged in 32 KB of LDS

struct RtGeom {
    const float *y;
    float *dy;
    long long s0, s1, s2, rows, nseg;
    int A, L, LA;
    const long long *segment;
};

struct RtRow {
    bool in, live;
    long long yoff, idx;                                        // the row's offset in y / dy; its (env-step, agent) index in the [N T, A] arrays
};

// row -> (b, t, a); a row past the end borrows the last row's address (nothing of it is loaded or stored)
HNS_DEV RtRow rt_row(const RtGeom &G, long long row) {
    RtRow R;
    R.in = row < G.rows;
    const long long rr = R.in ? row : G.rows - 1;
    const long long b = rr / G.LA;
    const int rem = (int)(rr - b * G.LA);
    const int t = rem / G.A, ag = rem - t * G.A;
    R.yoff = b * G.s0 + ag * G.s1 + t * G.s2;
    const long long seg = G.segment ? G.segment[b] : b;
    R.live = R.in && seg >= 0 && seg < G.nseg;
    R.idx = R.live ? (seg * G.L + t) * G.A + ag : 0;
    return R;
}

HNS_DEV float rt_sum8(float v) {
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    return v;
}

// the lane's 16 values of a 128-vector: x[4 i + u] = p[4 g + 32 i + u]
HNS_DEV void rt_load(const float *p, int g, float (&x)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const rt_f32x4 v = *reinterpret_cast<const rt_f32x4 *>(p + 4 * g + 32 * i);
#pragma unroll
        for (int u = 0; u < 4; ++u) x[4 * i + u] = v[u];
    }
}

HNS_DEV void rt_store(float *p, int g, const float (&x)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        rt_f32x4 v;
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = x[4 * i + u];
        *reinterpret_cast<rt_f32x4 *>(p + 4 * g + 32 * i) = v;
    }
}

HNS_DEV float rt_dot(const float (&w)[16], const float (&y)[16]) {
    float s = 0.0f;
#pragma unroll
    for (int q = 0; q < 16; ++q) s = __builtin_fmaf(w[q], y[q], s);
    return rt_sum8(s);
}

// the workgroup's 32 lane vectors of one 128-wide gradient row, added over the row groups in index order in fp64 -> dst[0 .. 128)
HNS_DEV void rt_flush(float (&red)[kRtRows][kRtE], const float (&x)[16], double *dst, int tid, int r, int g) {
    __syncthreads();
    rt_store(red[r], g, x);
    __syncthreads();
    if (tid < kRtE) {
        double s = 0.0;
        for (int rr = 0; rr < kRtRows; ++rr) s += (double)red[rr][tid];
        dst[tid] = s;
    }
}

struct RtActorArgs {
    RtGeom G;
    const float *head_w, *head_b, *log_std, *action, *logp_old, *adv;
    float clip_lo, clip_hi, inv_n;
    float *logp_new, *ratio;
    long long B;
    double *part;
};

#define RT_TRIP_ROWS a.G.rows
#define RT_TRIP_FIRST blockIdx.x
#define RT_TRIP_STEP gridDim.x
#define RT_ROW(p) (p)
__global__ __launch_bounds__(kRtThreads, 2) void hns_rnn_actor_rows_kernel(const RtActorArgs a) {
#include "hns_rnn_bodies.inc"
}
#undef RT_TRIP_ROWS
#undef RT_TRIP_FIRST
#undef RT_TRIP_STEP
#undef RT_ROW

// One head per agent (hns_rnn_actor_head_grad_agents): a0's head tensors are the stacked ones.  The grid is A gpa workgroups; workgroup w belongs
// to agent w / gpa for the whole launch — that agent's head in its registers, its partial that agent's alone — and takes trips w % gpa,
// w % gpa + gpa, ... of the agent's B L positions p = b L + t, 32 to a trip: row p A + agent.
#define RT_TRIP_ROWS (a.G.rows / a.G.A)
#define RT_TRIP_FIRST (blockIdx.x % gpa)
#define RT_TRIP_STEP gpa
#define RT_ROW(p) ((p) < a.G.rows / a.G.A ? (p) * a.G.A + agent : a.G.rows)
__global__ __launch_bounds__(kRtThreads, 2) void hns_rnn_actor_rows_agents_kernel(const RtActorArgs a0, int gpa) {
    const int agent = blockIdx.x / gpa;
    RtActorArgs a = a0;
    a.head_w += agent * kRtAct * kRtE;
    a.head_b += agent * kRtAct;
    a.log_std += agent * kRtAct;
#include "hns_rnn_bodies.inc"
}
#undef RT_TRIP_ROWS
#undef RT_TRIP_FIRST
#undef RT_TRIP_STEP
#undef RT_ROW

// the G workgroup partials of the block's kRtFinalElems elements e0 .. e0 + 7, staged through LDS (independent loads: a thread that walked the
// partials itself would pay one memory latency per partial) and added in workgroup order by the element's thread; returns the sum on tid < 8
HNS_DEV double rt_sum_partials(const double *part, int groups, int slots, int e0, int used, double (&stage)[kRtMaxGroups][kRtFinalElems], int tid) {
    const int j = tid % kRtFinalElems;
    for (int w = tid / kRtFinalElems; w < groups; w += kRtThreads / kRtFinalElems)
        stage[w][j] = e0 + j < used ? part[(long long)w * slots + e0 + j] : 0.0;
    __syncthreads();
    double s = 0.0;
    if (tid < kRtFinalElems)
        for (int w = 0; w < groups; ++w) s += stage[w][tid];
    return s;
}

// column c = (step, agent) of the [B, L A] ratios: exp(2 logsumexp_b(r) - logsumexp_b(2 r)), of the ratio itself, as the reference writes it.
// M = the column's largest ratio (a maximum has no order); thread i adds exp(r - M) and exp(2 (r - M)) of segments i, i + 256, ... in that
// order, thread 0 adds the 256 thread sums in index order.  A NaN ratio never becomes M and makes both sums NaN.
__global__ __launch_bounds__(kRtThreads) void hns_rnn_ess_kernel(const float *ratio, long long B, int LA, double *col) {
    __shared__ double sm[2][kRtThreads];
    const int tid = threadIdx.x, c = blockIdx.x;
    double mx = -1.0;
    for (long long b = tid; b < B; b += kRtThreads) {
        const double x = (double)ratio[(long long)c * B + b];
        mx = x > mx ? x : mx;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double y = __shfl_xor(mx, o, 64);
        mx = y > mx ? y : mx;
    }
    if ((tid & 63) == 0) sm[0][tid >> 6] = mx;
    __syncthreads();
    mx = sm[0][0];
#pragma unroll
    for (int w = 1; w < kRtThreads / 64; ++w) mx = sm[0][w] > mx ? sm[0][w] : mx;
    __syncthreads();
    double e1 = 0.0, e2 = 0.0;
    for (long long b = tid; b < B; b += kRtThreads) {
        const double x = (double)ratio[(long long)c * B + b];
        if (x >= 0.0 || x != x) {                               // -1 marks a row that is left out
            const double ex = exp(x - mx);
            e1 += ex;
            e2 += ex * ex;
        }
    }
    sm[0][tid] = e1; sm[1][tid] = e2;
    __syncthreads();
    if (tid == 0) {
        double a1 = 0.0, a2 = 0.0;
        for (int i = 0; i < kRtThreads; ++i) { a1 += sm[0][i]; a2 += sm[1][i]; }
        col[c] = a1 * a1 / a2;                                  // exp(2 (M + log a1) - (2 M + log a2))
    }
}

__global__ __launch_bounds__(kRtThreads) void hns_rnn_actor_final_kernel(const double *part, int groups, const double *col, int LA, double n, double batch,
                                                                         double entropy_coef, const float *log_std, float *d_head_w, float *d_head_b,
                                                                         float *d_log_std, float *policy_loss, float *entropy, float *ess) {
    __shared__ double stage[kRtMaxGroups][kRtFinalElems];
    __shared__ double cols[HNS_GRU_MAX_STEPS * HNS_MAX_AGENTS];
    const int tid = threadIdx.x, e0 = blockIdx.x * kRtFinalElems;
    const bool last = e0 + kRtFinalElems >= kRtActorUsed;       // the block of the loss sum: it forms the three scalars
    if (last)
        for (int c = tid; c < LA; c += kRtThreads) cols[c] = col[c];
    const double s = rt_sum_partials(part, groups, kRtActorSlots, e0, kRtActorUsed, stage, tid);
    const int e = e0 + tid;
    if (tid >= kRtFinalElems || e >= kRtActorUsed) return;
    if (e < kRtAct * kRtE) d_head_w[e] = (float)s;
    else if (e < kRtAct * kRtE + kRtAct) d_head_b[e - kRtAct * kRtE] = (float)s;
    else if (e < kRtAct * kRtE + 2 * kRtAct) d_log_std[e - kRtAct * kRtE - kRtAct] = (float)(s - entropy_coef);   // the entropy term's constant gradient, once
    else {
        policy_loss[0] = (float)(-(double)kRtAct * s / n);
        double ent = 0.0;
        for (int i = 0; i < kRtAct; ++i) ent += 0.5 + 0.9189385332046727 + (double)log_std[i];
        entropy[0] = (float)ent;
        double es = 0.0;
        for (int c = 0; c < LA; ++c) es += cols[c];
        ess[0] = (float)(es / (double)LA / batch);
    }
}

// One head per agent: workgroup (x, agent) is the final kernel's block x on the agent's gpa partials and slice of the stacked gradients; every
// agent's d log_std takes -entropy_coef / A once (the entropy is the mean over the agents of each agent's).  The loss sum — the one element of
// the last block — adds ALL A gpa partials in workgroup order (agent-major), in agent 0's block, which forms the three scalars.
static_assert(kRtActorUsed - 1 == (kRtActorUsed - 1) / kRtFinalElems * kRtFinalElems, "the loss sum must be the only element of the last final block");
__global__ __launch_bounds__(kRtThreads) void hns_rnn_actor_final_agents_kernel(const double *part, int gpa, int A, const double *col, int LA, double n, double batch,
                                                                                double entropy_coef, const float *log_std, float *d_head_w, float *d_head_b,
                                                                                float *d_log_std, float *policy_loss, float *entropy, float *ess) {
    __shared__ double stage[kRtMaxGroups][kRtFinalElems];
    __shared__ double cols[HNS_GRU_MAX_STEPS * HNS_MAX_AGENTS];
    const int tid = threadIdx.x, e0 = blockIdx.x * kRtFinalElems, agent = blockIdx.y;
    const bool last = e0 + kRtFinalElems >= kRtActorUsed;
    if (last && agent > 0) return;
    if (last)
        for (int c = tid; c < LA; c += kRtThreads) cols[c] = col[c];
    const double s = last ? rt_sum_partials(part, A * gpa, kRtActorSlots, e0, kRtActorUsed, stage, tid)
                          : rt_sum_partials(part + (long long)agent * gpa * kRtActorSlots, gpa, kRtActorSlots, e0, kRtActorUsed, stage, tid);
    const int e = e0 + tid;
    if (tid >= kRtFinalElems || e >= kRtActorUsed) return;
    if (e < kRtAct * kRtE) d_head_w[agent * kRtAct * kRtE + e] = (float)s;
    else if (e < kRtAct * kRtE + kRtAct) d_head_b[agent * kRtAct + e - kRtAct * kRtE] = (float)s;
    else if (e < kRtAct * kRtE + 2 * kRtAct) d_log_std[agent * kRtAct + e - kRtAct * kRtE - kRtAct] = (float)(s - entropy_coef / (double)A);
    else {
        policy_loss[0] = (float)(-(double)kRtAct * s / n);
        double ent = 0.0;                                       // each agent's four terms in index order, the agents in index order
        for (int ag = 0; ag < A; ++ag) {
            double ea = 0.0;
            for (int i = 0; i < kRtAct; ++i) ea += 0.5 + 0.9189385332046727 + (double)log_std[ag * kRtAct + i];
            ent += ea;
        }
        entropy[0] = (float)(ent / (double)A);
        double es = 0.0;
        for (int c = 0; c < LA; ++c) es += cols[c];
        ess[0] = (float)(es / (double)LA / batch);
    }
}

struct RtCriticArgs {
    RtGeom G;
    const float *head_w, *head_b, *bval, *bret;
    float clip, delta, inv_n;
    int mse;
    float *values, *v;                                          // the caller's [B, L, A] or NULL; the workspace's copy
    const float *ctl;
    double *part;
};

HNS_DEV float rt_dloss(float x, float delta, int mse) {         // d loss / d x before the 1 / n of the mean
    if (mse) return 2.0f * x;
    return x <= -delta ? -delta : (x >= delta ? delta : x);
}

HNS_DEV double rt_loss64(double x, double delta, int mse) {
    if (mse) return x * x;
    const double ax = fabs(x);
    return ax < delta ? 0.5 * x * x : delta * (ax - 0.5 * delta);
}

__global__ __launch_bounds__(kRtThreads, 2) void hns_rnn_critic_values_kernel(const RtCriticArgs a) {
    __shared__ double reds[kRtRows][5];
    const int tid = threadIdx.x, r = tid >> 3, g = tid & 7;
    float w[16];
    rt_load(a.head_w, g, w);
    const float hb = a.head_b[0];
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const long long trips = (a.G.rows + kRtRows - 1) / kRtRows;
    for (long long trip = blockIdx.x; trip < trips; trip += gridDim.x) {
        const long long row = trip * kRtRows + r;
        const RtRow R = rt_row(a.G, row);
        float y[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) y[q] = 0.0f;
        if (R.live) rt_load(a.G.y + R.yoff, g, y);
        const float v = rt_dot(w, y) + hb;
        if (R.live) {
            const float ret = a.bret[R.idx], bv = a.bval[R.idx];
            const float clipped = bv + fminf(fmaxf(v - bv, -a.clip), a.clip);
            const double e0 = (double)v - (double)ret, e1 = (double)clipped - (double)ret;
            acc[0] += rt_loss64(e0, (double)a.delta, a.mse);
            acc[1] += rt_loss64(e1, (double)a.delta, a.mse);
            acc[2] += e0 * e0;
            acc[3] += (double)ret;
            acc[4] += (double)ret * (double)ret;
        }
        if (R.in && g == 0) {
            a.v[row] = v;
            if (R.live && a.values) a.values[row] = v;
        }
    }
    if (g == 0) {
#pragma unroll
        for (int q = 0; q < 5; ++q) reds[r][q] = acc[q];
    }
    __syncthreads();
    if (tid < 5) {
        double s = 0.0;
        for (int rr = 0; rr < kRtRows; ++rr) s += reds[rr][tid];
        a.part[(long long)blockIdx.x * kRtSumSlots + tid] = s;
    }
}

// ct_loss_decide's rule on the five sums S over n rows: the branch weights, value_loss, explained_var (one thread)
HNS_DEV void rt_decide(const double *S, double n, float *ctl, float *value_loss, float *explained_var) {
    const double lo = S[0] / n, lc = S[1] / n;
    ctl[0] = lo > lc ? 1.0f : (lo < lc ? 0.0f : 0.5f);
    ctl[1] = lo > lc ? 0.0f : (lo < lc ? 1.0f : 0.5f);
    value_loss[0] = (float)(lo > lc ? lo : lc);
    const double var = (S[4] - S[3] * S[3] / n) / (n - 1.0);                 // unbiased, as Tensor.var()
    explained_var[0] = (float)(1.0 - (S[2] / n) / var);
}

// value_loss, explained_var and the branch weights of max(mean loss(v), mean loss(clipped)): ct_loss_decide's rule on the five sums over n rows
__global__ __launch_bounds__(kRtThreads) void hns_rnn_critic_decide_kernel(const double *part, int groups, double n, float *ctl, float *value_loss,
                                                                           float *explained_var) {
    __shared__ double stage[kRtMaxGroups][kRtFinalElems];
    __shared__ double S[kRtFinalElems];
    const double s = rt_sum_partials(part, groups, kRtSumSlots, 0, 5, stage, threadIdx.x);
    if (threadIdx.x < kRtFinalElems) S[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) rt_decide(S, n, ctl, value_loss, explained_var);
}

// the forward-only entry's second launch: the G partials of each of the five sums, added in the decide kernel's order, as they are (fp64)
__global__ __launch_bounds__(kRtThreads) void hns_rnn_critic_sums_kernel(const double *part, int groups, double *sums) {
    __shared__ double stage[kRtMaxGroups][kRtFinalElems];
    const double s = rt_sum_partials(part, groups, kRtSumSlots, 0, 5, stage, threadIdx.x);
    if (threadIdx.x < 5) sums[threadIdx.x] = s;
}

// the global entry's decision: the rule on the union's sums and its row count, given by the caller
__global__ void hns_rnn_critic_decide_global_kernel(const double *sums, double n, float *ctl, float *value_loss, float *explained_var) {
    if (threadIdx.x == 0) {
        double S[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) S[q] = sums[q];
        rt_decide(S, n, ctl, value_loss, explained_var);
    }
}

__global__ __launch_bounds__(kRtThreads, 2) void hns_rnn_critic_grad_kernel(const RtCriticArgs a) {
    __shared__ __align__(16) float red[kRtRows][kRtE];
    __shared__ double reds[kRtRows];
    const int tid = threadIdx.x, r = tid >> 3, g = tid & 7;
    float w[16], aw[16], ab = 0.0f;
    rt_load(a.head_w, g, w);
#pragma unroll
    for (int q = 0; q < 16; ++q) aw[q] = 0.0f;
    const float c0 = a.ctl[0], c1 = a.ctl[1];
    const long long trips = (a.G.rows + kRtRows - 1) / kRtRows;
    for (long long trip = blockIdx.x; trip < trips; trip += gridDim.x) {
        const long long row = trip * kRtRows + r;
        const RtRow R = rt_row(a.G, row);
        float y[16], dy[16], dv = 0.0f;
#pragma unroll
        for (int q = 0; q < 16; ++q) y[q] = 0.0f;
        if (R.live) {
            rt_load(a.G.y + R.yoff, g, y);
            const float v = a.v[row], ret = a.bret[R.idx], bv = a.bval[R.idx];
            const float d = v - bv;
            const float clipped = bv + fminf(fmaxf(d, -a.clip), a.clip);
            const float g0 = rt_dloss(v - ret, a.delta, a.mse);
            const float g1 = (d >= -a.clip && d <= a.clip) ? rt_dloss(clipped - ret, a.delta, a.mse) : 0.0f;   // clamp's backward: inside, bounds included
            dv = (c0 * g0 + c1 * g1) * a.inv_n;
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            dy[q] = dv * w[q];
            aw[q] += dv * y[q];                                 // d v_out.weight
        }
        ab += dv;
        if (R.in) rt_store(a.G.dy + R.yoff, g, dy);
    }
    double *part = a.part + (long long)blockIdx.x * kRtCriticSlots;
    rt_flush(red, aw, part, tid, r, g);
    if (g == 0) reds[r] = (double)ab;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int rr = 0; rr < kRtRows; ++rr) s += reds[rr];
        part[kRtE] = s;
    }
}

__global__ __launch_bounds__(kRtThreads) void hns_rnn_critic_final_kernel(const double *part, int groups, float *d_head_w, float *d_head_b) {
    __shared__ double stage[kRtMaxGroups][kRtFinalElems];
    const int e0 = blockIdx.x * kRtFinalElems;
    const double s = rt_sum_partials(part, groups, kRtCriticSlots, e0, kRtCriticUsed, stage, threadIdx.x);
    const int e = e0 + threadIdx.x;
    if (threadIdx.x >= kRtFinalElems || e >= kRtCriticUsed) return;
    if (e < kRtE) d_head_w[e] = (float)s;
    else d_head_b[0] = (float)s;
}

inline size_t rt_up(size_t x) { return (x + 255) & ~(size_t)255; }

inline bool rt_shape_ok(int64_t outer, int32_t inner, int32_t steps) {
    return outer >= 1 && inner >= 1 && inner <= HNS_MAX_AGENTS && steps >= 1 && steps <= HNS_GRU_MAX_STEPS && outer < ((int64_t)1 << 40) / (HNS_GRU_MAX_STEPS * 8);
}

inline int rt_groups(long long rows) {
    const long long t = (rows + kRtRows - 1) / kRtRows;
    return (int)(t > kRtMaxGroups ? kRtMaxGroups : t);
}

// the workspace's sections, each 256-byte aligned.  Actor: partials [G][528] fp64, ratios [L A][B] fp32, columns [L A] fp64.
// Critic: sum partials [G][8] fp64, gradient partials [G][136] fp64, the branch weights (2 fp32), v [rows] fp32.
struct RtActorWs { size_t part, ratio, col, bytes; };
struct RtCriticWs { size_t sums, part, ctl, v, bytes; };

inline RtActorWs rt_actor_ws(long long rows, int LA) {
    RtActorWs w;
    const size_t G = (size_t)rt_groups(rows);
    w.part = 0;
    w.ratio = w.part + rt_up(G * kRtActorSlots * sizeof(double));
    w.col = w.ratio + rt_up((size_t)rows * sizeof(float));
    w.bytes = w.col + rt_up((size_t)LA * sizeof(double));
    return w;
}

// one head per agent: sweep workgroups per agent, min(trips of an agent's B L positions, floor(512 / A)) — a function of the shape alone
inline int rt_groups_per_agent(long long rows, int A) {
    const long long t = (rows / A + kRtRows - 1) / kRtRows;
    return (int)(t > kRtMaxGroups / A ? kRtMaxGroups / A : t);
}

inline RtActorWs rt_actor_agents_ws(long long rows, int A, int LA) {
    RtActorWs w;
    const size_t G = (size_t)A * rt_groups_per_agent(rows, A);
    w.part = 0;
    w.ratio = w.part + rt_up(G * kRtActorSlots * sizeof(double));
    w.col = w.ratio + rt_up((size_t)rows * sizeof(float));
    w.bytes = w.col + rt_up((size_t)LA * sizeof(double));
    return w;
}

inline RtCriticWs rt_critic_ws(long long rows) {
    RtCriticWs w;
    const size_t G = (size_t)rt_groups(rows);
    w.sums = 0;
    w.part = w.sums + rt_up(G * kRtSumSlots * sizeof(double));
    w.ctl = w.part + rt_up(G * kRtCriticSlots * sizeof(double));
    w.v = w.ctl + 256;
    w.bytes = w.v + rt_up((size_t)rows * sizeof(float));
    return w;
}

// the refusals every entry shares, in the header's order; fills the kernels' geometry.  `needs_dy` false: the forward-only entry, which has no dy
inline int rt_check_rows(const char *fn, const hns_rnn_rows *rows, float *dy, RtGeom &G, bool needs_dy = true) {
    if (!rows) return hns_fail(fn, "null pointer (rows)");
    if (rows->inner < 1 || rows->inner > HNS_MAX_AGENTS || !rt_shape_ok(rows->outer, (int32_t)rows->inner, rows->steps))
        return hns_fail(fn, "outer must be >= 1 (and < 2^31), inner in [1, 7], steps in [1, HNS_GRU_MAX_STEPS]");
    if (!rows->y || (needs_dy && !dy)) return hns_fail(fn, "null pointer (y, dy)");
    if (!hns_aligned(rows->y, 16) || !hns_aligned(dy, 16)) return hns_fail(fn, "misaligned pointer: y and dy are read and written by float4 (16-byte aligned)");
    for (int d = 0; d < 3; ++d)
        if (rows->y_stride[d] < 0 || rows->y_stride[d] % 4) return hns_fail(fn, "y strides must be >= 0 and multiples of 4 floats");
    if (rows->segment && !hns_aligned(rows->segment, 8)) return hns_fail(fn, "misaligned pointer: segment holds int64 ids");
    if (rows->num_segments < 0) return hns_fail(fn, "num_segments must be >= 0");
    G.y = rows->y; G.dy = dy;
    G.s0 = rows->y_stride[0]; G.s1 = rows->y_stride[1]; G.s2 = rows->y_stride[2];
    G.A = (int)rows->inner; G.L = rows->steps; G.LA = G.A * G.L;
    G.rows = (long long)rows->outer * G.LA;
    G.nseg = rows->num_segments;
    G.segment = reinterpret_cast<const long long *>(rows->segment);
    return HNS_OK;
}

}  // namespace hns

namespace hns {

// the local and the global actor entry: n_rows is the row count every mean divides by (the call's own B L A, or the union's), share the part of
// the entropy term's constant gradient this call adds
static int rt_actor_entry(const char *fn, const float *head_w, const float *head_b, const float *log_std, const hns_rnn_rows *rows, const float *action,
                          const float *log_probs_old, const float *advantages, double clip_param, double entropy_coef, float *dy, float *d_head_w,
                          float *d_head_b, float *d_log_std, float *policy_loss, float *entropy, float *ess, float *log_probs, void *workspace,
                          size_t workspace_bytes, void *stream, bool global, int64_t global_rows, double entropy_share, bool agents = false) {
    RtActorArgs a;
    if (int rc = rt_check_rows(fn, rows, dy, a.G)) return rc;
    if (!head_w || !head_b || !log_std || !action || !log_probs_old || !advantages || !d_head_w || !d_head_b || !d_log_std || !policy_loss || !entropy ||
        !ess || !workspace)
        return hns_fail(fn, "null pointer");
    if (!hns_aligned(head_w, 16) || !hns_aligned(head_b, 16) || !hns_aligned(log_std, 16))
        return hns_fail(fn, "misaligned pointer: the head's tensors are 16-byte aligned");
    if (!hns_aligned(action, 4) || !hns_aligned(log_probs_old, 4) || !hns_aligned(advantages, 4) || !hns_aligned(d_head_w, 4) || !hns_aligned(d_head_b, 4) ||
        !hns_aligned(d_log_std, 4) || !hns_aligned(policy_loss, 4) || !hns_aligned(entropy, 4) || !hns_aligned(ess, 4) || !hns_aligned(log_probs, 4))
        return hns_fail(fn, "misaligned pointer: fp32 arrays and scalars are 4-byte aligned");
    if (!(clip_param >= 0.0) || entropy_coef != entropy_coef) return hns_fail(fn, "clip_param must be >= 0 and entropy_coef a number");
    if (global && global_rows < (int64_t)a.G.rows) return hns_fail(fn, "global_rows must be >= the call's own B L A rows");
    if (global && !(entropy_share - entropy_share == 0.0)) return hns_fail(fn, "entropy_share must be finite");
    const RtActorWs W = agents ? rt_actor_agents_ws(a.G.rows, a.G.A, a.G.LA) : rt_actor_ws(a.G.rows, a.G.LA);
    if (!hns_aligned(workspace, 256)) return hns_fail(fn, "misaligned pointer: the workspace is 256-byte aligned");
    if (workspace_bytes < W.bytes)
        return hns_fail(fn, agents ? "workspace shorter than hns_rnn_actor_head_agents_workspace_bytes" : "workspace shorter than hns_rnn_actor_head_workspace_bytes");
    char *ws = static_cast<char *>(workspace);
    const double n = global ? (double)global_rows : (double)a.G.rows;
    a.head_w = head_w; a.head_b = head_b; a.log_std = log_std;
    a.action = action; a.logp_old = log_probs_old; a.adv = advantages;
    a.clip_lo = (float)(1.0 - clip_param); a.clip_hi = (float)(1.0 + clip_param);
    a.inv_n = (float)(1.0 / n);
    a.logp_new = log_probs;
    a.B = rows->outer;
    a.part = reinterpret_cast<double *>(ws + W.part);
    a.ratio = reinterpret_cast<float *>(ws + W.ratio);
    double *col = reinterpret_cast<double *>(ws + W.col);
    const int groups = rt_groups(a.G.rows), gpa = rt_groups_per_agent(a.G.rows, a.G.A);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (agents) hipLaunchKernelGGL(hns_rnn_actor_rows_agents_kernel, dim3(a.G.A * gpa), dim3(kRtThreads), 0, st, a, gpa);
    else hipLaunchKernelGGL(hns_rnn_actor_rows_kernel, dim3(groups), dim3(kRtThreads), 0, st, a);
    HNS_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(hns_rnn_ess_kernel, dim3(a.G.LA), dim3(kRtThreads), 0, st, static_cast<const float *>(a.ratio), (long long)rows->outer, a.G.LA, col);
    HNS_CHECK_HIP(hipGetLastError());
    if (agents) {
        hipLaunchKernelGGL(hns_rnn_actor_final_agents_kernel, dim3((kRtActorUsed + kRtFinalElems - 1) / kRtFinalElems, a.G.A), dim3(kRtThreads), 0, st,
                           static_cast<const double *>(a.part), gpa, a.G.A, static_cast<const double *>(col), a.G.LA, n, (double)rows->outer,
                           global ? entropy_coef * entropy_share : entropy_coef,    // the kernel divides by A: (entropy_coef entropy_share) / A
                           log_std, d_head_w, d_head_b, d_log_std, policy_loss, entropy, ess);
        HNS_CHECK_HIP(hipGetLastError());
        return HNS_OK;
    }
    hipLaunchKernelGGL(hns_rnn_actor_final_kernel, dim3((kRtActorUsed + kRtFinalElems - 1) / kRtFinalElems), dim3(kRtThreads), 0, st,
                       static_cast<const double *>(a.part), groups, static_cast<const double *>(col), a.G.LA, n, (double)rows->outer,
                       global ? entropy_coef * entropy_share : entropy_coef, log_std, d_head_w, d_head_b, d_log_std, policy_loss, entropy, ess);
    HNS_CHECK_HIP(hipGetLastError());
    return HNS_OK;
}

enum RtCriticMode { kRtLocal, kRtSums, kRtGlobal };

// the three critic entries.  kRtLocal: values, the decision on the call's own sums, dy and the head's gradients.  kRtSums: values and the five
// sums, nothing else.  kRtGlobal: v again (into this call's workspace), the decision on the caller's sums over global_rows, dy and the gradients.
static int rt_critic_entry(const char *fn, RtCriticMode mode, const float *head_w, const float *head_b, const hns_rnn_rows *rows, const float *b_values,
                           const float *b_returns, float clip_param, int32_t loss_kind, float huber_delta, float *dy, float *d_head_w, float *d_head_b,
                           float *value_loss, float *explained_var, float *values, double *sums_out, const double *sums_in, int64_t global_rows,
                           void *workspace, size_t workspace_bytes, void *stream) {
    RtCriticArgs a;
    const bool grad = mode != kRtSums;
    if (int rc = rt_check_rows(fn, rows, dy, a.G, grad)) return rc;
    if (!head_w || !head_b || !b_values || !b_returns || !workspace) return hns_fail(fn, "null pointer");
    if (grad && (!d_head_w || !d_head_b || !value_loss || !explained_var)) return hns_fail(fn, "null pointer");
    if (!hns_aligned(head_w, 16) || !hns_aligned(head_b, 16)) return hns_fail(fn, "misaligned pointer: the head's tensors are 16-byte aligned");
    if (!hns_aligned(b_values, 4) || !hns_aligned(b_returns, 4) || !hns_aligned(d_head_w, 4) || !hns_aligned(d_head_b, 4) || !hns_aligned(value_loss, 4) ||
        !hns_aligned(explained_var, 4) || !hns_aligned(values, 4))
        return hns_fail(fn, "misaligned pointer: fp32 arrays and scalars are 4-byte aligned");
    if (loss_kind != HNS_CRITIC_LOSS_HUBER && loss_kind != HNS_CRITIC_LOSS_MSE) return hns_fail(fn, "loss_kind must be HNS_CRITIC_LOSS_HUBER or HNS_CRITIC_LOSS_MSE");
    if (!(clip_param >= 0.0f) || (loss_kind == HNS_CRITIC_LOSS_HUBER && !(huber_delta > 0.0f))) return hns_fail(fn, "clip_param must be >= 0 and huber_delta > 0");
    if (mode == kRtSums && (!sums_out || !hns_aligned(sums_out, 8))) return hns_fail(fn, "sums must be five fp64 device values, 8-byte aligned");
    if (mode == kRtGlobal && (!sums_in || !hns_aligned(sums_in, 8))) return hns_fail(fn, "sums must be five fp64 device values, 8-byte aligned");
    if (mode == kRtGlobal && global_rows < (int64_t)a.G.rows) return hns_fail(fn, "global_rows must be >= the call's own B L A rows");
    const RtCriticWs W = rt_critic_ws(a.G.rows);
    if (!hns_aligned(workspace, 256)) return hns_fail(fn, "misaligned pointer: the workspace is 256-byte aligned");
    if (workspace_bytes < W.bytes) return hns_fail(fn, "workspace shorter than hns_rnn_critic_head_workspace_bytes");
    char *ws = static_cast<char *>(workspace);
    const double n = mode == kRtGlobal ? (double)global_rows : (double)a.G.rows;
    a.head_w = head_w; a.head_b = head_b; a.bval = b_values; a.bret = b_returns;
    a.clip = clip_param; a.delta = huber_delta; a.mse = loss_kind == HNS_CRITIC_LOSS_MSE;
    a.inv_n = (float)(1.0 / n);
    a.values = mode == kRtGlobal ? nullptr : values;            // the global entry leaves them to hns_rnn_critic_head_sums
    a.v = reinterpret_cast<float *>(ws + W.v);
    float *ctl = reinterpret_cast<float *>(ws + W.ctl);
    a.ctl = ctl;
    double *sums = reinterpret_cast<double *>(ws + W.sums);
    const int groups = rt_groups(a.G.rows);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    a.part = sums;
    hipLaunchKernelGGL(hns_rnn_critic_values_kernel, dim3(groups), dim3(kRtThreads), 0, st, a);
    HNS_CHECK_HIP(hipGetLastError());
    if (mode == kRtSums) {
        hipLaunchKernelGGL(hns_rnn_critic_sums_kernel, dim3(1), dim3(kRtThreads), 0, st, static_cast<const double *>(sums), groups, sums_out);
        HNS_CHECK_HIP(hipGetLastError());
        return HNS_OK;
    }
    if (mode == kRtGlobal)
        hipLaunchKernelGGL(hns_rnn_critic_decide_global_kernel, dim3(1), dim3(64), 0, st, sums_in, n, ctl, value_loss, explained_var);
    else
        hipLaunchKernelGGL(hns_rnn_critic_decide_kernel, dim3(1), dim3(kRtThreads), 0, st, static_cast<const double *>(sums), groups, n, ctl, value_loss,
                           explained_var);
    HNS_CHECK_HIP(hipGetLastError());
    a.part = reinterpret_cast<double *>(ws + W.part);
    hipLaunchKernelGGL(hns_rnn_critic_grad_kernel, dim3(groups), dim3(kRtThreads), 0, st, a);
    HNS_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(hns_rnn_critic_final_kernel, dim3((kRtCriticUsed + kRtFinalElems - 1) / kRtFinalElems), dim3(kRtThreads), 0, st,
                       static_cast<const double *>(a.part), groups, d_head_w, d_head_b);
    HNS_CHECK_HIP(hipGetLastError());
    return HNS_OK;
}

}  // namespace hns

extern "C" {

size_t hns_rnn_actor_head_workspace_bytes(int64_t outer, int32_t inner, int32_t steps) {
    if (!hns::rt_shape_ok(outer, inner, steps)) return 0;
    return hns::rt_actor_ws((long long)outer * inner * steps, inner * steps).bytes;
}

size_t hns_rnn_critic_head_workspace_bytes(int64_t outer, int32_t inner, int32_t steps) {
    if (!hns::rt_shape_ok(outer, inner, steps)) return 0;
    return hns::rt_critic_ws((long long)outer * inner * steps).bytes;
}

int hns_rnn_actor_head_grad(const float *head_w, const float *head_b, const float *log_std, const hns_rnn_rows *rows, const float *action,
                            const float *log_probs_old, const float *advantages, double clip_param, double entropy_coef, float *dy, float *d_head_w,
                            float *d_head_b, float *d_log_std, float *policy_loss, float *entropy, float *ess, float *log_probs, void *workspace,
                            size_t workspace_bytes, void *stream) {
    return hns::rt_actor_entry("hns_rnn_actor_head_grad", head_w, head_b, log_std, rows, action, log_probs_old, advantages, clip_param, entropy_coef, dy,
                               d_head_w, d_head_b, d_log_std, policy_loss, entropy, ess, log_probs, workspace, workspace_bytes, stream, false, 0, 1.0);
}

size_t hns_rnn_actor_head_agents_workspace_bytes(int64_t outer, int32_t inner, int32_t steps) {
    if (!hns::rt_shape_ok(outer, inner, steps)) return 0;
    return hns::rt_actor_agents_ws((long long)outer * inner * steps, inner, inner * steps).bytes;
}

int hns_rnn_actor_head_grad_agents(const float *head_w, const float *head_b, const float *log_std, const hns_rnn_rows *rows, const float *action,
                                   const float *log_probs_old, const float *advantages, double clip_param, double entropy_coef, float *dy,
                                   float *d_head_w, float *d_head_b, float *d_log_std, float *policy_loss, float *entropy, float *ess, float *log_probs,
                                   void *workspace, size_t workspace_bytes, void *stream) {
    return hns::rt_actor_entry("hns_rnn_actor_head_grad_agents", head_w, head_b, log_std, rows, action, log_probs_old, advantages, clip_param,
                               entropy_coef, dy, d_head_w, d_head_b, d_log_std, policy_loss, entropy, ess, log_probs, workspace, workspace_bytes, stream,
                               false, 0, 1.0, true);
}

int hns_rnn_actor_head_grad_global(const float *head_w, const float *head_b, const float *log_std, const hns_rnn_rows *rows, const float *action,
                                   const float *log_probs_old, const float *advantages, double clip_param, double entropy_coef, float *dy,
                                   float *d_head_w, float *d_head_b, float *d_log_std, float *policy_loss, float *entropy, float *ess, float *log_probs,
                                   void *workspace, size_t workspace_bytes, void *stream, int64_t global_rows, double entropy_share) {
    return hns::rt_actor_entry("hns_rnn_actor_head_grad_global", head_w, head_b, log_std, rows, action, log_probs_old, advantages, clip_param,
                               entropy_coef, dy, d_head_w, d_head_b, d_log_std, policy_loss, entropy, ess, log_probs, workspace, workspace_bytes, stream,
                               true, global_rows, entropy_share);
}

int hns_rnn_actor_head_grad_agents_global(const float *head_w, const float *head_b, const float *log_std, const hns_rnn_rows *rows, const float *action,
                                          const float *log_probs_old, const float *advantages, double clip_param, double entropy_coef, float *dy,
                                          float *d_head_w, float *d_head_b, float *d_log_std, float *policy_loss, float *entropy, float *ess,
                                          float *log_probs, void *workspace, size_t workspace_bytes, void *stream, int64_t global_rows,
                                          double entropy_share) {
    return hns::rt_actor_entry("hns_rnn_actor_head_grad_agents_global", head_w, head_b, log_std, rows, action, log_probs_old, advantages, clip_param,
                               entropy_coef, dy, d_head_w, d_head_b, d_log_std, policy_loss, entropy, ess, log_probs, workspace, workspace_bytes, stream,
                               true, global_rows, entropy_share, true);
}

int hns_rnn_critic_head_grad(const float *head_w, const float *head_b, const hns_rnn_rows *rows, const float *b_values, const float *b_returns,
                             float clip_param, int32_t loss_kind, float huber_delta, float *dy, float *d_head_w, float *d_head_b, float *value_loss,
                             float *explained_var, float *values, void *workspace, size_t workspace_bytes, void *stream) {
    return hns::rt_critic_entry("hns_rnn_critic_head_grad", hns::kRtLocal, head_w, head_b, rows, b_values, b_returns, clip_param, loss_kind, huber_delta,
                                dy, d_head_w, d_head_b, value_loss, explained_var, values, nullptr, nullptr, 0, workspace, workspace_bytes, stream);
}

int hns_rnn_critic_head_sums(const float *head_w, const float *head_b, const hns_rnn_rows *rows, const float *b_values, const float *b_returns,
                             float clip_param, int32_t loss_kind, float huber_delta, double *sums, float *values, void *workspace, size_t workspace_bytes,
                             void *stream) {
    return hns::rt_critic_entry("hns_rnn_critic_head_sums", hns::kRtSums, head_w, head_b, rows, b_values, b_returns, clip_param, loss_kind, huber_delta,
                                nullptr, nullptr, nullptr, nullptr, nullptr, values, sums, nullptr, 0, workspace, workspace_bytes, stream);
}

int hns_rnn_critic_head_grad_global(const float *head_w, const float *head_b, const hns_rnn_rows *rows, const float *b_values, const float *b_returns,
                                    float clip_param, int32_t loss_kind, float huber_delta, float *dy, float *d_head_w, float *d_head_b,
                                    float *value_loss, float *explained_var, float *values, void *workspace, size_t workspace_bytes, void *stream,
                                    const double *sums, int64_t global_rows) {
    return hns::rt_critic_entry("hns_rnn_critic_head_grad_global", hns::kRtGlobal, head_w, head_b, rows, b_values, b_returns, clip_param, loss_kind,
                                huber_delta, dy, d_head_w, d_head_b, value_loss, explained_var, values, nullptr, sums, global_rows, workspace,
                                workspace_bytes, stream);
}

}  // extern "C"
