// hns_policy_train.hip — the MAPPO critic's and actor's updates on the device: value loss / PPO surrogate, backward pass of the
// PartialAttentionEncoder, total gradient norm.
//
// Reference: MAPPOPolicy.update_critic (omni_drones/learning/mappo.py:326-352) on make_critic's network at cfg/algo/mappo.yaml's defaults
// (critic_input obs, no rnn): values = v_out(encoder(obs)); clipped = b_values + clamp(values - b_values, +-clip); value_loss = max(mean loss(ret,
// clipped), mean loss(ret, values)) with nn.HuberLoss(delta) or nn.MSELoss; backward; clip_grad_norm_; torch.optim.Adam.  DESIGN.md §7.4.
//
// The network is the one of hns_policy.hip (single-query algebra): per row six 128 x 128 products forward (W_q, W_k^T, W_v, W_o, W_1,
// W_2) and six against the transposes backward, on v_mfma_f32_16x16x4_f32 for 32 rows at a time, and two token passes on the VALU.  The forward
// pass' pieces (tile shape, matrix-vector product, LayerNorm, token embedding, online-softmax step, parameter table, fragment order) are
// hns_encoder.h's, shared with hns_policy.hip; from the loss onwards everything is here.
//   hns_critic_pack_kernel   : the six matrices in both orientations in MFMA A-operand fragment order, the embedding weights transposed.
//   hns_critic_kernel<false> : forward of the minibatch rows: values, per-tile fp64 partials of sum loss(v), sum loss(clipped), sum (v - ret)^2,
//                              sum ret, sum ret^2.
//   hns_critic_loss_kernel   : one workgroup sums the partials in a fixed order: value_loss, explained_var and the branch weights of the max
//                              ((1, 0), (0, 1), or (1/2, 1/2) at an exact tie, as torch.maximum's backward).  Its two halves alone are
//                              hns_critic_sums_kernel (the five sums) and hns_critic_decide_kernel (the scalars and weights from given sums):
//                              the data-parallel entries' (DESIGN §7.9), which add the ranks' sums between them.
//   hns_critic_kernel<true>  : recomputes a tile's forward pass, forms dv from the branch weights and walks back to the embeddings.  The operand
//                              pairs (dy, x) of the six weight gradients are staged in the workspace ([rows, 128] each); LayerNorm, head and
//                              embedding gradients leave as two partial rows per tile (rows 0-15 and 16-31).
//   hns_critic_wgrad_kernel  : dW = sum_rows dy (x) x, split over row ranges: per (split, matrix) a 128 x 128 partial and the bias partial
//                              (column sums of dy).
//   hns_critic_reduce_kernel : every gradient value = the fp64 sum of its partials in index order, written in the PyTorch layout; per-block sums
//                              of squares;  hns_critic_norm_kernel adds those in order: the total gradient norm.
// The clip and the Adam step that follow are hns_adam.hip's.
// The actor (MAPPOPolicy.update_actor, mappo.py:271-324; DiagGaussian head fc_mean 128 -> 4 and a free log_std[4]) is the same
// encoder with a four-output head, selected by the tile kernel's HEAD template parameter.  The clipped surrogate's backward weight is per row, so
// ONE pass over the tiles gives the loss partials and the gradients:
//   hns_critic_kernel<true, 4> : forward, log-probability, ratio, surrogate and its d mu per row, then the encoder's backward pass as above; per
//                                tile the fp64 partials of sum min(surr1, surr2) and, per agent, (max, sum exp(r - max), sum exp(2 (r - max)))
//                                of the ratios; head_w [4][128], head_b [4] and log_std [4] leave in the tile's partial rows.
//   hns_actor_loss_kernel      : one workgroup adds the partials in a fixed order: policy_loss, entropy, ESS.
//   pack, wgrad, reduce (which adds -entropy_coef to d log_std, once) and norm kernels: the critic's.
// The encoder alone as a differentiable op (hns_encoder_forward / hns_encoder_backward; hns_amd.encoder) is the tile kernel
// with HEAD = 0 — no head, no loss:
//   hns_critic_kernel<false, 0> : forward up to y = LN2(x0' + ff); y leaves as fp32 [rows, 128], row = minibatch position x A + agent.
//   hns_critic_kernel<true, 0>  : recomputes the tile's forward pass, reads the row's dy from a [rows, 128] array (as given: no 1 / n) and runs the
//                                 backward pass above; a tile's partial rows carry no head entries.
//   wgrad as above; hns_encoder_reduce_kernel is the reduce kernel's body without the head's destinations; no norm launch.
// One actor per agent (share_actor: false: update_actor's else branch, mappo.py:288-291; hns_actor_train_grad_agents) is the actor's
// pipeline for all agents together on the STACKED tensors:
//   hns_actor_pack_agents_kernel   : A operand images, one per agent's slice.
//   hns_actor_agents_kernel        : the one-pass tile kernel's body (hns_policy_train_bodies.inc, shared as text with hns_critic_kernel) on tiles of
//                                    32 minibatch positions of ONE agent, numbered agent-major; the agent's image and slice formed once per tile.
//   hns_actor_loss_agents_kernel   : the scalars; entropy is the mean over the agents.
//   hns_critic_wgrad_kernel        : unchanged — an agent's tiles are padded to whole row ranges, so no range straddles two agents.
//   hns_actor_reduce_agents_kernel : each agent's partials into its slice of the stacked gradients (-entropy_coef / A on its d log_std);
//                                    hns_critic_norm_kernel: ONE norm over all agents' per-block sums.
// The encoder op on the stacked tensors (hns_encoder_forward_agents / hns_encoder_backward_agents; DESIGN.md §7.18: the encoder of one recurrent
// actor per agent) is the two above combined — HEAD = 0 on the per-agent tiles:
//   hns_actor_pack_agents_kernel       : as above.
//   hns_encoder_agents_kernel<BWD>     : the tile body with HEAD = 0 on hns_actor_agents_kernel's tiles; features and d features keep the shared
//                                        op's [rows, 128] layout, row = position x A + agent.
//   hns_critic_wgrad_kernel            : unchanged, on the padded agent-major tiles.
//   hns_encoder_reduce_agents_kernel   : each agent's partials into its slice of the 20 stacked encoder tensors; no norm launch.
// The centralised critic (critic_input: state; hns_critic_train_grad_central) is the critic's pipeline on tiles of 32 env-steps:
//   hns_critic_central_kernel<BWD>   : the tile body under CT_CENTRAL — a row's tokens are the A state_drones rows through ONE embedding, then the
//                                      cylinders; A values, loss terms and value gradients per row; d embed_self summed over all A drone tokens.
//   hns_critic_reduce_central_kernel : the reduce kernel's body with the central partial row's destinations (head_w [A][128], head_b [A]).
//   pack, loss, wgrad and norm kernels: the critic's, unchanged.
// Determinism: every sum has a fixed order, no float atomics: the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <string>

#include "hns_device.h"
#include "hns_encoder.h"
#include "hns_host.h"
#include "../../include/hns.h"

namespace hns {

// hns_encoder.h's tile under this file's names (the backward pass, the wgrad kernel and the host section use them throughout)
constexpr int kCtE = kEncE, kCtRows = kEncRows, kCtLd = kEncLd, kCtThreads = kEncThreads, kCtMat = kEncMat;
constexpr int kCtRedLd = kCtE + 4;           // LDS pitch of the [row][feature] images the cross-row sums read
constexpr int kCtMaxSplits = 48;             // row ranges of the weight-gradient kernel
constexpr int kCtGemmLd = kCtE + 16;         // LDS pitch of the staged operand tiles: the four k rows of an operand read fall in distinct banks
constexpr int kCtGemmOut = kCtMat + kCtE;    // a weight-gradient partial: dW, then the bias partial
constexpr int kCtMaxBlocks = 4096;           // upper bound of the reduce kernel's grid (its per-block sums of squares)
constexpr int kCtMaxSelf = HNS_POLICY_MAX_SELF_DIM;

// image: 12 matrices in fragment order — forward Q, K^T, V, O, L1, L2, then their transposes — and the embedding weights transposed
constexpr int I_EW = 12 * kCtMat;
static __host__ __device__ __forceinline__ long long ct_img_floats(int D) { return I_EW + (long long)(D + 8) * kCtE; }

// a tile's partial row (two per tile: rows 0-15 and 16-31)
enum : int {
    O_LNW = 0, O_LNB = 128, O_N1W = 256, O_N1B = 384, O_N2W = 512, O_N2B = 640, O_HW = 768, O_EBS = 896, O_EBO = 1024, O_EBC = 1152,
    O_EWO = 1280,                            // [3][128]
    O_EWC = O_EWO + 3 * kCtE,                // [5][128]
    O_HB = O_EWC + 5 * kCtE,                 // 1 value (+ 3 of padding)
    O_EWS = O_HB + 4,                        // [D][128]
};
// the actor's head (heads = 4): head_b's four values at O_HB, head_w row 0 at O_HW, and behind the state_self embedding rows 1-3 of head_w
// [3][128] and log_std [4]; the critic's layout (heads = 1) ends at the embedding
constexpr int kActDim = 4;                   // DiagGaussian's action dimension (fc_mean's rows)
constexpr int kActLossSlots = 1 + 3 * HNS_MAX_AGENTS;   // a tile's fp64 partials: sum of the surrogate, then (max, s1, s2) of the ratios per agent
// (heads = 0, the encoder op: the critic's layout, its O_HW and O_HB slots never written and never read)
static __host__ __device__ constexpr int ct_partial_floats(int D, int heads = 1) { return O_EWS + D * kCtE + (heads > 1 ? (heads - 1) * kCtE + heads : 0); }
static_assert((6 * kCtGemmOut + 31) / 32 + (ct_partial_floats(kCtMaxSelf, kActDim) + 31) / 32 <= kCtMaxBlocks, "the reduce kernel's grid outgrew its per-block sums");
// the centralised critic's head (v_out = Linear(128, A), A <= 7): head_w row 0 at O_HW, rows 1 .. 6 behind the state_drones
// embedding as the actor's, then head_b's up to seven values (+ 1 of padding); O_EBO, O_EWO and O_HB are never written and never read
static __host__ __device__ constexpr int ct_central_hb(int D) { return O_EWS + D * kCtE + (HNS_MAX_AGENTS - 1) * kCtE; }
static __host__ __device__ constexpr int ct_partial_central(int D) { return ct_central_hb(D) + 8; }
static_assert((6 * kCtGemmOut + 31) / 32 + (ct_partial_central(kCtMaxSelf) + 31) / 32 <= kCtMaxBlocks, "the reduce kernel's grid outgrew its per-block sums");

struct CtGrad {
    float *ew[3], *eb[3], *ln_w, *ln_b, *in_w, *in_b, *out_w, *out_b, *l1_w, *l1_b, *l2_w, *l2_b, *n1_w, *n1_b, *n2_w, *n2_b, *head_w, *head_b;
    float *log_std;                          // the actor's; NULL for the critic
};

__global__ __launch_bounds__(256) void hns_critic_pack_kernel(const EncNet s, int D, float *img) {
    const long long n = ct_img_floats(D);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float v;
        if (i < I_EW) v = enc_mat_src(s, (int)(i / kCtMat), (int)(i % kCtMat));
        else {
            const long long e = i - I_EW;
            const int in = (int)(e / kCtE), f = (int)(e % kCtE);
            if (in < D) v = s.ew[0][f * D + in];
            else if (in < D + 3) v = s.ew[1] ? s.ew[1][f * 3 + (in - D)] : 0.0f;
            else v = s.ew[2][f * 5 + (in - D - 3)];
        }
        img[i] = v;
    }
}

struct CtArgs {
    const float *img;
    EncNet net;
    const float *xs, *xo, *xc;               // element (n, t, a, [j,] i) at n s?[0] + t s?[1] + a s?[2] (+ j s?[3]) + i
    long long ss[3], so[4], sc[4];
    long long T, steps;                      // env-steps = num_envs T
    const long long *index;                  // [batch] env-steps, or NULL
    long long rows;                          // batch A
    int A, K, D, tiles;
    // [steps, A]: the critic's old values / the actor's old log-probabilities; the encoder op's d features [rows, 128]
    union { const float *bval; const float *logp_old; const float *dfeat; };
    union { const float *bret; const float *adv; };            // [steps, A]: the critic's returns / the actor's advantages
    float clip, delta, inv_n;
    int mse;
    // [rows] or NULL: the critic's values / the actor's new log-probabilities; the encoder op's features [rows, 128]
    union { float *values; float *logp_new; float *feat; };
    double *losspart;                        // [tiles][5]; the actor: [tiles][kActLossSlots]
    const float *ctl;                        // branch weights (written by hns_critic_loss_kernel)
    float *tilepart;                         // [2 tiles][P]
    int P;
    float *stage;                            // 12 arrays [stage_rows][128]: dy, x of Q, K, V, O, L1, L2
    long long stage_rows;
    // the actor (HEAD = 4) alone
    const float *action;                     // [steps, A, 4]
    float clip_lo, clip_hi;                  // f32(1 - clip_param), f32(1 + clip_param): torch.clamp's bounds on a float tensor
};

struct CtLds {
    double dred[5 * kCtRows];
    float a[kCtE * kCtLd], b[kCtE * kCtLd], c[kCtE * kCtLd];
    float p[kCtE * kCtLd];                   // (from here on: the backward kernel only)
    float red[kCtRows * kCtRedLd];
    float sx[kCtMaxSelf * kCtRows];
    float sc[kCtRows];
};
constexpr size_t kCtLdsFwd = offsetof(CtLds, p);

// LayerNorm backward: dx = rstd (g - mean(g) - xh mean(g xh)) with g = dy w; dw += dy xh, db += dy
HNS_DEV void ct_ln_bwd(const float (&dy)[16], const float (&xh)[16], float rstd, const float *w, int g, float (&dx)[16], float (&dw)[16], float (&db)[16]) {
    float wv[16], gi[16];
    enc_vec_load(w, g, wv);
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        gi[i] = dy[i] * wv[i];
        s1 += gi[i];
        s2 = __builtin_fmaf(gi[i], xh[i], s2);
        dw[i] = __builtin_fmaf(dy[i], xh[i], dw[i]);
        db[i] += dy[i];
    }
    const float m1 = row_sum8(s1) * (1.0f / kCtE), m2 = row_sum8(s2) * (1.0f / kCtE);
#pragma unroll
    for (int i = 0; i < 16; ++i) dx[i] = rstd * ((gi[i] - m1) - xh[i] * m2);
}

// a token of the updates: the bias joins last
HNS_DEV float ct_token(const float *ewT, const float *eb, const float *x, int n, const EncNet &N, int g, float (&xh)[16], float (&t)[16]) {
    asm volatile("" ::: "memory");                              // the embedding rows are loaded per token, not hoisted out of the token loops
    return enc_token<false>(ewT, eb, x, n, N.ln_w, N.ln_b, g, xh, t);
}

// the row's vector into a [row][feature] image (LDS pitch kCtRedLd, or a staging block at pitch 128)
HNS_DEV void crow_store(float *img, int pitch, int r, int g, const float (&x)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
        *reinterpret_cast<f32x4 *>(img + r * pitch + enc_feat(g, i, 0)) = f32x4{x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3]};
}

// sum of the vector over rows 0-15 and 16-31 of the tile, written to the tile's two partial rows at `off` (fixed order)
HNS_DEV void ct_flush(CtLds &L, const float (&v)[16], float *part, int P, int off, int tid, int r, int g) {
    crow_store(L.red, kCtRedLd, r, g, v);
    __syncthreads();
    const int f = tid & 127, half = tid >> 7;
    float s = 0.0f;
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) s += L.red[(half * 16 + rr) * kCtRedLd + f];
    float *d = part + (long long)half * P + off + f;
    *d = s;
    __syncthreads();
}

HNS_DEV float ct_dloss(float x, float delta, int mse) {         // d loss / d x before the 1 / n of the mean
    if (mse) return 2.0f * x;
    return x <= -delta ? -delta : (x >= delta ? delta : x);
}

HNS_DEV double ct_loss64(double x, double delta, int mse) {
    if (mse) return x * x;
    const double ax = fabs(x);
    return ax < delta ? 0.5 * x * x : delta * (ax - 0.5 * delta);
}

struct CtRow {
    bool live;
    long long e;                             // env-step
    int ag;
    const float *xs, *xo, *xc;
};

HNS_DEV CtRow ct_row(const CtArgs &a, long long row) {
    CtRow R;
    R.live = row < a.rows;
    const long long q = R.live ? row / a.A : 0;
    R.ag = R.live ? (int)(row % a.A) : 0;
    R.e = R.live ? (a.index ? a.index[q] : q) : 0;
    if (R.e < 0 || R.e >= a.steps) { R.live = false; R.e = 0; }   // an index outside the rollout contributes nothing (callers check the range)
    const long long n = R.e / a.T, t = R.e % a.T;
    R.xs = R.live ? a.xs + n * a.ss[0] + t * a.ss[1] + R.ag * a.ss[2] : nullptr;
    R.xo = R.live && a.xo ? a.xo + n * a.so[0] + t * a.so[1] + R.ag * a.so[2] : nullptr;
    R.xc = R.live ? a.xc + n * a.sc[0] + t * a.sc[1] + R.ag * a.sc[2] : nullptr;
    return R;
}

// token j >= 1 of the row
HNS_DEV float ct_token_j(const CtArgs &a, const CtRow &R, int j, int g, float (&xh)[16], float (&t)[16], const float *&x, int &n) {
    const float *ewo = a.img + I_EW + a.D * kCtE;
    if (j < a.A) {
        x = R.xo ? R.xo + (j - 1) * a.so[3] : nullptr;
        n = 3;
        return ct_token(ewo, a.net.eb[1], x, 3, a.net, g, xh, t);
    }
    x = R.xc ? R.xc + (j - a.A) * a.sc[3] : nullptr;
    n = 5;
    return ct_token(ewo + 3 * kCtE, a.net.eb[2], x, 5, a.net, g, xh, t);
}

// ---- the centralised critic (critic_input: state; include/hns.h: hns_critic_train_grad_central)
// a row is an env-step: its query is drone 0's row of state_drones (a.xs, ss[2] apart), its cylinders the rows at agent index 0 of a.xc
HNS_DEV CtRow ct_row_central(const CtArgs &a, long long row) {
    CtRow R;
    R.live = row < a.rows;
    R.ag = 0;
    R.e = R.live ? (a.index ? a.index[row] : row) : 0;
    if (R.e < 0 || R.e >= a.steps) { R.live = false; R.e = 0; }
    const long long n = R.e / a.T, t = R.e % a.T;
    R.xs = R.live ? a.xs + n * a.ss[0] + t * a.ss[1] : nullptr;
    R.xo = nullptr;
    R.xc = R.live ? a.xc + n * a.sc[0] + t * a.sc[1] : nullptr;
    return R;
}

// token j >= 1 of the row: drone j through token 0's embedding, then the cylinders
HNS_DEV float ct_token_j_central(const CtArgs &a, const CtRow &R, int j, int g, float (&xh)[16], float (&t)[16], const float *&x, int &n) {
    if (j < a.A) {
        x = R.xs ? R.xs + j * a.ss[2] : nullptr;
        n = a.D;
        return ct_token(a.img + I_EW, a.net.eb[0], x, a.D, a.net, g, xh, t);
    }
    x = R.xc ? R.xc + (j - a.A) * a.sc[3] : nullptr;
    n = 5;
    return ct_token(a.img + I_EW + (a.D + 3) * kCtE, a.net.eb[2], x, 5, a.net, g, xh, t);
}

// One drone token's part of d embed_self_{b,w} in the tile's two partial rows (`ph`: the half's; thread = feature ef of half eh): the sums over
// the half's 16 rows of de and of de (x) x, token 0's statements.  `add`: onto what an earlier token of the tile left there — the same thread
// wrote it, so the order of the sum is the order of the tokens.
HNS_DEV void ct_embed_self_sums(CtLds &L, const float (&de)[16], const float *x, int D, float *ph, int ef, int eh, int r, int g, bool add) {
    crow_store(L.red, kCtRedLd, r, g, de);
    for (int k = g; k < D; k += 8) L.sx[k * kCtRows + r] = x ? x[k] : 0.0f;
    __syncthreads();
    float sb = 0.0f;
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) sb += L.red[(eh * 16 + rr) * kCtRedLd + ef];
    ph[O_EBS + ef] = add ? ph[O_EBS + ef] + sb : sb;
    for (int k = 0; k < D; ++k) {
        float sw = 0.0f;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) sw = __builtin_fmaf(L.red[(eh * 16 + rr) * kCtRedLd + ef], L.sx[k * kCtRows + eh * 16 + rr], sw);
        ph[O_EWS + k * kCtE + ef] = add ? ph[O_EWS + k * kCtE + ef] + sw : sw;
    }
    __syncthreads();
}

// the critic's two tile kernels on tiles of 32 env-steps (a.rows = the minibatch's env-steps; b_values, b_returns and `values` [.., A])
template <bool BWD, int HEAD = 1>
__global__ __launch_bounds__(kCtThreads, BWD ? 1 : 2) void hns_critic_central_kernel(const CtArgs a) {
#define CT_BODY_TILE
#define CT_CENTRAL
#define CT_TILE_BLOCK blockIdx.x
#define CT_TILE_ROW ((long long)tile * kCtRows + r)
#define CT_TILE_FIRST 0
#define CT_TILE_STEP 1
#include "hns_policy_train_bodies.inc"
#undef CT_BODY_TILE
#undef CT_CENTRAL
#undef CT_TILE_BLOCK
#undef CT_TILE_ROW
#undef CT_TILE_FIRST
#undef CT_TILE_STEP
}

template <bool BWD, int HEAD = 1>
__global__ __launch_bounds__(kCtThreads, BWD ? 1 : 2) void hns_critic_kernel(const CtArgs a) {
#define CT_BODY_TILE
#define CT_TILE_BLOCK blockIdx.x
#define CT_TILE_ROW ((long long)tile * kCtRows + r)
#define CT_TILE_FIRST (int)((ag + a.A - (long long)tile * kCtRows % a.A) % a.A)
#define CT_TILE_STEP a.A
#include "hns_policy_train_bodies.inc"
#undef CT_TILE_BLOCK
#undef CT_TILE_ROW
#undef CT_TILE_FIRST
#undef CT_TILE_STEP
}

// One actor per agent (share_actor: false; include/hns.h: hns_actor_train_grad_agents).  `a0.net` holds the STACKED tensors
// ([A, ...]) and `a0.img` A packed images; workgroup (t, agent) runs tile t of the agent's a0.tiles / A tiles — minibatch positions 32 t .. 32 t + 31
// of that agent — on the agent's slice and image, formed here once per tile.  The tiles are numbered agent-major, so the staged operand pairs,
// partial rows and loss partials of an agent are contiguous and no row range of the weight-gradient kernel straddles two agents.  A position past
// the agent's last one (the tail of its last tile, and the tiles that pad its count to whole row ranges) is a row that is not live.
__global__ __launch_bounds__(kCtThreads, 1) void hns_actor_agents_kernel(const CtArgs a0) {
    constexpr bool BWD = true;
    constexpr int HEAD = kActDim;
    const int agent = blockIdx.y, tpa = a0.tiles / a0.A;
    CtArgs a = a0;
    a.img = a0.img + (long long)agent * ct_img_floats(a0.D);
    a.net = enc_agent_slice(a0.net, a0.D, kActDim, agent);
#define CT_TILE_BLOCK (agent * tpa + blockIdx.x)
#define CT_TILE_ROW (((long long)blockIdx.x * kCtRows + r) * a.A < a.rows ? ((long long)blockIdx.x * kCtRows + r) * a.A + agent : a.rows)
#define CT_TILE_FIRST (ag == agent ? 0 : kCtRows)
#define CT_TILE_STEP 1
#include "hns_policy_train_bodies.inc"
#undef CT_TILE_BLOCK
#undef CT_TILE_ROW
#undef CT_TILE_FIRST
#undef CT_TILE_STEP
}

// The encoder alone on the stacked tensors (hns_encoder_forward_agents / hns_encoder_backward_agents): hns_actor_agents_kernel's tiles, agent slice
// and image with HEAD = 0 — features [rows, 128] out, or d features in, at row = position x A + agent as the shared op has them.  The forward
// launch has no padding tiles (nothing is staged): its grid is the agents' live tiles alone.
template <bool BWD, int HEAD = 0>                              // (HEAD a parameter: the body's `if constexpr` discards only dependent branches)
__global__ __launch_bounds__(kCtThreads, BWD ? 1 : 2) void hns_encoder_agents_kernel(const CtArgs a0) {
    const int agent = blockIdx.y, tpa = a0.tiles / a0.A;
    CtArgs a = a0;
    a.img = a0.img + (long long)agent * ct_img_floats(a0.D);
    a.net = enc_agent_slice(a0.net, a0.D, 0, agent);
#define CT_TILE_BLOCK (agent * tpa + blockIdx.x)
#define CT_TILE_ROW (((long long)blockIdx.x * kCtRows + r) * a.A < a.rows ? ((long long)blockIdx.x * kCtRows + r) * a.A + agent : a.rows)
#define CT_TILE_FIRST (ag == agent ? 0 : kCtRows)
#define CT_TILE_STEP 1
#include "hns_policy_train_bodies.inc"
#undef CT_TILE_BLOCK
#undef CT_TILE_ROW
#undef CT_TILE_FIRST
#undef CT_TILE_STEP
#undef CT_BODY_TILE
}

// the A packed images of the stacked actors: hns_critic_pack_kernel's per agent (blockIdx.y)
__global__ __launch_bounds__(256) void hns_actor_pack_agents_kernel(const EncNet s0, int D, float *img) {
    const long long n = ct_img_floats(D);
    const EncNet s = enc_agent_slice(s0, D, kActDim, blockIdx.y);
    float *dst = img + blockIdx.y * n;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float v;
        if (i < I_EW) v = enc_mat_src(s, (int)(i / kCtMat), (int)(i % kCtMat));
        else {
            const long long e = i - I_EW;
            const int in = (int)(e / kCtE), f = (int)(e % kCtE);
            if (in < D) v = s.ew[0][f * D + in];
            else if (in < D + 3) v = s.ew[1] ? s.ew[1][f * 3 + (in - D)] : 0.0f;
            else v = s.ew[2][f * 5 + (in - D - 3)];
        }
        dst[i] = v;
    }
}

// The critic's scalars in two halves that hns_critic_loss_kernel runs back to back and the data-parallel entries run apart.
// Summing half: thread t adds the five partials of tiles t, t + 256, ... in that order; thread 0 then adds the 256 thread sums in index order.
HNS_DEV void ct_loss_thread_sums(const double *part, int tiles, double (&sm)[5][256], int tid) {
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < tiles; i += 256)
#pragma unroll
        for (int q = 0; q < 5; ++q) acc[q] += part[(long long)i * 5 + q];
#pragma unroll
    for (int q = 0; q < 5; ++q) sm[q][tid] = acc[q];
    __syncthreads();
}

HNS_DEV void ct_loss_total(const double (&sm)[5][256], double (&S)[5]) {
    for (int q = 0; q < 5; ++q) {
        double s = 0.0;
        for (int i = 0; i < 256; ++i) s += sm[q][i];
        S[q] = s;
    }
}

// Deciding half: value_loss, explained_var and the branch weights from the five sums over n rows
HNS_DEV void ct_loss_decide(const double (&S)[5], double n, float *ctl, float *value_loss, float *explained_var) {
    const double lo = S[0] / n, lc = S[1] / n;
    ctl[0] = lo > lc ? 1.0f : (lo < lc ? 0.0f : 0.5f);
    ctl[1] = lo > lc ? 0.0f : (lo < lc ? 1.0f : 0.5f);
    value_loss[0] = (float)(lo > lc ? lo : lc);
    const double var = (S[4] - S[3] * S[3] / n) / (n - 1.0);             // unbiased, as Tensor.var()
    explained_var[0] = (float)(1.0 - (S[2] / n) / var);
}

// sums the per-tile loss partials in a fixed order; value_loss, explained_var, branch weights
__global__ __launch_bounds__(256) void hns_critic_loss_kernel(const double *part, int tiles, double n, float *ctl, float *value_loss, float *explained_var) {
    __shared__ double sm[5][256];
    ct_loss_thread_sums(part, tiles, sm, threadIdx.x);
    if (threadIdx.x == 0) {
        double S[5];
        ct_loss_total(sm, S);
        ct_loss_decide(S, n, ctl, value_loss, explained_var);
    }
}

// the summing half alone: the five sums of this rank's rows, for the caller to add to the other ranks'
__global__ __launch_bounds__(256) void hns_critic_sums_kernel(const double *part, int tiles, double *sums) {
    __shared__ double sm[5][256];
    ct_loss_thread_sums(part, tiles, sm, threadIdx.x);
    if (threadIdx.x == 0) {
        double S[5];
        ct_loss_total(sm, S);
        for (int q = 0; q < 5; ++q) sums[q] = S[q];
    }
}

// the deciding half alone, on sums over all ranks' n rows
__global__ __launch_bounds__(64) void hns_critic_decide_kernel(const double *sums, double n, float *ctl, float *value_loss, float *explained_var) {
    if (threadIdx.x == 0) {
        double S[5];
        for (int q = 0; q < 5; ++q) S[q] = sums[q];
        ct_loss_decide(S, n, ctl, value_loss, explained_var);
    }
}

// the actor's scalars from the per-tile partials, in a fixed order: policy_loss = -k mean(min(surr1, surr2)); entropy of DiagGaussian (the same for
// every row); ESS = mean over agents of exp(2 logsumexp_batch(r) - logsumexp_batch(2 r)) / batch — of the ratio itself, as the reference writes it
__global__ __launch_bounds__(64) void hns_actor_loss_kernel(const double *part, int tiles, int A, double n, double batch, const float *log_std, float *policy_loss,
                                                            float *entropy, float *ess) {
#define CT_BODY_LOSS
#define CT_LOSS_NLS 1
#define CT_LOSS_ENTROPY ent
#include "hns_policy_train_bodies.inc"
#undef CT_LOSS_NLS
#undef CT_LOSS_ENTROPY
}

// one actor per agent: log_std [A][4]; the rows' mean entropy is the mean over the agents of each agent's
__global__ __launch_bounds__(64) void hns_actor_loss_agents_kernel(const double *part, int tiles, int A, double n, double batch, const float *log_std,
                                                                   float *policy_loss, float *entropy, float *ess) {
#define CT_LOSS_NLS A
#define CT_LOSS_ENTROPY (ent / (double)A)
#include "hns_policy_train_bodies.inc"
#undef CT_LOSS_NLS
#undef CT_LOSS_ENTROPY
#undef CT_BODY_LOSS
}

// dW partials: per (row range, matrix) the 128 x 128 product dy^T x over the range's rows, and the column sums of dy
__global__ __launch_bounds__(256, 2) void hns_critic_wgrad_kernel(const float *stage, long long stage_rows, int tiles, int tps, float *part) {
    __shared__ __align__(16) float sdy[kCtRows * kCtGemmLd];
    __shared__ __align__(16) float sxx[kCtRows * kCtGemmLd];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, col = lane & 15, kq = lane >> 4;
    const int m = blockIdx.y, split = blockIdx.x;
    const float *dy = stage + (long long)(2 * m) * stage_rows * kCtE, *x = stage + (long long)(2 * m + 1) * stage_rows * kCtE;
    const int t0 = split * tps, t1 = t0 + tps < tiles ? t0 + tps : tiles;
    f32x4 acc[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bs0 = 0.0f, bs1 = 0.0f;
    for (int t = t0; t < t1; ++t) {
        const long long base = (long long)t * kCtRows * kCtE;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i, rr = idx >> 5, c4 = idx & 31;
            *reinterpret_cast<f32x4 *>(&sdy[rr * kCtGemmLd + 4 * c4]) = *reinterpret_cast<const f32x4 *>(dy + base + rr * kCtE + 4 * c4);
            *reinterpret_cast<f32x4 *>(&sxx[rr * kCtGemmLd + 4 * c4]) = *reinterpret_cast<const f32x4 *>(x + base + rr * kCtE + 4 * c4);
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int k = 4 * s + kq;
            const float a0 = sdy[k * kCtGemmLd + (2 * w) * 16 + col], a1 = sdy[k * kCtGemmLd + (2 * w + 1) * 16 + col];
            bs0 += a0;
            bs1 += a1;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float b = sxx[k * kCtGemmLd + c * 16 + col];
                acc[0][c] = enc_mfma(a0, b, acc[0][c]);
                acc[1][c] = enc_mfma(a1, b, acc[1][c]);
            }
        }
        __syncthreads();
    }
    float *out = part + ((long long)split * 6 + m) * kCtGemmOut;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int c = 0; c < 8; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[((2 * w + i) * 16 + 4 * kq + r) * kCtE + c * 16 + col] = acc[i][c][r];
    bs0 += __shfl_xor(bs0, 16, 64);
    bs0 += __shfl_xor(bs0, 32, 64);
    bs1 += __shfl_xor(bs1, 16, 64);
    bs1 += __shfl_xor(bs1, 32, 64);
    if (kq == 0) {
        out[kCtMat + (2 * w) * 16 + col] = bs0;
        out[kCtMat + (2 * w + 1) * 16 + col] = bs1;
    }
}

// where gradient value e of the weight-gradient partials goes (zero: in_proj_bias' k third, whose gradient is identically 0)
HNS_DEV float *ct_dst_gemm(const CtGrad &g, int e, bool &zero) {
    const int m = e / kCtGemmOut, x = e % kCtGemmOut;
    zero = false;
    if (x < kCtMat) {
        switch (m) {
            case 0: case 1: case 2: return g.in_w + m * kCtMat + x;
            case 3: return g.out_w + x;
            case 4: return g.l1_w + x;
            default: return g.l2_w + x;
        }
    }
    const int f = x - kCtMat;
    switch (m) {
        case 0: return g.in_b + f;
        case 1: zero = true; return g.in_b + kCtE + f;
        case 2: return g.in_b + 2 * kCtE + f;
        case 3: return g.out_b + f;
        case 4: return g.l1_b + f;
        default: return g.l2_b + f;
    }
}

// HEADS false (the encoder op): head_w, head_b and log_std have no destination
template <bool HEADS>
HNS_DEV float *ct_dst_tile(const CtGrad &g, int D, int heads, int e) {
    if (e < O_EWO) {
        const int f = e & 127;
        switch (e >> 7) {
            case 0: return g.ln_w + f;
            case 1: return g.ln_b + f;
            case 2: return g.n1_w + f;
            case 3: return g.n1_b + f;
            case 4: return g.n2_w + f;
            case 5: return g.n2_b + f;
            case 6: return HEADS ? g.head_w + f : nullptr;
            case 7: return g.eb[0] + f;
            case 8: return g.eb[1] ? g.eb[1] + f : nullptr;
            default: return g.eb[2] + f;
        }
    }
    if (e < O_EWC) return g.ew[1] ? g.ew[1] + ((e - O_EWO) & 127) * 3 + ((e - O_EWO) >> 7) : nullptr;
    if (e < O_HB) return g.ew[2] + ((e - O_EWC) & 127) * 5 + ((e - O_EWC) >> 7);
    if (e < O_EWS) return HEADS && e - O_HB < heads ? g.head_b + (e - O_HB) : nullptr;
    if (e < O_EWS + D * kCtE) return g.ew[0] + ((e - O_EWS) & 127) * D + ((e - O_EWS) >> 7);
    if (!HEADS) return nullptr;
    const int x = e - (O_EWS + D * kCtE);                       // the actor's head: rows 1 .. heads - 1 of head_w, then log_std
    return x < (heads - 1) * kCtE ? g.head_w + kCtE + x : g.log_std + (x - (heads - 1) * kCtE);
}

// the centralised critic's partial row (ct_central_hb): v_out's A rows and A biases, no state_others embedding
HNS_DEV float *ct_dst_tile_central(const CtGrad &g, int D, int A, int e) {
    if (e < O_EWO) return (e >> 7) == 8 ? nullptr : ct_dst_tile<true>(g, D, 1, e);
    if (e < O_EWC || (e >= O_HB && e < O_EWS)) return nullptr;
    if (e < O_EWS + D * kCtE) return ct_dst_tile<true>(g, D, 1, e);
    const int x = e - (O_EWS + D * kCtE);
    if (x < (HNS_MAX_AGENTS - 1) * kCtE) return x < (A - 1) * kCtE ? g.head_w + kCtE + x : nullptr;
    return x - (HNS_MAX_AGENTS - 1) * kCtE < A ? g.head_b + (x - (HNS_MAX_AGENTS - 1) * kCtE) : nullptr;
}

// 32 gradient values per block, 8 threads each: slice s sums its range of the partials in fp64, the slices add up in order.  `ls_add` joins
// every log_std value's sum once (the actor's -entropy_coef: the entropy term's gradient is the same constant whatever the rows)
template <bool HEADS, bool CENTRAL = false>                    // CENTRAL: `heads` is v_out's A rows, the tile partials' places ct_dst_tile_central's
HNS_DEV void ct_reduce(const float *gpart, int splits, const float *tpart, int nt, int P, int gblocks, const CtGrad &g, int D, double *blockpart, int heads,
                       double ls_add) {
    __shared__ double sm[8][32];
    __shared__ double sq[32];
    const int tid = threadIdx.x, el = tid & 31, sl = tid >> 5;
    const bool gemm = (int)blockIdx.x < gblocks;
    const int e = (gemm ? blockIdx.x : blockIdx.x - gblocks) * 32 + el;
    const int n = gemm ? splits : nt;
    const long long stride = gemm ? 6LL * kCtGemmOut : P;
    const float *src = gemm ? gpart : tpart;
    float *dst = nullptr;
    bool zero = false;
    if (e < stride) {
        if constexpr (CENTRAL) dst = gemm ? ct_dst_gemm(g, e, zero) : ct_dst_tile_central(g, D, heads, e);
        else dst = gemm ? ct_dst_gemm(g, e, zero) : ct_dst_tile<HEADS>(g, D, heads, e);
    }
    double acc = 0.0;
    if (dst && !zero) {
        const int lo = (int)((long long)n * sl / 8), hi = (int)((long long)n * (sl + 1) / 8);
        for (int b = lo; b < hi; ++b) acc += (double)src[(long long)b * stride + e];
    }
    sm[sl][el] = acc;
    __syncthreads();
    if (tid < 32) {
        double tot = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) tot += sm[q][el];
        if (!CENTRAL && heads > 1 && !gemm && e >= P - heads && e < P) tot += ls_add;
        const float s = (float)tot;
        if (dst) dst[0] = s;
        sq[el] = dst ? (double)s * (double)s : 0.0;
    }
    __syncthreads();
    if (tid == 0) {
        double tot = 0.0;
        for (int q = 0; q < 32; ++q) tot += sq[q];
        blockpart[blockIdx.x] = tot;
    }
}

__global__ __launch_bounds__(256) void hns_critic_reduce_kernel(const float *gpart, int splits, const float *tpart, int nt, int P, int gblocks, const CtGrad g,
                                                                int D, double *blockpart, int heads, double ls_add) {
    ct_reduce<true>(gpart, splits, tpart, nt, P, gblocks, g, D, blockpart, heads, ls_add);
}

__global__ __launch_bounds__(256) void hns_critic_reduce_central_kernel(const float *gpart, int splits, const float *tpart, int nt, int P, int gblocks,
                                                                        const CtGrad g, int D, double *blockpart, int A) {
    ct_reduce<true, true>(gpart, splits, tpart, nt, P, gblocks, g, D, blockpart, A, 0.0);
}

// the encoder op's: the 20 encoder tensors alone (heads = 0); the per-block sums of squares are written and not used
__global__ __launch_bounds__(256) void hns_encoder_reduce_kernel(const float *gpart, int splits, const float *tpart, int nt, int P, int gblocks, const CtGrad g,
                                                                 int D, double *blockpart) {
    ct_reduce<false>(gpart, splits, tpart, nt, P, gblocks, g, D, blockpart, 0, 0.0);
}

// one actor per agent: workgroup (b, agent) is the reduce kernel's block b on the agent's weight-gradient partials (`spa` row ranges), partial rows
// (`ntpa`) and slice of the stacked gradient tensors; the per-block sums of squares of all agents lie side by side for ONE norm over everything
__global__ __launch_bounds__(256) void hns_actor_reduce_agents_kernel(const float *gpart, int spa, const float *tpart, int ntpa, int P, int gblocks, const CtGrad g0,
                                                                      int D, double *blockpart, double ls_add) {
    const int agent = blockIdx.y;
    const CtGrad g = enc_agent_slice(g0, D, kActDim, agent);
    ct_reduce<true>(gpart + (long long)agent * spa * 6 * kCtGemmOut, spa, tpart + (long long)agent * ntpa * P, ntpa, P, gblocks, g, D,
                    blockpart + (long long)agent * gridDim.x, kActDim, ls_add);
}

// the encoder op on the stacked tensors: hns_actor_reduce_agents_kernel without the head's destinations
__global__ __launch_bounds__(256) void hns_encoder_reduce_agents_kernel(const float *gpart, int spa, const float *tpart, int ntpa, int P, int gblocks, const CtGrad g0,
                                                                        int D, double *blockpart) {
    const int agent = blockIdx.y;
    const CtGrad g = enc_agent_slice(g0, D, 0, agent);
    ct_reduce<false>(gpart + (long long)agent * spa * 6 * kCtGemmOut, spa, tpart + (long long)agent * ntpa * P, ntpa, P, gblocks, g, D,
                     blockpart + (long long)agent * gridDim.x, 0, 0.0);
}

__global__ __launch_bounds__(256) void hns_critic_norm_kernel(const double *blockpart, int nb, float *grad_norm) {
    __shared__ double sm[256];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int i = tid; i < nb; i += 256) acc += blockpart[i];
    sm[tid] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < 256; ++i) s += sm[i];
        grad_norm[0] = (float)sqrt(s);
    }
}

}  // namespace hns

namespace {

size_t ct_up(size_t v) { return (v + 255) & ~(size_t)255; }

struct CtPlan {
    long long tiles, tps, splits, stage_rows;
    int P, gblocks, tblocks;
    size_t o_ctl, o_loss, o_block, o_img, o_tile, o_gemm, o_stage, total;
};

// central: the centralised critic — `rows` env-steps in tiles of 32, ct_partial_central's partial rows
bool ct_plan(int64_t rows, int32_t D, int32_t A, int32_t K, CtPlan &p, int heads = 1, bool central = false) {
    if (rows < 1 || rows > ((int64_t)1 << 31) - 64 || D < 1 || D > hns::kCtMaxSelf || A < 1 || A > HNS_MAX_AGENTS || K < 1 || K > HNS_MAX_CYLINDERS) return false;
    p.tiles = (rows + hns::kCtRows - 1) / hns::kCtRows;
    p.tps = (p.tiles + hns::kCtMaxSplits - 1) / hns::kCtMaxSplits;
    p.splits = (p.tiles + p.tps - 1) / p.tps;
    p.stage_rows = p.tiles * hns::kCtRows;
    p.P = central ? hns::ct_partial_central(D) : hns::ct_partial_floats(D, heads);
    p.gblocks = (6 * hns::kCtGemmOut + 31) / 32;
    p.tblocks = (p.P + 31) / 32;
    size_t o = 0;
    p.o_ctl = o; o += ct_up(64 * sizeof(float));
    p.o_loss = o; o += ct_up((size_t)p.tiles * (heads > 1 ? hns::kActLossSlots : 5) * sizeof(double));
    p.o_block = o; o += ct_up((size_t)hns::kCtMaxBlocks * sizeof(double));
    p.o_img = o; o += ct_up((size_t)hns::ct_img_floats(D) * sizeof(float));
    p.o_tile = o; o += ct_up((size_t)p.tiles * 2 * p.P * sizeof(float));
    p.o_gemm = o; o += ct_up((size_t)p.splits * 6 * hns::kCtGemmOut * sizeof(float));
    p.o_stage = o; o += ct_up((size_t)12 * p.stage_rows * hns::kCtE * sizeof(float));
    p.total = o;
    return true;
}

// One actor per agent: `batch` positions per agent in tiles of one agent, numbered agent-major.  An agent's tile count is padded to a whole number
// of the weight-gradient kernel's row ranges (tps tiles each; the padding tiles' rows are not live and stage dy = 0), so no range straddles two
// agents; an image and a set of per-block sums per agent.
bool ct_plan_agents(int64_t rows, int32_t D, int32_t A, int32_t K, CtPlan &p) {
    if (A < 1 || A > HNS_MAX_AGENTS || rows < A || rows % A || !ct_plan(rows, D, A, K, p, hns::kActDim)) return false;
    const long long tpa = (rows / A + hns::kCtRows - 1) / hns::kCtRows;
    long long spa = std::max(1, hns::kCtMaxSplits / A);
    p.tps = (tpa + spa - 1) / spa;
    spa = (tpa + p.tps - 1) / p.tps;
    p.tiles = (long long)A * spa * p.tps;
    p.splits = (long long)A * spa;
    p.stage_rows = p.tiles * hns::kCtRows;
    if (p.stage_rows > ((int64_t)1 << 31) - 64) return false;
    size_t o = 0;
    p.o_ctl = o; o += ct_up(64 * sizeof(float));
    p.o_loss = o; o += ct_up((size_t)p.tiles * hns::kActLossSlots * sizeof(double));
    p.o_block = o; o += ct_up((size_t)A * (p.gblocks + p.tblocks) * sizeof(double));
    p.o_img = o; o += ct_up((size_t)A * hns::ct_img_floats(D) * sizeof(float));
    p.o_tile = o; o += ct_up((size_t)p.tiles * 2 * p.P * sizeof(float));
    p.o_gemm = o; o += ct_up((size_t)p.splits * 6 * hns::kCtGemmOut * sizeof(float));
    p.o_stage = o; o += ct_up((size_t)12 * p.stage_rows * hns::kCtE * sizeof(float));
    p.total = o;
    return true;
}

// the encoder op's workspace (heads = 0: the critic's tile layout).  Forward: the packed operand image alone.  Backward: the image, the tiles'
// partial rows, the weight-gradient partials, the staged operand pairs and the reduce kernel's per-block sums — no branch weights, no loss partials
bool ct_plan_encoder(int64_t rows, int32_t D, int32_t A, int32_t K, bool backward, CtPlan &p) {
    if (!ct_plan(rows, D, A, K, p, 0)) return false;
    size_t o = 0;
    p.o_ctl = p.o_loss = 0;
    p.o_img = o; o += ct_up((size_t)hns::ct_img_floats(D) * sizeof(float));
    if (backward) {
        p.o_block = o; o += ct_up((size_t)hns::kCtMaxBlocks * sizeof(double));
        p.o_tile = o; o += ct_up((size_t)p.tiles * 2 * p.P * sizeof(float));
        p.o_gemm = o; o += ct_up((size_t)p.splits * 6 * hns::kCtGemmOut * sizeof(float));
        p.o_stage = o; o += ct_up((size_t)12 * p.stage_rows * hns::kCtE * sizeof(float));
    } else {
        p.o_block = p.o_tile = p.o_gemm = p.o_stage = 0;
    }
    p.total = o;
    return true;
}

// the encoder op on the stacked tensors: ct_plan_agents' tiles and row ranges with the encoder op's partial rows (heads = 0) and arrays — forward
// the A images alone
bool ct_plan_encoder_agents(int64_t rows, int32_t D, int32_t A, int32_t K, bool backward, CtPlan &p) {
    if (!ct_plan_agents(rows, D, A, K, p)) return false;
    p.P = hns::ct_partial_floats(D, 0);
    p.tblocks = (p.P + 31) / 32;
    size_t o = 0;
    p.o_ctl = p.o_loss = 0;
    p.o_img = o; o += ct_up((size_t)A * hns::ct_img_floats(D) * sizeof(float));
    if (backward) {
        p.o_block = o; o += ct_up((size_t)A * (p.gblocks + p.tblocks) * sizeof(double));
        p.o_tile = o; o += ct_up((size_t)p.tiles * 2 * p.P * sizeof(float));
        p.o_gemm = o; o += ct_up((size_t)p.splits * 6 * hns::kCtGemmOut * sizeof(float));
        p.o_stage = o; o += ct_up((size_t)12 * p.stage_rows * hns::kCtE * sizeof(float));
    } else {
        p.o_block = p.o_tile = p.o_gemm = p.o_stage = 0;
    }
    p.total = o;
    return true;
}

// What the critic's and the actor's entry points share.  hns_critic_batch and hns_actor_batch carry the same leading fields under the same names:
// the templates over the batch type read them from either.  Every refusal keeps the entry point's order: ct_check_shape, the entry's hyper-parameters,
// ct_bind_net, ct_check_obs, the entry's per-row pointers, ct_plan_call.

template <typename Batch>
int ct_check_shape(const char *fn, const Batch &b, int32_t self_dim, int32_t num_agents, int32_t num_cylinders) {
    if (self_dim < 1 || self_dim > hns::kCtMaxSelf) return hns_fail(fn, "self_dim must be in [1, " + std::to_string(hns::kCtMaxSelf) + "]");
    if (num_agents < 1 || num_agents > HNS_MAX_AGENTS) return hns_fail(fn, "num_agents must be in [1, 7]");
    if (num_cylinders < 1 || num_cylinders > HNS_MAX_CYLINDERS) return hns_fail(fn, "num_cylinders must be in [1, 16]");
    if (b.batch < 1) return hns_fail(fn, "batch must be >= 1 (the mean over an empty minibatch is NaN)");
    if (b.num_envs < 1 || b.num_steps < 1 || b.num_envs > ((int64_t)1 << 40) / b.num_steps) return hns_fail(fn, "num_envs, num_steps must be >= 1");
    if (b.batch > ((int64_t)1 << 31) / HNS_MAX_AGENTS) return hns_fail(fn, "batch too large");
    if (!b.index && b.batch > b.num_envs * b.num_steps) return hns_fail(fn, "batch exceeds the env-steps of the rollout (no index)");
    return HNS_OK;
}

// the parameter and gradient tables, checked and copied by ONE field list (heads > 1: the actor, whose log_std joins both; heads 0: the encoder
// op, whose head fields are ignored and left NULL).  grads NULL: a forward-only entry (hns_critic_train_sums, hns_encoder_forward) binds the
// parameters alone and `g` stays empty
int ct_bind_net(const char *fn, const hns_policy_net &net, const hns_policy_grads *grads, bool others, int heads, hns::EncNet &n, hns::CtGrad &g) {
    bool ok = true;
    const auto ignored = [&](const float *const *f) { return heads == 0 && (f == &net.head_w || f == &net.head_b); };
#define X(f, m)                                                                                                                \
    ok = ok && (ignored(&net.f) || (net.f && hns_aligned(net.f, 16) && (!grads || (grads->f && hns_aligned(grads->f, 4)))));  \
    n.m = ignored(&net.f) ? nullptr : net.f;                                                                                   \
    g.m = grads && !ignored(&net.f) ? grads->f : nullptr;
    HNS_CT_FIELDS(X)
#undef X
    if (heads > 1) ok = ok && net.log_std && hns_aligned(net.log_std, 16) && (!grads || (grads->log_std && hns_aligned(grads->log_std, 4)));
    n.log_std = heads > 1 ? net.log_std : nullptr;
    g.log_std = heads > 1 && grads ? grads->log_std : nullptr;
    if (!ok) return hns_fail(fn, "every parameter must be a non-NULL 16-byte aligned fp32 array, every gradient a non-NULL fp32 array");
    if (others && (!net.embed_others_w || !net.embed_others_b || !hns_aligned(net.embed_others_b, 16) ||
                   (grads && (!grads->embed_others_w || !grads->embed_others_b))))
        return hns_fail(fn, "state_others embedding (parameter or gradient) missing or misaligned (num_agents > 1)");
    n.ew[1] = others ? net.embed_others_w : nullptr; n.eb[1] = others ? net.embed_others_b : nullptr;
    g.ew[1] = others && grads ? grads->embed_others_w : nullptr; g.eb[1] = others && grads ? grads->embed_others_b : nullptr;
    return HNS_OK;
}

template <typename Batch>
int ct_check_obs(const char *fn, const Batch &b, bool others) {
    if (!b.obs_self || !b.obs_cylinders || (others && !b.obs_others)) return hns_fail(fn, "observation pointer missing");
    if (!hns_aligned(b.obs_self, 4) || !hns_aligned(b.obs_cylinders, 4) || (b.obs_others && !hns_aligned(b.obs_others, 4))) return hns_fail(fn, "misaligned observation");
    for (int k = 0; k < 3; ++k)
        if (b.self_stride[k] < 0) return hns_fail(fn, "negative stride");
    for (int k = 0; k < 4; ++k)
        if (b.others_stride[k] < 0 || b.cyl_stride[k] < 0) return hns_fail(fn, "negative stride");
    return HNS_OK;
}

// the last refusals (index, `outs`: the entry's fp32 outputs, a NULL optional one among them; the plan and the workspace), then the part of the
// kernel arguments that is the same for both networks: observations, index, shape, the workspace's arrays
// heads 0: the encoder op, whose plan is ct_plan_encoder's (`backward`: hns_encoder_backward's)
template <typename Batch>
int ct_plan_call(const char *fn, const Batch &b, std::initializer_list<const float *> outs, void *workspace, size_t workspace_bytes, int32_t self_dim,
                 int32_t num_agents, int32_t num_cylinders, int heads, CtPlan &p, hns::CtArgs &a, bool backward = true, bool agents = false,
                 bool central = false) {
    if (b.index && !hns_aligned(b.index, 8)) return hns_fail(fn, "misaligned index");
    bool ok = hns_aligned(workspace, 256);
    for (const float *o : outs) ok = ok && hns_aligned(o, 4);
    if (!ok) return hns_fail(fn, "misaligned output (scalars 4 bytes, workspace 256)");
    const int64_t rows = central ? b.batch : b.batch * num_agents;   // the centralised critic's rows are env-steps
    if (central ? !ct_plan(rows, self_dim, num_agents, num_cylinders, p, 1, true) :
        agents ? (heads == 0 ? !ct_plan_encoder_agents(rows, self_dim, num_agents, num_cylinders, backward, p)
                             : !ct_plan_agents(rows, self_dim, num_agents, num_cylinders, p))
               : (heads == 0 ? !ct_plan_encoder(rows, self_dim, num_agents, num_cylinders, backward, p) : !ct_plan(rows, self_dim, num_agents, num_cylinders, p, heads)))
        return hns_fail(fn, "invalid shape");
    if (workspace_bytes < p.total)
        return hns_fail(fn, central      ? "workspace too small (hns_critic_train_central_workspace_bytes)"
                            : agents     ? (heads == 0 ? "workspace too small (hns_encoder_agents_workspace_bytes)"
                                                        : "workspace too small (hns_actor_train_agents_workspace_bytes)")
                            : heads > 1  ? "workspace too small (hns_actor_train_workspace_bytes)"
                            : heads == 1 ? "workspace too small (hns_critic_train_workspace_bytes)"
                                         : "workspace too small (hns_encoder_workspace_bytes)");

    unsigned char *ws = static_cast<unsigned char *>(workspace);
    a.img = reinterpret_cast<float *>(ws + p.o_img);
    a.xs = b.obs_self; a.xo = num_agents > 1 && !central ? b.obs_others : nullptr; a.xc = b.obs_cylinders;
    for (int k = 0; k < 3; ++k) a.ss[k] = b.self_stride[k];
    for (int k = 0; k < 4; ++k) { a.so[k] = b.others_stride[k]; a.sc[k] = b.cyl_stride[k]; }
    a.T = b.num_steps; a.steps = b.num_envs * b.num_steps;
    a.index = reinterpret_cast<const long long *>(b.index);
    a.rows = rows; a.A = num_agents; a.K = num_cylinders; a.D = self_dim; a.tiles = (int)p.tiles;
    a.inv_n = (float)(1.0 / (double)(central ? rows * num_agents : rows));   // the mean is over every value: batch A of them either way
    a.losspart = reinterpret_cast<double *>(ws + p.o_loss);
    a.tilepart = reinterpret_cast<float *>(ws + p.o_tile);
    a.P = p.P;
    a.stage = reinterpret_cast<float *>(ws + p.o_stage);
    a.stage_rows = p.stage_rows;
    return HNS_OK;
}

// the launch in front of an entry's own: the packed operand image
int ct_launch_pack(hipStream_t st, const hns::CtArgs &a, const CtPlan &p, void *workspace) {
    float *img = reinterpret_cast<float *>(static_cast<unsigned char *>(workspace) + p.o_img);
    hipLaunchKernelGGL(hns::hns_critic_pack_kernel, dim3(256), dim3(256), 0, st, a.net, a.D, img);
    HNS_CHECK_HIP(hipGetLastError());
    return HNS_OK;
}

// the launches behind them: weight gradients, the fixed-order sums into the PyTorch layouts (`ls_add`: hns_critic_reduce_kernel's; heads 0: the
// encoder op's reduce), the total norm (grad_norm NULL: not launched)
int ct_launch_tail(hipStream_t st, const hns::CtArgs &a, const CtPlan &p, const hns::CtGrad &g, void *workspace, int heads, double ls_add, float *grad_norm,
                   bool central = false) {
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    float *gpart = reinterpret_cast<float *>(ws + p.o_gemm);
    hipLaunchKernelGGL(hns::hns_critic_wgrad_kernel, dim3((unsigned)p.splits, 6), dim3(256), 0, st, a.stage, a.stage_rows, (int)p.tiles, (int)p.tps, gpart);
    HNS_CHECK_HIP(hipGetLastError());
    double *blockpart = reinterpret_cast<double *>(ws + p.o_block);
    const int nb = p.gblocks + p.tblocks;
    if (central)
        hipLaunchKernelGGL(hns::hns_critic_reduce_central_kernel, dim3(nb), dim3(256), 0, st, gpart, (int)p.splits, a.tilepart, (int)(2 * p.tiles), p.P, p.gblocks,
                           g, a.D, blockpart, a.A);
    else if (heads == 0)
        hipLaunchKernelGGL(hns::hns_encoder_reduce_kernel, dim3(nb), dim3(256), 0, st, gpart, (int)p.splits, a.tilepart, (int)(2 * p.tiles), p.P, p.gblocks, g, a.D,
                           blockpart);
    else
        hipLaunchKernelGGL(hns::hns_critic_reduce_kernel, dim3(nb), dim3(256), 0, st, gpart, (int)p.splits, a.tilepart, (int)(2 * p.tiles), p.P, p.gblocks, g,
                           a.D, blockpart, heads, ls_add);
    HNS_CHECK_HIP(hipGetLastError());
    if (!grad_norm) return HNS_OK;                              // the data-parallel entries: the local norm means nothing (hns_grad_norm after the all-reduce)
    hipLaunchKernelGGL(hns::hns_critic_norm_kernel, dim3(1), dim3(256), 0, st, blockpart, nb, grad_norm);
    HNS_CHECK_HIP(hipGetLastError());
    return HNS_OK;
}

// The critic's three entries over one body.  kCtLocal: hns_critic_train_grad — the minibatch is the whole batch.  kCtSums: pack, forward, the
// summing half (`sums` out).  kCtGlobal: pack, the deciding half on the given `sums` over `global_rows`, backward scaled by 1 / global_rows, the tail.
enum CtMode { kCtLocal, kCtSums, kCtGlobal };

int ct_critic_call(const char *fn, CtMode mode, const hns_policy_net *critic, const hns_critic_batch *batch, int32_t self_dim, int32_t num_agents,
                   int32_t num_cylinders, float clip_param, int32_t loss_kind, float huber_delta, const hns_policy_grads *grads, float *value_loss,
                   float *explained_var, float *grad_norm, float *values, double *sums, int64_t global_rows, void *workspace, size_t workspace_bytes,
                   void *stream) {
    if (int rc = ct_check_shape(fn, *batch, self_dim, num_agents, num_cylinders)) return rc;
    if (loss_kind != HNS_CRITIC_LOSS_HUBER && loss_kind != HNS_CRITIC_LOSS_MSE) return hns_fail(fn, "loss_kind must be HNS_CRITIC_LOSS_HUBER or HNS_CRITIC_LOSS_MSE");
    if (!(clip_param >= 0.0f) || (loss_kind == HNS_CRITIC_LOSS_HUBER && !(huber_delta > 0.0f))) return hns_fail(fn, "clip_param >= 0, huber_delta > 0");
    if (mode == kCtGlobal && global_rows < batch->batch * num_agents) return hns_fail(fn, "global_rows must be >= this rank's rows (batch x num_agents)");
    hns::CtArgs a{};
    hns::CtGrad g{};
    CtPlan p;
    if (int rc = ct_bind_net(fn, *critic, grads, num_agents > 1, 1, a.net, g)) return rc;
    if (int rc = ct_check_obs(fn, *batch, num_agents > 1)) return rc;
    if (!batch->b_values || !batch->b_returns || !hns_aligned(batch->b_values, 4) || !hns_aligned(batch->b_returns, 4)) return hns_fail(fn, "b_values / b_returns missing or misaligned");
    if (int rc = ct_plan_call(fn, *batch, {value_loss, explained_var, grad_norm, values}, workspace, workspace_bytes, self_dim, num_agents, num_cylinders, 1, p, a)) return rc;
    float *ctl = reinterpret_cast<float *>(static_cast<unsigned char *>(workspace) + p.o_ctl);
    a.bval = batch->b_values; a.bret = batch->b_returns;
    a.clip = clip_param; a.delta = huber_delta; a.mse = loss_kind == HNS_CRITIC_LOSS_MSE;
    a.values = values;
    a.ctl = ctl;
    if (mode == kCtGlobal) a.inv_n = (float)(1.0 / (double)global_rows);

    const hipStream_t st = static_cast<hipStream_t>(stream);
    static const hipError_t attr_f = hipFuncSetAttribute(reinterpret_cast<const void *>(&hns::hns_critic_kernel<false>),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)hns::kCtLdsFwd);
    static const hipError_t attr_b = hipFuncSetAttribute(reinterpret_cast<const void *>(&hns::hns_critic_kernel<true>),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(hns::CtLds));
    HNS_CHECK_HIP(attr_f);
    HNS_CHECK_HIP(attr_b);
    if (int rc = ct_launch_pack(st, a, p, workspace)) return rc;
    if (mode != kCtGlobal) {
        hipLaunchKernelGGL(hns::hns_critic_kernel<false>, dim3((unsigned)p.tiles), dim3(hns::kCtThreads), hns::kCtLdsFwd, st, a);
        HNS_CHECK_HIP(hipGetLastError());
    }
    if (mode == kCtLocal) hipLaunchKernelGGL(hns::hns_critic_loss_kernel, dim3(1), dim3(256), 0, st, a.losspart, (int)p.tiles, (double)a.rows, ctl, value_loss, explained_var);
    else if (mode == kCtSums) hipLaunchKernelGGL(hns::hns_critic_sums_kernel, dim3(1), dim3(256), 0, st, a.losspart, (int)p.tiles, sums);
    else hipLaunchKernelGGL(hns::hns_critic_decide_kernel, dim3(1), dim3(64), 0, st, sums, (double)global_rows, ctl, value_loss, explained_var);
    HNS_CHECK_HIP(hipGetLastError());
    if (mode == kCtSums) return HNS_OK;
    hipLaunchKernelGGL(hns::hns_critic_kernel<true>, dim3((unsigned)p.tiles), dim3(hns::kCtThreads), sizeof(hns::CtLds), st, a);
    HNS_CHECK_HIP(hipGetLastError());
    return ct_launch_tail(st, a, p, g, workspace, 1, 0.0, grad_norm);
}

// hns_critic_train_grad_central: ct_critic_call's local mode on tiles of env-steps — the same refusals in the same order (the state has no
// state_others: a pointer there is refused), the same launches with the central tile and reduce kernels, the loss over batch A values
int ct_critic_central_call(const char *fn, const hns_policy_net *critic, const hns_critic_batch *batch, int32_t self_dim, int32_t num_agents,
                           int32_t num_cylinders, float clip_param, int32_t loss_kind, float huber_delta, const hns_policy_grads *grads, float *value_loss,
                           float *explained_var, float *grad_norm, float *values, void *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = ct_check_shape(fn, *batch, self_dim, num_agents, num_cylinders)) return rc;
    if (loss_kind != HNS_CRITIC_LOSS_HUBER && loss_kind != HNS_CRITIC_LOSS_MSE) return hns_fail(fn, "loss_kind must be HNS_CRITIC_LOSS_HUBER or HNS_CRITIC_LOSS_MSE");
    if (!(clip_param >= 0.0f) || (loss_kind == HNS_CRITIC_LOSS_HUBER && !(huber_delta > 0.0f))) return hns_fail(fn, "clip_param >= 0, huber_delta > 0");
    if (critic->embed_others_w || critic->embed_others_b || batch->obs_others) return hns_fail(fn, "the centralised critic has no state_others (embedding and obs_others must be NULL)");
    hns::CtArgs a{};
    hns::CtGrad g{};
    CtPlan p;
    if (int rc = ct_bind_net(fn, *critic, grads, false, 1, a.net, g)) return rc;
    if (int rc = ct_check_obs(fn, *batch, false)) return rc;
    if (!batch->b_values || !batch->b_returns || !hns_aligned(batch->b_values, 4) || !hns_aligned(batch->b_returns, 4)) return hns_fail(fn, "b_values / b_returns missing or misaligned");
    if (int rc = ct_plan_call(fn, *batch, {value_loss, explained_var, grad_norm, values}, workspace, workspace_bytes, self_dim, num_agents, num_cylinders, 1, p, a,
                              true, false, true))
        return rc;
    float *ctl = reinterpret_cast<float *>(static_cast<unsigned char *>(workspace) + p.o_ctl);
    a.bval = batch->b_values; a.bret = batch->b_returns;
    a.clip = clip_param; a.delta = huber_delta; a.mse = loss_kind == HNS_CRITIC_LOSS_MSE;
    a.values = values;
    a.ctl = ctl;

    const hipStream_t st = static_cast<hipStream_t>(stream);
    static const hipError_t attr_f = hipFuncSetAttribute(reinterpret_cast<const void *>(&hns::hns_critic_central_kernel<false>),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)hns::kCtLdsFwd);
    static const hipError_t attr_b = hipFuncSetAttribute(reinterpret_cast<const void *>(&hns::hns_critic_central_kernel<true>),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(hns::CtLds));
    HNS_CHECK_HIP(attr_f);
    HNS_CHECK_HIP(attr_b);
    if (int rc = ct_launch_pack(st, a, p, workspace)) return rc;
    hipLaunchKernelGGL(hns::hns_critic_central_kernel<false>, dim3((unsigned)p.tiles), dim3(hns::kCtThreads), hns::kCtLdsFwd, st, a);
    HNS_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(hns::hns_critic_loss_kernel, dim3(1), dim3(256), 0, st, a.losspart, (int)p.tiles, (double)(a.rows * a.A), ctl, value_loss, explained_var);
    HNS_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(hns::hns_critic_central_kernel<true>, dim3((unsigned)p.tiles), dim3(hns::kCtThreads), sizeof(hns::CtLds), st, a);
    HNS_CHECK_HIP(hipGetLastError());
    return ct_launch_tail(st, a, p, g, workspace, 1, 0.0, grad_norm, true);
}

// The actor's two entries over one body.  global: the rows' backward weight and policy_loss are scaled by 1 / global_rows instead of 1 / rows (this
// rank's share of the loss and of the gradient: the ranks' shares add up), the entropy term's constant gradient joins by `entropy_share` of it.
// `agents`: hns_actor_train_grad_agents — `actor` and `grads` hold the stacked tensors, every launch but the weight gradients' and the norm's is the
// per-agent kernel (same order, same count).  Both flags: hns_actor_train_grad_agents_global — the same launches with the global scalars (f32(1 /
// global_rows) on the rows, n = global_rows in the loss kernel, (-entropy_coef entropy_share) / A on each agent's d log_std); no kernel of its own.
int ct_actor_call(const char *fn, bool global, bool agents, const hns_policy_net *actor, const hns_actor_batch *batch, int32_t self_dim, int32_t num_agents,
                  int32_t num_cylinders, double clip_param, double entropy_coef, const hns_policy_grads *grads, float *policy_loss, float *entropy, float *ess,
                  float *grad_norm, float *log_probs, int64_t global_rows, double entropy_share, void *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = ct_check_shape(fn, *batch, self_dim, num_agents, num_cylinders)) return rc;
    if (!(clip_param >= 0.0) || !std::isfinite(clip_param) || !std::isfinite(entropy_coef)) return hns_fail(fn, "clip_param >= 0 and a finite entropy_coef");
    if (global && global_rows < batch->batch * num_agents) return hns_fail(fn, "global_rows must be >= this rank's rows (batch x num_agents)");
    if (global && !std::isfinite(entropy_share)) return hns_fail(fn, "entropy_share must be finite (1 / world)");
    hns::CtArgs a{};
    hns::CtGrad g{};
    CtPlan p;
    if (int rc = ct_bind_net(fn, *actor, grads, num_agents > 1, hns::kActDim, a.net, g)) return rc;
    if (int rc = ct_check_obs(fn, *batch, num_agents > 1)) return rc;
    if (!batch->action || !batch->log_probs_old || !batch->advantages || !hns_aligned(batch->action, 4) || !hns_aligned(batch->log_probs_old, 4) ||
        !hns_aligned(batch->advantages, 4))
        return hns_fail(fn, "action / log_probs_old / advantages missing or misaligned");
    if (int rc = ct_plan_call(fn, *batch, {policy_loss, entropy, ess, grad_norm, log_probs}, workspace, workspace_bytes, self_dim, num_agents, num_cylinders,
                              hns::kActDim, p, a, true, agents))
        return rc;
    a.logp_old = batch->log_probs_old; a.adv = batch->advantages; a.action = batch->action;
    a.clip_lo = (float)(1.0 - clip_param); a.clip_hi = (float)(1.0 + clip_param);
    a.logp_new = log_probs;
    if (global) a.inv_n = (float)(1.0 / (double)global_rows);

    const hipStream_t st = static_cast<hipStream_t>(stream);
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&hns::hns_critic_kernel<true, hns::kActDim>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(hns::CtLds));
    static const hipError_t attr_ag = hipFuncSetAttribute(reinterpret_cast<const void *>(&hns::hns_actor_agents_kernel),
                                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(hns::CtLds));
    HNS_CHECK_HIP(attr);
    HNS_CHECK_HIP(attr_ag);
    if (agents) {
        const int A = num_agents, nb = p.gblocks + p.tblocks;
        unsigned char *ws = static_cast<unsigned char *>(workspace);
        hipLaunchKernelGGL(hns::hns_actor_pack_agents_kernel, dim3(256, A), dim3(256), 0, st, a.net, a.D, reinterpret_cast<float *>(ws + p.o_img));
        HNS_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(hns::hns_actor_agents_kernel, dim3((unsigned)(p.tiles / A), A), dim3(hns::kCtThreads), sizeof(hns::CtLds), st, a);
        HNS_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(hns::hns_actor_loss_agents_kernel, dim3(1), dim3(64), 0, st, a.losspart, (int)p.tiles, A, (double)(global ? global_rows : a.rows),
                           (double)batch->batch, actor->log_std, policy_loss, entropy, ess);
        HNS_CHECK_HIP(hipGetLastError());
        float *gpart = reinterpret_cast<float *>(ws + p.o_gemm);
        hipLaunchKernelGGL(hns::hns_critic_wgrad_kernel, dim3((unsigned)p.splits, 6), dim3(256), 0, st, a.stage, a.stage_rows, (int)p.tiles, (int)p.tps, gpart);
        HNS_CHECK_HIP(hipGetLastError());
        double *blockpart = reinterpret_cast<double *>(ws + p.o_block);
        // each agent's d log_std takes its share of the mean entropy's constant gradient (global: this rank's entropy_share of it, formed before the
        // division so that a share of 1 leaves the local entry's constant)
        hipLaunchKernelGGL(hns::hns_actor_reduce_agents_kernel, dim3(nb, A), dim3(256), 0, st, gpart, (int)(p.splits / A), a.tilepart, (int)(2 * p.tiles / A), p.P,
                           p.gblocks, g, a.D, blockpart, (global ? -entropy_coef * entropy_share : -entropy_coef) / (double)A);
        HNS_CHECK_HIP(hipGetLastError());
        if (!grad_norm) return HNS_OK;                          // the data-parallel entry: hns_grad_norm after the all-reduce
        hipLaunchKernelGGL(hns::hns_critic_norm_kernel, dim3(1), dim3(256), 0, st, blockpart, nb * A, grad_norm);
        HNS_CHECK_HIP(hipGetLastError());
        return HNS_OK;
    }
    if (int rc = ct_launch_pack(st, a, p, workspace)) return rc;
    hipLaunchKernelGGL((hns::hns_critic_kernel<true, hns::kActDim>), dim3((unsigned)p.tiles), dim3(hns::kCtThreads), sizeof(hns::CtLds), st, a);
    HNS_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(hns::hns_actor_loss_kernel, dim3(1), dim3(64), 0, st, a.losspart, (int)p.tiles, (int)num_agents, (double)(global ? global_rows : a.rows),
                       (double)batch->batch, actor->log_std, policy_loss, entropy, ess);
    HNS_CHECK_HIP(hipGetLastError());
    return ct_launch_tail(st, a, p, g, workspace, hns::kActDim, global ? -entropy_coef * entropy_share : -entropy_coef, grad_norm);
}

// The encoder op's two entries over one body.  Forward: pack, the tile kernel without a head.  Backward: pack, the tile kernel from d features, the
// weight gradients and the reduce without the head's destinations; no norm.
int ct_encoder_call(const char *fn, bool backward, bool agents, const hns_policy_net *net, const hns_critic_batch *batch, int32_t self_dim, int32_t num_agents,
                    int32_t num_cylinders, float *features, const float *dfeatures, const hns_policy_grads *grads, void *workspace, size_t workspace_bytes,
                    void *stream) {
    if (int rc = ct_check_shape(fn, *batch, self_dim, num_agents, num_cylinders)) return rc;
    hns::CtArgs a{};
    hns::CtGrad g{};
    CtPlan p;
    if (int rc = ct_bind_net(fn, *net, grads, num_agents > 1, 0, a.net, g)) return rc;
    if (int rc = ct_check_obs(fn, *batch, num_agents > 1)) return rc;
    if (!hns_aligned(backward ? dfeatures : features, 16)) return hns_fail(fn, backward ? "misaligned dfeatures (16 bytes)" : "misaligned features (16 bytes)");
    if (int rc = ct_plan_call(fn, *batch, {}, workspace, workspace_bytes, self_dim, num_agents, num_cylinders, 0, p, a, backward, agents)) return rc;
    if (backward) a.dfeat = dfeatures;
    else a.feat = features;

    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (agents) {
        static const hipError_t ag_f = hipFuncSetAttribute(reinterpret_cast<const void *>(&hns::hns_encoder_agents_kernel<false>),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)hns::kCtLdsFwd);
        static const hipError_t ag_b = hipFuncSetAttribute(reinterpret_cast<const void *>(&hns::hns_encoder_agents_kernel<true>),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(hns::CtLds));
        HNS_CHECK_HIP(ag_f);
        HNS_CHECK_HIP(ag_b);
        const int A = num_agents, nb = p.gblocks + p.tblocks;
        unsigned char *ws = static_cast<unsigned char *>(workspace);
        hipLaunchKernelGGL(hns::hns_actor_pack_agents_kernel, dim3(256, A), dim3(256), 0, st, a.net, a.D, reinterpret_cast<float *>(ws + p.o_img));
        HNS_CHECK_HIP(hipGetLastError());
        if (!backward) {
            const unsigned live = (unsigned)((batch->batch + hns::kCtRows - 1) / hns::kCtRows);
            hipLaunchKernelGGL(hns::hns_encoder_agents_kernel<false>, dim3(live, A), dim3(hns::kCtThreads), hns::kCtLdsFwd, st, a);
            HNS_CHECK_HIP(hipGetLastError());
            return HNS_OK;
        }
        hipLaunchKernelGGL(hns::hns_encoder_agents_kernel<true>, dim3((unsigned)(p.tiles / A), A), dim3(hns::kCtThreads), sizeof(hns::CtLds), st, a);
        HNS_CHECK_HIP(hipGetLastError());
        float *gpart = reinterpret_cast<float *>(ws + p.o_gemm);
        hipLaunchKernelGGL(hns::hns_critic_wgrad_kernel, dim3((unsigned)p.splits, 6), dim3(256), 0, st, a.stage, a.stage_rows, (int)p.tiles, (int)p.tps, gpart);
        HNS_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(hns::hns_encoder_reduce_agents_kernel, dim3(nb, A), dim3(256), 0, st, gpart, (int)(p.splits / A), a.tilepart, (int)(2 * p.tiles / A), p.P,
                           p.gblocks, g, a.D, reinterpret_cast<double *>(ws + p.o_block));
        HNS_CHECK_HIP(hipGetLastError());
        return HNS_OK;
    }
    static const hipError_t attr_f = hipFuncSetAttribute(reinterpret_cast<const void *>(&hns::hns_critic_kernel<false, 0>),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)hns::kCtLdsFwd);
    static const hipError_t attr_b = hipFuncSetAttribute(reinterpret_cast<const void *>(&hns::hns_critic_kernel<true, 0>),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(hns::CtLds));
    HNS_CHECK_HIP(attr_f);
    HNS_CHECK_HIP(attr_b);
    if (int rc = ct_launch_pack(st, a, p, workspace)) return rc;
    if (!backward) {
        hipLaunchKernelGGL((hns::hns_critic_kernel<false, 0>), dim3((unsigned)p.tiles), dim3(hns::kCtThreads), hns::kCtLdsFwd, st, a);
        HNS_CHECK_HIP(hipGetLastError());
        return HNS_OK;
    }
    hipLaunchKernelGGL((hns::hns_critic_kernel<true, 0>), dim3((unsigned)p.tiles), dim3(hns::kCtThreads), sizeof(hns::CtLds), st, a);
    HNS_CHECK_HIP(hipGetLastError());
    return ct_launch_tail(st, a, p, g, workspace, 0, 0.0, nullptr);
}

}  // namespace

extern "C" {

size_t hns_critic_train_workspace_bytes(int64_t rows, int32_t self_dim, int32_t num_agents, int32_t num_cylinders) {
    CtPlan p;
    return ct_plan(rows, self_dim, num_agents, num_cylinders, p) ? p.total : 0;
}

int hns_critic_train_grad(const hns_policy_net *critic, const hns_critic_batch *batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders,
                          float clip_param, int32_t loss_kind, float huber_delta, const hns_policy_grads *grads, float *value_loss,
                          float *explained_var, float *grad_norm, float *values, void *workspace, size_t workspace_bytes, void *stream) {
    const char *fn = "hns_critic_train_grad";
    if (!critic || !batch || !grads || !value_loss || !explained_var || !grad_norm || !workspace) return hns_fail(fn, "null pointer");
    return ct_critic_call(fn, kCtLocal, critic, batch, self_dim, num_agents, num_cylinders, clip_param, loss_kind, huber_delta, grads, value_loss, explained_var,
                          grad_norm, values, nullptr, 0, workspace, workspace_bytes, stream);
}

int hns_critic_train_sums(const hns_policy_net *critic, const hns_critic_batch *batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders,
                          float clip_param, int32_t loss_kind, float huber_delta, double *sums, float *values, void *workspace, size_t workspace_bytes,
                          void *stream) {
    const char *fn = "hns_critic_train_sums";
    if (!critic || !batch || !sums || !workspace) return hns_fail(fn, "null pointer");
    if (!hns_aligned(sums, 8)) return hns_fail(fn, "misaligned sums (five fp64 values, 8-byte aligned)");
    return ct_critic_call(fn, kCtSums, critic, batch, self_dim, num_agents, num_cylinders, clip_param, loss_kind, huber_delta, nullptr, nullptr, nullptr, nullptr,
                          values, sums, 0, workspace, workspace_bytes, stream);
}

int hns_critic_train_grad_global(const hns_policy_net *critic, const hns_critic_batch *batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders,
                                 float clip_param, int32_t loss_kind, float huber_delta, const hns_policy_grads *grads, float *value_loss,
                                 float *explained_var, float *grad_norm, float *values, void *workspace, size_t workspace_bytes, void *stream,
                                 const double *sums, int64_t global_rows) {
    const char *fn = "hns_critic_train_grad_global";
    if (!critic || !batch || !grads || !value_loss || !explained_var || !workspace || !sums) return hns_fail(fn, "null pointer");
    if (!hns_aligned(sums, 8)) return hns_fail(fn, "misaligned sums (five fp64 values, 8-byte aligned)");
    return ct_critic_call(fn, kCtGlobal, critic, batch, self_dim, num_agents, num_cylinders, clip_param, loss_kind, huber_delta, grads, value_loss, explained_var,
                          grad_norm, values, const_cast<double *>(sums), global_rows, workspace, workspace_bytes, stream);
}

size_t hns_critic_train_central_workspace_bytes(int64_t batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders) {
    CtPlan p;
    return ct_plan(batch, self_dim, num_agents, num_cylinders, p, 1, true) ? p.total : 0;
}

int hns_critic_train_grad_central(const hns_policy_net *critic, const hns_critic_batch *batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders,
                                  float clip_param, int32_t loss_kind, float huber_delta, const hns_policy_grads *grads, float *value_loss,
                                  float *explained_var, float *grad_norm, float *values, void *workspace, size_t workspace_bytes, void *stream) {
    const char *fn = "hns_critic_train_grad_central";
    if (!critic || !batch || !grads || !value_loss || !explained_var || !grad_norm || !workspace) return hns_fail(fn, "null pointer");
    return ct_critic_central_call(fn, critic, batch, self_dim, num_agents, num_cylinders, clip_param, loss_kind, huber_delta, grads, value_loss, explained_var,
                                  grad_norm, values, workspace, workspace_bytes, stream);
}

size_t hns_actor_train_workspace_bytes(int64_t rows, int32_t self_dim, int32_t num_agents, int32_t num_cylinders) {
    CtPlan p;
    return ct_plan(rows, self_dim, num_agents, num_cylinders, p, hns::kActDim) ? p.total : 0;
}

int hns_actor_train_grad(const hns_policy_net *actor, const hns_actor_batch *batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders,
                         double clip_param, double entropy_coef, const hns_policy_grads *grads, float *policy_loss, float *entropy, float *ess,
                         float *grad_norm, float *log_probs, void *workspace, size_t workspace_bytes, void *stream) {
    const char *fn = "hns_actor_train_grad";
    if (!actor || !batch || !grads || !policy_loss || !entropy || !ess || !grad_norm || !workspace) return hns_fail(fn, "null pointer");
    return ct_actor_call(fn, false, false, actor, batch, self_dim, num_agents, num_cylinders, clip_param, entropy_coef, grads, policy_loss, entropy, ess, grad_norm,
                         log_probs, 0, 1.0, workspace, workspace_bytes, stream);
}

int hns_actor_train_grad_global(const hns_policy_net *actor, const hns_actor_batch *batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders,
                                double clip_param, double entropy_coef, const hns_policy_grads *grads, float *policy_loss, float *entropy, float *ess,
                                float *grad_norm, float *log_probs, void *workspace, size_t workspace_bytes, void *stream, int64_t global_rows,
                                double entropy_share) {
    const char *fn = "hns_actor_train_grad_global";
    if (!actor || !batch || !grads || !policy_loss || !entropy || !ess || !workspace) return hns_fail(fn, "null pointer");
    return ct_actor_call(fn, true, false, actor, batch, self_dim, num_agents, num_cylinders, clip_param, entropy_coef, grads, policy_loss, entropy, ess, grad_norm,
                         log_probs, global_rows, entropy_share, workspace, workspace_bytes, stream);
}

size_t hns_actor_train_agents_workspace_bytes(int64_t rows, int32_t self_dim, int32_t num_agents, int32_t num_cylinders) {
    CtPlan p;
    return ct_plan_agents(rows, self_dim, num_agents, num_cylinders, p) ? p.total : 0;
}

int hns_actor_train_grad_agents(const hns_policy_net *actors, const hns_actor_batch *batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders,
                                double clip_param, double entropy_coef, const hns_policy_grads *grads, float *policy_loss, float *entropy, float *ess,
                                float *grad_norm, float *log_probs, void *workspace, size_t workspace_bytes, void *stream) {
    const char *fn = "hns_actor_train_grad_agents";
    if (!actors || !batch || !grads || !policy_loss || !entropy || !ess || !grad_norm || !workspace) return hns_fail(fn, "null pointer");
    return ct_actor_call(fn, false, true, actors, batch, self_dim, num_agents, num_cylinders, clip_param, entropy_coef, grads, policy_loss, entropy, ess,
                         grad_norm, log_probs, 0, 1.0, workspace, workspace_bytes, stream);
}

int hns_actor_train_grad_agents_global(const hns_policy_net *actors, const hns_actor_batch *batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders,
                                       double clip_param, double entropy_coef, const hns_policy_grads *grads, float *policy_loss, float *entropy, float *ess,
                                       float *grad_norm, float *log_probs, void *workspace, size_t workspace_bytes, void *stream, int64_t global_rows,
                                       double entropy_share) {
    const char *fn = "hns_actor_train_grad_agents_global";
    if (!actors || !batch || !grads || !policy_loss || !entropy || !ess || !workspace) return hns_fail(fn, "null pointer");
    return ct_actor_call(fn, true, true, actors, batch, self_dim, num_agents, num_cylinders, clip_param, entropy_coef, grads, policy_loss, entropy, ess,
                         grad_norm, log_probs, global_rows, entropy_share, workspace, workspace_bytes, stream);
}

size_t hns_encoder_workspace_bytes(int64_t rows, int32_t self_dim, int32_t num_agents, int32_t num_cylinders, int32_t backward) {
    CtPlan p;
    return ct_plan_encoder(rows, self_dim, num_agents, num_cylinders, backward != 0, p) ? p.total : 0;
}

int hns_encoder_forward(const hns_policy_net *net, const hns_critic_batch *batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders,
                        float *features, void *workspace, size_t workspace_bytes, void *stream) {
    const char *fn = "hns_encoder_forward";
    if (!net || !batch || !features || !workspace) return hns_fail(fn, "null pointer");
    return ct_encoder_call(fn, false, false, net, batch, self_dim, num_agents, num_cylinders, features, nullptr, nullptr, workspace, workspace_bytes, stream);
}

int hns_encoder_backward(const hns_policy_net *net, const hns_critic_batch *batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders,
                         const float *dfeatures, const hns_policy_grads *grads, void *workspace, size_t workspace_bytes, void *stream) {
    const char *fn = "hns_encoder_backward";
    if (!net || !batch || !dfeatures || !grads || !workspace) return hns_fail(fn, "null pointer");
    return ct_encoder_call(fn, true, false, net, batch, self_dim, num_agents, num_cylinders, nullptr, dfeatures, grads, workspace, workspace_bytes, stream);
}

size_t hns_encoder_agents_workspace_bytes(int64_t rows, int32_t self_dim, int32_t num_agents, int32_t num_cylinders, int32_t backward) {
    CtPlan p;
    return ct_plan_encoder_agents(rows, self_dim, num_agents, num_cylinders, backward != 0, p) ? p.total : 0;
}

int hns_encoder_forward_agents(const hns_policy_net *nets, const hns_critic_batch *batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders,
                               float *features, void *workspace, size_t workspace_bytes, void *stream) {
    const char *fn = "hns_encoder_forward_agents";
    if (!nets || !batch || !features || !workspace) return hns_fail(fn, "null pointer");
    return ct_encoder_call(fn, false, true, nets, batch, self_dim, num_agents, num_cylinders, features, nullptr, nullptr, workspace, workspace_bytes, stream);
}

int hns_encoder_backward_agents(const hns_policy_net *nets, const hns_critic_batch *batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders,
                                const float *dfeatures, const hns_policy_grads *grads, void *workspace, size_t workspace_bytes, void *stream) {
    const char *fn = "hns_encoder_backward_agents";
    if (!nets || !batch || !dfeatures || !grads || !workspace) return hns_fail(fn, "null pointer");
    return ct_encoder_call(fn, true, true, nets, batch, self_dim, num_agents, num_cylinders, nullptr, dfeatures, grads, workspace, workspace_bytes, stream);
}

}  // extern "C"
