// hns_policy.hip — the MAPPO actor and critic forward pass on the device (collector step, evaluation, train_op's next_value).
//
// Reference: MAPPOPolicy.__call__ + value_op (omni_drones/learning/mappo.py:221-250) with cfg/algo/mappo.yaml's defaults (share_actor, critic_input obs,
// no rnn, tanh false): make_encoder's composite branch (learning/common.py) builds a PartialAttentionEncoder (modules/networks.py:250-313) per
// network — SplitEmbedding (one Linear(in, 128) per key in spec order state_self, state_others, cylinders; one LayerNorm(128) over every token),
// single-query nn.MultiheadAttention (one head, packed in_proj), x0' = LN1(x0 + attn), y = LN2(x0' + W2 gelu(W1 x0' + b1) + b2) — then
// DiagGaussian (modules/distributions.py:66-82: loc = fc_mean(y), scale = exp(log_std)) for the actor and v_out = Linear(128, 1) for the critic.
//
// Single-query algebra: with q = W_q t_0 + b_q the score of token j is q.(W_k t_j + b_k) / sqrt(128) = (W_k^T q / sqrt(128)).t_j
// plus a term that is the same for every j and cancels in the softmax, and sum_j a_j (W_v t_j + b_v) = W_v (sum_j a_j t_j) + b_v.  Per row and
// network that leaves six 128 x 128 matrix-vector products (W_q, W_k^T, W_v, W_o, W_1, W_2), which run on v_mfma_f32_16x16x4_f32 for a tile of
// kEncRows rows at a time, and a token pass on the VALU (embedding, LayerNorm, score, online softmax, weighted sum) that never stores a token.
//
// The encoder's shared pieces — tile shape, matrix-vector product, LayerNorm, token embedding, online-softmax step, the parameter table and the
// matrices' fragment order — are hns_encoder.h's, which hns_policy_train.hip uses too.  Here: the packed image's vector sections, the head,
// sampling, the log-probability, the entry points.
//
// The tile (pol_tile): one workgroup of four waves per kEncRows rows.  Activations live in LDS as [128 features][kEncRows rows]; wave w owns
// output row blocks 2w, 2w + 1 of every product, so each weight element is read once per workgroup.  The embedding starts its fma chain from the
// bias (enc_token<true>; the updates add it last: DESIGN §7.3).  Per network: pol_encoder, [one GRU step], the head.  Eight kernels are that ONE
// body under three compile-time flags — the same tile, LDS (PolLds, taken dynamically) and launch bounds, the same per-row device functions in
// the same order, so what two of them both compute has the same bits:
//   AGENTS : one actor per agent (share_actor: false).  The image holds A actor images, then the critic's; a workgroup's
//            rows are 32 consecutive envs of ONE agent (blockIdx.y) and its actor pass reads that agent's image(s).  A row keeps its number
//            e A + a (outputs, eps, the Philox counter, the state rows: pol_gru_step<true>), so row (e, a) has the shared kernel's bits with
//            agent a's image(s) as the actor.  Without the flag rows are tiled as they lie and the image is [actor, critic].
//   RNN    : the recurrent configuration (actor.rnn / critic.rnn: a GRU behind each encoder).  ONE GRU step on the features the
//            encoder left in registers (six more 128 x 128 products from a second packed image, the gates in the products' accumulator
//            layout), LayerNorm(h + f), then the head.  The state comes from and goes to HBM once per network; the features never do.
//   ACT    : the actor's pass alone, action = loc (and the actor's new state) and nothing else read or written: evaluation reads neither the
//            value nor the log-probability.  Bit for bit the forward's deterministic action (and actor state).
//
//   kernel                                  AGENTS  RNN  ACT
//   hns_policy_forward_kernel                  -     -    -
//   hns_policy_act_kernel                      -     -    x
//   hns_policy_forward_rnn_kernel              -     x    -
//   hns_policy_act_rnn_kernel                  -     x    x
//   hns_policy_forward_agents_kernel           x     -    -
//   hns_policy_act_agents_kernel               x     -    x
//   hns_policy_forward_rnn_agents_kernel       x     x    -
//   hns_policy_act_rnn_agents_kernel           x     x    x
//
//   hns_policy_pack_agents_kernel     : parameter tensors (PyTorch layouts) -> packed images, one per blockIdx.y: the six matrices in MFMA A-operand
//                                       fragment order (one float4 per lane per four k-steps), the vectors, the head, the embedding weights
//                                       transposed.  The shared image [actor, critic] is the per-agent image [A actors, critic] at one actor.
//   hns_policy_rnn_pack_agents_kernel : the GRUs' tensors -> their packed images, the same way.
//   hns_policy_forward_central_kernel : the centralised critic's configuration (critic_input: state): the grid is the shared
//                                       actor's tiles — pol_tile's actor pass — followed by the critic's tiles of 32 ENVS on pol_encoder<true>
//                                       (the state's tokens) and a head of A rows; hns_policy_pack_central_kernel builds its image.
//   hns_policy_forward_central_agents_kernel : both at once (share_actor: false with critic_input: state): the grid is
//                                       dim3(tiles of 32 envs, A + 1) — blockIdx.y < A is agent blockIdx.y's range, pol_tile<AGENTS>'s actor
//                                       pass on that agent's image, and blockIdx.y == A the centralised critic's range, the kernel above's
//                                       critic branch; hns_policy_pack_central_agents_kernel builds its image [A actors, the central critic].
//   hns_policy_bump_kernel            : the device call counter += 1 after a sampling call (Philox counter; a captured graph draws fresh noise
//                                       per replay).
// Determinism: fixed reduction orders (butterflies over the eight lanes of a row), no atomics.
#include <hip/hip_runtime.h>

#include <string>

#include "hns_device.h"
#include "hns_encoder.h"
#include "hns_host.h"
#include "../../include/hns.h"

namespace hns {

constexpr int kPolMaxSelf = HNS_POLICY_MAX_SELF_DIM;

// packed network image, in floats (every section a multiple of 4 floats: float4 loads)
enum : int {
    P_MAT = 0,                               // 6 matrices: Q, K^T, V, O, L1, L2 (fragment order)
    P_BQ = 6 * kEncMat, P_BV = P_BQ + kEncE, P_BO = P_BV + kEncE, P_B1 = P_BO + kEncE, P_B2 = P_B1 + kEncE,
    P_LNW = P_B2 + kEncE, P_LNB = P_LNW + kEncE, P_N1W = P_LNB + kEncE, P_N1B = P_N1W + kEncE, P_N2W = P_N1B + kEncE, P_N2B = P_N2W + kEncE,
    P_EB = P_N2B + kEncE,                    // embedding biases [3][128]: self, others, cylinders
    P_HW = P_EB + 3 * kEncE,                 // head weight [4][128] (the critic: row 0)
    P_HB = P_HW + 4 * kEncE,                 // head bias [4]
    P_SCALE = P_HB + 4,                      // exp(log_std) [4]
    P_LOGSCALE = P_SCALE + 4,                // log(scale) [4]
    P_EW = P_LOGSCALE + 4,                   // embedding weights transposed: self [D][128], others [3][128], cylinders [5][128]
};
static __host__ __device__ __forceinline__ long long pol_net_floats(int D) { return P_EW + (long long)(D + 8) * kEncE; }

// source value of image float i of one network
HNS_DEV float pol_src(const EncNet &s, int D, long long i) {
    if (i < P_BQ) return enc_mat_src(s, (int)(i / kEncMat), (int)(i % kEncMat));
    const int j = (int)(i - P_BQ);
    if (i < P_EB) {
        const int sec = j / kEncE, f = j % kEncE;
        switch (sec) {
            case 0: return s.in_b[f];
            case 1: return s.in_b[2 * kEncE + f];
            case 2: return s.out_b[f];
            case 3: return s.l1_b[f];
            case 4: return s.l2_b[f];
            case 5: return s.ln_w[f];
            case 6: return s.ln_b[f];
            case 7: return s.n1_w[f];
            case 8: return s.n1_b[f];
            case 9: return s.n2_w[f];
            default: return s.n2_b[f];
        }
    }
    if (i < P_HW) {
        const int key = (int)((i - P_EB) / kEncE), f = (int)((i - P_EB) % kEncE);
        return s.eb[key] ? s.eb[key][f] : 0.0f;
    }
    if (i < P_HB) {
        const int o = (int)((i - P_HW) / kEncE), f = (int)((i - P_HW) % kEncE);
        return o < s.head_n ? s.head_w[o * kEncE + f] : 0.0f;
    }
    if (i < P_SCALE) return (int)(i - P_HB) < s.head_n ? s.head_b[i - P_HB] : 0.0f;
    if (i < P_LOGSCALE) return s.log_std ? expf(s.log_std[i - P_SCALE]) : 1.0f;
    if (i < P_EW) return s.log_std ? logf(expf(s.log_std[i - P_LOGSCALE])) : 0.0f;   // torch Normal: scale.log()
    const long long e = i - P_EW;
    const int in = (int)(e / kEncE), f = (int)(e % kEncE);
    if (in < D) return s.ew[0][f * D + in];
    if (in < D + 3) return s.ew[1] ? s.ew[1][f * 3 + (in - D)] : 0.0f;
    return s.ew[2][f * 5 + (in - D - 3)];
}

// the centralised critic's image (critic_input: state), in floats: a network's sections up to its embedding biases (the
// state_others slot zeros: the state has no such key), then a head of up to seven rows and the two embeddings it has
enum : int {
    C_HW = P_HW,                             // head weight [8][128]: v_out's A rows, zeros behind them
    C_HB = C_HW + 8 * kEncE,                 // head bias [8]
    C_EW = C_HB + 8,                         // embedding weights transposed: state_drones [D][128], cylinders [5][128]
};
static __host__ __device__ __forceinline__ long long pol_central_floats(int D) { return C_EW + (long long)(D + 5) * kEncE; }

HNS_DEV float pol_central_src(const EncNet &s, int D, long long i) {
    if (i < C_HW) return pol_src(s, D, i);
    if (i < C_HB) {
        const int o = (int)((i - C_HW) / kEncE), f = (int)((i - C_HW) % kEncE);
        return o < s.head_n ? s.head_w[o * kEncE + f] : 0.0f;
    }
    if (i < C_EW) return (int)(i - C_HB) < s.head_n ? s.head_b[i - C_HB] : 0.0f;
    const long long e = i - C_EW;
    const int in = (int)(e / kEncE), f = (int)(e % kEncE);
    return in < D ? s.ew[0][f * D + in] : s.ew[2][f * 5 + (in - D)];
}

struct PolNets {
    EncNet n[HNS_MAX_AGENTS + 1];            // the actor — with one actor per agent the agents' slices of the stacked actor (formed on the host) — then the critic
};

__global__ __launch_bounds__(256) void hns_policy_pack_agents_kernel(const PolNets nets, int D, float *img) {
    const long long n = pol_net_floats(D);
    float *dst = img + blockIdx.y * n;                           // image blockIdx.y: the actors', then the critic's
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) dst[i] = pol_src(nets.n[blockIdx.y], D, i);
}

// [the shared actor's image as hns_policy_pack_agents_kernel writes it, the centralised critic's]: nets.n[0], nets.n[1]
__global__ __launch_bounds__(256) void hns_policy_pack_central_kernel(const PolNets nets, int D, float *img) {
    const bool critic = blockIdx.y;
    const long long n = critic ? pol_central_floats(D) : pol_net_floats(D);
    float *dst = img + (critic ? pol_net_floats(D) : 0);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        dst[i] = critic ? pol_central_src(nets.n[1], D, i) : pol_src(nets.n[0], D, i);
}

// [the A actors' images as hns_policy_pack_agents_kernel writes them, the centralised critic's as hns_policy_pack_central_kernel does]:
// nets.n[0 .. A - 1], nets.n[A]; image blockIdx.y, every one pol_net_floats behind the one before
__global__ __launch_bounds__(256) void hns_policy_pack_central_agents_kernel(const PolNets nets, int D, int A, float *img) {
    const bool critic = blockIdx.y == (unsigned)A;
    const long long n = critic ? pol_central_floats(D) : pol_net_floats(D);
    float *dst = img + blockIdx.y * pol_net_floats(D);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        dst[i] = critic ? pol_central_src(nets.n[blockIdx.y], D, i) : pol_src(nets.n[blockIdx.y], D, i);
}

struct PolArgs {
    const float *img;                       // the actor image(s), then the critic's, net_floats each
    long long net_floats;
    const float *xs, *xo, *xc;               // obs_self [E, A, D], obs_others [E, A, A - 1, 3], obs_cylinders [E, A, K, 5]
    long long sse, ssa, soe, soa, sot, sce, sca, sct;
    const float *eps;                        // [rows, 4] or NULL
    const unsigned long long *counter;       // Philox call counter (device) — read only here
    unsigned long long seed;
    float *action, *loc, *logp, *value;      // [rows, 4], [rows, 4] or NULL, [rows], [rows]
    long long rows;
    int A, K, D, deterministic, value_only;
};

struct PolLds {
    float x0[kEncE * kEncLd];                // token 0 / LN1 output
    float t1[kEncE * kEncLd];
    float t2[kEncE * kEncLd];
};

// one network on the workgroup's rows; leaves the encoder output y (the thread's 16 features of row r) in `y`.
// CENTRAL (the centralised critic's image): a row is an ENV (a.rows of them); its tokens are the A rows of a.xs (state_drones,
// sse / ssa apart) through the ONE embedding of token 0, then the K rows of a.xc (the state's cylinders [E, K, 5]: sce / sct apart).  The
// statements behind the tokens are the same ones; without the flag the function compiles to what it was.
template <bool CENTRAL = false>
HNS_DEV void pol_encoder(const PolArgs &a, const float *net, PolLds &L, int w, int lane, int r, int g, long long row, float (&y)[16]) {
    const bool live = row < a.rows;
    const long long e = live ? (CENTRAL ? row : row / a.A) : 0;
    const int ag = live && !CENTRAL ? (int)(row % a.A) : 0;
    const int D = a.D, es = CENTRAL ? C_EW : P_EW, eo = P_EW + D * kEncE, ec = CENTRAL ? C_EW + D * kEncE : eo + 3 * kEncE;
    const float *xs = live ? a.xs + e * a.sse + ag * a.ssa : nullptr;
    const float *xo = live && a.xo ? a.xo + e * a.soe + ag * a.soa : nullptr;
    const float *xc = live ? a.xc + e * a.sce + ag * a.sca : nullptr;

    // the image's sections are `net + offset` at each call: pointers formed once in front of the token loop made the kernel 5 % slower
    // (profiles/r15_encoder_fold.txt)
    float t[16], xh[16];                                          // xh: the normalised vectors, which only a backward pass reads
    enc_token<true>(net + es, net + P_EB, xs, D, net + P_LNW, net + P_LNB, g, xh, t);            // token 0
    enc_lds_store(L.x0, r, g, t);
    __syncthreads();
    enc_matvec<0>(net + P_MAT + 0 * kEncMat, net + P_BQ, L.x0, L.t1, nullptr, nullptr, w, lane);     // q
    __syncthreads();
    enc_matvec<2>(net + P_MAT + 1 * kEncMat, nullptr, L.t1, L.t2, nullptr, nullptr, w, lane);        // W_k^T q / sqrt(128)
    __syncthreads();

    // token pass: scores and online softmax, z = sum_j a_j t_j
    float kq[16], z[16];
    enc_lds_load(L.t2, r, g, kq);
    float m = enc_score(kq, t), l = 1.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = t[i];
    const int N = a.A + a.K;
    for (int j = 1; j < N; ++j) {
        if (CENTRAL && j < a.A) enc_token<true>(net + es, net + P_EB, xs ? xs + j * a.ssa : nullptr, D, net + P_LNW, net + P_LNB, g, xh, t);
        else if (j < a.A) enc_token<true>(net + eo, net + P_EB + kEncE, xo ? xo + (j - 1) * a.sot : nullptr, 3, net + P_LNW, net + P_LNB, g, xh, t);
        else enc_token<true>(net + ec, net + P_EB + 2 * kEncE, xc ? xc + (j - a.A) * a.sct : nullptr, 5, net + P_LNW, net + P_LNB, g, xh, t);
        enc_softmax_step(kq, t, m, l, z);
    }
    const float il = 1.0f / l;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] *= il;
    enc_lds_store(L.t1, r, g, z);
    __syncthreads();
    enc_matvec<0>(net + P_MAT + 2 * kEncMat, net + P_BV, L.t1, L.t2, nullptr, nullptr, w, lane);     // v = W_v z + b_v
    __syncthreads();
    enc_matvec<0>(net + P_MAT + 3 * kEncMat, net + P_BO, L.t2, L.t1, nullptr, nullptr, w, lane);     // attn = W_o v + b_o
    __syncthreads();
    float x[16], u[16];
    enc_lds_load(L.x0, r, g, u);
    enc_lds_load(L.t1, r, g, t);
#pragma unroll
    for (int i = 0; i < 16; ++i) u[i] += t[i];
    enc_layernorm(u, net + P_N1W, net + P_N1B, g, xh, x);         // x0' = LN1(x0 + attn)
    enc_lds_store(L.x0, r, g, x);
    __syncthreads();
    enc_matvec<1>(net + P_MAT + 4 * kEncMat, net + P_B1, L.x0, L.t1, nullptr, nullptr, w, lane);     // gelu(W_1 x0' + b_1)
    __syncthreads();
    enc_matvec<0>(net + P_MAT + 5 * kEncMat, net + P_B2, L.t1, L.t2, nullptr, nullptr, w, lane);     // W_2 h + b_2
    __syncthreads();
    enc_lds_load(L.t2, r, g, t);
#pragma unroll
    for (int i = 0; i < 16; ++i) u[i] = x[i] + t[i];
    enc_layernorm(u, net + P_N2W, net + P_N2B, g, xh, y);         // y = LN2(x0' + ff)
}

HNS_DEV float pol_head(const float *net, int o, const float (&y)[16], int g) {
    const float *hw = net + P_HW + o * kEncE;
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f32x4 wv = *reinterpret_cast<const f32x4 *>(hw + enc_feat(g, i, 0));
#pragma unroll
        for (int u = 0; u < 4; ++u) s = __builtin_fmaf(wv[u], y[4 * i + u], s);
    }
    return row_sum8(s) + net[P_HB + o];
}

// the row's action (the caller's eps, Philox noise, or the mode), its log-probability and loc, written by the row's first lane
HNS_DEV void pol_sample(const PolArgs &a, const float *net, const float (&loc)[4], long long row, bool live, int g) {
    float eps[4] = {0.f, 0.f, 0.f, 0.f};
    if (!a.deterministic) {
        if (a.eps) {
            if (live) {
#pragma unroll
                for (int o = 0; o < 4; ++o) eps[o] = a.eps[row * 4 + o];
            }
        } else {
            // Philox4x32-10: key = seed, counter = (call counter, row); Box-Muller on both pairs
            const unsigned long long c = a.counter[0];
            uint32_t u[4];
            d_philox((uint32_t)a.seed, (uint32_t)(a.seed >> 32), (uint32_t)c, (uint32_t)(c >> 32), (uint32_t)row, (uint32_t)(row >> 32), u);
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const float u1 = (float)((u[2 * p] >> 8) + 1u) * 5.9604644775390625e-8f;   // (0, 1]
                const float u2 = (float)(u[2 * p + 1] >> 8) * 5.9604644775390625e-8f;       // [0, 1)
                const float rad = __builtin_sqrtf(-2.0f * logf(u1));
                float sn, cs;
                sincosf(6.283185307179586f * u2, &sn, &cs);
                eps[2 * p] = rad * cs;
                eps[2 * p + 1] = rad * sn;
            }
        }
    }
    if (live && g == 0) {
        float lp = 0.0f;
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const float sc = net[P_SCALE + o];
            const float act = a.deterministic ? loc[o] : loc[o] + sc * eps[o];
            const float d = act - loc[o];
            const float term = (-(d * d) / (2.0f * (sc * sc)) - net[P_LOGSCALE + o]) - 0.91893853320467274f;  // Normal.log_prob
            lp = o == 0 ? term : lp + term;
            a.action[row * 4 + o] = act;
            if (a.loc) a.loc[row * 4 + o] = loc[o];
        }
        a.logp[row] = lp;
    }
}

// ---- the recurrent configuration: one GRU step between the encoder and the head (include/hns.h: hns_policy_forward_rnn)
// packed GRU image of one network, in floats: the six gate matrices in the encoder matrices' fragment order, then the vectors
enum : int {
    R_MAT = 0,                               // W_ir, W_iz, W_in, W_hr, W_hz, W_hn
    R_BR = 6 * kEncMat,                      // b_ir + b_hr (one rounding, at pack time)
    R_BZ = R_BR + kEncE,                     // b_iz + b_hz
    R_BIN = R_BZ + kEncE, R_BHN = R_BIN + kEncE, R_LNW = R_BHN + kEncE, R_LNB = R_LNW + kEncE,
    R_NET = R_LNB + kEncE,
};

struct GruSrc {
    const float *w_ih, *w_hh, *b_ih, *b_hh, *ln_w, *ln_b;
};

HNS_DEV float pol_rnn_src(const GruSrc &s, int i) {
    if (i < R_BR) {
        const int m = i / kEncMat, x = i % kEncMat;
        const int u = x & 3, lane = (x >> 2) & 63, s4 = (x >> 8) & 7, rb = x >> 11;         // enc_mat_src's fragment order
        const int row = rb * 16 + (lane & 15), k = 4 * (4 * s4 + u) + (lane >> 4);
        return (m < 3 ? s.w_ih : s.w_hh)[((m % 3) * kEncE + row) * kEncE + k];
    }
    const int sec = (i - R_BR) / kEncE, f = (i - R_BR) % kEncE;
    switch (sec) {
        case 0: return s.b_ih[f] + s.b_hh[f];
        case 1: return s.b_ih[kEncE + f] + s.b_hh[kEncE + f];
        case 2: return s.b_ih[2 * kEncE + f];
        case 3: return s.b_hh[2 * kEncE + f];
        case 4: return s.ln_w[f];
        default: return s.ln_b[f];
    }
}

struct GruSrcs {
    GruSrc n[HNS_MAX_AGENTS + 1];            // the actor's GRU — with one actor per agent the agents' slices of the stacked GRU (formed on the host) — then the critic's
};

__global__ __launch_bounds__(256) void hns_policy_rnn_pack_agents_kernel(const GruSrcs nets, float *img) {
    float *dst = img + (long long)blockIdx.y * R_NET;            // image blockIdx.y: the actors' GRUs, then the critic's
    for (int i = blockIdx.x * 256 + threadIdx.x; i < R_NET; i += gridDim.x * 256) dst[i] = pol_rnn_src(nets.n[blockIdx.y], i);
}

struct PolRnnArgs {
    const float *img;                        // the actor GRU image(s), then the critic's, R_NET floats each
    const float *h_in[2];                    // actor, critic: [rows, 128] or NULL (zeros)
    float *h_out[2];
    const unsigned char *is_init;            // [E] or NULL
};

HNS_DEV float pol_sigm(float z) { return 1.0f / (1.0f + expf(-z)); }

// acc = the bias of the wave's output rows (row blocks 2 w, 2 w + 1; the lane's four features of each, both column blocks)
HNS_DEV void pol_gate_start(const float *bias, int w, int kq, f32x4 (&acc)[2][2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const f32x4 b = *reinterpret_cast<const f32x4 *>(bias + (2 * w + i) * 16 + 4 * kq);
        acc[i][0] = b;
        acc[i][1] = b;
    }
}

// acc += W[128][128] IN[128][R]: enc_matvec's product (same operands, same k order) onto accumulators that stay in registers
HNS_DEV void pol_gate_prod(const float *__restrict__ W, const float *in, int w, int lane, f32x4 (&acc)[2][2]) {
    const int col = lane & 15, kq = lane >> 4;
    const f32x4 *A0 = reinterpret_cast<const f32x4 *>(W) + (2 * w) * 8 * 64 + lane;
    const f32x4 *A1 = A0 + 8 * 64;
#pragma unroll
    for (int s4 = 0; s4 < 8; ++s4) {
        const f32x4 a0 = A0[s4 * 64], a1 = A1[s4 * 64];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = 4 * (4 * s4 + u) + kq;
            const float b0 = in[k * kEncLd + col], b1 = in[k * kEncLd + 16 + col];
            acc[0][0] = enc_mfma(a0[u], b0, acc[0][0]);
            acc[0][1] = enc_mfma(a0[u], b1, acc[0][1]);
            acc[1][0] = enc_mfma(a1[u], b0, acc[1][0]);
            acc[1][1] = enc_mfma(a1[u], b1, acc[1][1]);
        }
    }
}

// one GRU step of the workgroup's rows on the features `y` the encoder left in registers: y <- LayerNorm(h' + y), h' -> h_out.  The gate
// products run one after another onto one set of accumulators; the three gates of a (feature, row) pair land in the same lane, so the cell
// runs in the accumulator layout and only h' crosses the LDS back to the eight-lanes-per-row layout.  Every read of h_in precedes the first
// barrier and every write of h_out follows it, and a workgroup touches its own rows only: h_out may be h_in.
//
// AGENTS (one actor per agent): the tile is 32 consecutive envs of agent blockIdx.y, so `row0` is the tile's first ENV and `rows`
// the number of envs; tile position p is live iff row0 + p < rows, its state row is (row0 + p) A + agent — A 512 bytes apart instead of
// contiguous, on the load (position r) and on the accumulator-layout store (position rr) alike — and its flag is_init[row0 + p].  The
// arithmetic is the same statements; the shared form (AGENTS false) compiles to what it was.
template <bool AGENTS>
HNS_DEV void pol_gru_step(const float *rn, const float *h_in, float *h_out, const unsigned char *is_init, int A, long long row0, long long rows,
                          PolLds &L, int w, int lane, int r, int g, float (&y)[16]) {
    float h[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) h[i] = 0.0f;
    bool read;
    long long hr;
    if constexpr (AGENTS) {
        read = h_in && row0 + r < rows && !(is_init && is_init[row0 + r]);
        hr = (row0 + r) * A + blockIdx.y;
    } else {
        read = h_in && row0 + r < rows && !(is_init && is_init[(row0 + r) / A]);     // the env's flag holds for all of its agents
        hr = row0 + r;
    }
    if (read) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(h_in + hr * kEncE + enc_feat(g, i, 0));
#pragma unroll
            for (int u = 0; u < 4; ++u) h[4 * i + u] = v[u];
        }
    }
    enc_lds_store(L.x0, r, g, y);                                 // (the encoder's last reads were of t2)
    enc_lds_store(L.t1, r, g, h);
    __syncthreads();
    const int col = lane & 15, kq = lane >> 4;
    f32x4 acc[2][2], n[2][2];
    pol_gate_start(rn + R_BR, w, kq, acc);                        // r = sigmoid(b_r + W_ir f + W_hr h)
    pol_gate_prod(rn + R_MAT + 0 * kEncMat, L.x0, w, lane, acc);
    pol_gate_prod(rn + R_MAT + 3 * kEncMat, L.t1, w, lane, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q) n[i][c][q] = pol_sigm(acc[i][c][q]);
    pol_gate_start(rn + R_BHN, w, kq, acc);                       // r (b_hn + W_hn h)
    pol_gate_prod(rn + R_MAT + 5 * kEncMat, L.t1, w, lane, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q) n[i][c][q] = n[i][c][q] * acc[i][c][q];
    pol_gate_start(rn + R_BIN, w, kq, acc);                       // n = tanh(b_in + W_in f + r (...))
    pol_gate_prod(rn + R_MAT + 2 * kEncMat, L.x0, w, lane, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q) n[i][c][q] = tanhf(acc[i][c][q] + n[i][c][q]);
    pol_gate_start(rn + R_BZ, w, kq, acc);                        // z = sigmoid(b_z + W_iz f + W_hz h)
    pol_gate_prod(rn + R_MAT + 1 * kEncMat, L.x0, w, lane, acc);
    pol_gate_prod(rn + R_MAT + 4 * kEncMat, L.t1, w, lane, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int f0 = (2 * w + i) * 16 + 4 * kq;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int rr = c * 16 + col;
            f32x4 o;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float z = pol_sigm(acc[i][c][q]);
                o[q] = (1.0f - z) * n[i][c][q] + z * L.t1[(f0 + q) * kEncLd + rr];       // h' = (1 - z) n + z h
                L.t2[(f0 + q) * kEncLd + rr] = o[q];
            }
            if (row0 + rr < rows) {
                const long long orow = AGENTS ? (row0 + rr) * A + blockIdx.y : row0 + rr;
                *reinterpret_cast<f32x4 *>(h_out + orow * kEncE + f0) = o;
            }
        }
    }
    __syncthreads();
    float u[16], xh[16];
    enc_lds_load(L.t2, r, g, h);
    enc_lds_load(L.x0, r, g, u);                                  // f again: not held in registers across the products
#pragma unroll
    for (int i = 0; i < 16; ++i) u[i] = h[i] + u[i];
    enc_layernorm(u, rn + R_LNW, rn + R_LNB, g, xh, y);           // y = LayerNorm(h' + f)
}

// the row of thread row r of an agent-major workgroup: env (tile, r) of agent blockIdx.y; past the last env a row that is not live
HNS_DEV long long pol_agent_row(const PolArgs &a, int r) {
    const long long e = (long long)blockIdx.x * kEncRows + r;
    return e * a.A < a.rows ? e * a.A + blockIdx.y : a.rows;
}

// ---- the tile: the body of all eight kernels (the flags: the head of this file; include/hns.h: hns_policy_forward and its seven siblings)
// AGENTS: the images hold A actor images / A actor-GRU images, then the critic's one of each; the actor pass reads
// agent blockIdx.y's, the critic pass the shared ones.  The row keeps its number env * A + agent and its arithmetic is pol_encoder /
// pol_gru_step / pol_head / pol_sample untouched: row (e, a) has the bits the shared kernels give it with agent a's images as the actor.
template <bool AGENTS, bool RNN, bool ACT>
HNS_DEV void pol_tile(const PolArgs &a, const PolRnnArgs &ra) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    PolLds &L = *reinterpret_cast<PolLds *>(lds_raw);
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = tid >> 3, g = tid & 7;
    // what pol_gru_step tiles: rows as they lie, or the envs of one agent (its state-row addressing note)
    const long long row0 = (long long)blockIdx.x * kEncRows, rows0 = AGENTS ? a.rows / a.A : a.rows;
    long long row;
    if constexpr (AGENTS) row = pol_agent_row(a, r);
    else row = row0 + r;
    // their places in both images (long long straight from the unsigned blockIdx.y: through an int it is sign-extended, three instructions more)
    const long long actor = AGENTS ? blockIdx.y : 0, critic = AGENTS ? a.A : 1;
    const bool live = row < a.rows;
    float y[16];

    bool actor_pass = true;
    if constexpr (!ACT) actor_pass = !a.value_only;
    if (actor_pass) {
        const float *net = a.img + actor * a.net_floats;          // the agent's actor (and its GRU), formed once per tile
        pol_encoder(a, net, L, w, lane, r, g, row, y);
        if constexpr (RNN) pol_gru_step<AGENTS>(ra.img + actor * R_NET, ra.h_in[0], ra.h_out[0], ra.is_init, a.A, row0, rows0, L, w, lane, r, g, y);
        float loc[4];
#pragma unroll
        for (int o = 0; o < 4; ++o) loc[o] = pol_head(net, o, y, g);
        if constexpr (ACT) {                                      // the mode of the distribution (evaluation), nothing else read or written
            if (live && g == 0) {
#pragma unroll
                for (int o = 0; o < 4; ++o) a.action[row * 4 + o] = loc[o];
            }
        } else {
            pol_sample(a, net, loc, row, live, g);
            __syncthreads();                                      // the critic reuses the LDS
        }
    }
    if constexpr (!ACT) {
        const float *net = a.img + critic * a.net_floats;         // the (shared) critic and its GRU, behind the actors'
        pol_encoder(a, net, L, w, lane, r, g, row, y);
        if constexpr (RNN) pol_gru_step<AGENTS>(ra.img + critic * R_NET, ra.h_in[1], ra.h_out[1], ra.is_init, a.A, row0, rows0, L, w, lane, r, g, y);
        const float v = pol_head(net, 0, y, g);
        if (live && g == 0) a.value[row] = v;
    }
}

// the kernels' names are the records' (profiles/, rocprofv3 output): one per set of flags, <AGENTS, RNN, ACT>
__global__ __launch_bounds__(kEncThreads, 2) void hns_policy_forward_kernel(const PolArgs a) { pol_tile<false, false, false>(a, PolRnnArgs{}); }
__global__ __launch_bounds__(kEncThreads, 2) void hns_policy_act_kernel(const PolArgs a) { pol_tile<false, false, true>(a, PolRnnArgs{}); }
__global__ __launch_bounds__(kEncThreads, 2) void hns_policy_forward_rnn_kernel(const PolArgs a, const PolRnnArgs ra) { pol_tile<false, true, false>(a, ra); }
__global__ __launch_bounds__(kEncThreads, 2) void hns_policy_act_rnn_kernel(const PolArgs a, const PolRnnArgs ra) { pol_tile<false, true, true>(a, ra); }
__global__ __launch_bounds__(kEncThreads, 2) void hns_policy_forward_agents_kernel(const PolArgs a) { pol_tile<true, false, false>(a, PolRnnArgs{}); }
__global__ __launch_bounds__(kEncThreads, 2) void hns_policy_act_agents_kernel(const PolArgs a) { pol_tile<true, false, true>(a, PolRnnArgs{}); }
__global__ __launch_bounds__(kEncThreads, 2) void hns_policy_forward_rnn_agents_kernel(const PolArgs a, const PolRnnArgs ra) { pol_tile<true, true, false>(a, ra); }
__global__ __launch_bounds__(kEncThreads, 2) void hns_policy_act_rnn_agents_kernel(const PolArgs a, const PolRnnArgs ra) { pol_tile<true, true, true>(a, ra); }

// ---- the centralised critic (critic_input: state; include/hns.h: hns_policy_central_forward)
// pol_head on the central image: row o of v_out (the same chain, so one row gives pol_head's bits)
HNS_DEV float pol_head_central(const float *net, int o, const float (&y)[16], int g) {
    const float *hw = net + C_HW + o * kEncE;
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f32x4 wv = *reinterpret_cast<const f32x4 *>(hw + enc_feat(g, i, 0));
#pragma unroll
        for (int u = 0; u < 4; ++u) s = __builtin_fmaf(wv[u], y[4 * i + u], s);
    }
    return row_sum8(s) + net[C_HB + o];
}

// The grid is two ranges of workgroups: the first `actor_tiles` are the shared actor's tiles of 32 (env, agent) rows — pol_tile's actor pass,
// statement for statement, on `a` — and the rest the critic's tiles of 32 ENVS on `c` (img: the central image; xs / xc: the state), each env's
// A values from A evaluations of the head on its one feature row.  The two never share a workgroup: at 2 048 envs x 3 that is 192 + 64
// workgroups side by side instead of 192 running both passes back to back.
__global__ __launch_bounds__(kEncThreads, 2) void hns_policy_forward_central_kernel(const PolArgs a, const PolArgs c, const unsigned actor_tiles) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    PolLds &L = *reinterpret_cast<PolLds *>(lds_raw);
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = tid >> 3, g = tid & 7;
    float y[16];
    if (blockIdx.x < actor_tiles) {
        const long long row = (long long)blockIdx.x * kEncRows + r;
        pol_encoder(a, a.img, L, w, lane, r, g, row, y);
        float loc[4];
#pragma unroll
        for (int o = 0; o < 4; ++o) loc[o] = pol_head(a.img, o, y, g);
        pol_sample(a, a.img, loc, row, row < a.rows, g);
    } else {
        const long long env = (long long)(blockIdx.x - actor_tiles) * kEncRows + r;
        pol_encoder<true>(c, c.img, L, w, lane, r, g, env, y);
        for (int o = 0; o < c.A; ++o) {
            const float v = pol_head_central(c.img, o, y, g);
            if (env < c.rows && g == 0) c.value[env * c.A + o] = v;
        }
    }
}

// One actor per agent beside the centralised critic (share_actor: false with critic_input: state; include/hns.h:
// hns_policy_central_forward_agents).  The grid is dim3(tiles of 32 envs, ranges): range blockIdx.y < `agents` is agent
// blockIdx.y's — pol_tile<AGENTS = true>'s actor pass, statement for statement, on `a`: 32 envs of one agent, pol_agent_row, that agent's
// image, pol_head, pol_sample on row e A + a — and range blockIdx.y == `agents` the critic's — the kernel above's critic branch, statement
// for statement, on `c`: 32 envs, pol_encoder<true>, pol_head_central A times — with exactly as many tiles as one agent's.  A value-only
// call launches one range with agents = 0: the critic's alone, `a` never read.  The two passes never share a workgroup.
__global__ __launch_bounds__(kEncThreads, 2) void hns_policy_forward_central_agents_kernel(const PolArgs a, const PolArgs c, const unsigned agents) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    PolLds &L = *reinterpret_cast<PolLds *>(lds_raw);
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = tid >> 3, g = tid & 7;
    float y[16];
    if (blockIdx.y < agents) {
        const long long row = pol_agent_row(a, r), actor = blockIdx.y;
        const float *net = a.img + actor * a.net_floats;          // the agent's actor, formed once per tile
        pol_encoder(a, net, L, w, lane, r, g, row, y);
        float loc[4];
#pragma unroll
        for (int o = 0; o < 4; ++o) loc[o] = pol_head(net, o, y, g);
        pol_sample(a, net, loc, row, row < a.rows, g);
    } else {
        const long long env = (long long)blockIdx.x * kEncRows + r;
        pol_encoder<true>(c, c.img, L, w, lane, r, g, env, y);
        for (int o = 0; o < c.A; ++o) {
            const float v = pol_head_central(c.img, o, y, g);
            if (env < c.rows && g == 0) c.value[env * c.A + o] = v;
        }
    }
}

__global__ void hns_policy_bump_kernel(unsigned long long *counter) { counter[0] += 1ull; }

}  // namespace hns

namespace {

// one network's table from hns_encoder.h's field list (ct_bind_net of hns_policy_train.hip fills the same struct)
int pol_net(const char *fn, const hns_policy_net *n, int has_others, bool actor, hns::EncNet &s) {
    if (!n) return hns_fail(fn, "null network");
    bool ok = true;
#define X(f, m)                                \
    ok = ok && n->f && hns_aligned(n->f, 4); \
    s.m = n->f;
    HNS_CT_FIELDS(X)
#undef X
    if (!ok) return hns_fail(fn, "every parameter pointer must be a non-NULL fp32 array");
    if (has_others && (!n->embed_others_w || !n->embed_others_b)) return hns_fail(fn, "state_others embedding missing (num_agents > 1)");
    if (actor && !n->log_std) return hns_fail(fn, "the actor needs log_std");
    s.ew[1] = has_others ? n->embed_others_w : nullptr; s.eb[1] = has_others ? n->embed_others_b : nullptr;
    s.log_std = actor ? n->log_std : nullptr; s.head_n = actor ? 4 : 1;
    return HNS_OK;
}

// the checks hns_policy_forward and hns_policy_act share, in the forward's order: image / io / shape, then the observation
int pol_check_shape(const char *fn, const void *packed, int32_t self_dim, int64_t num_envs, int32_t num_agents, int32_t num_cylinders,
                    const hns_policy_io *io) {
    if (!packed || !io || !hns_aligned(packed, 16)) return hns_fail(fn, "null or misaligned packed image / io");
    if (self_dim < 1 || self_dim > hns::kPolMaxSelf) return hns_fail(fn, "self_dim must be in [1, " + std::to_string(hns::kPolMaxSelf) + "]");
    if (num_agents < 1 || num_agents > HNS_MAX_AGENTS) return hns_fail(fn, "num_agents must be in [1, 7]");
    if (num_cylinders < 1 || num_cylinders > HNS_MAX_CYLINDERS) return hns_fail(fn, "num_cylinders must be in [1, 16]");
    if (num_envs < 1 || num_envs > ((int64_t)1 << 31) / HNS_MAX_AGENTS) return hns_fail(fn, "num_envs must be in [1, 2^31 / 7]");
    return HNS_OK;
}

int pol_check_obs(const char *fn, int32_t num_agents, const hns_policy_io *io) {
    if (!io->obs_self || !io->obs_cylinders || (num_agents > 1 && !io->obs_others)) return hns_fail(fn, "observation pointer missing");
    if (!hns_aligned(io->obs_self, 4) || !hns_aligned(io->obs_cylinders, 4) || (io->obs_others && !hns_aligned(io->obs_others, 4)))
        return hns_fail(fn, "misaligned observation");
    for (int k = 0; k < 2; ++k)
        if (io->self_stride[k] < 0) return hns_fail(fn, "negative stride");
    for (int k = 0; k < 3; ++k)
        if (io->others_stride[k] < 0 || io->cyl_stride[k] < 0) return hns_fail(fn, "negative stride");
    return HNS_OK;
}

// the forward's outputs, noise and counter (hns_policy_forward, hns_policy_forward_rnn)
int pol_check_outputs(const char *fn, const hns_policy_io *io, bool value_only, bool det, const uint64_t *counter) {
    if (!io->value || !hns_aligned(io->value, 4)) return hns_fail(fn, "value output missing or misaligned");
    if (!value_only) {
        if (!io->action || !io->log_prob || !hns_aligned(io->action, 4) || !hns_aligned(io->log_prob, 4) || (io->loc && !hns_aligned(io->loc, 4)))
            return hns_fail(fn, "action / log_prob outputs missing or misaligned");
        if (!det && !io->eps && (!counter || !hns_aligned(counter, 8))) return hns_fail(fn, "sampling without eps needs the device call counter");
        if (io->eps && !hns_aligned(io->eps, 4)) return hns_fail(fn, "misaligned eps");
    }
    return HNS_OK;
}

int pol_gru_net(const char *fn, const hns_gru_net *n, hns::GruSrc &s) {
    if (!n) return hns_fail(fn, "null GRU network");
    const float *p[6] = {n->weight_ih, n->weight_hh, n->bias_ih, n->bias_hh, n->ln_w, n->ln_b};
    for (const float *q : p)
        if (!q || !hns_aligned(q, 4)) return hns_fail(fn, "every GRU parameter pointer must be a non-NULL fp32 array");
    s = hns::GruSrc{n->weight_ih, n->weight_hh, n->bias_ih, n->bias_hh, n->ln_w, n->ln_b};
    return HNS_OK;
}

// hns_policy_pack and hns_policy_pack_agents: `actors` images of the (stacked) actor's slices — one: the tensors themselves — then the critic's
int pol_pack_call(const char *fn, const hns_policy_net *actor, const hns_policy_net *critic, int32_t self_dim, int32_t num_agents, bool per_agent,
                  void *packed, void *stream) {
    if (self_dim < 1 || self_dim > hns::kPolMaxSelf) return hns_fail(fn, "self_dim must be in [1, " + std::to_string(hns::kPolMaxSelf) + "]");
    if (num_agents < 1 || num_agents > HNS_MAX_AGENTS) return hns_fail(fn, "num_agents must be in [1, 7]");
    if (!packed || !hns_aligned(packed, 16)) return hns_fail(fn, "packed image must be a 16-byte aligned device array");
    hns::EncNet sa{}, sc{};
    int rc = pol_net(fn, actor, num_agents > 1, true, sa);
    if (rc != HNS_OK) return rc;
    rc = pol_net(fn, critic, num_agents > 1, false, sc);
    if (rc != HNS_OK) return rc;
    const int actors = per_agent ? num_agents : 1;
    hns::PolNets nets{};
    for (int ag = 0; ag < actors; ++ag) nets.n[ag] = hns::enc_agent_slice(sa, self_dim, 4, ag);
    nets.n[actors] = sc;
    hipLaunchKernelGGL(hns::hns_policy_pack_agents_kernel, dim3(256, (unsigned)actors + 1), dim3(256), 0, static_cast<hipStream_t>(stream), nets,
                       (int)self_dim, static_cast<float *>(packed));
    HNS_CHECK_HIP(hipGetLastError());
    return HNS_OK;
}

// hns_policy_rnn_pack and hns_policy_rnn_pack_agents, the same way
int pol_rnn_pack_call(const char *fn, const hns_gru_net *actor_rnn, const hns_gru_net *critic_rnn, int actors, void *rnn_packed, void *stream) {
    if (!rnn_packed || !hns_aligned(rnn_packed, 16)) return hns_fail(fn, "packed image must be a 16-byte aligned device array");
    hns::GruSrc sa{}, sc{};
    int rc = pol_gru_net(fn, actor_rnn, sa);
    if (rc != HNS_OK) return rc;
    rc = pol_gru_net(fn, critic_rnn, sc);
    if (rc != HNS_OK) return rc;
    hns::GruSrcs nets{};
    constexpr long long E = hns::kEncE;
    for (int ag = 0; ag < actors; ++ag)                           // agent ag's slice of the stacked tensors: [A, 384, 128] x2, [A, 384] x2, [A, 128] x2
        nets.n[ag] = hns::GruSrc{sa.w_ih + ag * 3 * E * E, sa.w_hh + ag * 3 * E * E, sa.b_ih + ag * 3 * E, sa.b_hh + ag * 3 * E, sa.ln_w + ag * E,
                                 sa.ln_b + ag * E};
    nets.n[actors] = sc;
    hipLaunchKernelGGL(hns::hns_policy_rnn_pack_agents_kernel, dim3(128, (unsigned)actors + 1), dim3(256), 0, static_cast<hipStream_t>(stream), nets,
                       static_cast<float *>(rnn_packed));
    HNS_CHECK_HIP(hipGetLastError());
    return HNS_OK;
}

// the tile kernels by 4 agents + 2 recurrent + actor-only (the table at the head of this file)
#define K(name) reinterpret_cast<const void *>(&hns::name)
const void *const kPolKernels[8] = {K(hns_policy_forward_kernel),        K(hns_policy_act_kernel),        K(hns_policy_forward_rnn_kernel),
                                    K(hns_policy_act_rnn_kernel),        K(hns_policy_forward_agents_kernel), K(hns_policy_act_agents_kernel),
                                    K(hns_policy_forward_rnn_agents_kernel), K(hns_policy_act_rnn_agents_kernel)};
#undef K

// All eight entries: the same refusals in the same order, one set of arguments, one launch.  `agents` picks the agent-major tile and its grid,
// `rnn` adds the GRU image and the states, `act` is the actor's pass alone (flags 0, no counter): its eps, counter, loc, log_prob, value and
// critic states stay NULL and are never touched, as the actor's states are under HNS_POLICY_VALUE_ONLY.
int pol_call(const char *fn, bool agents, bool rnn, bool act, const void *packed, const void *rnn_packed, int32_t self_dim, int64_t num_envs,
             int32_t num_agents, int32_t num_cylinders, const hns_policy_io *io, const hns_policy_rnn_io *rio, int32_t flags, uint64_t seed,
             uint64_t *counter, void *stream) {
    int rc = pol_check_shape(fn, packed, self_dim, num_envs, num_agents, num_cylinders, io);
    if (rc != HNS_OK) return rc;
    if (rnn && (!rnn_packed || !rio || !hns_aligned(rnn_packed, 16) || !hns_aligned(rio, 8))) return hns_fail(fn, "null or misaligned packed GRU image / rnn io");
    if (flags & ~(HNS_POLICY_DETERMINISTIC | HNS_POLICY_VALUE_ONLY)) return hns_fail(fn, "unknown flag");
    const bool value_only = flags & HNS_POLICY_VALUE_ONLY, det = flags & HNS_POLICY_DETERMINISTIC;
    rc = pol_check_obs(fn, num_agents, io);
    if (rc != HNS_OK) return rc;
    if (act) {
        if (!io->action || !hns_aligned(io->action, 4)) return hns_fail(fn, "action output missing or misaligned");
    } else {
        rc = pol_check_outputs(fn, io, value_only, det, counter);
        if (rc != HNS_OK) return rc;
    }
    hns::PolRnnArgs ra{};
    if (rnn) {
        const bool actor_h = !value_only, critic_h = !act;       // the states the call touches
        if ((critic_h && (!rio->critic_h_out || !hns_aligned(rio->critic_h_out, 16))) || (actor_h && (!rio->actor_h_out || !hns_aligned(rio->actor_h_out, 16))))
            return hns_fail(fn, "state output missing or not 16-byte aligned");
        if ((critic_h && !hns_aligned(rio->critic_h_in, 16)) || (actor_h && !hns_aligned(rio->actor_h_in, 16))) return hns_fail(fn, "state input not 16-byte aligned");
        ra.img = static_cast<const float *>(rnn_packed);
        if (actor_h) { ra.h_in[0] = rio->actor_h_in; ra.h_out[0] = rio->actor_h_out; }
        if (critic_h) { ra.h_in[1] = rio->critic_h_in; ra.h_out[1] = rio->critic_h_out; }
        ra.is_init = rio->is_init;
    }
    hns::PolArgs a{};
    a.img = static_cast<const float *>(packed);
    a.net_floats = hns::pol_net_floats(self_dim);
    a.xs = io->obs_self; a.xo = io->obs_others; a.xc = io->obs_cylinders;
    a.sse = io->self_stride[0]; a.ssa = io->self_stride[1];
    a.soe = io->others_stride[0]; a.soa = io->others_stride[1]; a.sot = io->others_stride[2];
    a.sce = io->cyl_stride[0]; a.sca = io->cyl_stride[1]; a.sct = io->cyl_stride[2];
    a.action = io->action;
    a.rows = num_envs * num_agents; a.A = num_agents; a.K = num_cylinders; a.D = self_dim;
    if (!act) {
        a.eps = io->eps; a.counter = reinterpret_cast<const unsigned long long *>(counter); a.seed = seed;
        a.loc = io->loc; a.logp = io->log_prob; a.value = io->value;
        a.deterministic = det; a.value_only = value_only;
    }
    static const hipError_t attr = [] {                           // 72 KB of dynamic LDS: above the default cap
        hipError_t e = hipSuccess;
        for (const void *k : kPolKernels)
            if (e == hipSuccess) e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(hns::PolLds));
        return e;
    }();
    HNS_CHECK_HIP(attr);
    // a tile: kEncRows rows as they lie, or (agents) kEncRows consecutive envs of one agent, blockIdx.y
    const long long tiles = ((agents ? num_envs : a.rows) + hns::kEncRows - 1) / hns::kEncRows;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    void *args[] = {&a, &ra};                                     // the kernels without a GRU take `a` alone
    HNS_CHECK_HIP(hipLaunchKernel(kPolKernels[4 * agents + 2 * rnn + act], dim3((unsigned)tiles, agents ? (unsigned)num_agents : 1u), dim3(hns::kEncThreads), args,
                                  sizeof(hns::PolLds), st));
    if (!act && !value_only && !det && !io->eps) {
        hipLaunchKernelGGL(hns::hns_policy_bump_kernel, dim3(1), dim3(1), 0, st, reinterpret_cast<unsigned long long *>(counter));
        HNS_CHECK_HIP(hipGetLastError());
    }
    return HNS_OK;
}

// hns_policy_central_forward and hns_policy_central_forward_agents: the same refusals in the same order, one set of arguments, one launch.
// `agents` picks the per-agent image [A actors, the central critic], the agent-major actor tiles and the grid of A + 1 ranges.
int pol_central_call(const char *fn, bool agents, const void *packed, int32_t self_dim, int64_t num_envs, int32_t num_agents, int32_t num_cylinders,
                     const hns_policy_io *io, const hns_policy_state *state, int32_t flags, uint64_t seed, uint64_t *counter, void *stream) {
    int rc = pol_check_shape(fn, packed, self_dim, num_envs, num_agents, num_cylinders, io);
    if (rc != HNS_OK) return rc;
    if (flags & ~(HNS_POLICY_DETERMINISTIC | HNS_POLICY_VALUE_ONLY)) return hns_fail(fn, "unknown flag");
    const bool value_only = flags & HNS_POLICY_VALUE_ONLY, det = flags & HNS_POLICY_DETERMINISTIC;
    if (!value_only) {                                            // the critic workgroups never read the observation
        rc = pol_check_obs(fn, num_agents, io);
        if (rc != HNS_OK) return rc;
    }
    if (!state || !state->state_drones || !state->cylinders || !hns_aligned(state->state_drones, 4) || !hns_aligned(state->cylinders, 4))
        return hns_fail(fn, "state pointer missing or misaligned");
    for (int k = 0; k < 2; ++k)
        if (state->drones_stride[k] < 0 || state->cyl_stride[k] < 0) return hns_fail(fn, "negative stride");
    rc = pol_check_outputs(fn, io, value_only, det, counter);
    if (rc != HNS_OK) return rc;
    hns::PolArgs a{}, c{};
    a.img = static_cast<const float *>(packed);
    a.net_floats = hns::pol_net_floats(self_dim);
    a.rows = num_envs * num_agents; a.A = num_agents; a.K = num_cylinders; a.D = self_dim;
    c = a;
    c.img = a.img + (agents ? num_agents : 1) * a.net_floats;     // behind the actor's image(s)
    c.xs = state->state_drones; c.sse = state->drones_stride[0]; c.ssa = state->drones_stride[1];
    c.xc = state->cylinders; c.sce = state->cyl_stride[0]; c.sct = state->cyl_stride[1];
    c.rows = num_envs; c.value = io->value;
    if (!value_only) {
        a.xs = io->obs_self; a.xo = io->obs_others; a.xc = io->obs_cylinders;
        a.sse = io->self_stride[0]; a.ssa = io->self_stride[1];
        a.soe = io->others_stride[0]; a.soa = io->others_stride[1]; a.sot = io->others_stride[2];
        a.sce = io->cyl_stride[0]; a.sca = io->cyl_stride[1]; a.sct = io->cyl_stride[2];
        a.eps = io->eps; a.counter = reinterpret_cast<const unsigned long long *>(counter); a.seed = seed;
        a.action = io->action; a.loc = io->loc; a.logp = io->log_prob; a.deterministic = det;
    }
    static const hipError_t attr = [] {                           // 72 KB of dynamic LDS: above the default cap
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&hns::hns_policy_forward_central_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(hns::PolLds));
        if (e == hipSuccess)
            e = hipFuncSetAttribute(reinterpret_cast<const void *>(&hns::hns_policy_forward_central_agents_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(hns::PolLds));
        return e;
    }();
    HNS_CHECK_HIP(attr);
    const unsigned critic_tiles = (unsigned)((num_envs + hns::kEncRows - 1) / hns::kEncRows);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (agents) {
        // ranges of critic_tiles tiles of 32 envs: one per agent, then the critic's (value-only: the critic's alone)
        const unsigned actor_ranges = value_only ? 0u : (unsigned)num_agents;
        hipLaunchKernelGGL(hns::hns_policy_forward_central_agents_kernel, dim3(critic_tiles, actor_ranges + 1), dim3(hns::kEncThreads),
                           sizeof(hns::PolLds), st, a, c, actor_ranges);
    } else {
        const unsigned actor_tiles = value_only ? 0u : (unsigned)((a.rows + hns::kEncRows - 1) / hns::kEncRows);
        hipLaunchKernelGGL(hns::hns_policy_forward_central_kernel, dim3(actor_tiles + critic_tiles), dim3(hns::kEncThreads), sizeof(hns::PolLds), st, a, c,
                           actor_tiles);
    }
    HNS_CHECK_HIP(hipGetLastError());
    if (!value_only && !det && !io->eps) {
        hipLaunchKernelGGL(hns::hns_policy_bump_kernel, dim3(1), dim3(1), 0, st, reinterpret_cast<unsigned long long *>(counter));
        HNS_CHECK_HIP(hipGetLastError());
    }
    return HNS_OK;
}

}  // namespace

extern "C" {

size_t hns_policy_packed_central_bytes(int32_t self_dim, int32_t num_agents) {
    if (self_dim < 1 || self_dim > hns::kPolMaxSelf || num_agents < 1 || num_agents > HNS_MAX_AGENTS) return 0;
    return (size_t)(hns::pol_net_floats(self_dim) + hns::pol_central_floats(self_dim)) * sizeof(float);
}

int hns_policy_pack_central(const hns_policy_net *actor, const hns_policy_net *critic, int32_t self_dim, int32_t num_agents, void *packed, void *stream) {
    const char *fn = "hns_policy_pack_central";
    if (self_dim < 1 || self_dim > hns::kPolMaxSelf) return hns_fail(fn, "self_dim must be in [1, " + std::to_string(hns::kPolMaxSelf) + "]");
    if (num_agents < 1 || num_agents > HNS_MAX_AGENTS) return hns_fail(fn, "num_agents must be in [1, 7]");
    if (!packed || !hns_aligned(packed, 16)) return hns_fail(fn, "packed image must be a 16-byte aligned device array");
    hns::PolNets nets{};
    int rc = pol_net(fn, actor, num_agents > 1, true, nets.n[0]);
    if (rc != HNS_OK) return rc;
    rc = pol_net(fn, critic, false, false, nets.n[1]);
    if (rc != HNS_OK) return rc;
    if (critic->embed_others_w || critic->embed_others_b) return hns_fail(fn, "the centralised critic has no state_others embedding");
    nets.n[1].head_n = num_agents;                               // v_out = Linear(128, A)
    hipLaunchKernelGGL(hns::hns_policy_pack_central_kernel, dim3(256, 2), dim3(256), 0, static_cast<hipStream_t>(stream), nets, (int)self_dim,
                       static_cast<float *>(packed));
    HNS_CHECK_HIP(hipGetLastError());
    return HNS_OK;
}

int hns_policy_central_forward(const void *packed, int32_t self_dim, int64_t num_envs, int32_t num_agents, int32_t num_cylinders,
                               const hns_policy_io *io, const hns_policy_state *state, int32_t flags, uint64_t seed, uint64_t *counter, void *stream) {
    return pol_central_call("hns_policy_central_forward", false, packed, self_dim, num_envs, num_agents, num_cylinders, io, state, flags, seed, counter, stream);
}

size_t hns_policy_packed_central_agents_bytes(int32_t self_dim, int32_t num_agents) {
    if (self_dim < 1 || self_dim > hns::kPolMaxSelf || num_agents < 1 || num_agents > HNS_MAX_AGENTS) return 0;
    return (size_t)(num_agents * hns::pol_net_floats(self_dim) + hns::pol_central_floats(self_dim)) * sizeof(float);
}

int hns_policy_pack_central_agents(const hns_policy_net *actors, const hns_policy_net *critic, int32_t self_dim, int32_t num_agents, void *packed,
                                   void *stream) {
    const char *fn = "hns_policy_pack_central_agents";
    if (self_dim < 1 || self_dim > hns::kPolMaxSelf) return hns_fail(fn, "self_dim must be in [1, " + std::to_string(hns::kPolMaxSelf) + "]");
    if (num_agents < 1 || num_agents > HNS_MAX_AGENTS) return hns_fail(fn, "num_agents must be in [1, 7]");
    if (!packed || !hns_aligned(packed, 16)) return hns_fail(fn, "packed image must be a 16-byte aligned device array");
    hns::EncNet sa{};
    hns::PolNets nets{};
    int rc = pol_net(fn, actors, num_agents > 1, true, sa);
    if (rc != HNS_OK) return rc;
    rc = pol_net(fn, critic, false, false, nets.n[num_agents]);
    if (rc != HNS_OK) return rc;
    if (critic->embed_others_w || critic->embed_others_b) return hns_fail(fn, "the centralised critic has no state_others embedding");
    for (int ag = 0; ag < num_agents; ++ag) nets.n[ag] = hns::enc_agent_slice(sa, self_dim, 4, ag);      // as hns_policy_pack_agents forms them
    nets.n[num_agents].head_n = num_agents;                      // v_out = Linear(128, A)
    hipLaunchKernelGGL(hns::hns_policy_pack_central_agents_kernel, dim3(256, (unsigned)num_agents + 1), dim3(256), 0, static_cast<hipStream_t>(stream),
                       nets, (int)self_dim, (int)num_agents, static_cast<float *>(packed));
    HNS_CHECK_HIP(hipGetLastError());
    return HNS_OK;
}

int hns_policy_central_forward_agents(const void *packed, int32_t self_dim, int64_t num_envs, int32_t num_agents, int32_t num_cylinders,
                                      const hns_policy_io *io, const hns_policy_state *state, int32_t flags, uint64_t seed, uint64_t *counter,
                                      void *stream) {
    return pol_central_call("hns_policy_central_forward_agents", true, packed, self_dim, num_envs, num_agents, num_cylinders, io, state, flags, seed, counter,
                            stream);
}

size_t hns_policy_packed_agents_bytes(int32_t self_dim, int32_t num_agents) {
    if (self_dim < 1 || self_dim > hns::kPolMaxSelf || num_agents < 1 || num_agents > HNS_MAX_AGENTS) return 0;
    return (size_t)((num_agents + 1) * hns::pol_net_floats(self_dim)) * sizeof(float);
}

size_t hns_policy_packed_bytes(int32_t self_dim) { return hns_policy_packed_agents_bytes(self_dim, 1); }

size_t hns_policy_rnn_packed_agents_bytes(int32_t num_agents) {
    if (num_agents < 1 || num_agents > HNS_MAX_AGENTS) return 0;
    return (size_t)((num_agents + 1) * hns::R_NET) * sizeof(float);
}

size_t hns_policy_rnn_packed_bytes(void) { return hns_policy_rnn_packed_agents_bytes(1); }

int hns_policy_pack(const hns_policy_net *actor, const hns_policy_net *critic, int32_t self_dim, int32_t num_agents, void *packed, void *stream) {
    return pol_pack_call("hns_policy_pack", actor, critic, self_dim, num_agents, false, packed, stream);
}

int hns_policy_pack_agents(const hns_policy_net *actors, const hns_policy_net *critic, int32_t self_dim, int32_t num_agents, void *packed, void *stream) {
    return pol_pack_call("hns_policy_pack_agents", actors, critic, self_dim, num_agents, true, packed, stream);
}

int hns_policy_rnn_pack(const hns_gru_net *actor_rnn, const hns_gru_net *critic_rnn, void *rnn_packed, void *stream) {
    return pol_rnn_pack_call("hns_policy_rnn_pack", actor_rnn, critic_rnn, 1, rnn_packed, stream);
}

int hns_policy_rnn_pack_agents(const hns_gru_net *actor_rnns, const hns_gru_net *critic_rnn, int32_t num_agents, void *rnn_packed, void *stream) {
    if (num_agents < 1 || num_agents > HNS_MAX_AGENTS) return hns_fail("hns_policy_rnn_pack_agents", "num_agents must be in [1, 7]");
    return pol_rnn_pack_call("hns_policy_rnn_pack_agents", actor_rnns, critic_rnn, num_agents, rnn_packed, stream);
}

int hns_policy_forward(const void *packed, int32_t self_dim, int64_t num_envs, int32_t num_agents, int32_t num_cylinders, const hns_policy_io *io,
                       int32_t flags, uint64_t seed, uint64_t *counter, void *stream) {
    return pol_call("hns_policy_forward", false, false, false, packed, nullptr, self_dim, num_envs, num_agents, num_cylinders, io, nullptr, flags, seed, counter, stream);
}

int hns_policy_forward_agents(const void *packed, int32_t self_dim, int64_t num_envs, int32_t num_agents, int32_t num_cylinders, const hns_policy_io *io,
                              int32_t flags, uint64_t seed, uint64_t *counter, void *stream) {
    return pol_call("hns_policy_forward_agents", true, false, false, packed, nullptr, self_dim, num_envs, num_agents, num_cylinders, io, nullptr, flags, seed, counter, stream);
}

int hns_policy_forward_rnn(const void *packed, const void *rnn_packed, int32_t self_dim, int64_t num_envs, int32_t num_agents, int32_t num_cylinders,
                           const hns_policy_io *io, const hns_policy_rnn_io *rio, int32_t flags, uint64_t seed, uint64_t *counter, void *stream) {
    return pol_call("hns_policy_forward_rnn", false, true, false, packed, rnn_packed, self_dim, num_envs, num_agents, num_cylinders, io, rio, flags, seed, counter, stream);
}

int hns_policy_forward_rnn_agents(const void *packed, const void *rnn_packed, int32_t self_dim, int64_t num_envs, int32_t num_agents,
                                  int32_t num_cylinders, const hns_policy_io *io, const hns_policy_rnn_io *rio, int32_t flags, uint64_t seed,
                                  uint64_t *counter, void *stream) {
    return pol_call("hns_policy_forward_rnn_agents", true, true, false, packed, rnn_packed, self_dim, num_envs, num_agents, num_cylinders, io, rio, flags, seed, counter, stream);
}

int hns_policy_act(const void *packed, int32_t self_dim, int64_t num_envs, int32_t num_agents, int32_t num_cylinders, const hns_policy_io *io,
                   void *stream) {
    return pol_call("hns_policy_act", false, false, true, packed, nullptr, self_dim, num_envs, num_agents, num_cylinders, io, nullptr, 0, 0, nullptr, stream);
}

int hns_policy_act_agents(const void *packed, int32_t self_dim, int64_t num_envs, int32_t num_agents, int32_t num_cylinders, const hns_policy_io *io,
                          void *stream) {
    return pol_call("hns_policy_act_agents", true, false, true, packed, nullptr, self_dim, num_envs, num_agents, num_cylinders, io, nullptr, 0, 0, nullptr, stream);
}

int hns_policy_act_rnn(const void *packed, const void *rnn_packed, int32_t self_dim, int64_t num_envs, int32_t num_agents, int32_t num_cylinders,
                       const hns_policy_io *io, const hns_policy_rnn_io *rio, void *stream) {
    return pol_call("hns_policy_act_rnn", false, true, true, packed, rnn_packed, self_dim, num_envs, num_agents, num_cylinders, io, rio, 0, 0, nullptr, stream);
}

int hns_policy_act_rnn_agents(const void *packed, const void *rnn_packed, int32_t self_dim, int64_t num_envs, int32_t num_agents, int32_t num_cylinders,
                              const hns_policy_io *io, const hns_policy_rnn_io *rio, void *stream) {
    return pol_call("hns_policy_act_rnn_agents", true, true, true, packed, rnn_packed, self_dim, num_envs, num_agents, num_cylinders, io, rio, 0, 0, nullptr, stream);
}

}  // extern "C"
