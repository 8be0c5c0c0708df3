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
// kPolRows rows at a time, and a token pass on the VALU (embedding, LayerNorm, score, online softmax, weighted sum) that never stores a token.
//
//   hns_policy_pack_kernel    : parameter tensors (PyTorch layouts) -> the packed image: the six matrices in MFMA A-operand fragment order (one
//                               float4 per lane per four k-steps), the vectors, the head, the embedding weights transposed.
//   hns_policy_forward_kernel : one workgroup of four waves per kPolRows rows.  Activations live in LDS as [128 features][kPolRows rows]; wave w
//                               owns output row blocks 2w, 2w + 1 of every product, so each weight element is read once per workgroup.
//   hns_policy_bump_kernel    : the device call counter += 1 after a sampling call (Philox counter; a captured graph draws fresh noise per replay).
// Determinism: fixed reduction orders (butterflies over the eight lanes of a row), no atomics.
#include <hip/hip_runtime.h>

#include <string>

#include "hns_device.h"
#include "hns_host.h"
#include "../../include/hns.h"

namespace hns {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kPolE = 128;                   // embed_dim = dim_feedforward
constexpr int kPolRows = 32;                 // rows per workgroup (two 16-wide MFMA column blocks)
constexpr int kPolLd = kPolRows + 16;        // LDS row pitch in floats: the four k-quads of a B-operand read fall in distinct bank groups
constexpr int kPolThreads = 256;
constexpr int kPolMat = kPolE * kPolE;
constexpr int kPolMaxSelf = HNS_POLICY_MAX_SELF_DIM;

// packed network image, in floats (every section a multiple of 4 floats: float4 loads)
enum : int {
    P_MAT = 0,                               // 6 matrices: Q, K^T, V, O, L1, L2 (fragment order)
    P_BQ = 6 * kPolMat, P_BV = P_BQ + kPolE, P_BO = P_BV + kPolE, P_B1 = P_BO + kPolE, P_B2 = P_B1 + kPolE,
    P_LNW = P_B2 + kPolE, P_LNB = P_LNW + kPolE, P_N1W = P_LNB + kPolE, P_N1B = P_N1W + kPolE, P_N2W = P_N1B + kPolE, P_N2B = P_N2W + kPolE,
    P_EB = P_N2B + kPolE,                    // embedding biases [3][128]: self, others, cylinders
    P_HW = P_EB + 3 * kPolE,                 // head weight [4][128] (the critic: row 0)
    P_HB = P_HW + 4 * kPolE,                 // head bias [4]
    P_SCALE = P_HB + 4,                      // exp(log_std) [4]
    P_LOGSCALE = P_SCALE + 4,                // log(scale) [4]
    P_EW = P_LOGSCALE + 4,                   // embedding weights transposed: self [D][128], others [3][128], cylinders [5][128]
};
static __host__ __device__ __forceinline__ long long pol_net_floats(int D) { return P_EW + (long long)(D + 8) * kPolE; }

struct PolNetSrc {                           // one network's parameters (PyTorch layouts)
    const float *ew[3], *eb[3], *ln_w, *ln_b, *in_w, *in_b, *out_w, *out_b, *l1_w, *l1_b, *l2_w, *l2_b, *n1_w, *n1_b, *n2_w, *n2_b;
    const float *head_w, *head_b, *log_std;  // log_std: the actor only
    int head_n;                              // 4 (actor) / 1 (critic)
};

// source value of image float i of one network
HNS_DEV float pol_src(const PolNetSrc &s, int D, long long i) {
    if (i < P_BQ) {
        const int m = (int)(i / kPolMat), x = (int)(i % kPolMat);
        const int u = x & 3, lane = (x >> 2) & 63, s4 = (x >> 8) & 7, rb = x >> 11;
        const int row = rb * 16 + (lane & 15), k = 4 * (4 * s4 + u) + (lane >> 4);
        switch (m) {
            case 0: return s.in_w[row * kPolE + k];
            case 1: return s.in_w[(kPolE + k) * kPolE + row];      // W_k^T
            case 2: return s.in_w[(2 * kPolE + row) * kPolE + k];
            case 3: return s.out_w[row * kPolE + k];
            case 4: return s.l1_w[row * kPolE + k];
            default: return s.l2_w[row * kPolE + k];
        }
    }
    const int j = (int)(i - P_BQ);
    if (i < P_EB) {
        const int sec = j / kPolE, f = j % kPolE;
        switch (sec) {
            case 0: return s.in_b[f];
            case 1: return s.in_b[2 * kPolE + f];
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
        const int key = (int)((i - P_EB) / kPolE), f = (int)((i - P_EB) % kPolE);
        return s.eb[key] ? s.eb[key][f] : 0.0f;
    }
    if (i < P_HB) {
        const int o = (int)((i - P_HW) / kPolE), f = (int)((i - P_HW) % kPolE);
        return o < s.head_n ? s.head_w[o * kPolE + f] : 0.0f;
    }
    if (i < P_SCALE) return (int)(i - P_HB) < s.head_n ? s.head_b[i - P_HB] : 0.0f;
    if (i < P_LOGSCALE) return s.log_std ? expf(s.log_std[i - P_SCALE]) : 1.0f;
    if (i < P_EW) return s.log_std ? logf(expf(s.log_std[i - P_LOGSCALE])) : 0.0f;   // torch Normal: scale.log()
    const long long e = i - P_EW;
    const int in = (int)(e / kPolE), f = (int)(e % kPolE);
    if (in < D) return s.ew[0][f * D + in];
    if (in < D + 3) return s.ew[1] ? s.ew[1][f * 3 + (in - D)] : 0.0f;
    return s.ew[2][f * 5 + (in - D - 3)];
}

__global__ __launch_bounds__(256) void hns_policy_pack_kernel(const PolNetSrc actor, const PolNetSrc critic, int D, float *img) {
    const long long n = pol_net_floats(D);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < 2 * n; i += (long long)gridDim.x * 256)
        img[i] = i < n ? pol_src(actor, D, i) : pol_src(critic, D, i - n);
}

struct PolArgs {
    const float *img;                        // actor image, critic image at + net_floats
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
    float x0[kPolE * kPolLd];                // token 0 / LN1 output
    float t1[kPolE * kPolLd];
    float t2[kPolE * kPolLd];
};

HNS_DEV f32x4 pmfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// OUT[128][R] = W[128][128] IN[128][R] + bias, then epilogue: 0 none, 1 exact gelu, 2 times 1/sqrt(128) (no bias)
template <int EPI>
HNS_DEV void pol_matvec(const float *__restrict__ W, const float *__restrict__ bias, const float *in, float *out, int w, int lane) {
    const int col = lane & 15, kq = lane >> 4;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 *A0 = reinterpret_cast<const f32x4 *>(W) + (2 * w) * 8 * 64 + lane;
    const f32x4 *A1 = A0 + 8 * 64;
#pragma unroll
    for (int s4 = 0; s4 < 8; ++s4) {
        const f32x4 a0 = A0[s4 * 64], a1 = A1[s4 * 64];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = 4 * (4 * s4 + u) + kq;
            const float b0 = in[k * kPolLd + col], b1 = in[k * kPolLd + 16 + col];
            acc[0][0] = pmfma(a0[u], b0, acc[0][0]);
            acc[0][1] = pmfma(a0[u], b1, acc[0][1]);
            acc[1][0] = pmfma(a1[u], b0, acc[1][0]);
            acc[1][1] = pmfma(a1[u], b1, acc[1][1]);
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int f = (2 * w + i) * 16 + 4 * kq + r;
            const float b = EPI == 2 ? 0.0f : bias[f];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                float v = acc[i][c][r];
                if (EPI == 2) v = v * 0.08838834764831845f;        // 1 / sqrt(128)
                else v = v + b;
                if (EPI == 1) v = 0.5f * v * (1.0f + erff(v * 0.7071067811865476f));
                out[f * kPolLd + c * 16 + col] = v;
            }
        }
}

// the thread's 16 features of a row: f = 4 g + 32 i + u (g = the lane in the row's group of eight)
HNS_DEV int pfeat(int g, int i, int u) { return 4 * g + 32 * i + u; }

HNS_DEV float row_sum8(float v) {
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    return v;
}

// LayerNorm(128) of the row's vector (16 values per thread), eps 1e-5, affine w / b from the image
HNS_DEV void pol_layernorm(float (&x)[16], const float *w, const float *b, int g) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += x[i];
    const float mean = row_sum8(s) * (1.0f / kPolE);
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        x[i] -= mean;
        q = __builtin_fmaf(x[i], x[i], q);
    }
    const float rstd = 1.0f / __builtin_sqrtf(row_sum8(q) * (1.0f / kPolE) + 1e-5f);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f32x4 wv = *reinterpret_cast<const f32x4 *>(w + pfeat(g, i, 0)), bv = *reinterpret_cast<const f32x4 *>(b + pfeat(g, i, 0));
#pragma unroll
        for (int u = 0; u < 4; ++u) x[4 * i + u] = (x[4 * i + u] * rstd) * wv[u] + bv[u];
    }
}

// token = LN(E^T-packed embedding of the n inputs at x (NULL: a padding row, zeros) + bias)
HNS_DEV void pol_token(const float *net, int key_off, int bias_off, const float *x, int n, int g, float (&t)[16]) {
    const float *eb = net + bias_off;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f32x4 b = *reinterpret_cast<const f32x4 *>(eb + pfeat(g, i, 0));
#pragma unroll
        for (int u = 0; u < 4; ++u) t[4 * i + u] = b[u];
    }
    if (x) {
        for (int k = 0; k < n; ++k) {
            const float xv = x[k];
            const float *wr = net + key_off + k * kPolE;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 wv = *reinterpret_cast<const f32x4 *>(wr + pfeat(g, i, 0));
#pragma unroll
                for (int u = 0; u < 4; ++u) t[4 * i + u] = __builtin_fmaf(wv[u], xv, t[4 * i + u]);
            }
        }
    }
    pol_layernorm(t, net + P_LNW, net + P_LNB, g);
}

HNS_DEV void lds_row_load(const float *buf, int r, int g, float (&x)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int u = 0; u < 4; ++u) x[4 * i + u] = buf[pfeat(g, i, u) * kPolLd + r];
}

HNS_DEV void lds_row_store(float *buf, int r, int g, const float (&x)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int u = 0; u < 4; ++u) buf[pfeat(g, i, u) * kPolLd + r] = x[4 * i + u];
}

// one network on the workgroup's rows; leaves the encoder output y (the thread's 16 features of row r) in `y`
HNS_DEV void pol_encoder(const PolArgs &a, const float *net, PolLds &L, int w, int lane, int r, int g, long long row, float (&y)[16]) {
    const bool live = row < a.rows;
    const long long e = live ? row / a.A : 0;
    const int ag = live ? (int)(row % a.A) : 0;
    const int D = a.D, eo = P_EW + D * kPolE, ec = eo + 3 * kPolE;
    const float *xs = live ? a.xs + e * a.sse + ag * a.ssa : nullptr;
    const float *xo = live && a.xo ? a.xo + e * a.soe + ag * a.soa : nullptr;
    const float *xc = live ? a.xc + e * a.sce + ag * a.sca : nullptr;

    float t[16];
    pol_token(net, P_EW, P_EB, xs, D, g, t);                      // token 0
    lds_row_store(L.x0, r, g, t);
    __syncthreads();
    pol_matvec<0>(net + P_MAT + 0 * kPolMat, net + P_BQ, L.x0, L.t1, w, lane);       // q
    __syncthreads();
    pol_matvec<2>(net + P_MAT + 1 * kPolMat, nullptr, L.t1, L.t2, w, lane);          // W_k^T q / sqrt(128)
    __syncthreads();

    // token pass: scores and online softmax, z = sum_j a_j t_j
    float kq[16], z[16];
    lds_row_load(L.t2, r, g, kq);
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s = __builtin_fmaf(kq[i], t[i], s);
    float m = row_sum8(s), l = 1.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = t[i];
    const int N = a.A + a.K;
    for (int j = 1; j < N; ++j) {
        if (j < a.A) pol_token(net, eo, P_EB + kPolE, xo ? xo + (j - 1) * a.sot : nullptr, 3, g, t);
        else pol_token(net, ec, P_EB + 2 * kPolE, xc ? xc + (j - a.A) * a.sct : nullptr, 5, g, t);
        s = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) s = __builtin_fmaf(kq[i], t[i], s);
        s = row_sum8(s);
        const float mn = s > m ? s : m;
        const float c = expf(m - mn), p = expf(s - mn);
        l = l * c + p;
#pragma unroll
        for (int i = 0; i < 16; ++i) z[i] = __builtin_fmaf(p, t[i], z[i] * c);
        m = mn;
    }
    const float il = 1.0f / l;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] *= il;
    lds_row_store(L.t1, r, g, z);
    __syncthreads();
    pol_matvec<0>(net + P_MAT + 2 * kPolMat, net + P_BV, L.t1, L.t2, w, lane);       // v = W_v z + b_v
    __syncthreads();
    pol_matvec<0>(net + P_MAT + 3 * kPolMat, net + P_BO, L.t2, L.t1, w, lane);       // attn = W_o v + b_o
    __syncthreads();
    float x[16];
    lds_row_load(L.x0, r, g, x);
    lds_row_load(L.t1, r, g, t);
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] += t[i];
    pol_layernorm(x, net + P_N1W, net + P_N1B, g);                // x0' = LN1(x0 + attn)
    lds_row_store(L.x0, r, g, x);
    __syncthreads();
    pol_matvec<1>(net + P_MAT + 4 * kPolMat, net + P_B1, L.x0, L.t1, w, lane);       // gelu(W_1 x0' + b_1)
    __syncthreads();
    pol_matvec<0>(net + P_MAT + 5 * kPolMat, net + P_B2, L.t1, L.t2, w, lane);       // W_2 h + b_2
    __syncthreads();
    lds_row_load(L.t2, r, g, t);
#pragma unroll
    for (int i = 0; i < 16; ++i) y[i] = x[i] + t[i];
    pol_layernorm(y, net + P_N2W, net + P_N2B, g);                // y = LN2(x0' + ff)
}

HNS_DEV float pol_head(const float *net, int o, const float (&y)[16], int g) {
    const float *hw = net + P_HW + o * kPolE;
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f32x4 wv = *reinterpret_cast<const f32x4 *>(hw + pfeat(g, i, 0));
#pragma unroll
        for (int u = 0; u < 4; ++u) s = __builtin_fmaf(wv[u], y[4 * i + u], s);
    }
    return row_sum8(s) + net[P_HB + o];
}

__global__ __launch_bounds__(kPolThreads, 2) void hns_policy_forward_kernel(const PolArgs a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    PolLds &L = *reinterpret_cast<PolLds *>(lds_raw);
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = tid >> 3, g = tid & 7;
    const long long row = (long long)blockIdx.x * kPolRows + r;
    const bool live = row < a.rows;
    float y[16];

    if (!a.value_only) {
        const float *net = a.img;
        pol_encoder(a, net, L, w, lane, r, g, row, y);
        float loc[4];
#pragma unroll
        for (int o = 0; o < 4; ++o) loc[o] = pol_head(net, o, y, g);
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
        __syncthreads();                                          // the critic reuses the LDS
    }
    const float *net = a.img + a.net_floats;
    pol_encoder(a, net, L, w, lane, r, g, row, y);
    const float v = pol_head(net, 0, y, g);
    if (live && g == 0) a.value[row] = v;
}

__global__ void hns_policy_bump_kernel(unsigned long long *counter) { counter[0] += 1ull; }

}  // namespace hns

namespace {

int pol_net(const char *fn, const hns_policy_net *n, int D, int has_others, bool actor, hns::PolNetSrc &s) {
    if (!n) return hns_fail(fn, "null network");
    const float *req[] = {n->embed_self_w, n->embed_self_b, n->embed_cyl_w, n->embed_cyl_b, n->ln_w, n->ln_b, n->in_proj_w, n->in_proj_b,
                          n->out_proj_w, n->out_proj_b, n->linear1_w, n->linear1_b, n->linear2_w, n->linear2_b, n->norm1_w, n->norm1_b,
                          n->norm2_w, n->norm2_b, n->head_w, n->head_b};
    for (const float *p : req)
        if (!p || !hns_aligned(p, 4)) return hns_fail(fn, "every parameter pointer must be a non-NULL fp32 array");
    if (has_others && (!n->embed_others_w || !n->embed_others_b)) return hns_fail(fn, "state_others embedding missing (num_agents > 1)");
    if (actor && !n->log_std) return hns_fail(fn, "the actor needs log_std");
    s.ew[0] = n->embed_self_w; s.eb[0] = n->embed_self_b;
    s.ew[1] = has_others ? n->embed_others_w : nullptr; s.eb[1] = has_others ? n->embed_others_b : nullptr;
    s.ew[2] = n->embed_cyl_w; s.eb[2] = n->embed_cyl_b;
    s.ln_w = n->ln_w; s.ln_b = n->ln_b; s.in_w = n->in_proj_w; s.in_b = n->in_proj_b; s.out_w = n->out_proj_w; s.out_b = n->out_proj_b;
    s.l1_w = n->linear1_w; s.l1_b = n->linear1_b; s.l2_w = n->linear2_w; s.l2_b = n->linear2_b;
    s.n1_w = n->norm1_w; s.n1_b = n->norm1_b; s.n2_w = n->norm2_w; s.n2_b = n->norm2_b;
    s.head_w = n->head_w; s.head_b = n->head_b; s.log_std = actor ? n->log_std : nullptr; s.head_n = actor ? 4 : 1;
    (void)D;
    return HNS_OK;
}

}  // namespace

extern "C" {

size_t hns_policy_packed_bytes(int32_t self_dim) {
    if (self_dim < 1 || self_dim > hns::kPolMaxSelf) return 0;
    return (size_t)(2 * hns::pol_net_floats(self_dim)) * sizeof(float);
}

int hns_policy_pack(const hns_policy_net *actor, const hns_policy_net *critic, int32_t self_dim, int32_t num_agents, void *packed, void *stream) {
    const char *fn = "hns_policy_pack";
    if (self_dim < 1 || self_dim > hns::kPolMaxSelf) return hns_fail(fn, "self_dim must be in [1, " + std::to_string(hns::kPolMaxSelf) + "]");
    if (num_agents < 1 || num_agents > HNS_MAX_AGENTS) return hns_fail(fn, "num_agents must be in [1, 7]");
    if (!packed || !hns_aligned(packed, 16)) return hns_fail(fn, "packed image must be a 16-byte aligned device array");
    hns::PolNetSrc sa{}, sc{};
    int rc = pol_net(fn, actor, self_dim, num_agents > 1, true, sa);
    if (rc != HNS_OK) return rc;
    rc = pol_net(fn, critic, self_dim, num_agents > 1, false, sc);
    if (rc != HNS_OK) return rc;
    hipLaunchKernelGGL(hns::hns_policy_pack_kernel, dim3(512), dim3(256), 0, static_cast<hipStream_t>(stream), sa, sc, (int)self_dim,
                       static_cast<float *>(packed));
    HNS_CHECK_HIP(hipGetLastError());
    return HNS_OK;
}

int hns_policy_forward(const void *packed, int32_t self_dim, int64_t num_envs, int32_t num_agents, int32_t num_cylinders, const hns_policy_io *io,
                       int32_t flags, uint64_t seed, uint64_t *counter, void *stream) {
    const char *fn = "hns_policy_forward";
    if (!packed || !io || !hns_aligned(packed, 16)) return hns_fail(fn, "null or misaligned packed image / io");
    if (self_dim < 1 || self_dim > hns::kPolMaxSelf) return hns_fail(fn, "self_dim must be in [1, " + std::to_string(hns::kPolMaxSelf) + "]");
    if (num_agents < 1 || num_agents > HNS_MAX_AGENTS) return hns_fail(fn, "num_agents must be in [1, 7]");
    if (num_cylinders < 1 || num_cylinders > HNS_MAX_CYLINDERS) return hns_fail(fn, "num_cylinders must be in [1, 16]");
    if (num_envs < 1 || num_envs > ((int64_t)1 << 31) / HNS_MAX_AGENTS) return hns_fail(fn, "num_envs must be in [1, 2^31 / 7]");
    if (flags & ~(HNS_POLICY_DETERMINISTIC | HNS_POLICY_VALUE_ONLY)) return hns_fail(fn, "unknown flag");
    const bool value_only = flags & HNS_POLICY_VALUE_ONLY, det = flags & HNS_POLICY_DETERMINISTIC;
    if (!io->obs_self || !io->obs_cylinders || (num_agents > 1 && !io->obs_others)) return hns_fail(fn, "observation pointer missing");
    if (!hns_aligned(io->obs_self, 4) || !hns_aligned(io->obs_cylinders, 4) || (io->obs_others && !hns_aligned(io->obs_others, 4)))
        return hns_fail(fn, "misaligned observation");
    for (int k = 0; k < 2; ++k)
        if (io->self_stride[k] < 0) return hns_fail(fn, "negative stride");
    for (int k = 0; k < 3; ++k)
        if (io->others_stride[k] < 0 || io->cyl_stride[k] < 0) return hns_fail(fn, "negative stride");
    if (!io->value || !hns_aligned(io->value, 4)) return hns_fail(fn, "value output missing or misaligned");
    if (!value_only) {
        if (!io->action || !io->log_prob || !hns_aligned(io->action, 4) || !hns_aligned(io->log_prob, 4) || (io->loc && !hns_aligned(io->loc, 4)))
            return hns_fail(fn, "action / log_prob outputs missing or misaligned");
        if (!det && !io->eps && (!counter || !hns_aligned(counter, 8))) return hns_fail(fn, "sampling without eps needs the device call counter");
        if (io->eps && !hns_aligned(io->eps, 4)) return hns_fail(fn, "misaligned eps");
    }
    hns::PolArgs a{};
    a.img = static_cast<const float *>(packed);
    a.net_floats = hns::pol_net_floats(self_dim);
    a.xs = io->obs_self; a.xo = io->obs_others; a.xc = io->obs_cylinders;
    a.sse = io->self_stride[0]; a.ssa = io->self_stride[1];
    a.soe = io->others_stride[0]; a.soa = io->others_stride[1]; a.sot = io->others_stride[2];
    a.sce = io->cyl_stride[0]; a.sca = io->cyl_stride[1]; a.sct = io->cyl_stride[2];
    a.eps = io->eps; a.counter = reinterpret_cast<const unsigned long long *>(counter); a.seed = seed;
    a.action = io->action; a.loc = io->loc; a.logp = io->log_prob; a.value = io->value;
    a.rows = num_envs * num_agents; a.A = num_agents; a.K = num_cylinders; a.D = self_dim;
    a.deterministic = det; a.value_only = value_only;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&hns::hns_policy_forward_kernel),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(hns::PolLds));   // 72 KB: above the default cap
    HNS_CHECK_HIP(attr);
    const long long grid = (a.rows + hns::kPolRows - 1) / hns::kPolRows;
    hipLaunchKernelGGL(hns::hns_policy_forward_kernel, dim3((unsigned)grid), dim3(hns::kPolThreads), sizeof(hns::PolLds), st, a);
    HNS_CHECK_HIP(hipGetLastError());
    if (!value_only && !det && !io->eps) {
        hipLaunchKernelGGL(hns::hns_policy_bump_kernel, dim3(1), dim3(1), 0, st, reinterpret_cast<unsigned long long *>(counter));
        HNS_CHECK_HIP(hipGetLastError());
    }
    return HNS_OK;
}

}  // extern "C"
