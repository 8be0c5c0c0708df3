// hns_encoder.h — what the forward pass (hns_policy.hip) and the updates (hns_policy_train.hip) share of the PartialAttentionEncoder, each piece
// once: the tile shape, the MFMA matrix-vector product, the eight-lanes-per-row helpers, LayerNorm, the token embedding, the online-softmax
// step, the parameter table and the packed fragment order of the 128 x 128 matrices.
//
// Tile: kEncRows rows per workgroup of kEncThreads threads.  Activations live in LDS as [128 features][kEncRows rows] at pitch kEncLd; wave w
// owns output row blocks 2w, 2w + 1 of every product.  On the VALU phases row r = tid >> 3 belongs to the eight lanes g = tid & 7, 16 features
// each (enc_feat); sums over a row are a fixed butterfly over those lanes (row_sum8).  The functions take plain pointers: the forward kernel
// hands them sections of its packed image, the training kernel the live tensors.
#pragma once
#include <hip/hip_runtime.h>

#include "hns_device.h"

namespace hns {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kEncE = 128;                   // embed_dim = dim_feedforward
constexpr int kEncRows = 32;                 // rows per tile (two 16-wide MFMA column blocks)
constexpr int kEncLd = kEncRows + 16;        // LDS row pitch in floats: the four k-quads of a B-operand read fall in distinct bank groups
constexpr int kEncThreads = 256;
constexpr int kEncMat = kEncE * kEncE;

// one network's parameters (PyTorch layouts)
struct EncNet {
    const float *ew[3], *eb[3], *ln_w, *ln_b, *in_w, *in_b, *out_w, *out_b, *l1_w, *l1_b, *l2_w, *l2_b, *n1_w, *n1_b, *n2_w, *n2_b, *head_w, *head_b;
    const float *log_std;                    // the actor only (NULL: the critic)
    int head_n;                              // 4 (actor) / 1 (critic); the forward pass' pack kernel alone reads it
};

// X(field of hns_policy_net and hns_policy_grads, member of EncNet and CtGrad): every tensor both networks always have.  The state_others embedding
// (absent with one agent) and log_std (the actor's) follow by hand where a table is filled.
#define HNS_CT_FIELDS(X)                                                                                                                       \
    X(embed_self_w, ew[0]) X(embed_self_b, eb[0]) X(embed_cyl_w, ew[2]) X(embed_cyl_b, eb[2]) X(ln_w, ln_w) X(ln_b, ln_b) X(in_proj_w, in_w)   \
    X(in_proj_b, in_b) X(out_proj_w, out_w) X(out_proj_b, out_b) X(linear1_w, l1_w) X(linear1_b, l1_b) X(linear2_w, l2_w) X(linear2_b, l2_b)   \
    X(norm1_w, n1_w) X(norm1_b, n1_b) X(norm2_w, n2_w) X(norm2_b, n2_b) X(head_w, head_w) X(head_b, head_b)

// One actor per agent (share_actor: false): every tensor is stacked over the agents, [A, ...] in its PyTorch layout, so agent
// `ag`'s slice is a contiguous network of its own.  T: EncNet, or the training kernels' gradient table (the same members); `heads`: head_w's rows.
template <typename T>
static __host__ __device__ __forceinline__ T enc_agent_slice(T s, int D, int heads, int ag) {
    s.ew[0] += ag * kEncE * D; s.eb[0] += ag * kEncE;
    if (s.ew[1]) { s.ew[1] += ag * kEncE * 3; s.eb[1] += ag * kEncE; }
    s.ew[2] += ag * kEncE * 5; s.eb[2] += ag * kEncE;
    s.ln_w += ag * kEncE; s.ln_b += ag * kEncE;
    s.in_w += ag * 3 * kEncMat; s.in_b += ag * 3 * kEncE;
    s.out_w += ag * kEncMat; s.out_b += ag * kEncE;
    s.l1_w += ag * kEncMat; s.l1_b += ag * kEncE; s.l2_w += ag * kEncMat; s.l2_b += ag * kEncE;
    s.n1_w += ag * kEncE; s.n1_b += ag * kEncE; s.n2_w += ag * kEncE; s.n2_b += ag * kEncE;
    s.head_w += ag * heads * kEncE; s.head_b += ag * heads;
    if (s.log_std) s.log_std += ag * heads;
    return s;
}

// float x of packed matrix m, in MFMA A-operand fragment order (one float4 per lane per four k-steps): m 0-5 are Q, K^T, V, O, L1, L2, m 6-11
// their transposes (the backward pass' operands)
HNS_DEV float enc_mat_src(const EncNet &s, int m, int x) {
    const int u = x & 3, lane = (x >> 2) & 63, s4 = (x >> 8) & 7, rb = x >> 11;
    const int row = rb * 16 + (lane & 15), k = 4 * (4 * s4 + u) + (lane >> 4);
    const int a = m >= 6 ? k : row, b = m >= 6 ? row : k;            // element [a][b] of the forward-orientation matrix
    switch (m % 6) {
        case 0: return s.in_w[a * kEncE + b];
        case 1: return s.in_w[(kEncE + b) * kEncE + a];              // W_k^T
        case 2: return s.in_w[(2 * kEncE + a) * kEncE + b];
        case 3: return s.out_w[a * kEncE + b];
        case 4: return s.l1_w[a * kEncE + b];
        default: return s.l2_w[a * kEncE + b];
    }
}

HNS_DEV f32x4 enc_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// OUT[128][R] = W[128][128] IN[128][R]; EPI 0: + bias; 1: gelu(. + bias); 2: times 1/sqrt(128); 3: nothing; 4: . + bias to out2, its gelu to out.
// `stage` (or NULL): the tile's [32][128] block of a staging array, receives what `out` receives.
template <int EPI>
HNS_DEV void enc_matvec(const float *__restrict__ W, const float *__restrict__ bias, const float *in, float *out, float *out2, float *stage, int w, int lane) {
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
            const float b0 = in[k * kEncLd + col], b1 = in[k * kEncLd + 16 + col];
            acc[0][0] = enc_mfma(a0[u], b0, acc[0][0]);
            acc[0][1] = enc_mfma(a0[u], b1, acc[0][1]);
            acc[1][0] = enc_mfma(a1[u], b0, acc[1][0]);
            acc[1][1] = enc_mfma(a1[u], b1, acc[1][1]);
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int f0 = (2 * w + i) * 16 + 4 * kq;
        f32x4 o[2];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float b = (EPI == 2 || EPI == 3) ? 0.0f : bias[f0 + r];
#pragma unroll
            for (int c = 0; c < 2; ++c) {                           // the two column blocks side by side: their LDS stores pair
                float v = acc[i][c][r];
                if (EPI == 2) v = v * 0.08838834764831845f;        // 1 / sqrt(128)
                else if (EPI != 3) v = v + b;
                if (EPI == 4) out2[(f0 + r) * kEncLd + c * 16 + col] = v;
                if (EPI == 1 || EPI == 4) v = 0.5f * v * (1.0f + erff(v * 0.7071067811865476f));
                out[(f0 + r) * kEncLd + c * 16 + col] = v;
                o[c][r] = v;
            }
        }
        if (stage) {
#pragma unroll
            for (int c = 0; c < 2; ++c) *reinterpret_cast<f32x4 *>(stage + (c * 16 + col) * kEncE + f0) = o[c];
        }
    }
}

// the thread's 16 features of a row: f = 4 g + 32 i + u (g = the lane in the row's group of eight)
HNS_DEV int enc_feat(int g, int i, int u) { return 4 * g + 32 * i + u; }

HNS_DEV float row_sum8(float v) {
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    return v;
}

// the thread's 16 values of a [128] vector
HNS_DEV void enc_vec_load(const float *p, int g, float (&x)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(p + enc_feat(g, i, 0));
#pragma unroll
        for (int u = 0; u < 4; ++u) x[4 * i + u] = v[u];
    }
}

// row r of a [feature][row] LDS buffer
HNS_DEV void enc_lds_load(const float *buf, int r, int g, float (&x)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int u = 0; u < 4; ++u) x[4 * i + u] = buf[enc_feat(g, i, u) * kEncLd + r];
}

HNS_DEV void enc_lds_store(float *buf, int r, int g, const float (&x)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int u = 0; u < 4; ++u) buf[enc_feat(g, i, u) * kEncLd + r] = x[4 * i + u];
}

// LayerNorm(128) of the row's vector, eps 1e-5: xh = the normalised vector, y = xh w + b; returns 1 / std
HNS_DEV float enc_layernorm(const float (&x)[16], const float *w, const float *b, int g, float (&xh)[16], float (&y)[16]) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += x[i];
    const float mean = row_sum8(s) * (1.0f / kEncE);
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        xh[i] = x[i] - mean;
        q = __builtin_fmaf(xh[i], xh[i], q);
    }
    const float rstd = 1.0f / __builtin_sqrtf(row_sum8(q) * (1.0f / kEncE) + 1e-5f);
    float wv[16], bv[16];
    enc_vec_load(w, g, wv);
    enc_vec_load(b, g, bv);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        xh[i] = xh[i] * rstd;
        y[i] = xh[i] * wv[i] + bv[i];
    }
    return rstd;
}

// token = LN(embedding of the n inputs at x (NULL: a padding row, zeros) + bias): t, its normalised vector xh; returns 1 / std.  ewT: the
// embedding weight transposed, [n][128].  BIAS_FIRST: the fma chain starts from the bias (the forward pass); otherwise the bias joins last, one
// rounding at its magnitude as F.linear (the updates: near-constant tokens).  The two orders give different bits.  The first
// bias is one float4 per four features at its use, not enc_vec_load: the forward kernel's register allocation follows that shape, and with
// enc_vec_load it was 5 % slower (profiles/r15_encoder_fold.txt).
template <bool BIAS_FIRST>
HNS_DEV float enc_token(const float *ewT, const float *eb, const float *x, int n, const float *lnw, const float *lnb, int g, float (&xh)[16], float (&t)[16]) {
    float e[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f32x4 b = BIAS_FIRST ? *reinterpret_cast<const f32x4 *>(eb + enc_feat(g, i, 0)) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 4; ++u) e[4 * i + u] = b[u];
    }
    if (x) {
        for (int k = 0; k < n; ++k) {
            const float xv = x[k];
            const float *wr = ewT + k * kEncE;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 wv = *reinterpret_cast<const f32x4 *>(wr + enc_feat(g, i, 0));
#pragma unroll
                for (int u = 0; u < 4; ++u) e[4 * i + u] = __builtin_fmaf(wv[u], xv, e[4 * i + u]);
            }
        }
    }
    if (!BIAS_FIRST) {
        float eb16[16];
        enc_vec_load(eb, g, eb16);
#pragma unroll
        for (int i = 0; i < 16; ++i) e[i] += eb16[i];
    }
    return enc_layernorm(e, lnw, lnb, g, xh, t);
}

// the row's score of token t against kq = W_k^T q / sqrt(128)
HNS_DEV float enc_score(const float (&kq)[16], const float (&t)[16]) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s = __builtin_fmaf(kq[i], t[i], s);
    return row_sum8(s);
}

// one online-softmax step: token t joins the running max m, the sum l and z = sum_j exp(s_j - m) t_j
HNS_DEV void enc_softmax_step(const float (&kq)[16], const float (&t)[16], float &m, float &l, float (&z)[16]) {
    const float s = enc_score(kq, t);
    const float mn = s > m ? s : m;
    const float c = expf(m - mn), p = expf(s - mn);
    l = l * c + p;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = __builtin_fmaf(p, t[i], z[i] * c);
    m = mn;
}

}  // namespace hns
