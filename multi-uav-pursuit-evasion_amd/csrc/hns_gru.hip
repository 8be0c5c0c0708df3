// hns_gru.hip — the recurrent block of the reference's rnn heads as a differentiable op: forward pass and backpropagation through time.
//
// Reference: modules/rnn.py:32-89 (GRU: an nn.GRUCell stepped over the sequence, the carried state multiplied by 1 - is_init before every step,
// LayerNorm(h + x) behind it), input size = hidden size = 128.  include/hns.h states the semantics; DESIGN.md §7.11 the design.
//   hns_gru_fwd_kernel    : persistent workgroups of EIGHT waves walk 16-sequence tiles.  Wave w owns hidden units 16 w .. 16 w + 15 (the 48 gate
//                           rows r, z, n of them).  Its slice of W_hh (96 values per lane) stays in registers for the whole launch; W_ih's does
//                           not fit beside it in the 256 registers of two waves per SIMD (both: 8 registers spilled forward, 63 backward), so
//                           it is streamed from L2 every step as eight 16-byte loads per gate (196 KB per workgroup and step).  Per step the
//                           tile's x_t and masked h go through the LDS as the products' B operands; the accumulator tiles of the three gates
//                           hold the same (unit, sequence) pairs in the same lanes, so the cell runs in registers; the LayerNorm's two sums
//                           over the 128 units cross the waves through the LDS in a fixed order.
//   hns_gru_bwd_kernel    : the same tiles from t = L - 1 down to 0.  Each step recomputes its gates from x_t and h_{t-1} (h_hist), walks back
//                           through the LayerNorm and the cell, leaves the four gate gradients (d a_r, d a_z, d a_n, d a_hn) in the workspace for
//                           the weight gradients, and forms dx_t = W_ih^T dA_i + d LN and dh_{t-1} = W_hh^T dA_h + dh z: each wave the 16 units it
//                           owns over all 384 gate rows, the transposed operands streamed from L2 (no cross-wave sum).  LayerNorm gradients leave
//                           as one partial row per workgroup.
//   hns_gru_wgrad_kernel  : dW = sum_rows dA (x) operand over row ranges, per (range, matrix) a 128 x 128 partial and the bias partial (column sums
//                           of dA); x is read in place through its strides, h_{t-1} (masked) from h_hist / h0.
//   hns_gru_reduce_kernel : every gradient value = the fp64 sum of its partials in index order, written in the PyTorch layouts.
// Arithmetic: every matrix product is v_mfma_f32_16x16x4_f32 (exact f32 products, one rounding per accumulation step); the gates use the
// predictor's sigmoid and tanh (hns_tp_train.hip).  The x products come first in every gate's chain, then the h products: the order does not
// depend on L or on the tile, which is what makes a chained one-step call give the bits of the whole sequence.
// Determinism: tiles go to workgroups by index, every sum has a fixed order, no float atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "hns_device.h"
#include "hns_host.h"
#include "../../include/hns.h"

namespace hns {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kGruH = HNS_GRU_HIDDEN;        // input size = hidden size
constexpr int kGruTile = 16;                 // sequences per tile (the 16-wide MFMA column)
constexpr int kGruThreads = 512;             // eight waves, one per 16 hidden units
constexpr int kGruWaves = kGruThreads / 64;
constexpr int kGruMaxGroups = 256;           // one workgroup per CU of an MI355X (two waves per SIMD at 256 registers each)
constexpr int kGruMat = kGruH * kGruH;
constexpr int kGruGate = 4 * kGruH;          // floats per row of the gate gradients: d a_r, d a_z, d a_n, d a_hn
constexpr int kGruWgRows = 32;               // rows per staged tile of the weight-gradient kernel
constexpr int kGruWgLd = kGruH + 4;          // its LDS row stride
constexpr int kGruWgOut = kGruMat + kGruH;   // floats per (range, matrix) partial: the matrix, then the bias
constexpr int kGruMaxSplits = 256;
constexpr float kGruEps = 1e-5f;

struct GruArgs {
    const float *w_ih, *w_hh, *b_ih, *b_hh, *ln_w, *ln_b;
    const float *x;                          // sequence q, step t: x + (q / inner) s0 + (q % inner) s1 + t s2
    long long s0, s1, s2, inner, S;
    int L, tiles;
    const float *h0;                         // [S, 128] or NULL
    const unsigned char *is_init;            // [S, L] or NULL
    float *out, *h_last, *h_hist;            // forward
    const float *hist, *dout, *dh_last;      // backward
    float *dx, *dh0, *dgate, *lnpart;
};

HNS_DEV float gru_sigm(float z) { return 1.0f / (1.0f + expf(-z)); }
HNS_DEV f32x4 gru_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
HNS_DEV long long gru_seq_off(const GruArgs &a, long long q) { return (q / a.inner) * a.s0 + (q % a.inner) * a.s1; }

// LDS: x_t and the masked h_{t-1} of the tile as B operands [k][sequence]; the waves' partial sums of the LayerNorm; (backward) the gate gradients
struct GruLds {
    float xs[kGruH * kGruTile];
    float hs[kGruH * kGruTile];
    float red[4][kGruWaves][kGruTile];
};
struct GruBwdLds {
    GruLds f;
    float da[4][kGruH * kGruTile];
};

// a wave's operand slice of W_hh: row g 128 + 16 w + col, k = 4 s + kq
struct GruWeights {
    float hh[3][32];
};

// where value k of x_t sits in L.xs: the x products take k = 32 kq + s at step s (a lane's W_ih operands are then 32 consecutive floats of its
// row: eight 16-byte loads), and slot 4 s + kq keeps the B operand's LDS reads linear in the lane
HNS_DEV int gru_xslot(int k) { return 4 * (k & 31) + (k >> 5); }

HNS_DEV void gru_load_weights(const GruArgs &a, int w, int col, int kq, GruWeights &W) {
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int s = 0; s < 32; ++s) {
            W.hh[g][s] = a.w_hh[(g * kGruH + 16 * w + col) * kGruH + 4 * s + kq];
        }
}

// x_t of the tile into L.xs (thread: sequence tid & 15, values 4 (tid >> 4) ..), the lane's masked h cells into L.hs
HNS_DEV void gru_stage(GruLds &L, const GruArgs &a, const float *xrow, int t, int tid, int u0, int col, const f32x4 &h) {
    const int sseq = tid & 15, i4 = tid >> 4;
    const f32x4 xv = xrow ? *reinterpret_cast<const f32x4 *>(xrow + (long long)t * a.s2 + 4 * i4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) L.xs[gru_xslot(4 * i4 + j) * kGruTile + sseq] = xv[j];
#pragma unroll
    for (int r = 0; r < 4; ++r) L.hs[(u0 + r) * kGruTile + col] = h[r];
}

// the step's pre-activations: acc[0] = a_r, acc[1] = a_z (x part, then h part, on b_i + b_h), acc[2] = W_in x + b_in, acc[3] = W_hn h + b_hn;
// rows 4 kq + r of the wave's 16 units, column = the lane's sequence
HNS_DEV void gru_gates(const GruLds &L, const GruWeights &W, const GruArgs &a, int w, int u0, int col, int kq, f32x4 acc[4]) {
    const f32x4 bir = *reinterpret_cast<const f32x4 *>(a.b_ih + u0), bhr = *reinterpret_cast<const f32x4 *>(a.b_hh + u0);
    const f32x4 biz = *reinterpret_cast<const f32x4 *>(a.b_ih + kGruH + u0), bhz = *reinterpret_cast<const f32x4 *>(a.b_hh + kGruH + u0);
    acc[0] = bir + bhr;
    acc[1] = biz + bhz;
    acc[2] = *reinterpret_cast<const f32x4 *>(a.b_ih + 2 * kGruH + u0);
    acc[3] = *reinterpret_cast<const f32x4 *>(a.b_hh + 2 * kGruH + u0);
    // W_ih does not fit beside W_hh in 256 registers: its slice is streamed from L2 every step
    const float *wr = a.w_ih + (16 * w + col) * kGruH + 32 * kq;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const f32x4 w0 = *reinterpret_cast<const f32x4 *>(wr + 4 * j), w1 = *reinterpret_cast<const f32x4 *>(wr + kGruMat + 4 * j);
        const f32x4 w2 = *reinterpret_cast<const f32x4 *>(wr + 2 * kGruMat + 4 * j);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float b = L.xs[(4 * (4 * j + i) + kq) * kGruTile + col];
            acc[0] = gru_mfma(w0[i], b, acc[0]);
            acc[1] = gru_mfma(w1[i], b, acc[1]);
            acc[2] = gru_mfma(w2[i], b, acc[2]);
        }
    }
#pragma unroll
    for (int s = 0; s < 32; ++s) {
        const float b = L.hs[(4 * s + kq) * kGruTile + col];
        acc[0] = gru_mfma(W.hh[0][s], b, acc[0]);
        acc[1] = gru_mfma(W.hh[1][s], b, acc[1]);
        acc[3] = gru_mfma(W.hh[2][s], b, acc[3]);
    }
}

// the sum over a sequence's 128 units of the lanes' values `v` (already summed over the lane's four units): over kq in the wave, then the
// eight waves in index order through red[slot]; one barrier
HNS_DEV float gru_unit_sum(GruLds &L, int slot, float v, int w, int col, int kq) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (kq == 0) L.red[slot][w][col] = v;
    __syncthreads();
    float s = L.red[slot][0][col];
#pragma unroll
    for (int k = 1; k < kGruWaves; ++k) s += L.red[slot][k][col];
    return s;
}

__global__ __launch_bounds__(kGruThreads, 2) void hns_gru_fwd_kernel(const GruArgs a) {
    __shared__ __align__(16) GruLds L;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, col = lane & 15, kq = lane >> 4;
    const int u0 = 16 * w + 4 * kq;                             // the lane's four units
    GruWeights W;
    gru_load_weights(a, w, col, kq, W);
    const int Ls = a.L;
    for (int tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const long long q0 = (long long)tile * kGruTile, qc = q0 + col, qs = q0 + (tid & 15);
        const bool valid = qc < a.S;
        const long long xoff = valid ? gru_seq_off(a, qc) : 0;
        const float *xrow = qs < a.S ? a.x + gru_seq_off(a, qs) : nullptr;
        f32x4 h = (valid && a.h0) ? *reinterpret_cast<const f32x4 *>(a.h0 + qc * kGruH + u0) : f32x4{0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < Ls; ++t) {
            const float m = (valid && a.is_init && a.is_init[qc * Ls + t]) ? 0.0f : 1.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) h[r] = h[r] * m;
            gru_stage(L, a, xrow, t, tid, u0, col, h);
            __syncthreads();
            f32x4 acc[4];
            gru_gates(L, W, a, w, u0, col, kq, acc);
            f32x4 y;
            float s1 = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float rg = gru_sigm(acc[0][r]), zg = gru_sigm(acc[1][r]), ng = tanhf(acc[2][r] + rg * acc[3][r]);
                h[r] = (1.0f - zg) * ng + zg * h[r];
                y[r] = h[r] + L.xs[gru_xslot(u0 + r) * kGruTile + col];
                s1 += y[r];
            }
            const float mean = gru_unit_sum(L, 0, s1, w, col, kq) * (1.0f / kGruH);
            float s2 = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                y[r] = y[r] - mean;
                s2 += y[r] * y[r];
            }
            const float rstd = 1.0f / sqrtf(gru_unit_sum(L, 1, s2, w, col, kq) * (1.0f / kGruH) + kGruEps);
            if (valid) {
                const f32x4 lw = *reinterpret_cast<const f32x4 *>(a.ln_w + u0), lb = *reinterpret_cast<const f32x4 *>(a.ln_b + u0);
                f32x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = (y[r] * rstd) * lw[r] + lb[r];
                *reinterpret_cast<f32x4 *>(a.out + xoff + (long long)t * a.s2 + u0) = o;
                if (a.h_hist) *reinterpret_cast<f32x4 *>(a.h_hist + (qc * Ls + t) * kGruH + u0) = h;
            }
        }
        if (valid) *reinterpret_cast<f32x4 *>(a.h_last + qc * kGruH + u0) = h;
        __syncthreads();                                        // (the next tile's staging rewrites the LDS)
    }
}

__global__ __launch_bounds__(kGruThreads, 2) void hns_gru_bwd_kernel(const GruArgs a) {
    __shared__ __align__(16) GruBwdLds B;
    GruLds &L = B.f;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, col = lane & 15, kq = lane >> 4;
    const int u0 = 16 * w + 4 * kq;
    GruWeights W;
    gru_load_weights(a, w, col, kq, W);
    const int Ls = a.L;
    f32x4 dlnw = f32x4{0.f, 0.f, 0.f, 0.f}, dlnb = f32x4{0.f, 0.f, 0.f, 0.f};      // the lane's sequence only; summed over the lanes at the end
    for (int tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const long long q0 = (long long)tile * kGruTile, qc = q0 + col, qs = q0 + (tid & 15);
        const bool valid = qc < a.S;
        const long long xoff = valid ? gru_seq_off(a, qc) : 0;
        const float *xrow = qs < a.S ? a.x + gru_seq_off(a, qs) : nullptr;
        f32x4 dh = (valid && a.dh_last) ? *reinterpret_cast<const f32x4 *>(a.dh_last + qc * kGruH + u0) : f32x4{0.f, 0.f, 0.f, 0.f};
        for (int t = Ls - 1; t >= 0; --t) {
            f32x4 hp = f32x4{0.f, 0.f, 0.f, 0.f};
            if (valid) {
                if (t > 0) hp = *reinterpret_cast<const f32x4 *>(a.hist + (qc * Ls + t - 1) * kGruH + u0);
                else if (a.h0) hp = *reinterpret_cast<const f32x4 *>(a.h0 + qc * kGruH + u0);
            }
            const float m = (valid && a.is_init && a.is_init[qc * Ls + t]) ? 0.0f : 1.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) hp[r] = hp[r] * m;
            gru_stage(L, a, xrow, t, tid, u0, col, hp);
            __syncthreads();
            f32x4 acc[4];
            gru_gates(L, W, a, w, u0, col, kq, acc);
            f32x4 rg, zg, ng, xh;
            float s1 = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                rg[r] = gru_sigm(acc[0][r]);
                zg[r] = gru_sigm(acc[1][r]);
                ng[r] = tanhf(acc[2][r] + rg[r] * acc[3][r]);
                const float hn = (1.0f - zg[r]) * ng[r] + zg[r] * hp[r];
                xh[r] = hn + L.xs[gru_xslot(u0 + r) * kGruTile + col];
                s1 += xh[r];
            }
            const float mean = gru_unit_sum(L, 0, s1, w, col, kq) * (1.0f / kGruH);
            float s2 = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                xh[r] = xh[r] - mean;
                s2 += xh[r] * xh[r];
            }
            const float rstd = 1.0f / sqrtf(gru_unit_sum(L, 1, s2, w, col, kq) * (1.0f / kGruH) + kGruEps);
            // LayerNorm backward: dy = rstd (g - mean(g) - xhat mean(g xhat)), g = dout ln_w
            const f32x4 dout = valid ? *reinterpret_cast<const f32x4 *>(a.dout + xoff + (long long)t * a.s2 + u0) : f32x4{0.f, 0.f, 0.f, 0.f};
            const f32x4 lw = *reinterpret_cast<const f32x4 *>(a.ln_w + u0);
            f32x4 g;
            float sg = 0.0f, sgx = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                xh[r] = xh[r] * rstd;
                g[r] = dout[r] * lw[r];
                sg += g[r];
                sgx += g[r] * xh[r];
                dlnw[r] += dout[r] * xh[r];
                dlnb[r] += dout[r];
            }
            // (two sums behind one barrier: the slots differ)
            sg += __shfl_xor(sg, 16, 64);
            sg += __shfl_xor(sg, 32, 64);
            sgx += __shfl_xor(sgx, 16, 64);
            sgx += __shfl_xor(sgx, 32, 64);
            if (kq == 0) {
                L.red[2][w][col] = sg;
                L.red[3][w][col] = sgx;
            }
            __syncthreads();
            float mg = L.red[2][0][col], mgx = L.red[3][0][col];
#pragma unroll
            for (int k = 1; k < kGruWaves; ++k) {
                mg += L.red[2][k][col];
                mgx += L.red[3][k][col];
            }
            mg *= 1.0f / kGruH;
            mgx *= 1.0f / kGruH;
            f32x4 dy, dhz, dar, daz, dan, dahn;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                dy[r] = rstd * ((g[r] - mg) - xh[r] * mgx);
                const float dht = dh[r] + dy[r];                // d h_t: from the steps after t, and from out_t
                const float dn = dht * (1.0f - zg[r]), dz = dht * (hp[r] - ng[r]);
                dan[r] = dn * (1.0f - ng[r] * ng[r]);
                daz[r] = dz * (zg[r] * (1.0f - zg[r]));
                dar[r] = (dan[r] * acc[3][r]) * (rg[r] * (1.0f - rg[r]));
                dahn[r] = dan[r] * rg[r];
                dhz[r] = dht * zg[r];
                const int e = (u0 + r) * kGruTile + col;
                B.da[0][e] = dar[r];
                B.da[1][e] = daz[r];
                B.da[2][e] = dan[r];
                B.da[3][e] = dahn[r];
            }
            if (valid) {
                float *dg = a.dgate + (qc * Ls + t) * kGruGate + u0;
                *reinterpret_cast<f32x4 *>(dg) = dar;
                *reinterpret_cast<f32x4 *>(dg + kGruH) = daz;
                *reinterpret_cast<f32x4 *>(dg + 2 * kGruH) = dan;
                *reinterpret_cast<f32x4 *>(dg + 3 * kGruH) = dahn;
            }
            __syncthreads();
            // dx_t = W_ih^T dA_i, dh_{t-1} = W_hh^T dA_h for the wave's 16 units: k = gate row j = 4 s + kq over all 384 rows
            f32x4 dxa = f32x4{0.f, 0.f, 0.f, 0.f}, dha = f32x4{0.f, 0.f, 0.f, 0.f};
            const float *wi = a.w_ih + 16 * w + col, *wh = a.w_hh + 16 * w + col;
#pragma unroll 8
            for (int s = 0; s < 96; ++s) {
                const int j = 4 * s + kq, gt = s >> 5, e = (j & (kGruH - 1)) * kGruTile + col;
                const float bi = B.da[gt][e], bh = gt == 2 ? B.da[3][e] : bi;
                dxa = gru_mfma(wi[(long long)j * kGruH], bi, dxa);
                dha = gru_mfma(wh[(long long)j * kGruH], bh, dha);
            }
            if (valid) {
                f32x4 dxv;
#pragma unroll
                for (int r = 0; r < 4; ++r) dxv[r] = dxa[r] + dy[r];
                *reinterpret_cast<f32x4 *>(a.dx + xoff + (long long)t * a.s2 + u0) = dxv;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) dh[r] = (dha[r] + dhz[r]) * m;
        }
        if (valid && a.dh0) *reinterpret_cast<f32x4 *>(a.dh0 + qc * kGruH + u0) = dh;
        __syncthreads();
    }
    // this workgroup's LayerNorm partials: over the 16 sequences (lanes col = 0 .. 15 of this kq), fixed butterfly
    float *lp = a.lnpart + (long long)blockIdx.x * (2 * kGruH);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float sw = dlnw[r], sb = dlnb[r];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            sw += __shfl_xor(sw, o, 64);
            sb += __shfl_xor(sb, o, 64);
        }
        if (col == 0) {
            lp[u0 + r] = sw;
            lp[kGruH + u0 + r] = sb;
        }
    }
}

// dW partials: per (row range, matrix) the 128 x 128 product dA^T operand over the range's rows, and the column sums of dA.  Matrices 0-2:
// W_ih's r, z, n thirds (dA blocks 0, 1, 2; operand x_t); 3-5: W_hh's (dA blocks 0, 1, 3; operand the masked h_{t-1}).  Row = s L + t.
__global__ __launch_bounds__(256, 2) void hns_gru_wgrad_kernel(const GruArgs a, long long rows, int tiles, int tps, float *part) {
    __shared__ __align__(16) float sdy[kGruWgRows * kGruWgLd];
    __shared__ __align__(16) float sxx[kGruWgRows * kGruWgLd];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, col = lane & 15, kq = lane >> 4;
    const int m = blockIdx.y, split = blockIdx.x;
    const int blk = m < 3 ? m : (m == 5 ? 3 : m - 3);
    const int t0 = split * tps, t1 = t0 + tps < tiles ? t0 + tps : tiles;
    f32x4 acc[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bs0 = 0.0f, bs1 = 0.0f;
    for (int t = t0; t < t1; ++t) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i, rr = idx >> 5, c4 = idx & 31;
            const long long row = (long long)t * kGruWgRows + rr;
            f32x4 dv = f32x4{0.f, 0.f, 0.f, 0.f}, ov = f32x4{0.f, 0.f, 0.f, 0.f};
            if (row < rows) {
                dv = *reinterpret_cast<const f32x4 *>(a.dgate + row * kGruGate + blk * kGruH + 4 * c4);
                const long long q = row / a.L;
                const int st = (int)(row - q * a.L);
                if (m < 3) {
                    ov = *reinterpret_cast<const f32x4 *>(a.x + gru_seq_off(a, q) + (long long)st * a.s2 + 4 * c4);
                } else {
                    if (st > 0) ov = *reinterpret_cast<const f32x4 *>(a.hist + (row - 1) * kGruH + 4 * c4);
                    else if (a.h0) ov = *reinterpret_cast<const f32x4 *>(a.h0 + q * kGruH + 4 * c4);
                    const float mk = (a.is_init && a.is_init[row]) ? 0.0f : 1.0f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) ov[j] = ov[j] * mk;
                }
            }
            *reinterpret_cast<f32x4 *>(&sdy[rr * kGruWgLd + 4 * c4]) = dv;
            *reinterpret_cast<f32x4 *>(&sxx[rr * kGruWgLd + 4 * c4]) = ov;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int k = 4 * s + kq;
            const float a0 = sdy[k * kGruWgLd + (2 * w) * 16 + col], a1 = sdy[k * kGruWgLd + (2 * w + 1) * 16 + col];
            bs0 += a0;
            bs1 += a1;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float b = sxx[k * kGruWgLd + c * 16 + col];
                acc[0][c] = gru_mfma(a0, b, acc[0][c]);
                acc[1][c] = gru_mfma(a1, b, acc[1][c]);
            }
        }
        __syncthreads();
    }
    float *out = part + ((long long)split * 6 + m) * kGruWgOut;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int c = 0; c < 8; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[((2 * w + i) * 16 + 4 * kq + r) * kGruH + c * 16 + col] = acc[i][c][r];
    bs0 += __shfl_xor(bs0, 16, 64);
    bs0 += __shfl_xor(bs0, 32, 64);
    bs1 += __shfl_xor(bs1, 16, 64);
    bs1 += __shfl_xor(bs1, 32, 64);
    if (kq == 0) {
        out[kGruMat + (2 * w) * 16 + col] = bs0;
        out[kGruMat + (2 * w + 1) * 16 + col] = bs1;
    }
}

struct GruGradOut {
    float *w_ih, *w_hh, *b_ih, *b_hh, *ln_w, *ln_b;
};

constexpr int kGruReduceN = 6 * kGruWgOut + 2 * kGruH;

// gradient value e: the fp64 sum of its partials in index order, rounded once.  e < 6 (128 128 + 128): matrix m's value or bias over the row
// ranges; then ln_w [128], ln_b [128] over the sweep's workgroups
__global__ __launch_bounds__(256) void hns_gru_reduce_kernel(const float *wpart, int splits, const float *lnpart, int groups, const GruGradOut o) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= kGruReduceN) return;
    double acc = 0.0;
    if (e < 6 * kGruWgOut) {
        const int m = e / kGruWgOut, x = e % kGruWgOut;
        for (int s = 0; s < splits; ++s) acc += (double)wpart[((long long)s * 6 + m) * kGruWgOut + x];
        const float v = (float)acc;
        if (x < kGruMat) (m < 3 ? o.w_ih + m * kGruMat : o.w_hh + (m - 3) * kGruMat)[x] = v;
        else (m < 3 ? o.b_ih + m * kGruH : o.b_hh + (m - 3) * kGruH)[x - kGruMat] = v;
    } else {
        const int f = e - 6 * kGruWgOut;
        for (int g = 0; g < groups; ++g) acc += (double)lnpart[(long long)g * (2 * kGruH) + f];
        (f < kGruH ? o.ln_w : o.ln_b - kGruH)[f] = (float)acc;
    }
}

}  // namespace hns

namespace {

struct GruPlan {
    long long rows;
    int tiles, groups, wg_tiles, tps, splits;
    size_t o_gate, o_wpart, o_ln, bytes;
};

size_t gru_round(size_t n) { return (n + 255) / 256 * 256; }

bool gru_plan(int64_t seqs, int32_t steps, GruPlan &p) {
    if (seqs < 1 || steps < 1 || steps > HNS_GRU_MAX_STEPS || seqs >= ((int64_t)1 << 40) / steps) return false;
    p.rows = seqs * steps;
    const long long tiles = (seqs + hns::kGruTile - 1) / hns::kGruTile;
    if (tiles > 0x7fffffffLL) return false;
    p.tiles = (int)tiles;
    p.groups = (int)std::min<long long>(tiles, hns::kGruMaxGroups);
    const long long wg = (p.rows + hns::kGruWgRows - 1) / hns::kGruWgRows;
    if (wg > 0x7fffffffLL) return false;
    p.wg_tiles = (int)wg;
    p.tps = (p.wg_tiles + hns::kGruMaxSplits - 1) / hns::kGruMaxSplits;
    p.splits = (p.wg_tiles + p.tps - 1) / p.tps;
    p.o_gate = 0;
    p.o_wpart = gru_round((size_t)p.rows * hns::kGruGate * sizeof(float));
    p.o_ln = p.o_wpart + gru_round((size_t)p.splits * 6 * hns::kGruWgOut * sizeof(float));
    p.bytes = p.o_ln + gru_round((size_t)p.groups * 2 * hns::kGruH * sizeof(float));
    return true;
}

// the checks both entries share; fills the kernels' arguments
int gru_check(const char *fn, const hns_gru_net *net, const hns_gru_seq *seq, hns::GruArgs &a, GruPlan &p) {
    if (!net || !seq) return hns_fail(fn, "null pointer");
    const float *pw[6] = {net->weight_ih, net->weight_hh, net->bias_ih, net->bias_hh, net->ln_w, net->ln_b};
    for (int k = 0; k < 6; ++k)
        if (!pw[k] || !hns_aligned(pw[k], 16)) return hns_fail(fn, "parameter pointers must be non-NULL and 16-byte aligned");
    if (!seq->x || !hns_aligned(seq->x, 16)) return hns_fail(fn, "x must be non-NULL and 16-byte aligned");
    if (seq->steps < 1 || seq->steps > HNS_GRU_MAX_STEPS) return hns_fail(fn, "steps must be in [1, 64]");
    if (seq->outer < 1 || seq->inner < 1) return hns_fail(fn, "outer and inner must be >= 1");
    if (seq->outer >= ((int64_t)1 << 40) / seq->inner || !gru_plan(seq->outer * seq->inner, seq->steps, p))
        return hns_fail(fn, "outer x inner x steps must be below 2^40");
    for (int k = 0; k < 3; ++k)
        if (seq->x_stride[k] < 0 || (seq->x_stride[k] & 3)) return hns_fail(fn, "strides must be >= 0 and multiples of 4 floats");
    if ((seq->h0 && !hns_aligned(seq->h0, 16))) return hns_fail(fn, "h0 must be 16-byte aligned");
    a = hns::GruArgs{};
    a.w_ih = pw[0]; a.w_hh = pw[1]; a.b_ih = pw[2]; a.b_hh = pw[3]; a.ln_w = pw[4]; a.ln_b = pw[5];
    a.x = seq->x; a.s0 = seq->x_stride[0]; a.s1 = seq->x_stride[1]; a.s2 = seq->x_stride[2];
    a.inner = seq->inner; a.S = seq->outer * seq->inner; a.L = seq->steps; a.tiles = p.tiles;
    a.h0 = seq->h0; a.is_init = seq->is_init;
    return HNS_OK;
}

}  // namespace

extern "C" {

size_t hns_gru_workspace_bytes(int64_t seqs, int32_t steps, int32_t backward) {
    GruPlan p;
    if (!gru_plan(seqs, steps, p)) return 0;
    return backward ? p.bytes : 0;
}

int hns_gru_forward(const hns_gru_net *net, const hns_gru_seq *seq, float *out, float *h_last, float *h_hist, void *workspace, size_t workspace_bytes,
                    void *stream) {
    const char *fn = "hns_gru_forward";
    hns::GruArgs a;
    GruPlan p;
    const int rc = gru_check(fn, net, seq, a, p);
    if (rc != HNS_OK) return rc;
    (void)workspace_bytes;
    if (!out || !h_last || !hns_aligned(out, 16) || !hns_aligned(h_last, 16)) return hns_fail(fn, "out and h_last must be non-NULL and 16-byte aligned");
    if (h_hist && !hns_aligned(h_hist, 16)) return hns_fail(fn, "h_hist must be 16-byte aligned");
    if (workspace && !hns_aligned(workspace, 256)) return hns_fail(fn, "workspace must be 256-byte aligned");
    a.out = out; a.h_last = h_last; a.h_hist = h_hist;
    hipLaunchKernelGGL(hns::hns_gru_fwd_kernel, dim3(p.groups), dim3(hns::kGruThreads), 0, static_cast<hipStream_t>(stream), a);
    HNS_CHECK_HIP(hipGetLastError());
    return HNS_OK;
}

int hns_gru_backward(const hns_gru_net *net, const hns_gru_seq *seq, const float *h_hist, const float *dout, const float *dh_last,
                     const hns_gru_grads *grads, float *dx, float *dh0, void *workspace, size_t workspace_bytes, void *stream) {
    const char *fn = "hns_gru_backward";
    hns::GruArgs a;
    GruPlan p;
    const int rc = gru_check(fn, net, seq, a, p);
    if (rc != HNS_OK) return rc;
    if (!grads) return hns_fail(fn, "null pointer");
    float *gw[6] = {grads->weight_ih, grads->weight_hh, grads->bias_ih, grads->bias_hh, grads->ln_w, grads->ln_b};
    for (int k = 0; k < 6; ++k)
        if (!gw[k] || !hns_aligned(gw[k], 16)) return hns_fail(fn, "gradient pointers must be non-NULL and 16-byte aligned");
    if (!h_hist) return hns_fail(fn, "h_hist is required: the forward pass's hidden states");
    if (!dout || !dx || !hns_aligned(h_hist, 16) || !hns_aligned(dout, 16) || !hns_aligned(dx, 16))
        return hns_fail(fn, "h_hist, dout and dx must be non-NULL and 16-byte aligned");
    if ((dh_last && !hns_aligned(dh_last, 16)) || (dh0 && !hns_aligned(dh0, 16))) return hns_fail(fn, "dh_last and dh0 must be 16-byte aligned");
    if (!workspace || !hns_aligned(workspace, 256)) return hns_fail(fn, "workspace must be non-NULL and 256-byte aligned");
    if (workspace_bytes < p.bytes) return hns_fail(fn, "workspace too small");
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    float *wpart = reinterpret_cast<float *>(ws + p.o_wpart);
    a.hist = h_hist; a.dout = dout; a.dh_last = dh_last; a.dx = dx; a.dh0 = dh0;
    a.dgate = reinterpret_cast<float *>(ws + p.o_gate);
    a.lnpart = reinterpret_cast<float *>(ws + p.o_ln);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(hns::hns_gru_bwd_kernel, dim3(p.groups), dim3(hns::kGruThreads), 0, st, a);
    HNS_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(hns::hns_gru_wgrad_kernel, dim3(p.splits, 6), dim3(256), 0, st, a, p.rows, p.wg_tiles, p.tps, wpart);
    HNS_CHECK_HIP(hipGetLastError());
    const hns::GruGradOut o{gw[0], gw[1], gw[2], gw[3], gw[4], gw[5]};
    hipLaunchKernelGGL(hns::hns_gru_reduce_kernel, dim3((hns::kGruReduceN + 255) / 256), dim3(256), 0, st, wpart, p.splits, a.lnpart, p.groups, o);
    HNS_CHECK_HIP(hipGetLastError());
    return HNS_OK;
}

}  // extern "C"
