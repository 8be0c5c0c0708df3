// hns_tp_train.hip — the trajectory predictor's training step on the device: loss and gradients of one minibatch (the Adam step is hns_adam.hip's).
//
// Reference: MAPPOPolicy.update_TP (omni_drones/learning/mappo.py:252-268) driven by train_op (:405-441): TP_net (:572-589: LSTM(I -> 64, one
// layer, zero initial state, gate order i, f, g, o) + Linear(64 -> 3F) + tanh) on a [B, T, I] minibatch, nn.MSELoss against [B, 3F], autograd
// backward, torch.optim.Adam(lr 1e-4).  Here
//   hns_tp_grad_kernel   : persistent workgroups of four waves walk 16-sequence tiles.  Per tile: the forward sweep keeps h_t / c_t of every step
//                          in LDS (T x 8 KB), the output layer and the MSE derivative run on the VALU, the backward sweep recomputes each step's
//                          gates from x_t and h_{t-1} and accumulates dW_ih, dW_hh and the bias gradient in registers.  Wave w owns hidden units
//                          16 w .. 16 w + 15 (the 64 gate rows i, f, g, o of them): its 16x16 accumulator tiles hold the four gates of the same
//                          (unit, sequence) pairs in the same lanes, so the cell runs in registers.  dh_{t-1} = W_hh^T dA_t is summed over the
//                          four waves' partial products in LDS in a fixed order.  Each workgroup writes its partial gradients to the workspace.
//   hns_tp_grad_sum_kernel : one thread per gradient value sums the workgroups' partials in index order in fp64, writes b_ih and b_hh from the same sum.
// Arithmetic: every matrix product is v_mfma_f32_16x16x4_f32 (exact f32 products, one rounding per accumulation step); the activations use
// the library's expf / tanhf.  Determinism: tiles go to workgroups by index, every sum has a fixed order, no float atomics — the same inputs
// give the same bits on every run.  Workspace: kTrainMaxGroups partial-gradient rows at most, whatever B and T are.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "hns_device.h"
#include "hns_host.h"
#include "../../include/hns.h"

namespace hns {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTrainTile = 16;               // sequences per tile (the 16-wide MFMA column)
constexpr int kTrainThreads = 256;           // four waves, one per 16 hidden units
constexpr int kTrainMaxGroups = 256;         // one workgroup per CU of an MI355X; the grid depends on the shape alone
constexpr int kTrainH = HNS_TP_HIDDEN;
constexpr int kTrainG = 4 * kTrainH;         // gate rows
constexpr int kTrainMaxT = 16, kTrainMaxI = 80, kTrainMaxF3 = 30;

struct TrainArgs {
    const float *x;                          // row r of the flattened [E, S]: x + (r / S) sE + (r % S) sS, a contiguous [T, I] block
    long long sE, sS, S, rows;               // rows = E S
    const float *y;                          // [rows, 3F]
    const long long *index;                  // [B] or NULL (rows 0 .. B - 1)
    long long B;
    const float *w_ih, *w_hh, *b_ih, *b_hh, *w_fc, *b_fc;
    int T, I, F3, tiles, P;                  // P: floats per workgroup partial
    float gscale;                            // 2 / (B 3F): d(mean sq)/d(diff)
    float *part;
};

// partial row layout: [dW_ih 256 I][dW_hh 256 64][db 256][dW_fc 3F 64][db_fc 3F][sum sq]
static __host__ __device__ __forceinline__ long long off_whh(int I) { return (long long)kTrainG * I; }
static __host__ __device__ __forceinline__ long long off_b(int I) { return off_whh(I) + kTrainG * kTrainH; }
static __host__ __device__ __forceinline__ long long off_wfc(int I) { return off_b(I) + kTrainG; }
static __host__ __device__ __forceinline__ long long off_bfc(int I, int F3) { return off_wfc(I) + (long long)F3 * kTrainH; }

HNS_DEV float sigm(float z) { return 1.0f / (1.0f + expf(-z)); }

HNS_DEV f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// the row of flattened sequence r (or NULL: past B or an index outside [0, rows))
HNS_DEV const float *seq_row(const TrainArgs &a, long long q) {
    if (q >= a.B) return nullptr;
    const long long r = a.index ? a.index[q] : q;
    if (r < 0 || r >= a.rows) return nullptr;
    return a.x + (r / a.S) * a.sE + (r % a.S) * a.sS;
}

HNS_DEV long long seq_id(const TrainArgs &a, long long q) { return a.index ? a.index[q] : q; }

// LDS: h history [T][64 units][16 seqs], c history [T][4 waves][4][64 lanes] (lane-private), dA / dh partials [4 waves][64][16], dz [30][16]
struct TrainLds {
    float h[kTrainMaxT][kTrainH * kTrainTile];
    float c[kTrainMaxT][kTrainThreads * 4];
    float da[4][kTrainH * kTrainTile];
    float dz[kTrainMaxF3 * kTrainTile];
    float red[kTrainThreads / 64];
};

// pre-activations of the wave's 64 gate rows for the 16 sequences of the tile at step t: acc[g] rows 4 kq + r of gate g's 16-row block
// (units 16 w + 4 kq + r), column = the lane's sequence
template <int NXC>
HNS_DEV void gates(const TrainArgs &a, const TrainLds &L, const float whh[4][16], const float (&bias)[4][4], const float *xrow_col, int t, int w,
                   int col, int kq, f32x4 acc[4]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = f32x4{bias[g][0], bias[g][1], bias[g][2], bias[g][3]};
    const int I = a.I;
#pragma unroll
    for (int s = 0; s < 4 * NXC; ++s) {
        const int k = 4 * s + kq;
        const bool in = k < I;
        const float b = (in && xrow_col) ? xrow_col[t * I + k] : 0.0f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float wa = in ? a.w_ih[(long long)(g * kTrainH + 16 * w + col) * I + k] : 0.0f;
            acc[g] = mfma4(wa, b, acc[g]);
        }
    }
    if (t > 0) {
        const float *hp = L.h[t - 1];
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const float b = hp[(4 * s + kq) * kTrainTile + col];
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = mfma4(whh[g][s], b, acc[g]);
        }
    }
}

template <int NXC>
__global__ __launch_bounds__(kTrainThreads, 1) void hns_tp_grad_kernel(const TrainArgs a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    TrainLds &L = *reinterpret_cast<TrainLds *>(lds_raw);
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, col = lane & 15, kq = lane >> 4;
    const int T = a.T, I = a.I, F3 = a.F3;

    // the wave's slice of W_hh as the gates' A operand: row g 64 + 16 w + col, k = 4 s + kq
    float whh[4][16];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int s = 0; s < 16; ++s) whh[g][s] = a.w_hh[(g * kTrainH + 16 * w + col) * kTrainH + 4 * s + kq];
    float bias[4][4];                                           // b_ih + b_hh of the lane's accumulator rows
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = g * kTrainH + 16 * w + 4 * kq + r;
            bias[g][r] = a.b_ih[row] + a.b_hh[row];
        }

    f32x4 dwhh[4][4], dwih[4][NXC];                             // [gate][unit block] / [gate][feature block]: rows 4 kq + r, column col
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
        for (int u = 0; u < 4; ++u) dwhh[g][u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < NXC; ++u) dwih[g][u] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float db[4][4] = {};                                        // the lane's sequence only; summed over lanes at the end
    float dwfc[8] = {};                                         // entries tid + 256 k of dW_fc [3F, 64]
    float dbfc = 0.0f, sq = 0.0f;

    for (int tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const long long q0 = (long long)tile * kTrainTile;
        const float *xcol = seq_row(a, q0 + col);               // the lane's sequence (gates' B operand, cell column)
        const float *xk[4];                                     // sequences 4 s + kq (dW_ih's B operand)
#pragma unroll
        for (int s = 0; s < 4; ++s) xk[s] = seq_row(a, q0 + 4 * s + kq);

        // ---- forward sweep
        f32x4 c = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < T; ++t) {
            f32x4 acc[4];
            gates<NXC>(a, L, whh, bias, xcol, t, w, col, kq, acc);
            f32x4 h;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float ig = sigm(acc[0][r]), fg = sigm(acc[1][r]), gg = tanhf(acc[2][r]), og = sigm(acc[3][r]);
                c[r] = fg * c[r] + ig * gg;
                h[r] = og * tanhf(c[r]);
                L.h[t][(16 * w + 4 * kq + r) * kTrainTile + col] = h[r];
            }
            *reinterpret_cast<f32x4 *>(&L.c[t][4 * tid]) = c;
            __syncthreads();
        }

        // ---- output layer, MSE and its derivative: thread (qq, j) pairs, j = the sequence
        const float *hT = L.h[T - 1];
        for (int e = tid; e < F3 * kTrainTile; e += kTrainThreads) {
            const int qq = e / kTrainTile, j = e % kTrainTile;
            float z = a.b_fc[qq];
            for (int u = 0; u < kTrainH; ++u) z += a.w_fc[qq * kTrainH + u] * hT[u * kTrainTile + j];
            const float o = tanhf(z);
            float dz = 0.0f;
            const long long q = q0 + j;
            if (q < a.B && seq_row(a, q)) {
                const float d = o - a.y[seq_id(a, q) * F3 + qq];
                sq += d * d;
                dz = (a.gscale * d) * (1.0f - o * o);
            }
            L.dz[qq * kTrainTile + j] = dz;
        }
        __syncthreads();
        for (int k = 0; k < 8; ++k) {
            const int e = tid + kTrainThreads * k;
            if (e < F3 * kTrainH) {
                const int qq = e / kTrainH, u = e % kTrainH;
                float s = 0.0f;
                for (int j = 0; j < kTrainTile; ++j) s += L.dz[qq * kTrainTile + j] * hT[u * kTrainTile + j];
                dwfc[k] += s;
            }
        }
        if (tid < F3) {
            float s = 0.0f;
            for (int j = 0; j < kTrainTile; ++j) s += L.dz[tid * kTrainTile + j];
            dbfc += s;
        }
        // dh_T of the lane's (unit, sequence) cells
        f32x4 dh, dc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int u = 16 * w + 4 * kq + r;
            float s = 0.0f;
            for (int qq = 0; qq < F3; ++qq) s += a.w_fc[qq * kTrainH + u] * L.dz[qq * kTrainTile + col];
            dh[r] = s;
        }

        // ---- backward sweep
        for (int t = T - 1; t >= 0; --t) {
            f32x4 acc[4];
            gates<NXC>(a, L, whh, bias, xcol, t, w, col, kq, acc);
            const f32x4 cp = t > 0 ? *reinterpret_cast<const f32x4 *>(&L.c[t - 1][4 * tid]) : f32x4{0.f, 0.f, 0.f, 0.f};
            float *da = L.da[w];                                // [64 wave rows g 16 + unit][16 seqs]
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float ig = sigm(acc[0][r]), fg = sigm(acc[1][r]), gg = tanhf(acc[2][r]), og = sigm(acc[3][r]);
                const float ct = fg * cp[r] + ig * gg, tc = tanhf(ct);
                const float dct = dc[r] + dh[r] * og * (1.0f - tc * tc);
                const float dai = dct * gg * ig * (1.0f - ig), daf = dct * cp[r] * fg * (1.0f - fg);
                const float dag = dct * ig * (1.0f - gg * gg), dao = dh[r] * tc * og * (1.0f - og);
                dc[r] = dct * fg;
                const int u = 4 * kq + r;
                db[0][r] += dai; db[1][r] += daf; db[2][r] += dag; db[3][r] += dao;
                da[(0 * 16 + u) * kTrainTile + col] = dai;
                da[(1 * 16 + u) * kTrainTile + col] = daf;
                da[(2 * 16 + u) * kTrainTile + col] = dag;
                da[(3 * 16 + u) * kTrainTile + col] = dao;
            }
            __syncthreads();
            // dW_hh += dA h_{t-1}^T, dW_ih += dA x_t^T (sum over the tile's sequences: k = 4 s + kq)
            if (t > 0) {
                const float *hp = L.h[t - 1];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    float av[4];
#pragma unroll
                    for (int g = 0; g < 4; ++g) av[g] = da[(g * 16 + col) * kTrainTile + 4 * s + kq];
#pragma unroll
                    for (int ub = 0; ub < 4; ++ub) {
                        const float b = hp[(16 * ub + col) * kTrainTile + 4 * s + kq];
#pragma unroll
                        for (int g = 0; g < 4; ++g) dwhh[g][ub] = mfma4(av[g], b, dwhh[g][ub]);
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                float av[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) av[g] = da[(g * 16 + col) * kTrainTile + 4 * s + kq];
#pragma unroll
                for (int cb = 0; cb < NXC; ++cb) {
                    const int f = 16 * cb + col;
                    const float b = (f < I && xk[s]) ? xk[s][t * I + f] : 0.0f;
#pragma unroll
                    for (int g = 0; g < 4; ++g) dwih[g][cb] = mfma4(av[g], b, dwih[g][cb]);
                }
            }
            if (t == 0) { __syncthreads(); break; }             // (the next tile's forward sweep rewrites the LDS)
            // this wave's part of dh_{t-1} = W_hh^T dA over its 64 rows: [64 units][16 seqs], k = wave row 4 s + kq = gate (s / 4), unit 4 (s % 4) + kq
            f32x4 pd[4];
#pragma unroll
            for (int ub = 0; ub < 4; ++ub) pd[ub] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int g = s >> 2, ul = 4 * (s & 3) + kq;
                const float b = da[(g * 16 + ul) * kTrainTile + col];
                const float *wr = a.w_hh + (g * kTrainH + 16 * w + ul) * kTrainH;
#pragma unroll
                for (int ub = 0; ub < 4; ++ub) pd[ub] = mfma4(wr[16 * ub + col], b, pd[ub]);
            }
            __syncthreads();                                    // every wave is done reading its dA: the region takes the partials
#pragma unroll
            for (int ub = 0; ub < 4; ++ub)
#pragma unroll
                for (int r = 0; r < 4; ++r) da[(16 * ub + 4 * kq + r) * kTrainTile + col] = pd[ub][r];
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 4; ++r) {                       // units 16 w + 4 kq + r: block w, row 4 kq + r of every wave's partial
                const int idx = (16 * w + 4 * kq + r) * kTrainTile + col;
                dh[r] = ((L.da[0][idx] + L.da[1][idx]) + L.da[2][idx]) + L.da[3][idx];
            }
            __syncthreads();
        }
    }

    // ---- this workgroup's partial gradients
    float *out = a.part + (long long)blockIdx.x * a.P;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = g * kTrainH + 16 * w + 4 * kq + r;
#pragma unroll
            for (int ub = 0; ub < 4; ++ub) out[off_whh(I) + row * kTrainH + 16 * ub + col] = dwhh[g][ub][r];
#pragma unroll
            for (int cb = 0; cb < NXC; ++cb)
                if (16 * cb + col < I) out[(long long)row * I + 16 * cb + col] = dwih[g][cb][r];
            float s = db[g][r];                                 // over the 16 sequences (lanes col = 0 .. 15 of this kq), fixed butterfly
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) s += __shfl_xor(s, o, 64);
            if (col == 0) out[off_b(I) + row] = s;
        }
    for (int k = 0; k < 8; ++k) {
        const int e = tid + kTrainThreads * k;
        if (e < F3 * kTrainH) out[off_wfc(I) + e] = dwfc[k];
    }
    if (tid < F3) out[off_bfc(I, F3) + tid] = dbfc;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sq += __shfl_xor(sq, o, 64);
    if (lane == 0) L.red[w] = sq;
    __syncthreads();
    if (tid == 0) out[off_bfc(I, F3) + F3] = ((L.red[0] + L.red[1]) + L.red[2]) + L.red[3];
}

struct GradOut {
    float *w_ih, *w_hh, *b_ih, *b_hh, *w_fc, *b_fc, *loss;
};

__global__ __launch_bounds__(256) void hns_tp_grad_sum_kernel(const float *part, int groups, int P, int I, int F3, double inv_n, const GradOut o) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= P) return;
    double acc = 0.0;                                           // fp64, index order: one rounding for up to 256 partials
    for (int b = 0; b < groups; ++b) acc += (double)part[(long long)b * P + e];
    const float s = (float)acc;
    if (e < off_whh(I)) o.w_ih[e] = s;
    else if (e < off_b(I)) o.w_hh[e - off_whh(I)] = s;
    else if (e < off_wfc(I)) { o.b_ih[e - off_b(I)] = s; o.b_hh[e - off_b(I)] = s; }
    else if (e < off_bfc(I, F3)) o.w_fc[e - off_wfc(I)] = s;
    else if (e < off_bfc(I, F3) + F3) o.b_fc[e - off_bfc(I, F3)] = s;
    else o.loss[0] = (float)(acc * inv_n);
}

}  // namespace hns

namespace {

long long train_groups(long long B) { return std::min<long long>((B + hns::kTrainTile - 1) / hns::kTrainTile, hns::kTrainMaxGroups); }
long long train_partial(int I, int F3) { return (long long)hns::kTrainG * (I + hns::kTrainH + 1) + (long long)F3 * (hns::kTrainH + 1) + 1; }

template <int NXC>
hipError_t launch_grad(int grid, const hns::TrainArgs &a, hipStream_t st) {
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&hns::hns_tp_grad_kernel<NXC>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(hns::TrainLds));   // 146 KB: above the default cap
    if (attr != hipSuccess) return attr;
    hipLaunchKernelGGL((hns::hns_tp_grad_kernel<NXC>), dim3(grid), dim3(hns::kTrainThreads), sizeof(hns::TrainLds), st, a);
    return hipGetLastError();
}

}  // namespace

extern "C" {

size_t hns_tp_train_workspace_bytes(int64_t batch, int32_t input_dim, int32_t future_step) {
    if (batch < 1 || input_dim < 1 || input_dim > hns::kTrainMaxI || future_step < 1 || 3 * future_step > hns::kTrainMaxF3) return 0;
    return (size_t)train_groups(batch) * (size_t)train_partial(input_dim, 3 * future_step) * sizeof(float);
}

int hns_tp_train_grad(const hns_tp_params *params, const float *x, int64_t num_envs, int64_t num_steps, int64_t stride_env, int64_t stride_step,
                      int32_t history_step, int32_t input_dim, const float *y, const int64_t *index, int64_t batch, int32_t future_step,
                      const hns_tp_grads *grads, float *loss, void *workspace, size_t workspace_bytes, void *stream) {
    const char *fn = "hns_tp_train_grad";
    if (!params || !grads || !x || !y || !loss || !workspace) return hns_fail(fn, "null pointer");
    const float *pw[6] = {params->w_ih, params->w_hh, params->b_ih, params->b_hh, params->w_fc, params->b_fc};
    float *gw[6] = {grads->w_ih, grads->w_hh, grads->b_ih, grads->b_hh, grads->w_fc, grads->b_fc};
    for (int k = 0; k < 6; ++k)
        if (!pw[k] || !gw[k] || !hns_aligned(pw[k], 4) || !hns_aligned(gw[k], 4)) return hns_fail(fn, "parameter / gradient pointers must be non-NULL fp32 arrays");
    if (!hns_aligned(x, 4) || !hns_aligned(y, 4) || !hns_aligned(loss, 4) || (reinterpret_cast<uintptr_t>(workspace) & 15) ||
        (index && (reinterpret_cast<uintptr_t>(index) & 7)))
        return hns_fail(fn, "misaligned array (x / y / loss 4 bytes, index 8, workspace 16)");
    if (history_step < 1 || history_step > hns::kTrainMaxT) return hns_fail(fn, "history_step must be in [1, 16]");
    if (input_dim < 1 || input_dim > hns::kTrainMaxI) return hns_fail(fn, "input_dim must be in [1, 80]");
    if (future_step < 1 || 3 * future_step > hns::kTrainMaxF3) return hns_fail(fn, "future_step must be in [1, 10]");
    if (batch < 1) return hns_fail(fn, "batch must be >= 1 (the mean over an empty batch is NaN)");
    if (num_envs < 1 || num_steps < 1 || num_envs * num_steps >= ((int64_t)1 << 40)) return hns_fail(fn, "num_envs, num_steps must be >= 1");
    if (stride_step < (int64_t)history_step * input_dim || stride_env < stride_step * num_steps)
        return hns_fail(fn, "strides must keep the [T, I] blocks apart: stride_step >= T I, stride_env >= stride_step S");
    if (!index && batch > num_envs * num_steps) return hns_fail(fn, "batch exceeds the rows of x (no index)");
    if (workspace_bytes < hns_tp_train_workspace_bytes(batch, input_dim, future_step)) return hns_fail(fn, "workspace too small");
    hns::TrainArgs a{};
    a.x = x; a.sE = stride_env; a.sS = stride_step; a.S = num_steps; a.rows = num_envs * num_steps;
    a.y = y; a.index = reinterpret_cast<const long long *>(index); a.B = batch;
    a.w_ih = pw[0]; a.w_hh = pw[1]; a.b_ih = pw[2]; a.b_hh = pw[3]; a.w_fc = pw[4]; a.b_fc = pw[5];
    a.T = history_step; a.I = input_dim; a.F3 = 3 * future_step;
    a.tiles = (int)((batch + hns::kTrainTile - 1) / hns::kTrainTile);
    a.P = (int)train_partial(input_dim, a.F3);
    const double n = (double)batch * a.F3;
    a.gscale = (float)(2.0 / n);
    a.part = static_cast<float *>(workspace);
    const int grid = (int)train_groups(batch);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    switch ((input_dim + 15) / 16) {
        case 1: HNS_CHECK_HIP(launch_grad<1>(grid, a, st)); break;
        case 2: HNS_CHECK_HIP(launch_grad<2>(grid, a, st)); break;
        case 3: HNS_CHECK_HIP(launch_grad<3>(grid, a, st)); break;
        case 4: HNS_CHECK_HIP(launch_grad<4>(grid, a, st)); break;
        default: HNS_CHECK_HIP(launch_grad<5>(grid, a, st)); break;
    }
    const hns::GradOut o{gw[0], gw[1], gw[2], gw[3], gw[4], gw[5], loss};
    hipLaunchKernelGGL(hns::hns_tp_grad_sum_kernel, dim3((a.P + 255) / 256), dim3(256), 0, st, static_cast<const float *>(workspace), grid, a.P,
                       input_dim, a.F3, 1.0 / n, o);
    HNS_CHECK_HIP(hipGetLastError());
    return HNS_OK;
}

}  // extern "C"
