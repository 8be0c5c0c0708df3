// hns_gae.hip — the rollout boundary on the device: GAE with its moment row, and the in-place normalisation after the all-gather.
//
// Reference: compute_gae / compute_gae_ (omni_drones/learning/utils/gae.py:27-75), driven by MAPPOPolicy.train_op (learning/mappo.py:370-402)
// with ValueNorm1.denormalize / normalize (learning/utils/valuenorm.py:93-106).  There a rollout is a Python loop over T of ~8 elementwise
// launches per step; here it is
//   hns_gae_staged_kernel  : batch-major [N, T, K] — a tile of nb envs is one contiguous span; reward / value / not-done are staged through LDS
//                            with coalesced loads, one thread per (env, k) column scans t backwards in LDS, advantages / returns go back the same way
//   hns_gae_direct_kernel  : time-major [T, N, K] (every t row is contiguous, so threads over (env, k) walking t are coalesced), and batch-major
//                            spans too large to stage (a thread walks its column in global memory)
//   hns_gae_moments_kernel : one workgroup sums the per-workgroup fp64 partials (GAE's four sums and a slice of the success values each) in a
//                            fixed order into the rank's moment row (sharding.MOMENT_DIM)
//   hns_rollout_normalise_kernel : (adv - m_a) / d_a and (ret - m_r) / s_r in place, operands read from device scalars
//
// Bit-exactness: every fp32 statement is the reference's, in its order (the build compiles with -ffp-contract=off; division is IEEE):
//   v' = v * scale + shift (denormalize), nd = 1 - float(done), delta = (r + (g * nv) * nd) - v', gae = delta + ((gl * nd) * gae), ret = gae + v'
// with g = fp32(gamma), gl = fp32(gamma * lambda) (the Python float product, rounded once) and gae starting at +0.0f with the first
// multiply-add executed (the reference's `gae = 0` turns a -0.0 delta into +0.0).
// Determinism: a workgroup's tiles are fixed by the grid (a function of the shape alone); each thread sums its columns in t order, the
// workgroup reduces in a fixed tree, and the finaliser sums the workgroups' partials in index order — the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <string>

#include "hns_device.h"
#include "hns_host.h"
#include "../../include/hns.h"

namespace hns {

constexpr int kGaeThreads = 256;
constexpr int kGaePartial = 5;                                  // per workgroup: sum adv, sum adv^2, sum ret, sum ret^2, sum success
constexpr int kGaeMaxGroups = HNS_GAE_WORKSPACE_DOUBLES / kGaePartial;   // grid cap: one partial per workgroup
constexpr int kGaeFinThreads = 1024;
constexpr int kGaeUnroll = 4;                                   // staged loads in flight per thread and array
constexpr int kGaeLdsFloats = 12288;                            // 48 KB of staging per workgroup: three workgroups per CU

struct GaeArgs {
    const float *reward, *value, *next_value;
    const void *done;
    const float *scale, *shift;              // both NULL or both device scalars
    float *adv, *ret;
    double *partial;                         // NULL: no moments
    const float *success;                    // [m]: workgroup b sums [b ms, (b + 1) ms)
    long long m, ms;
    long long n, t, k, kd;
    long long sN, sT;                        // element (n, t, k) at n sN + t sT + k
    long long dN, dT;                        // done (n, t, kd) at n dN + t dT + (kd == 1 ? 0 : k)
    float g, gl;
    int done_f32;
    int nb, S, Sd, tiles;                    // staged kernel: envs per tile, padded env strides (reward / value, not-done) in LDS
};

HNS_DEV float not_done_of(const void *done, int done_f32, long long i) {
    return done_f32 ? 1.0f - static_cast<const float *>(done)[i] : 1.0f - (float)static_cast<const unsigned char *>(done)[i];
}

HNS_DEV double wave_sum(double x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// the workgroup's five sums -> partial[blockIdx.x * 5 ..]: the workgroup's share of the success values first (a contiguous slice: the success row
// needs no launch of its own), then wave trees and the waves in index order
HNS_DEV void write_partials(const GaeArgs &p, double a, double a2, double b, double b2) {
    __shared__ double red[kGaeThreads / 64][kGaePartial];
    double c = 0.0;
    const long long s0 = (long long)blockIdx.x * p.ms, s1 = s0 + p.ms < p.m ? s0 + p.ms : p.m;
    for (long long i = s0 + threadIdx.x; i < s1; i += kGaeThreads) c += (double)p.success[i];
    a = wave_sum(a); a2 = wave_sum(a2); b = wave_sum(b); b2 = wave_sum(b2); c = wave_sum(c);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[w][0] = a; red[w][1] = a2; red[w][2] = b; red[w][3] = b2; red[w][4] = c; }
    __syncthreads();
    if (threadIdx.x < kGaePartial) {
        double s = 0.0;
        for (int i = 0; i < kGaeThreads / 64; ++i) s += red[i][threadIdx.x];
        p.partial[(size_t)blockIdx.x * kGaePartial + threadIdx.x] = s;
    }
}

template <bool DENORM, bool MOMENTS>
__global__ __launch_bounds__(kGaeThreads) void hns_gae_direct_kernel(GaeArgs p) {
    const float scale = DENORM ? *p.scale : 1.0f, shift = DENORM ? *p.shift : 0.0f;
    double a = 0.0, a2 = 0.0, b = 0.0, b2 = 0.0;
    const long long cols = p.n * p.k;
    for (long long c = (long long)blockIdx.x * kGaeThreads + threadIdx.x; c < cols; c += (long long)gridDim.x * kGaeThreads) {
        const long long e = c / p.k, k = c - e * p.k;
        const long long base = e * p.sN + k, dbase = e * p.dN + (p.kd == 1 ? 0 : k);
        float nv = p.next_value[c];
        if (DENORM) nv = nv * scale + shift;
        float gae = 0.0f;
        for (long long t = p.t - 1; t >= 0; --t) {
            const long long i = base + t * p.sT;
            float v = p.value[i];
            if (DENORM) v = v * scale + shift;
            const float nd = not_done_of(p.done, p.done_f32, dbase + t * p.dT);
            const float delta = (p.reward[i] + (p.g * nv) * nd) - v;
            gae = delta + ((p.gl * nd) * gae);
            const float r = gae + v;
            p.adv[i] = gae;
            p.ret[i] = r;
            nv = v;
            if (MOMENTS) { const double x = gae, y = r; a += x; a2 += x * x; b += y; b2 += y * y; }
        }
    }
    if (MOMENTS) write_partials(p, a, a2, b, b2);
}

// batch-major, staged: tile = envs [e0, e0 + nb) = floats [e0 T K, (e0 + nb) T K) of every array.  In LDS env e's row starts at e S (reward, then
// advantages) / nbS + e S (value, then returns) / 2 nb S + e Sd (not-done).  S = T K padded to S = K (mod 32): column thread j = e K + k reads
// e S + t K + k = j + t K (mod 32) — consecutive lanes on consecutive banks; Sd likewise with Kd.
template <bool DENORM, bool MOMENTS>
__global__ __launch_bounds__(kGaeThreads) void hns_gae_staged_kernel(GaeArgs p) {
    __shared__ float lds[kGaeLdsFloats];
    const float scale = DENORM ? *p.scale : 1.0f, shift = DENORM ? *p.shift : 0.0f;
    const int T = (int)p.t, K = (int)p.k, Kd = (int)p.kd, TK = T * K, TKd = T * Kd, nb = p.nb, S = p.S, Sd = p.Sd;
    float *R = lds, *V = lds + nb * S, *D = lds + 2 * nb * S;
    double a = 0.0, a2 = 0.0, b = 0.0, b2 = 0.0;
    const int j = threadIdx.x, je = j / K, jk = j - je * K;
    for (int tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const long long e0 = (long long)tile * nb;
        const int ne = (int)((p.n - e0) < nb ? (p.n - e0) : nb);
        const size_t g0 = (size_t)e0 * TK, gd0 = (size_t)e0 * TKd;
        // coalesced loads of the span: flat index f = e TK + r, (e, r) advanced by 256 per round without a division; kGaeUnroll rounds of
        // loads are issued before their LDS stores
        {
            const int span = ne * TK, q = kGaeThreads / TK, rem = kGaeThreads - q * TK;
            int e = j / TK, r = j - e * TK;
            for (int f0 = j; f0 < span; f0 += kGaeUnroll * kGaeThreads) {
                float rv[kGaeUnroll], vv[kGaeUnroll];
                int at[kGaeUnroll];
#pragma unroll
                for (int u = 0; u < kGaeUnroll; ++u) {
                    const int f = f0 + u * kGaeThreads;
                    at[u] = e * S + r;
                    if (f < span) { rv[u] = p.reward[g0 + f]; vv[u] = p.value[g0 + f]; }
                    e += q; r += rem;
                    if (r >= TK) { r -= TK; ++e; }
                }
#pragma unroll
                for (int u = 0; u < kGaeUnroll; ++u) {
                    if (f0 + u * kGaeThreads < span) {
                        float v = vv[u];
                        if (DENORM) v = v * scale + shift;
                        R[at[u]] = rv[u];
                        V[at[u]] = v;
                    }
                }
            }
            const int dspan = ne * TKd, qd = kGaeThreads / TKd, remd = kGaeThreads - qd * TKd;
            e = j / TKd; r = j - e * TKd;
            for (int f0 = j; f0 < dspan; f0 += kGaeUnroll * kGaeThreads) {
                float dv[kGaeUnroll];
                int at[kGaeUnroll];
#pragma unroll
                for (int u = 0; u < kGaeUnroll; ++u) {
                    const int f = f0 + u * kGaeThreads;
                    at[u] = e * Sd + r;
                    if (f < dspan) dv[u] = not_done_of(p.done, p.done_f32, (long long)(gd0 + f));
                    e += qd; r += remd;
                    if (r >= TKd) { r -= TKd; ++e; }
                }
#pragma unroll
                for (int u = 0; u < kGaeUnroll; ++u)
                    if (f0 + u * kGaeThreads < dspan) D[at[u]] = dv[u];
            }
        }
        __syncthreads();
        if (je < ne) {
            float nv = p.next_value[(size_t)(e0 + je) * K + jk];
            if (DENORM) nv = nv * scale + shift;
            float gae = 0.0f;
            float *Rc = R + je * S + jk, *Vc = V + je * S + jk;
            const float *Dc = D + je * Sd + (Kd == 1 ? 0 : jk);
            for (int t = T - 1; t >= 0; --t) {
                const float v = Vc[t * K], nd = Dc[t * Kd];
                const float delta = (Rc[t * K] + (p.g * nv) * nd) - v;
                gae = delta + ((p.gl * nd) * gae);
                const float r = gae + v;
                Rc[t * K] = gae;
                Vc[t * K] = r;
                nv = v;
                if (MOMENTS) { const double x = gae, y = r; a += x; a2 += x * x; b += y; b2 += y * y; }
            }
        }
        __syncthreads();
        {
            const int span = ne * TK, q = kGaeThreads / TK, rem = kGaeThreads - q * TK;
            int e = j / TK, r = j - e * TK;
            for (int f = j; f < span; f += kGaeThreads) {
                p.adv[g0 + f] = R[e * S + r];
                p.ret[g0 + f] = V[e * S + r];
                e += q; r += rem;
                if (r >= TK) { r -= TK; ++e; }
            }
        }
        __syncthreads();
    }
    if (MOMENTS) write_partials(p, a, a2, b, b2);
}

// out[0..7] = [sum adv, sum adv^2, n, sum success, m, sum ret, sum ret^2, n] from `groups` partials, one workgroup, fixed order: thread t sums
// partials t, t + 1024, ... (all loads issued first), then a tree over the 1024 threads
__global__ __launch_bounds__(kGaeFinThreads) void hns_gae_moments_kernel(const double *__restrict__ partial, int groups, long long m, double count,
                                                                          double *__restrict__ out) {
    constexpr int kPer = (kGaeMaxGroups + kGaeFinThreads - 1) / kGaeFinThreads;
    __shared__ double red[kGaePartial][kGaeFinThreads];
    const int t = threadIdx.x;
    double x[kPer][kGaePartial];
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
        const int i = t + u * kGaeFinThreads;
#pragma unroll
        for (int q = 0; q < kGaePartial; ++q) x[u][q] = i < groups ? partial[(size_t)i * kGaePartial + q] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < kGaePartial; ++q) {
        double acc = 0.0;
#pragma unroll
        for (int u = 0; u < kPer; ++u) acc += x[u][q];
        red[q][t] = acc;
    }
    __syncthreads();
    for (int w = kGaeFinThreads / 2; w >= 1; w >>= 1) {
        if (t < w) {
#pragma unroll
            for (int r = 0; r < kGaePartial; ++r) red[r][t] += red[r][t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        out[0] = red[0][0]; out[1] = red[1][0]; out[2] = count; out[3] = red[4][0]; out[4] = (double)m;
        out[5] = red[2][0]; out[6] = red[3][0]; out[7] = count;
    }
}

// x = (x - m) / d in place; blockIdx.y picks the array (0: advantages, 1: returns, or the one array given); float4 body when the pointer is
// 16-byte aligned, scalar tail
struct NormArgs {
    float *x[2];
    long long n[2];
    const float *m[2], *d[2];
};

__global__ __launch_bounds__(kGaeThreads) void hns_rollout_normalise_kernel(NormArgs p) {
    const int y = blockIdx.y;
    float *__restrict__ x = p.x[y];
    const long long n = p.n[y];
    const float m = *p.m[y], d = *p.d[y];
    const long long n4 = ((reinterpret_cast<uintptr_t>(x) & 15) == 0) ? n / 4 : 0;
    float4 *x4 = reinterpret_cast<float4 *>(x);
    const long long stride = (long long)gridDim.x * kGaeThreads;
    for (long long i = (long long)blockIdx.x * kGaeThreads + threadIdx.x; i < n4; i += stride) {
        float4 q = x4[i];
        q.x = (q.x - m) / d; q.y = (q.y - m) / d; q.z = (q.z - m) / d; q.w = (q.w - m) / d;
        x4[i] = q;
    }
    for (long long i = 4 * n4 + (long long)blockIdx.x * kGaeThreads + threadIdx.x; i < n; i += stride) x[i] = (x[i] - m) / d;
}

}  // namespace hns

namespace {

template <bool D, bool M>
void launch_gae(bool staged, int grid, const hns::GaeArgs &a, hipStream_t st) {
    if (staged) hipLaunchKernelGGL((hns::hns_gae_staged_kernel<D, M>), dim3(grid), dim3(hns::kGaeThreads), 0, st, a);
    else hipLaunchKernelGGL((hns::hns_gae_direct_kernel<D, M>), dim3(grid), dim3(hns::kGaeThreads), 0, st, a);
}

int pad_to(int len, int k) { return len + ((k - len % 32) % 32 + 32) % 32; }   // smallest S >= len with S = k (mod 32)

}  // namespace

extern "C" {

int hns_gae(const float *reward, const float *value, const void *done, const float *next_value, int64_t n, int64_t t, int64_t k, int64_t kd,
            int32_t layout, int32_t done_dtype, double gamma, double lambda, const float *scale, const float *shift, const float *success, int64_t m,
            float *advantages, float *returns, double *moments, double *workspace, void *stream) {
    const char *fn = "hns_gae";
    if (!reward || !value || !done || !next_value || !advantages || !returns) return hns_fail(fn, "null array pointer");
    if (n < 1 || t < 1 || k < 1) return hns_fail(fn, "n, t and k must be >= 1");
    if (kd != 1 && kd != k) return hns_fail(fn, "kd (done's trailing size) must be 1 or k");
    if (n > (int64_t)1 << 31 || t > (int64_t)1 << 31 || k > (int64_t)1 << 31 || n * k > ((int64_t)1 << 31) || n * t * k > ((int64_t)1 << 40))
        return hns_fail(fn, "shape too large");
    if (layout != HNS_GAE_BATCH_MAJOR && layout != HNS_GAE_TIME_MAJOR) return hns_fail(fn, "layout must be HNS_GAE_BATCH_MAJOR or HNS_GAE_TIME_MAJOR");
    if (done_dtype != HNS_GAE_DONE_U8 && done_dtype != HNS_GAE_DONE_F32) return hns_fail(fn, "done_dtype must be HNS_GAE_DONE_U8 or HNS_GAE_DONE_F32");
    if (!scale != !shift) return hns_fail(fn, "scale and shift go together (both NULL or both device scalars)");
    if (m < 0 || (m > 0 && !success)) return hns_fail(fn, "success: m >= 0 values, non-NULL when m > 0");
    if (moments && !workspace) return hns_fail(fn, "moments need a workspace of HNS_GAE_WORKSPACE_DOUBLES doubles");
    if (!(gamma == gamma) || !(lambda == lambda)) return hns_fail(fn, "gamma and lambda must be numbers");
    hns::GaeArgs a{};
    a.reward = reward; a.value = value; a.next_value = next_value; a.done = done; a.scale = scale; a.shift = shift;
    a.adv = advantages; a.ret = returns; a.partial = workspace; a.success = success; a.m = m;
    a.n = n; a.t = t; a.k = k; a.kd = kd;
    if (layout == HNS_GAE_BATCH_MAJOR) { a.sN = t * k; a.sT = k; a.dN = t * kd; a.dT = kd; }
    else { a.sN = k; a.sT = n * k; a.dN = kd; a.dT = n * kd; }
    a.g = (float)gamma;
    a.gl = (float)(gamma * lambda);
    a.done_f32 = done_dtype == HNS_GAE_DONE_F32;
    // staging: envs per tile from the LDS budget and the 256 column threads
    bool staged = false;
    if (layout == HNS_GAE_BATCH_MAJOR && t * k <= hns::kGaeLdsFloats && k <= hns::kGaeThreads) {
        const int S = pad_to((int)(t * k), (int)k), Sd = pad_to((int)(t * kd), (int)kd);
        long long nb = hns::kGaeLdsFloats / (2LL * S + Sd);
        nb = std::min<long long>(std::min<long long>(nb, hns::kGaeThreads / k), n);
        if (nb >= 1) { staged = true; a.nb = (int)nb; a.S = S; a.Sd = Sd; a.tiles = (int)((n + nb - 1) / nb); }
    }
    const long long work = staged ? a.tiles : (n * k + hns::kGaeThreads - 1) / hns::kGaeThreads;
    const int grid = (int)std::min<long long>(work, hns::kGaeMaxGroups);
    a.ms = (m + grid - 1) / grid;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (scale) { if (moments) launch_gae<true, true>(staged, grid, a, st); else launch_gae<true, false>(staged, grid, a, st); }
    else { if (moments) launch_gae<false, true>(staged, grid, a, st); else launch_gae<false, false>(staged, grid, a, st); }
    HNS_CHECK_HIP(hipGetLastError());
    if (moments) {
        hipLaunchKernelGGL(hns::hns_gae_moments_kernel, dim3(1), dim3(hns::kGaeFinThreads), 0, st, static_cast<const double *>(workspace), grid,
                           (long long)m, (double)(n * t * k), moments);
        HNS_CHECK_HIP(hipGetLastError());
    }
    return HNS_OK;
}

int hns_rollout_normalise(float *advantages, int64_t n_adv, const float *adv_mean, const float *adv_den, float *returns, int64_t n_ret,
                          const float *ret_mean, const float *ret_scale, void *stream) {
    const bool do_adv = adv_mean || adv_den, do_ret = ret_mean || ret_scale;
    if (!do_adv && !do_ret) { hns_set_error("hns_rollout_normalise: neither operand pair given"); return HNS_ERR_INVALID_ARG; }
    if (do_adv && (!adv_mean || !adv_den || !advantages || n_adv < 0)) {
        hns_set_error("hns_rollout_normalise: advantages need the array, n >= 0 and both device scalars (mean, std + eps)");
        return HNS_ERR_INVALID_ARG;
    }
    if (do_ret && (!ret_mean || !ret_scale || !returns || n_ret < 0)) {
        hns_set_error("hns_rollout_normalise: returns need the array, n >= 0 and both device scalars (mean, sqrt(var))");
        return HNS_ERR_INVALID_ARG;
    }
    hns::NormArgs a{};
    int arrays = 0;
    if (do_adv && n_adv > 0) { a.x[arrays] = advantages; a.n[arrays] = n_adv; a.m[arrays] = adv_mean; a.d[arrays] = adv_den; ++arrays; }
    if (do_ret && n_ret > 0) { a.x[arrays] = returns; a.n[arrays] = n_ret; a.m[arrays] = ret_mean; a.d[arrays] = ret_scale; ++arrays; }
    if (arrays == 0) return HNS_OK;
    // one launch for both arrays: a float4 per thread per round, at most 1 024 workgroups per array, a grid-stride loop takes the rest
    const int64_t longest = std::max<int64_t>(a.n[0], arrays == 2 ? a.n[1] : 0);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((longest / 4 + hns::kGaeThreads - 1) / hns::kGaeThreads, 1024));
    hipLaunchKernelGGL(hns::hns_rollout_normalise_kernel, dim3(grid, arrays), dim3(hns::kGaeThreads), 0, static_cast<hipStream_t>(stream), a);
    HNS_CHECK_HIP(hipGetLastError());
    return HNS_OK;
}

}  // extern "C"
