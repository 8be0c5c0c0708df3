// hns_learner.hip — the info row of MAPPOPolicy.train_op (learning/mappo.py:463-472) on the device: the means over the minibatches of what
// update_actor / update_critic returned, and action_norm = tensordict[act_name].norm(dim=-1).mean().
//
// There the row is a torch.stack of ~128 small TensorDicts, a mean and an .item() per key (12 host synchronisations) and three launches for the
// action norm; here the updates write their scalars straight into one [minibatches, columns] fp32 table (hns_amd.learner hands them pointers
// into its rows) and ONE call makes the row:
//   hns_learner_norm_kernel : workgroup b sums sqrt(sum_i a_i^2) over its rows in fp64 (thread t of the grid takes rows t, t + G, t + 2 G, ...
//                             with G the grid's thread count; a wave tree, then the waves in index order) -> partial[b]
//   hns_learner_info_kernel : one wave; thread c < columns sums column c of the table in row order in fp64, divides by `minibatches` and rounds
//                             once to fp32; thread `columns` sums the partials in index order, divides by `rows` and rounds once
// Determinism: the grid is a function of `rows` alone and every sum has a fixed order — the same inputs give the same bits; no float atomics.
// Each row's squares are summed in fp64 from the fp32 values (exact: 8 products of 48 bits), the square root is fp64's.
//
// hns_grad_norm — the 2-norm of one flat fp32 gradient bucket (hns_amd.policy_train.GradBucket): what a data-parallel learner
// hands hns_adam_clipped after the buckets' all-reduce, when no update call's own norm describes the summed gradient.
//   hns_grad_norm_partial_kernel : the bucket as quads of four consecutive floats (the last one short by numel % 4 values, read one by one,
//                                  the missing ones 0).  With G = hns_grad_norm's grid (below) and T = 256 G, thread t of the grid takes quads
//                                  t, t + T, t + 2 T, ... in that order and adds ((x x + y y) + z z) + w w of each to its fp64 sum (the products
//                                  are exact in fp64).  A workgroup's 256 sums: per wave the butterfly s += s[lane ^ o] for o = 32, 16, 8, 4, 2, 1,
//                                  then the four waves in index order -> partial[b]
//   hns_grad_norm_final_kernel   : thread 0 adds partial[0 .. G) in index order and writes (float)sqrt(sum)
// G = clamp(ceil(quads / 1024), 1, 64): four quads a thread up to 65 536 quads — a bucket of ~1e5 floats is 25 workgroups, sized for launch
// latency, not bandwidth.  No atomics, no host synchronisation, capturable; the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <string>

#include "hns_device.h"
#include "hns_host.h"
#include "../../include/hns.h"

namespace hns {

constexpr int kInfoThreads = 256;
constexpr int kInfoRowsPerThread = 8;                           // a workgroup's share: 2 048 rows (32 KB of float4 actions)
constexpr int kInfoMaxGroups = 1024;                            // grid cap: above 2 M rows the threads stride on
constexpr int kInfoMaxActDim = 8;
constexpr int kInfoMaxColumns = 16;

HNS_DEV double info_wave_sum(double x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

template <bool VEC4>
__global__ __launch_bounds__(kInfoThreads) void hns_learner_norm_kernel(const float *__restrict__ action, long long s0, long long s1, long long rows,
                                                                        int act_dim, double *__restrict__ partial) {
    __shared__ double red[kInfoThreads / 64];
    const long long stride = (long long)gridDim.x * kInfoThreads;
    double acc = 0.0;
    for (long long r = (long long)blockIdx.x * kInfoThreads + threadIdx.x; r < rows; r += stride) {
        double ss;
        if (VEC4) {
            const float4 a = *reinterpret_cast<const float4 *>(action + r * s0);
            const double x = a.x, y = a.y, z = a.z, w = a.w;
            ss = ((x * x + y * y) + z * z) + w * w;
        } else {
            const float *row = action + r * s0;
            ss = 0.0;
            for (int i = 0; i < act_dim; ++i) { const double x = row[i * s1]; ss += x * x; }
        }
        acc += sqrt(ss);
    }
    acc = info_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < kInfoThreads / 64; ++w) s += red[w];
        partial[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(64) void hns_learner_info_kernel(const double *__restrict__ partial, int groups, long long rows,
                                                              const float *__restrict__ table, int minibatches, int columns, float *__restrict__ out) {
    const int t = threadIdx.x;
    if (t < columns) {
        double s = 0.0;
        for (int m = 0; m < minibatches; ++m) s += (double)table[(size_t)m * columns + t];
        out[t] = (float)(s / (double)minibatches);
    } else if (t == columns) {
        double s = 0.0;
        for (int g = 0; g < groups; ++g) s += partial[g];
        out[columns] = (float)(s / (double)rows);
    }
}

constexpr int kNormQuadsPerGroup = 4 * kInfoThreads;           // four float4 loads a thread
constexpr int kNormMaxGroups = 64;

__global__ __launch_bounds__(kInfoThreads) void hns_grad_norm_partial_kernel(const float *__restrict__ flat, long long numel, double *__restrict__ partial) {
    __shared__ double red[kInfoThreads / 64];
    const long long full = numel >> 2, quads = (numel + 3) >> 2;
    const long long stride = (long long)gridDim.x * kInfoThreads;
    double acc = 0.0;
    for (long long q = (long long)blockIdx.x * kInfoThreads + threadIdx.x; q < quads; q += stride) {
        float4 a = {0.0f, 0.0f, 0.0f, 0.0f};
        if (q < full) a = *reinterpret_cast<const float4 *>(flat + 4 * q);
        else {                                                  // the short last quad: 1 to 3 values, never a read past numel
            const long long left = numel - 4 * q;
            a.x = flat[4 * q];
            if (left > 1) a.y = flat[4 * q + 1];
            if (left > 2) a.z = flat[4 * q + 2];
        }
        const double x = a.x, y = a.y, z = a.z, w = a.w;
        acc += ((x * x + y * y) + z * z) + w * w;
    }
    acc = info_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < kInfoThreads / 64; ++w) s += red[w];
        partial[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(64) void hns_grad_norm_final_kernel(const double *__restrict__ partial, int groups, float *__restrict__ norm) {
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int g = 0; g < groups; ++g) s += partial[g];
        norm[0] = (float)sqrt(s);
    }
}

inline int norm_groups(long long numel) {
    const long long quads = (numel + 3) / 4;
    const long long g = (quads + kNormQuadsPerGroup - 1) / kNormQuadsPerGroup;
    return (int)(g < 1 ? 1 : g > kNormMaxGroups ? kNormMaxGroups : g);
}

inline int info_groups(long long rows) {
    const long long per = (long long)kInfoThreads * kInfoRowsPerThread;
    const long long g = (rows + per - 1) / per;
    return (int)(g < 1 ? 1 : g > kInfoMaxGroups ? kInfoMaxGroups : g);
}

}  // namespace hns

extern "C" {

size_t hns_learner_info_workspace_bytes(long long rows) {
    if (rows < 1) return 0;
    return ((size_t)hns::info_groups(rows) * sizeof(double) + 255) & ~(size_t)255;
}

int hns_learner_info(const float *action, const int64_t action_stride[2], long long rows, int act_dim, const float *table, int minibatches,
                     int columns, float *out, void *workspace, size_t workspace_bytes, void *stream) {
    const char *fn = "hns_learner_info";
    if (!action || !action_stride || !table || !out || !workspace) return hns_fail(fn, "null pointer (action, action_stride, table, out, workspace)");
    if (!hns_aligned(action, 4) || !hns_aligned(table, 4) || !hns_aligned(out, 4)) return hns_fail(fn, "misaligned pointer: action, table and out hold fp32 values");
    if (!hns_aligned(workspace, 8)) return hns_fail(fn, "misaligned pointer: the workspace holds fp64 partials (8-byte aligned)");
    if (rows < 1) return hns_fail(fn, "rows must be >= 1");
    if (act_dim < 1 || act_dim > hns::kInfoMaxActDim) return hns_fail(fn, "act_dim outside [1, 8]");
    if (minibatches < 1) return hns_fail(fn, "minibatches must be >= 1");
    if (columns < 1 || columns > hns::kInfoMaxColumns) return hns_fail(fn, "columns outside [1, 16]");
    if (action_stride[0] < 0 || action_stride[1] < 0) return hns_fail(fn, "action strides must be >= 0");
    if (workspace_bytes < hns_learner_info_workspace_bytes(rows)) return hns_fail(fn, "workspace shorter than hns_learner_info_workspace_bytes(rows)");
    const int groups = hns::info_groups(rows);
    const long long s0 = action_stride[0], s1 = action_stride[1];
    const bool vec4 = act_dim == 4 && s1 == 1 && s0 % 4 == 0 && hns_aligned(action, 16);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    double *partial = static_cast<double *>(workspace);
    if (vec4) hipLaunchKernelGGL(hns::hns_learner_norm_kernel<true>, dim3(groups), dim3(hns::kInfoThreads), 0, st, action, s0, s1, rows, act_dim, partial);
    else hipLaunchKernelGGL(hns::hns_learner_norm_kernel<false>, dim3(groups), dim3(hns::kInfoThreads), 0, st, action, s0, s1, rows, act_dim, partial);
    HNS_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(hns::hns_learner_info_kernel, dim3(1), dim3(64), 0, st, static_cast<const double *>(partial), groups, rows, table, minibatches,
                       columns, out);
    HNS_CHECK_HIP(hipGetLastError());
    return HNS_OK;
}

size_t hns_grad_norm_workspace_bytes(long long numel) {
    if (numel < 1) return 0;
    return ((size_t)hns::norm_groups(numel) * sizeof(double) + 255) & ~(size_t)255;
}

int hns_grad_norm(const float *flat, long long numel, float *norm, void *workspace, size_t workspace_bytes, void *stream) {
    const char *fn = "hns_grad_norm";
    if (!flat || !norm || !workspace) return hns_fail(fn, "null pointer (flat, norm, workspace)");
    if (!hns_aligned(flat, 16)) return hns_fail(fn, "misaligned pointer: the bucket is read by float4 (16-byte aligned)");
    if (!hns_aligned(norm, 4)) return hns_fail(fn, "misaligned pointer: norm holds one fp32 value");
    if (!hns_aligned(workspace, 8)) return hns_fail(fn, "misaligned pointer: the workspace holds fp64 partials (8-byte aligned)");
    if (numel < 1) return hns_fail(fn, "numel must be >= 1");
    if (workspace_bytes < hns_grad_norm_workspace_bytes(numel)) return hns_fail(fn, "workspace shorter than hns_grad_norm_workspace_bytes(numel)");
    const int groups = hns::norm_groups(numel);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    double *partial = static_cast<double *>(workspace);
    hipLaunchKernelGGL(hns::hns_grad_norm_partial_kernel, dim3(groups), dim3(hns::kInfoThreads), 0, st, flat, numel, partial);
    HNS_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(hns::hns_grad_norm_final_kernel, dim3(1), dim3(64), 0, st, static_cast<const double *>(partial), groups, norm);
    HNS_CHECK_HIP(hipGetLastError());
    return HNS_OK;
}

}  // extern "C"
