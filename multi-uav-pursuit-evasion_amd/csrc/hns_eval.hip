// hns_eval.hip — the evaluator's statistic means: ONE launch turns up to 64 per-env rows (the 24 task statistics after an evaluation rollout's
// last step) into their NaN-skipping means over the envs a mask selects — torch.nanmean restricted to the mask (hns_amd.evaluator).
//
// The rows travel by value in the kernel arguments, as hns_rollout_store's segments do (no device-side table, no allocation).  One workgroup of
// 256 threads per row: thread t adds its elements t, t + 256, ... in that order in fp64 and counts them, a fixed-order tree in LDS joins the 256
// partials, thread 0 divides once and rounds once to fp32.  No atomics of any kind: the result is a pure function of the inputs.  A NaN is
// skipped, +-inf enters the sum as IEEE addition has it (inf + -inf = NaN), a row with nothing entering gives NaN.
//
// Accuracy (n <= num_envs <= 2^20 values): an fp64 sum in any order is off by at most (n - 1) 2^-53 sum|x|, the division adds 2^-53 |exact|,
// together at most n 2^-53 mean|x| <= 2^-33 mean|x|; the one rounding to fp32 adds 2^-24 |exact|:
// |mean - exact| <= 2^-24 |exact| + 2^-33 mean|x|.
#include <hip/hip_runtime.h>

#include <string>

#include "hns_device.h"
#include "hns_host.h"
#include "../../include/hns.h"

namespace hns {

constexpr int kEvalThreads = 256;

struct EvalArgs {
    hns_eval_row row[HNS_EVAL_MAX_ROWS];
    long long num_envs;
    const unsigned char *mask;                                  // [num_envs] or NULL: every env
    float *mean;                                                // [count]
    long long *used;                                            // [count + 1]: values per row, then the masked envs
    int count;
};

__global__ __launch_bounds__(kEvalThreads) void hns_eval_means_kernel(const EvalArgs a) {
    __shared__ double s_sum[kEvalThreads];
    __shared__ long long s_used[kEvalThreads], s_masked[kEvalThreads];
    const int tid = threadIdx.x;
    const float *src = a.row[blockIdx.x].src;
    const long long stride = a.row[blockIdx.x].stride;
    double sum = 0.0;
    long long used = 0, masked = 0;
    for (long long e = tid; e < a.num_envs; e += kEvalThreads) {
        if (a.mask && !a.mask[e]) continue;
        ++masked;
        const float v = src[e * stride];
        if (v != v) continue;                                   // NaN: nanmean skips it
        sum += (double)v;
        ++used;
    }
    s_sum[tid] = sum; s_used[tid] = used; s_masked[tid] = masked;
    __syncthreads();
    for (int half = kEvalThreads / 2; half > 0; half >>= 1) {   // fixed order: partial t takes partial t + half
        if (tid < half) {
            s_sum[tid] += s_sum[tid + half];
            s_used[tid] += s_used[tid + half];
            s_masked[tid] += s_masked[tid + half];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const long long n = s_used[0];
        a.mean[blockIdx.x] = n ? (float)(s_sum[0] / (double)n) : __builtin_nanf("");
        a.used[blockIdx.x] = n;
        if (blockIdx.x == 0) a.used[a.count] = s_masked[0];
    }
}

}  // namespace hns

extern "C" {

int hns_eval_means(const hns_eval_row *rows, int32_t count, int64_t num_envs, const uint8_t *mask, float *mean, int64_t *used, void *stream) {
    const char *fn = "hns_eval_means";
    if (!rows) return hns_fail(fn, "rows is a null pointer");
    if (!mean || !hns_aligned(mean, 4)) return hns_fail(fn, "mean is a null or misaligned pointer");
    if (!used || !hns_aligned(used, 8)) return hns_fail(fn, "used is a null or misaligned pointer");
    if (count < 1 || count > HNS_EVAL_MAX_ROWS) return hns_fail(fn, "count outside [1, 64]");
    if (num_envs < 1) return hns_fail(fn, "num_envs must be >= 1");
    hns::EvalArgs args = {};
    for (int i = 0; i < count; ++i) {
        const std::string at = "rows[" + std::to_string(i) + "].";
        if (!rows[i].src) return hns_fail(fn, at + "src is a null pointer");
        if (!hns_aligned(rows[i].src, 4)) return hns_fail(fn, at + "src is misaligned");
        if (rows[i].stride < 1) return hns_fail(fn, at + "stride must be >= 1");
        if (rows[i].stride > INT64_MAX / 4 / num_envs) return hns_fail(fn, at + "stride: num_envs * stride * 4 overflows int64");
        args.row[i] = rows[i];
    }
    args.num_envs = num_envs;
    args.mask = mask;
    args.mean = mean;
    args.used = reinterpret_cast<long long *>(used);
    args.count = count;
    hipLaunchKernelGGL(hns::hns_eval_means_kernel, dim3((unsigned)count), dim3(hns::kEvalThreads), 0, static_cast<hipStream_t>(stream), args);
    HNS_CHECK_HIP(hipGetLastError());
    return HNS_OK;
}

}  // extern "C"
