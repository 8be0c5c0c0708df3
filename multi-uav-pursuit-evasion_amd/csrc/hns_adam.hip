// hns_adam.hip — the optimiser step of every device update: clip_grad_norm_'s scaling (optional) and torch.optim.Adam over any number of tensors.
//
// Reference: MAPPOPolicy.update_TP, update_critic and update_actor (omni_drones/learning/mappo.py:252-352) end in torch.optim.Adam's step
// (amsgrad off, weight decay 0, maximize off), the latter two behind nn.utils.clip_grad_norm_.  DESIGN.md §7.2.
//   hns_adam_clipped_kernel : the clip and Adam's single-tensor statements, element-wise over up to 64 tensors per launch (a grid-stride loop per
//                             tensor, so the mapping of elements to threads changes no bit).  It reads the device step counter and never writes it:
//                             every launch of one step sees the same step + 1.
//   hns_adam_bump_kernel    : bumps the counter once, after the last launch.  No host value anywhere, so a step can be captured.
// hns_adam_clipped and hns_tp_adam are two entries over one host function: the predictor's passes no norm and keeps its cap of 8 tensors.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>

#include "hns_host.h"
#include "../../include/hns.h"

static_assert(sizeof(hns_tp_adam_tensor) == sizeof(hns_adam_tensor) && offsetof(hns_tp_adam_tensor, param) == offsetof(hns_adam_tensor, param) &&
                  offsetof(hns_tp_adam_tensor, grad) == offsetof(hns_adam_tensor, grad) &&
                  offsetof(hns_tp_adam_tensor, exp_avg) == offsetof(hns_adam_tensor, exp_avg) &&
                  offsetof(hns_tp_adam_tensor, exp_avg_sq) == offsetof(hns_adam_tensor, exp_avg_sq) &&
                  offsetof(hns_tp_adam_tensor, numel) == offsetof(hns_adam_tensor, numel),
              "hns_tp_adam reads its descriptors as hns_adam_tensor");

namespace hns {

constexpr int kCAdamMax = 64;                // tensors per launch (the descriptors travel in the kernel arguments)
struct CAdamArgs {
    float *p[kCAdamMax], *g[kCAdamMax], *m[kCAdamMax], *v[kCAdamMax];
    long long n[kCAdamMax];
    int count, clip;
    const float *step, *norm;
    float max_norm;
    double lr, beta1, beta2, eps;
};

// clip_grad_norm_: g *= min(max_norm / (norm + 1e-6), 1) (torch: reciprocal, then times max_norm), then torch.optim.Adam's single-tensor path,
// statement for statement with torch's CPU kernels, with step = *step + 1 (the counter itself is bumped by hns_adam_bump_kernel after every tensor is done):
//   m = lerp(m, g, 1 - beta1) = fma(1 - beta1, g - m, m);  v = fma((1 - beta2) g, g, v beta2)
//   bc1 = 1 - beta1^step, bc2 = 1 - beta2^step (double);  denom = sqrt(v) / f32(sqrt(bc2)) + f32(eps);  p = p + (f32(-lr / bc1) m) / denom
__global__ __launch_bounds__(256) void hns_adam_clipped_kernel(const CAdamArgs a) {
    const float step = a.step[0] + 1.0f;
    float coef = 1.0f;
    if (a.clip) {
        coef = (1.0f / (a.norm[0] + 1e-6f)) * a.max_norm;
        coef = coef > 1.0f ? 1.0f : coef;                       // (a NaN norm stays NaN, as torch's clamp)
    }
    const double bc1 = 1.0 - pow(a.beta1, (double)step), bc2 = 1.0 - pow(a.beta2, (double)step);
    const float w1 = (float)(1.0 - a.beta1), b2 = (float)a.beta2, w2 = (float)(1.0 - a.beta2);
    const float ss = (float)(-(a.lr / bc1)), bc2s = (float)sqrt(bc2), eps = (float)a.eps;
    for (int k = 0; k < a.count; ++k) {
        float *p = a.p[k], *m = a.m[k], *v = a.v[k], *g = a.g[k];
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.n[k]; i += (long long)gridDim.x * 256) {
            float gi = g[i];
            if (a.clip) {
                gi = gi * coef;
                g[i] = gi;
            }
            const float mi = __builtin_fmaf(w1, gi - m[i], m[i]);
            const float vi = __builtin_fmaf(w2 * gi, gi, v[i] * b2);
            const float den = __builtin_sqrtf(vi) / bc2s + eps;
            m[i] = mi;
            v[i] = vi;
            p[i] = p[i] + (ss * mi) / den;
        }
    }
}

__global__ void hns_adam_bump_kernel(float *step) { step[0] = step[0] + 1.0f; }

}  // namespace hns

namespace {

// the descriptor checks, then one launch per 64 tensors (the grid by the largest of them) and the bump; norm NULL: no clip
int adam_step(const char *fn, const hns_adam_tensor *tensors, int count, float *step, const float *norm, double max_norm, double lr, double beta1,
              double beta2, double eps, void *stream) {
    for (int k = 0; k < count; ++k) {
        const hns_adam_tensor &t = tensors[k];
        if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq || t.numel < 0) return hns_fail(fn, "tensor with a NULL array or numel < 0");
        if (!hns_aligned(t.param, 4) || !hns_aligned(t.grad, 4) || !hns_aligned(t.exp_avg, 4) || !hns_aligned(t.exp_avg_sq, 4))
            return hns_fail(fn, "misaligned fp32 array");
    }
    const hipStream_t st = static_cast<hipStream_t>(stream);
    for (int k0 = 0; k0 < count; k0 += hns::kCAdamMax) {
        hns::CAdamArgs a{};
        a.count = std::min<int>(hns::kCAdamMax, count - k0);
        a.clip = norm != nullptr && std::isfinite(max_norm);
        a.step = step; a.norm = norm; a.max_norm = (float)max_norm;
        a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
        long long most = 1;
        for (int k = 0; k < a.count; ++k) {
            const hns_adam_tensor &t = tensors[k0 + k];
            a.p[k] = t.param; a.g[k] = t.grad; a.m[k] = t.exp_avg; a.v[k] = t.exp_avg_sq; a.n[k] = t.numel;
            most = std::max<long long>(most, t.numel);
        }
        const int grid = (int)std::min<long long>((most + 255) / 256, 256);
        hipLaunchKernelGGL(hns::hns_adam_clipped_kernel, dim3(grid), dim3(256), 0, st, a);
        HNS_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(hns::hns_adam_bump_kernel, dim3(1), dim3(1), 0, st, step);
    HNS_CHECK_HIP(hipGetLastError());
    return HNS_OK;
}

}  // namespace

extern "C" {

int hns_adam_clipped(const hns_adam_tensor *tensors, int32_t count, float *step, const float *total_norm, double max_norm, double lr, double beta1,
                     double beta2, double eps, void *stream) {
    const char *fn = "hns_adam_clipped";
    if (!tensors || !step || count < 1) return hns_fail(fn, "at least one tensor and a device step counter");
    if (!hns_aligned(step, 4) || (total_norm && !hns_aligned(total_norm, 4))) return hns_fail(fn, "misaligned step counter / norm");
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(max_norm >= 0.0))
        return hns_fail(fn, "lr >= 0, 0 <= beta < 1, eps >= 0, max_norm >= 0");
    return adam_step(fn, tensors, count, step, total_norm, max_norm, lr, beta1, beta2, eps, stream);
}

int hns_tp_adam(const hns_tp_adam_tensor *tensors, int32_t count, float *step, double lr, double beta1, double beta2, double eps, void *stream) {
    const char *fn = "hns_tp_adam";
    if (!tensors || !step || count < 1 || count > 8) return hns_fail(fn, "1 to 8 tensors and a device step counter");
    if (!hns_aligned(step, 4)) return hns_fail(fn, "misaligned step counter");
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0))
        return hns_fail(fn, "lr >= 0, 0 <= beta < 1, eps >= 0");
    return adam_step(fn, reinterpret_cast<const hns_adam_tensor *>(tensors), count, step, nullptr, INFINITY, lr, beta1, beta2, eps, stream);
}

}  // extern "C"
