// hns_rollout.hip — the collector's per-step store: ONE launch copies up to 16 per-env rows (observation keys, action, log-prob, value, or
// reward, done, the predictor's entries) into time slot `slot` of their batch-major [N, T, ...] storage (hns_amd.collector).
//
// As torch `copy_` calls that is one launch per tensor; here the segments travel by value in the kernel arguments (no device-side table, no
// allocation), blockIdx.y is the segment and blockIdx.x grid-strides over its envs, a power-of-two group of threads per env's row.  The host
// picks each segment's copy unit: 16 bytes when both bases, both strides and the row length are multiples of 16, 4 bytes under the same rule, else single bytes — plain
// vector loads and stores of that width, no atomics, no LDS.  Every segment reads and writes whole rows only: nothing outside
// [dst + e dst_stride + slot row_bytes, ... + row_bytes) is touched.
#include <hip/hip_runtime.h>

#include <string>

#include "hns_device.h"
#include "hns_host.h"
#include "../../include/hns.h"

namespace hns {

constexpr int kStoreThreads = 256;
constexpr int kStoreMaxGroups = 1024;                           // grid cap per segment: four workgroups for each of an MI355X's 256 CUs
constexpr long long kStoreMaxRowBytes = 1ll << 20;

struct StoreSegment {
    const unsigned char *src;
    unsigned char *dst;                                         // storage base + slot * row_bytes
    long long src_stride, dst_stride, units;                    // strides in bytes; units per row
    int unit;                                                   // 16, 4 or 1 bytes
    int lanes_log2;                                             // 2^lanes_log2 threads share an env's row (<= kStoreThreads)
};
struct StoreArgs {
    StoreSegment seg[HNS_ROLLOUT_MAX_SEGMENTS];
    long long num_envs;
};

// 2^lanes_log2 neighbouring threads take one env's row, unit u = lane, lane + 2^lanes_log2, ...; a workgroup covers kStoreThreads >> lanes_log2
// envs and strides on by the grid's share.  Shifts and masks only: no division per unit (rows of 1 .. 12 bytes are one or three units).
template <typename U>
HNS_DEV void store_rows(const StoreSegment &s, long long num_envs) {
    const int lanes = 1 << s.lanes_log2, per_group = kStoreThreads >> s.lanes_log2;
    const int lane = threadIdx.x & (lanes - 1);
    const long long step = (long long)gridDim.x * per_group;
    for (long long e = (long long)blockIdx.x * per_group + (threadIdx.x >> s.lanes_log2); e < num_envs; e += step) {
        const U *from = reinterpret_cast<const U *>(s.src + e * s.src_stride);
        U *to = reinterpret_cast<U *>(s.dst + e * s.dst_stride);
        for (long long u = lane; u < s.units; u += lanes) to[u] = from[u];
    }
}

__global__ __launch_bounds__(kStoreThreads) void hns_rollout_store_kernel(const StoreArgs args) {
    const StoreSegment &s = args.seg[blockIdx.y];
    if (s.unit == 16) store_rows<uint4>(s, args.num_envs);
    else if (s.unit == 4) store_rows<uint32_t>(s, args.num_envs);
    else store_rows<unsigned char>(s, args.num_envs);
}

}  // namespace hns

extern "C" {

int hns_rollout_store(const hns_rollout_segment *segments, int32_t count, int64_t num_envs, int64_t slot, int64_t num_slots, void *stream) {
    const char *fn = "hns_rollout_store";
    if (!segments) return hns_fail(fn, "segments is a null pointer");
    if (count < 1 || count > HNS_ROLLOUT_MAX_SEGMENTS) return hns_fail(fn, "count outside [1, 16]");
    if (num_envs < 1) return hns_fail(fn, "num_envs must be >= 1");
    if (num_slots < 1) return hns_fail(fn, "num_slots must be >= 1");
    if (slot < 0 || slot >= num_slots) return hns_fail(fn, "slot outside [0, num_slots)");
    hns::StoreArgs args = {};
    args.num_envs = num_envs;
    long long most = 0;
    for (int i = 0; i < count; ++i) {
        const hns_rollout_segment &g = segments[i];
        const std::string at = "segments[" + std::to_string(i) + "].";
        if (!g.src) return hns_fail(fn, at + "src is a null pointer");
        if (!g.dst) return hns_fail(fn, at + "dst is a null pointer");
        if (g.row_bytes < 1 || g.row_bytes > hns::kStoreMaxRowBytes) return hns_fail(fn, at + "row_bytes outside [1, 1048576]");
        if (g.src_stride < g.row_bytes) return hns_fail(fn, at + "src_stride is shorter than row_bytes");
        if (num_slots > INT64_MAX / g.row_bytes || g.dst_stride < num_slots * g.row_bytes)
            return hns_fail(fn, at + "dst_stride is shorter than num_slots * row_bytes");
        if (num_envs > INT64_MAX / g.dst_stride) return hns_fail(fn, at + "dst_stride: num_envs * dst_stride overflows int64");
        if (num_envs > INT64_MAX / g.src_stride) return hns_fail(fn, at + "src_stride: num_envs * src_stride overflows int64");
        hns::StoreSegment &s = args.seg[i];
        s.src = static_cast<const unsigned char *>(g.src);
        s.dst = static_cast<unsigned char *>(g.dst) + slot * g.row_bytes;
        s.src_stride = g.src_stride;
        s.dst_stride = g.dst_stride;
        // the widest unit every address of the segment is a multiple of (slot * row_bytes is one when row_bytes is)
        const uintptr_t bits = reinterpret_cast<uintptr_t>(g.src) | reinterpret_cast<uintptr_t>(g.dst) | (uintptr_t)g.src_stride | (uintptr_t)g.dst_stride |
                               (uintptr_t)g.row_bytes;
        s.unit = (bits & 15) == 0 ? 16 : (bits & 3) == 0 ? 4 : 1;
        s.units = g.row_bytes / s.unit;
        while (s.lanes_log2 < 8 && (1ll << s.lanes_log2) < s.units) ++s.lanes_log2;      // the smallest power of two >= units, at most 256
        const long long per_group = hns::kStoreThreads >> s.lanes_log2;
        const long long need = (num_envs + per_group - 1) / per_group;                   // workgroups that cover every env once
        if (need > most) most = need;
    }
    long long groups = most;
    if (groups > hns::kStoreMaxGroups) groups = hns::kStoreMaxGroups;
    hipLaunchKernelGGL(hns::hns_rollout_store_kernel, dim3((unsigned)groups, (unsigned)count), dim3(hns::kStoreThreads), 0, static_cast<hipStream_t>(stream), args);
    HNS_CHECK_HIP(hipGetLastError());
    return HNS_OK;
}

}  // extern "C"
