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
// One GRU per agent (the stacked actor of share_actor: false; hns_gru_forward_agents / hns_gru_backward_agents) is the same
// four bodies on tensors stacked over `inner` = A, sequence (b, a) on slice a:
//   hns_gru_fwd_agents_kernel, hns_gru_bwd_agents_kernel : a tile is 16 sequences of ONE agent (b = 16 i .. 16 i + 15 at fixed a).  The grid is
//                           A x gpa workgroups, gpa = min(ceil(outer / 16), floor(256 / A)): workgroup g belongs to agent g / gpa for the whole
//                           launch (its W_hh slice in registers as above) and walks that agent's tiles g % gpa, g % gpa + gpa, ...
//   hns_gru_wgrad_agents_kernel : the gate gradients are numbered agent-major, each agent's outer L rows padded to spa row ranges of tps 32-row
//                           tiles (spa = ceil(t / tps), tps = ceil(t / max(1, floor(256 / A))), t = ceil(outer L / 32)), so no range holds two
//                           agents; range r belongs to agent r / spa.  The padding rows are never read.
//   hns_gru_reduce_agents_kernel : agent a's spa weight partials and gpa LayerNorm partial rows, in index order, into slice a.
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

// One GRU per agent: what the _agents kernels take beside GruArgs, whose six parameter pointers are then the STACKED tensors, `tiles` the tiles
// of ONE agent and `dgate` the agent-major workspace
struct GruAgents {
    long long outer;                         // sequences per agent
    long long rpa;                           // gate-gradient rows per agent, padded to whole row ranges
    int gpa, spa;                            // sweep workgroups and weight-gradient row ranges per agent
};

// agent `ag`'s arguments: its slices of the stacked parameters and its block of the gate gradients
HNS_DEV GruArgs gru_agent_args(const GruArgs &a0, const GruAgents &g, int ag) {
    GruArgs a = a0;
    a.w_ih += (long long)ag * 3 * (kGruH * kGruH);
    a.w_hh += (long long)ag * 3 * (kGruH * kGruH);
    a.b_ih += ag * 3 * kGruH;
    a.b_hh += ag * 3 * kGruH;
    a.ln_w += ag * kGruH;
    a.ln_b += ag * kGruH;
    if (a.dgate) a.dgate += (long long)ag * g.rpa * (4 * kGruH);
    return a;
}

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

// The sweeps' and the weight-gradient kernel's bodies are hns_gru_bodies.inc, included as text by the shared kernels and by the _agents ones
// (one GRU per agent) under the macros that file names.  First the shared kernels: a tile is 16 consecutive sequences, tiles go round the grid.
#define GRU_TILE_FIRST blockIdx.x
#define GRU_TILE_STEP gridDim.x
#define GRU_SEQ(p) (p)
#define GRU_LIVE(p, q) ((q) < a.S)
#define GRU_GATE_SEQ qc
#define GRU_WG_RANGE split
#define GRU_WG_HROW row
__global__ __launch_bounds__(kGruThreads, 2) void hns_gru_fwd_kernel(const GruArgs a) {
#define GRU_BODY_FWD
#include "hns_gru_bodies.inc"
#undef GRU_BODY_FWD
}

__global__ __launch_bounds__(kGruThreads, 2) void hns_gru_bwd_kernel(const GruArgs a) {
#define GRU_BODY_BWD
#include "hns_gru_bodies.inc"
#undef GRU_BODY_BWD
}

// dW partials: per (row range, matrix) the 128 x 128 product dA^T operand over the range's rows, and the column sums of dA.  Matrices 0-2:
// W_ih's r, z, n thirds (dA blocks 0, 1, 2; operand x_t); 3-5: W_hh's (dA blocks 0, 1, 3; operand the masked h_{t-1}).  Row = s L + t.
__global__ __launch_bounds__(256, 2) void hns_gru_wgrad_kernel(const GruArgs a, long long rows, int tiles, int tps, float *part) {
#define GRU_BODY_WGRAD
#include "hns_gru_bodies.inc"
#undef GRU_BODY_WGRAD
}

#undef GRU_TILE_FIRST
#undef GRU_TILE_STEP
#undef GRU_SEQ
#undef GRU_LIVE
#undef GRU_GATE_SEQ
#undef GRU_WG_RANGE
#undef GRU_WG_HROW

// One GRU per agent: `g` says how the grid is divided, `a` is the agent's (gru_agent_args).
#define GRU_TILE_FIRST (blockIdx.x % g.gpa)
#define GRU_TILE_STEP g.gpa
#define GRU_SEQ(p) ((p) * a.inner + agent)
#define GRU_LIVE(p, q) ((p) < g.outer)
#define GRU_GATE_SEQ (q0 + col)
#define GRU_WG_RANGE (split % g.spa)
#define GRU_WG_HROW (q * a.L + st)
// one GRU per agent: workgroup blockIdx.x belongs to agent blockIdx.x / gpa for the whole launch and walks that agent's tiles
__global__ __launch_bounds__(kGruThreads, 2) void hns_gru_fwd_agents_kernel(const GruArgs a0, const GruAgents g) {
    const int agent = blockIdx.x / g.gpa;
    const GruArgs a = gru_agent_args(a0, g, agent);
#define GRU_BODY_FWD
#include "hns_gru_bodies.inc"
#undef GRU_BODY_FWD
}

// (the LayerNorm partial row is the workgroup's, hence one agent's)
__global__ __launch_bounds__(kGruThreads, 2) void hns_gru_bwd_agents_kernel(const GruArgs a0, const GruAgents g) {
    const int agent = blockIdx.x / g.gpa;
    const GruArgs a = gru_agent_args(a0, g, agent);
#define GRU_BODY_BWD
#include "hns_gru_bodies.inc"
#undef GRU_BODY_BWD
}

// one GRU per agent: range blockIdx.x is range blockIdx.x % spa of agent blockIdx.x / spa.  `rows`: ONE agent's live rows (row = b L + t of its
// block of the gate gradients; the sequence is b inner + agent everywhere else); `tiles`: its padded tile count, whole ranges
__global__ __launch_bounds__(256, 2) void hns_gru_wgrad_agents_kernel(const GruArgs a0, const GruAgents g, int tps, float *part) {
    const int agent = blockIdx.x / g.spa;
    const GruArgs a = gru_agent_args(a0, g, agent);
    const long long rows = g.outer * a.L;
    const int tiles = g.spa * tps;
#define GRU_BODY_WGRAD
#include "hns_gru_bodies.inc"
#undef GRU_BODY_WGRAD
}

#undef GRU_TILE_FIRST
#undef GRU_TILE_STEP
#undef GRU_SEQ
#undef GRU_LIVE
#undef GRU_GATE_SEQ
#undef GRU_WG_RANGE
#undef GRU_WG_HROW

struct GruGradOut {
    float *w_ih, *w_hh, *b_ih, *b_hh, *ln_w, *ln_b;
};

constexpr int kGruReduceN = 6 * kGruWgOut + 2 * kGruH;

// gradient value e: the fp64 sum of its partials in index order, rounded once.  e < 6 (128 128 + 128): matrix m's value or bias over the row
// ranges; then ln_w [128], ln_b [128] over the sweep's workgroups
HNS_DEV void gru_reduce_body(const float *wpart, int splits, const float *lnpart, int groups, const GruGradOut &o) {
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

__global__ __launch_bounds__(256) void hns_gru_reduce_kernel(const float *wpart, int splits, const float *lnpart, int groups, const GruGradOut o) {
    gru_reduce_body(wpart, splits, lnpart, groups, o);
}

// one GRU per agent: workgroup (b, agent) is the reduce kernel's block b on the agent's `spa` weight partials and `gpa` LayerNorm partial rows,
// written into the agent's slice of the stacked gradients
__global__ __launch_bounds__(256) void hns_gru_reduce_agents_kernel(const float *wpart, int spa, const float *lnpart, int gpa, const GruGradOut o0) {
    const int ag = blockIdx.y;
    const GruGradOut o{o0.w_ih + (long long)ag * 3 * kGruMat, o0.w_hh + (long long)ag * 3 * kGruMat, o0.b_ih + ag * 3 * kGruH, o0.b_hh + ag * 3 * kGruH,
                       o0.ln_w + ag * kGruH, o0.ln_b + ag * kGruH};
    gru_reduce_body(wpart + (long long)ag * spa * 6 * kGruWgOut, spa, lnpart + (long long)ag * gpa * (2 * kGruH), gpa, o);
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

// One GRU per agent: `outer` sequences per agent, `inner` = A agents.  The sweeps' A gpa workgroups and the weight-gradient kernel's A spa row
// ranges are divided evenly among the agents (both a function of the shape alone); the gate gradients hold rpa rows per agent
struct GruAgentsPlan {
    int tpa, gpa, tps, spa;
    long long rpa;
    size_t o_gate, o_wpart, o_ln, bytes;
};

bool gru_plan_agents(int64_t outer, int64_t inner, int32_t steps, GruAgentsPlan &p) {
    GruPlan one;
    if (inner < 1 || inner > HNS_MAX_AGENTS || outer < 1 || outer >= ((int64_t)1 << 40) / inner || !gru_plan(outer * inner, steps, one)) return false;
    const int A = (int)inner;
    p.tpa = (int)((outer + hns::kGruTile - 1) / hns::kGruTile);
    p.gpa = std::min(p.tpa, hns::kGruMaxGroups / A);
    const long long wg = (outer * steps + hns::kGruWgRows - 1) / hns::kGruWgRows;
    p.tps = (int)((wg + hns::kGruMaxSplits / A - 1) / (hns::kGruMaxSplits / A));
    p.spa = (int)((wg + p.tps - 1) / p.tps);
    p.rpa = (long long)p.spa * p.tps * hns::kGruWgRows;
    p.o_gate = 0;
    p.o_wpart = gru_round((size_t)A * p.rpa * hns::kGruGate * sizeof(float));
    p.o_ln = p.o_wpart + gru_round((size_t)A * p.spa * 6 * hns::kGruWgOut * sizeof(float));
    p.bytes = p.o_ln + gru_round((size_t)A * p.gpa * 2 * hns::kGruH * sizeof(float));
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

// hns_gru_forward and hns_gru_forward_agents (`agents`: the parameters stacked over seq->inner, one GRU per agent)
int gru_forward(const char *fn, bool agents, const hns_gru_net *net, const hns_gru_seq *seq, float *out, float *h_last, float *h_hist, void *workspace,
                void *stream) {
    hns::GruArgs a;
    GruPlan p;
    GruAgentsPlan pa;
    const int rc = gru_check(fn, net, seq, a, p);
    if (rc != HNS_OK) return rc;
    if (agents && !gru_plan_agents(seq->outer, seq->inner, seq->steps, pa)) return hns_fail(fn, "inner (one GRU per agent) must be in [1, 7]");
    if (!out || !h_last || !hns_aligned(out, 16) || !hns_aligned(h_last, 16)) return hns_fail(fn, "out and h_last must be non-NULL and 16-byte aligned");
    if (h_hist && !hns_aligned(h_hist, 16)) return hns_fail(fn, "h_hist must be 16-byte aligned");
    if (workspace && !hns_aligned(workspace, 256)) return hns_fail(fn, "workspace must be 256-byte aligned");
    a.out = out; a.h_last = h_last; a.h_hist = h_hist;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (agents) {
        a.tiles = pa.tpa;
        const hns::GruAgents g{seq->outer, pa.rpa, pa.gpa, pa.spa};
        hipLaunchKernelGGL(hns::hns_gru_fwd_agents_kernel, dim3((int)seq->inner * pa.gpa), dim3(hns::kGruThreads), 0, st, a, g);
    } else {
        hipLaunchKernelGGL(hns::hns_gru_fwd_kernel, dim3(p.groups), dim3(hns::kGruThreads), 0, st, a);
    }
    HNS_CHECK_HIP(hipGetLastError());
    return HNS_OK;
}

// hns_gru_backward and hns_gru_backward_agents
int gru_backward(const char *fn, bool agents, const hns_gru_net *net, const hns_gru_seq *seq, const float *h_hist, const float *dout, const float *dh_last,
                 const hns_gru_grads *grads, float *dx, float *dh0, void *workspace, size_t workspace_bytes, void *stream) {
    hns::GruArgs a;
    GruPlan p;
    GruAgentsPlan pa;
    const int rc = gru_check(fn, net, seq, a, p);
    if (rc != HNS_OK) return rc;
    if (agents && !gru_plan_agents(seq->outer, seq->inner, seq->steps, pa)) return hns_fail(fn, "inner (one GRU per agent) must be in [1, 7]");
    if (!grads) return hns_fail(fn, "null pointer");
    float *gw[6] = {grads->weight_ih, grads->weight_hh, grads->bias_ih, grads->bias_hh, grads->ln_w, grads->ln_b};
    for (int k = 0; k < 6; ++k)
        if (!gw[k] || !hns_aligned(gw[k], 16)) return hns_fail(fn, "gradient pointers must be non-NULL and 16-byte aligned");
    if (!h_hist) return hns_fail(fn, "h_hist is required: the forward pass's hidden states");
    if (!dout || !dx || !hns_aligned(h_hist, 16) || !hns_aligned(dout, 16) || !hns_aligned(dx, 16))
        return hns_fail(fn, "h_hist, dout and dx must be non-NULL and 16-byte aligned");
    if ((dh_last && !hns_aligned(dh_last, 16)) || (dh0 && !hns_aligned(dh0, 16))) return hns_fail(fn, "dh_last and dh0 must be 16-byte aligned");
    if (!workspace || !hns_aligned(workspace, 256)) return hns_fail(fn, "workspace must be non-NULL and 256-byte aligned");
    if (workspace_bytes < (agents ? pa.bytes : p.bytes)) return hns_fail(fn, "workspace too small");
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    float *wpart = reinterpret_cast<float *>(ws + (agents ? pa.o_wpart : p.o_wpart));
    a.hist = h_hist; a.dout = dout; a.dh_last = dh_last; a.dx = dx; a.dh0 = dh0;
    a.dgate = reinterpret_cast<float *>(ws + (agents ? pa.o_gate : p.o_gate));
    a.lnpart = reinterpret_cast<float *>(ws + (agents ? pa.o_ln : p.o_ln));
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const hns::GruGradOut o{gw[0], gw[1], gw[2], gw[3], gw[4], gw[5]};
    const dim3 reduce((hns::kGruReduceN + 255) / 256, agents ? (int)seq->inner : 1);
    if (agents) {
        const int A = (int)seq->inner;
        a.tiles = pa.tpa;
        const hns::GruAgents g{seq->outer, pa.rpa, pa.gpa, pa.spa};
        hipLaunchKernelGGL(hns::hns_gru_bwd_agents_kernel, dim3(A * pa.gpa), dim3(hns::kGruThreads), 0, st, a, g);
        HNS_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(hns::hns_gru_wgrad_agents_kernel, dim3(A * pa.spa, 6), dim3(256), 0, st, a, g, pa.tps, wpart);
        HNS_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(hns::hns_gru_reduce_agents_kernel, reduce, dim3(256), 0, st, wpart, pa.spa, a.lnpart, pa.gpa, o);
    } else {
        hipLaunchKernelGGL(hns::hns_gru_bwd_kernel, dim3(p.groups), dim3(hns::kGruThreads), 0, st, a);
        HNS_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(hns::hns_gru_wgrad_kernel, dim3(p.splits, 6), dim3(256), 0, st, a, p.rows, p.wg_tiles, p.tps, wpart);
        HNS_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(hns::hns_gru_reduce_kernel, reduce, dim3(256), 0, st, wpart, p.splits, a.lnpart, p.groups, o);
    }
    HNS_CHECK_HIP(hipGetLastError());
    return HNS_OK;
}

}  // namespace

extern "C" {

size_t hns_gru_workspace_bytes(int64_t seqs, int32_t steps, int32_t backward) {
    GruPlan p;
    if (!gru_plan(seqs, steps, p)) return 0;
    return backward ? p.bytes : 0;
}

size_t hns_gru_agents_workspace_bytes(int64_t outer, int64_t inner, int32_t steps, int32_t backward) {
    GruAgentsPlan p;
    if (!gru_plan_agents(outer, inner, steps, p)) return 0;
    return backward ? p.bytes : 0;
}

int hns_gru_forward(const hns_gru_net *net, const hns_gru_seq *seq, float *out, float *h_last, float *h_hist, void *workspace, size_t workspace_bytes,
                    void *stream) {
    (void)workspace_bytes;
    return gru_forward("hns_gru_forward", false, net, seq, out, h_last, h_hist, workspace, stream);
}

int hns_gru_forward_agents(const hns_gru_net *nets, const hns_gru_seq *seq, float *out, float *h_last, float *h_hist, void *workspace,
                           size_t workspace_bytes, void *stream) {
    (void)workspace_bytes;
    return gru_forward("hns_gru_forward_agents", true, nets, seq, out, h_last, h_hist, workspace, stream);
}

int hns_gru_backward(const hns_gru_net *net, const hns_gru_seq *seq, const float *h_hist, const float *dout, const float *dh_last,
                     const hns_gru_grads *grads, float *dx, float *dh0, void *workspace, size_t workspace_bytes, void *stream) {
    return gru_backward("hns_gru_backward", false, net, seq, h_hist, dout, dh_last, grads, dx, dh0, workspace, workspace_bytes, stream);
}

int hns_gru_backward_agents(const hns_gru_net *nets, const hns_gru_seq *seq, const float *h_hist, const float *dout, const float *dh_last,
                            const hns_gru_grads *grads, float *dx, float *dh0, void *workspace, size_t workspace_bytes, void *stream) {
    return gru_backward("hns_gru_backward_agents", true, nets, seq, h_hist, dout, dh_last, grads, dx, dh0, workspace, workspace_bytes, stream);
}

}  // extern "C"
