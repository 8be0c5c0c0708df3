// hns_step_kernel.h — the fused HideAndSeek step kernel (one launch per env.step) for gfx950; instantiated per pursuer count by
// hns_inst.hip.  Reference call tree: transforms.py:425-459 -> lee_position_controller.py:476-550 -> hideandseek.py:725-744 ->
// multirotor.py:466-508 -> rotor_group.py:55-71 -> [PhysX sim.step() replaced by d_integrate] -> hideandseek.py:746-917 -> :919-1065.
// No MFMA: there is no dense contraction on this path.
#pragma once
#include "hns_common.h"

namespace hns {

// =================================================================================================
// The fused step kernel, third design (one evader, whole 64-env tiles): no workgroup barrier in front of the
// controller, loads issued in the order they are needed.
// =================================================================================================
// Wave-specialised step kernel (full tiles, one evader).  What the profiles of the first design showed: a launch is one
// residency round, so the load burst, each wave's serial instruction stream and the store drain were paid one after the other.  Here
//   * a pursuer wave needs nobody else's data for the controller: it loads ITS OWN 64 rigid-state rows (one contiguous
//     3.3 KB slice) through its private LDS slab, so the controller starts as soon as the first-issued loads have landed;
//   * the env wave owns everything about the evader: it fetches its envs' cylinders and evader position itself, stages
//     the cylinders for phase 3 and runs the potential field while the pursuer waves run controller and integration;
//   * pursuer <-> pursuer and pursuer <-> evader exchange goes through small published records (position at t, thrust
//     vector, position at t+1, line-of-sight flag), three workgroup barriers in all (six before);
//   * every store is a whole-line store from a wave-private slab.
// Arithmetic, evaluation order and results are those of hns_step_kernel (bit-identical; tests/test_hip_parity.py).
constexpr int kPub = 11;  // published per pursuer: position at t (3), thrust vector (3), position at t+1 (3), 1 / (|thrust| + 1e-6); odd stride
struct LdsV3 { int slab, slab_stride, pub, cyl, cyl_stride, tp, red, envout, term, term_stride, total; };
// per env: (tx, ty) of every cylinder's push on the second evader; odd stride.  Sized by the env's cylinder count since round 6: with the maximum's 33 floats
// a 3v2 / 8-cylinder workgroup took 53.5 KB of LDS — 0.5 KB too much for a third workgroup per CU (49.4 KB then; 39.5 KB = a FOURTH with v4_small_slabs, below)
__host__ __device__ constexpr int term_stride(int C) { return 2 * C + 1; }
// Rows per staging pass of the tile mapping's slabs (hns_common.h: slab_rows).  Three pursuers with two evaders stage half a wave at a time as the wide
// workgroups do: with whole-wave slabs of 24-value rows a workgroup took 49.4 KB of LDS and 131 registers = THREE workgroups per CU, i.e. 768 of a
// 65 536-env launch's 1 024 workgroups in a first round and 256 in a second (49 152 envs: 15.85 us, 65 536 envs: 24.4 us, tools/small_batch.py --targets=2, round 6).
// Half-wave slabs, the env wave's staging inside the (by then dead) cylinder-term region and the 128-register cap make it four per CU: one round.
__host__ __device__ constexpr bool v4_small_slabs(int A, int NT) { return NT == 2 && A == 3; }
__host__ __device__ constexpr int slab_rows_v4(int A, int NT) { return (A > 4 || v4_small_slabs(A, NT)) ? 32 : 64; }
__host__ __device__ inline int slab_floats_v4(int A, int K, int NT) {
    const int rows = slab_rows_v4(A, NT);
    int m = rows * (NT == 2 ? 24 : HNS_SELF_DIM);
    if (K > kMaxK) K = 0;                       // wide selections are stored by their threads, not staged
    if (rows * K * 5 > m) m = rows * K * 5;
    if (rows * (A - 1) * 3 > m) m = rows * (A - 1) * 3;
    return r4(m);
}
__host__ __device__ inline LdsV3 lds_layout_v3(int A, int C, int K, int NT = 1) {
    LdsV3 L;
    int o = 0;
    L.slab_stride = slab_floats_v4(A, K, NT);
    if (L.slab_stride < 64 * 13 + 4) L.slab_stride = r4(64 * 13 + 4);
    L.slab = o;  o += A * L.slab_stride;
    L.pub = o;   o += r4(kEPB * A * kPub);
    L.cyl_stride = (3 * C) | 1;
    L.cyl = o;   o += r4(kEPB * L.cyl_stride);
    L.tp = o;    o += r4(kEPB * (3 * NT + 1));               // evader(s) at t+1 ([64][3 NT], contiguous: stored as one slice) + the step counter
    L.red = o;   o += r4(kEPB * A * red_stride(NT));
    const int envout = r4(kEPB * (A > 3 * NT ? A : 3 * NT));  // the env wave's own staging: evader velocity [64,3 NT], rewards [64,A]
    L.term_stride = term_stride(C);
    const int term = NT == 2 ? r4(kEPB * L.term_stride) : 0;  // two evaders: the pursuer lanes' share of the evader policy (below)
    if (v4_small_slabs(A, NT) && term >= envout) {
        // the env wave is the term region's only reader (right behind barrier 1, before it stages anything) and the staging's only user: one region
        L.term = o; L.envout = o; o += term;
    } else {
        L.envout = o; o += envout;
        L.term = o;  o += term;
    }
    L.total = o;
    return L;
}

// env wave: `n` floats that sit contiguously in LDS -> one contiguous, 16-byte aligned slice of global memory, 16 B per lane
// (n % 4 == 0), write-through.  Per-lane 4-byte stores at a 12-byte stride would each be a partial-line write.
// (generic instantiation: only the first `nvalid` floats exist — 4-byte stores.)
template <bool GEN>
HNS_DEV void env_store_slice(const float *lds, float *g, int n, int lane, int nvalid) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if constexpr (GEN) {
        for (int i = lane; i < nvalid; i += 64) st_f1(g + i, lds[i]);
    } else {
        for (int i = lane; i < n / 4; i += 64) st_f4(reinterpret_cast<float4 *>(g) + i, reinterpret_cast<const float4 *>(lds)[i]);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Relative to the third design (same structure) the env wave — ONE wave, issuing one instruction every 5-7 cycles — relieved of most of its serial
// work (tools/phase_timeline.py: in the third design 5.8 us of the 14.5 us of a workgroup's life were env-wave work that the pursuer
// waves waited for):
//   * the line of sight evader -> pursuer at t (:1080) is not evaluated at all: it is the test the previous step (or the reset) ran on
//     the same positions for the observation (:786), carried in the fourth column of pid_last_rate (hns.h);
//   * the pursuers publish their reward terms BEFORE they build and store their observation rows, so the env wave's reductions, reward,
//     statistics and done run beside those stores instead of behind them; the detection mask of the evader's relative position
//     (:791-794) is applied by the pursuers themselves (was: the env wave patched the stored rows);
//   * everything but the pointers behind the first loads comes from a device-resident block through the scalar cache (StepArgs).
// Three workgroup barriers.
//
// Instantiations (hns_inst.hip): <A, NT, GEN, KM, PROF, CS>.  GEN = false is the kernel described above: whole 64-env tiles, k <= 4, nothing
// predicated.  GEN = true serves every other shape with the SAME phases, barriers, arithmetic and evaluation order (the buffers are
// bit-identical where both apply; tests/test_hip_parity.py): a ragged last tile (E % 64 != 0 — lanes beyond the batch load the last
// env's data again, compute, and store nothing; slices end at the batch through their buffer descriptors) and, with KM = kWideK,
// selections of up to 16 nearest cylinders (rows stored by their threads, not staged).  It reads the parameter block before its
// first loads and loads rigid-state rows per thread: correct, not tuned — no configuration of the reference's cfg/ needs it.
// CS > 0: the cylinder count as a compile-time constant, with k = 3 — the shapes of the reference's task files and of BASELINE's configurations
// (5, 8, 16 slots; obs_max_cylinder 3).  Same arithmetic, same order; the cylinder loops unroll completely and the k-nearest predicates
// fold away: 6v2 / 16 cylinders 50.4 -> 48.5 us, 3v1 / 8 cylinders 18.7 -> 18.5 us (A/B/A/B on one box, tools/lab/r04_batch18.sh).
// MOTOR (cfg.action_input = HNS_ACTION_MOTOR, include/hns.h): `action` holds the rotor commands of the caller's own controller transform
// (transforms.py:455-456) — the step starts at _pre_sim_step (hideandseek.py:725-744): no tanh / CTBR / PID; the action error is read from the
// bound buffer (:731), `prev_action`, `pid_integ`, `ctbr`, `target_rate` are left alone.  Served by the generic instantiation only (a
// compatibility path: the torch controller in front costs twenty times this kernel).
// Waves per SIMD the two-evader instantiations are compiled for (the second __launch_bounds__ argument; 512 / it = the VGPR budget).  Six pursuers —
// BASELINE configuration 5 — fit two 7-wave workgroups per CU at 4 (109 VGPRs).  With one to three pursuers every pursuer lane carries MORE of the second
// evader's share (3 * 16 / A staged cylinder values, 16 / A own cylinders: 195 / 134 / 131 VGPRs unconstrained), and at 128 the compiler spilled
// (31-35, 24, 3 registers to scratch: VERDICT r5 weak #8); their workgroups are 2-4 waves, so 2 / 3 / 3 waves per SIMD still place 4 / 4 / 3 of them on a CU.
__host__ __device__ constexpr int step_waves_per_simd(int A, int NT, int KM, bool MOTOR, int CS) {
    // (three pursuers: four with the cylinder count as a compile-time constant — 102-118 registers; the runtime-count instantiation needs 131 and stays at three)
    return (NT == 2 && KM == kMaxK && !MOTOR) ? (A == 1 ? 2 : A == 2 ? 3 : (A == 3 && CS == 0) ? 3 : 4) : 1;
}
// ---- contact response (include/hns.h): fp32, no FMA (the library builds with -ffp-contract=off), correctly rounded sqrt and / ----
// Stage 2 / 4: a body against the cylinder slots of its env, ascending; active slots (!(cz < 0)) whose top is above the body.  VEL: the inward
// radial velocity is removed as well (pursuers); the evader's position only.
template <bool VEL, int CS>
HNS_DEV void d_contact_cylinders(V3 &p, float &vx, float &vy, const float *cyl, int C, float R, float R2, float ch) {
    auto slot = [&](int k) {
        const float cx = cyl[3 * k], cy = cyl[3 * k + 1], cz = cyl[3 * k + 2];
        if (!(cz < 0.0f) && p.z < ch) {
            const float dx = p.x - cx, dy = p.y - cy;
            const float d2 = dx * dx + dy * dy;
            if (d2 < R2 && d2 > 0.0f) {
                const float r = __builtin_sqrtf(d2), inv = 1.0f / r;
                const float nx = dx * inv, ny = dy * inv;
                p.x = cx + nx * R;
                p.y = cy + ny * R;
                if constexpr (VEL) {
                    const float vn = vx * nx + vy * ny;
                    if (vn < 0.0f) { vx = vx - vn * nx; vy = vy - vn * ny; }
                }
            }
        }
    };
    if constexpr (CS > 0) {
#pragma unroll
        for (int k = 0; k < CS; ++k) slot(k);
    } else {
#pragma unroll 4
        for (int k = 0; k < C; ++k) slot(k);
    }
}
// Stages 1-3 for pursuer `a` of an env: `red` = the env's first pursuer record (integrated position at R_CPOS, velocity at R_CVEL), `cyl` its cylinder row.
template <int A, int CS, class Cfg>
HNS_DEV void d_contact_step(const Cfg &c, Rigid &s, int a, const float *red, const float *cyl, int C) {
    constexpr int kRedS = red_stride(1);
    const float D = c.contact_dd, D2 = c.contact_dd2;
    float cpx = 0.0f, cpy = 0.0f, cpz = 0.0f, cvx = 0.0f, cvy = 0.0f, cvz = 0.0f;
#pragma unroll
    for (int o = 0; o < A - 1; ++o) {                                           // stage 1: one Jacobi pass over the peers, ascending
        const int j = o + (o >= a ? 1 : 0);
        const float *rj = red + j * kRedS;
        const float dx = s.pos.x - rj[R_CPOS], dy = s.pos.y - rj[R_CPOS + 1], dz = s.pos.z - rj[R_CPOS + 2];
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 < D2 && d2 > 0.0f) {
            const float r = __builtin_sqrtf(d2), inv = 1.0f / r;
            const float nx = dx * inv, ny = dy * inv, nz = dz * inv;
            const float h = (D - r) * 0.5f;
            cpx = cpx + h * nx; cpy = cpy + h * ny; cpz = cpz + h * nz;
            const float vn = ((s.lin.x - rj[R_CVEL]) * nx + (s.lin.y - rj[R_CVEL + 1]) * ny) + (s.lin.z - rj[R_CVEL + 2]) * nz;
            if (vn < 0.0f) {
                const float g = -(vn * 0.5f);
                cvx = cvx + g * nx; cvy = cvy + g * ny; cvz = cvz + g * nz;
            }
        }
    }
    s.pos.x = s.pos.x + cpx; s.pos.y = s.pos.y + cpy; s.pos.z = s.pos.z + cpz;
    s.lin.x = s.lin.x + cvx; s.lin.y = s.lin.y + cvy; s.lin.z = s.lin.z + cvz;
    d_contact_cylinders<true, CS>(s.pos, s.lin.x, s.lin.y, cyl, C, c.contact_rd, c.contact_rd2, c.cylinder_height);   // stage 2
    if (c.ground_clamp && s.pos.z < 0.0f) {                                     // stage 3: the integrator's clamp again
        s.pos.z = 0.0f;
        if (s.lin.z < 0.0f) s.lin.z = 0.0f;
    }
}


// The kernel body (hns_step_body.inc) is shared by hns_step_v4_kernel (CONTACT = false: the step described above) and hns_step_contact_kernel
// (CONTACT = true: the contact response of include/hns.h between the integrator and everything that reads S_{t+1}).  It is included
// into both kernels rather than called as a __forceinline__ function: the inlined call compiled the CONTACT = false kernels to different code (the
// callee is simplified on its own before it is inlined), the textual body compiles them to exactly what the single kernel compiled to.
template <int A, int NT, bool GEN, int KM, bool PROF, int CS = 0, bool MOTOR = false>
__global__ __launch_bounds__(Geo<A>::T, step_waves_per_simd(A, NT, KM, MOTOR, CS)) void hns_step_v4_kernel(HNS_STEP_PARAMS) {
    constexpr bool CONTACT = false;
#include "hns_step_body.inc"
}

// The same step with the contact response (cfg.contact_response = 1; one evader, no phase stamps).  Selected by hns_inst.hip: the tuned tile mapping
// (whole tiles, k <= 4, CS in {0, 5, 8}, policy input) and the generic one (ragged, wide k, motor input); never the small-batch mapping.
template <int A, int NT, bool GEN, int KM, int CS, bool MOTOR>
__global__ __launch_bounds__(Geo<A>::T, step_waves_per_simd(A, NT, KM, MOTOR, CS)) void hns_step_contact_kernel(HNS_STEP_PARAMS) {
    constexpr bool PROF = false, CONTACT = true;
    static_assert(NT == 1, "contact response: one evader");
#include "hns_step_body.inc"
}

}  // namespace hns
