/*
 * hns.h — C ABI of the MI355X-native HideAndSeek environment step.
 *
 * The reference (thu-uav/Multi-UAV-pursuit-evasion) has no FFI: its environment is the Python
 * class `HideAndSeek(IsaacEnv)` and the physics is PhysX behind `omni.isaac.core`.  This
 * header is the boundary a maintainer binds *below* that Python class; each entry point names
 * the reference code it replaces (paths relative to the reference repo):
 *
 *   hns_step   <->  TransformedEnv.step = PIDRateController._inv_call
 *                   (omni_drones/utils/torchrl/transforms.py:425-459)
 *                   + IsaacEnv._step (omni_drones/envs/isaac_env.py:231-240)
 *                   = HideAndSeek._pre_sim_step (envs/hide_and_seek/hideandseek.py:725-744)
 *                   + sim.step() [PhysX; replaced by the documented integrator, DESIGN.md §A5]
 *                   + _compute_state_and_obs (:746-917) + _compute_reward_and_done (:919-1065)
 *   hns_reset  <->  IsaacEnv._reset (isaac_env.py:210-225) = HideAndSeek._reset_idx
 *                   (hideandseek.py:609-723) + MultirotorBase._reset_idx
 *                   (robots/drone/multirotor.py:635-650) + the reset-time obs pass
 *   hns_create <->  IsaacEnv.__init__/HideAndSeek.__init__ parameter capture
 *                   (isaac_env.py:54-151, hideandseek.py:236-325, 435-455)
 *
 * Conventions: plain C types only; every `float*`/`uint8_t*` in hns_buffers is a DEVICE
 * pointer owned by the caller (e.g. torch tensors) that must stay valid while bound;
 * functions return 0 on success and a negative hns_status on error, never throw, never
 * allocate device memory after hns_create, never synchronise a stream or the device (three documented exceptions: hns_bind's FIRST
 * call does one blocking 1 KB upload; hns_step_kernel_ms waits for its last sample; a configuration setter waits only if eight
 * earlier changes are still queued).  hns_step / hns_reset / hns_tp_observe / the setters are legal inside a stream capture (a configuration change made inside a capture takes one of 16 pinned images made by hns_create and keeps it for the env's lifetime; HNS_ERR_CONFIG once they are used up).
 * The configuration setters (hns_set_v_prey, hns_set_smoothness_coef, hns_set_phase_profile) and a repeated hns_bind change a
 * device-resident parameter block with ONE stream-ordered copy enqueued on the stream of the latest hns_step / hns_reset / hns_tp_observe call
 * (the null stream before the first): launches already enqueued there keep the old values, later launches and graph replays on
 * that stream see the new ones.  The HIP device current at the call must be the env's.  Quaternions are
 * (w,x,y,z) (omni_drones/utils/torch.py:62,125).  All tensors are C-contiguous fp32 unless noted.
 */
#ifndef HNS_H_
#define HNS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HNS_ABI_VERSION 8
#define HNS_MAX_AGENTS 7    /* pursuers per env: a workgroup is 64 envs = A pursuer waves + one env wave (<= 512 threads) */
#define HNS_MAX_CYLINDERS 16
#define HNS_NUM_STATS 24    /* hideandseek.py:400-425 */
#define HNS_SELF_DIM 20     /* state_self without TP prediction, hideandseek.py:856-863 */

typedef enum hns_status {
    HNS_OK = 0,
    HNS_ERR_INVALID_ARG = -1,
    HNS_ERR_NOT_BOUND = -2,
    HNS_ERR_DEVICE = -3,   /* HIP runtime error, see hns_last_error() */
    HNS_ERR_NO_DEVICE = -4,
    HNS_ERR_CONFIG = -5    /* e.g. fewer free grid cells than cylinders, hideandseek.py:112-113 */
} hns_status;

/* row index of each statistic in hns_buffers.stats ([HNS_NUM_STATS][E]); order = spec order */
typedef enum hns_stat {
    HNS_ST_SUCCESS = 0, HNS_ST_COLLISION, HNS_ST_BLOCKED, HNS_ST_DISTANCE_REWARD,
    HNS_ST_DISTANCE_PREDICTED_REWARD, HNS_ST_SPEED_REWARD, HNS_ST_COLLISION_REWARD,
    HNS_ST_COLLISION_WALL, HNS_ST_COLLISION_CYLINDER, HNS_ST_COLLISION_DRONE,
    HNS_ST_DETECT_REWARD, HNS_ST_CATCH_REWARD, HNS_ST_SMOOTHNESS_REWARD, HNS_ST_SMOOTHNESS_MEAN,
    HNS_ST_SMOOTHNESS_MAX, HNS_ST_FIRST_CAPTURE_STEP, HNS_ST_SUM_DETECT_STEP, HNS_ST_RETURN,
    HNS_ST_ACTION_ERROR_ORDER1_MEAN, HNS_ST_ACTION_ERROR_ORDER1_MAX, HNS_ST_TARGET_PREDICTED_ERROR,
    HNS_ST_DISTANCE_THRESHOLD_L, HNS_ST_OUT_OF_ARENA, HNS_ST_SMOOTHNESS_COEF
} hns_stat;

/* What hns_step's `action` is — i.e. on which side of the boundary the reference's action transform runs (scripts/train.py:165-171).
 *   HNS_ACTION_POLICY: the raw policy output (pre-tanh).  hns_step runs PIDRateController._inv_call (transforms.py:425-459) and the
 *                      body-rate PID (lee_position_controller.py:476-550) itself; `prev_action`, `action_error`, `pid_*` are its state / outputs.
 *   HNS_ACTION_MOTOR:  the four rotor commands that transform left in ("agents","action") (transforms.py:455-456: the caller keeps
 *                      `action_transform: PIDrate` and runs the torch controller in front, as the reference's own task file has it).  hns_step
 *                      starts at HideAndSeek._pre_sim_step (hideandseek.py:725-744): `action` goes straight to the rotors (A3); `prev_action` and
 *                      `action_error` are INPUTS — what the transform set under ("info","prev_action") / ("stats","action_error_order1"),
 *                      copied into the bound buffers by the caller (:729-731) — and are not written; `pid_integ`, `reset_pid`, `ctbr`, `target_rate`
 *                      are not touched (the caller's controller owns that state); of `pid_last_rate` only the line-of-sight column (w) is. */
typedef enum hns_action_input { HNS_ACTION_POLICY = 0, HNS_ACTION_MOTOR = 1 } hns_action_input;

/* How reset places bodies (hideandseek.py:613-689). */
typedef enum hns_init_mode {
    HNS_INIT_RANDOM = 0,   /* use_random_cylinder=1, use_eval=0: uniform boxes + grid cylinders */
    HNS_INIT_EVAL = 1,     /* use_random_cylinder=1, use_eval=1: fixed xy, random z, zero rpy */
    HNS_INIT_SCENARIO = 2  /* use_random_cylinder=0: fixed drone/target/cylinder positions */
} hns_init_mode;

/*
 * All scalars the step/reset math needs, resolved on the host from cfg/task/HideAndSeek*.yaml
 * and robots/assets/usd/crazyflie.yaml.  Derived values are computed by the host in fp32
 * exactly as the reference computes them (noted per field).
 */
typedef struct hns_cfg {
    int32_t abi_version;       /* = HNS_ABI_VERSION */
    int32_t num_envs;          /* E  (this process' shard) */
    int32_t num_agents;        /* A  cfg.task.num_agents */
    int32_t num_cylinders;     /* C  cfg.task.cylinder.max_num (slots incl. inactive) */
    int32_t obs_max_cylinder;  /* k  cfg.task.cylinder.obs_max_cylinder (<= C) */
    int32_t max_episode_length;
    int32_t use_deployment;    /* smoothness reward on/off, hideandseek.py:993 */
    int32_t fixed_yaw;         /* crazyflie.yaml:6 */
    int32_t ground_clamp;      /* integrator: inelastic ground plane at z=0 */
    int32_t write_critic_state;/* also fill buffers.state_drones */
    int32_t init_mode;         /* hns_init_mode */
    int32_t cyl_min_num;       /* cylinder.min_num */
    int32_t cyl_fixed_num;     /* cylinder.fixed_num, -1 = null */
    int32_t grid_num;          /* int(arena*2/(2*size)) = 9, hideandseek.py:579 */
    int32_t env_index_offset;  /* global index of local env 0 (multi-GPU shard); keys the reset RNG */
    int32_t num_targets;       /* evaders per env: 0 or 1 = the reference (one evader); 2 = two-evader extension (below) */

    float dt;                  /* cfg.sim.dt */
    float gravity;             /* 9.81 */
    /* task */
    float arena_size, max_height, cylinder_size, cylinder_height;
    float catch_radius, drone_detect_radius, target_detect_radius, collision_radius;
    float v_drone;             /* speed-penalty threshold AND PhysX max_linear_velocity (hideandseek.py:539) */
    float v_prey;              /* v_drone * cfg.task.v_prey (hideandseek.py:263); runtime-updatable */
    float dist_reward_coef, catch_reward_coef, detect_reward_coef, collision_coef, speed_coef;
    float smoothness_coef;     /* min(max_smoothness_coef, init + smooth_lr*update_epoch), :988-989 */
    float mask_value;          /* -5, hideandseek.py:305 */
    float invalid_z;           /* -20, hideandseek.py:451 */
    float grid_size;           /* 2*cylinder_size */
    float arena_sq;            /* fp32(arena_size**2): python-double square, then cast (hideandseek.py:1096,979) */
    float coll_drone_dist;     /* fp32(2.0*collision_radius) (hideandseek.py:973) */
    float boundary;            /* arena_size - 0.1 */
    /* drone (Crazyflie) */
    float mass;
    float inertia[3];          /* diagonal */
    float kf[4];               /* max_rot_vel^2 * force_constant, rotor_group.py:41 */
    float km[4];               /* max_rot_vel^2 * moment_constant, rotor_group.py:42 */
    float rotor_dir[4];        /* directions */
    float rotor_px[4];         /* arm_length*cos(angle): torque_y = -sum(px*T) */
    float rotor_py[4];         /* arm_length*sin(angle): torque_x =  sum(py*T) */
    float tau_up, tau_down;    /* dt / clamp(time_constant,0,1), rotor_group.py:58-61 */
    float max_thrust_ratio, target_clip;
    float hover_throttle;      /* sqrt(m*g / sum(kf)), multirotor.py:647-648 */
    float pid_kp[3], pid_ki[3], pid_kd[3], pid_ilimit[3], pid_outlimit; /* lee_position_controller.py:446-452 */
    /* integrator (PhysX-like) */
    float lin_damp_factor;     /* max(0, 1 - dt*linear_damping)  (robots/config.py:32) */
    float ang_damp_factor;     /* max(0, 1 - dt*angular_damping) (robots/config.py:34) */
    float max_ang_vel;         /* 1000 rad/s (robots/config.py:38) */
    float inv_mass;            /* fp32(1/mass), fp32(1/inertia): the integrator multiplies by reciprocals */
    float inv_inertia[3];
    float inv_num_agents;      /* 1.0f/A: torch's CUDA mean multiplies the sum by 1/N (ReduceMomentKernel.cu) */
    float inv_max_episode_length; /* 1.0f/max_len: CUDA `tensor / python_scalar` multiplies by the fp32 reciprocal */
    float max_lin_vel;         /* v_drone*(1-1e-6): PhysX max_linear_velocity (hideandseek.py:539), set a hair
                                  inside so the clamped speed never trips `speed > v_drone` (:952) by rounding */
    float inv_dt;              /* fp32(1/fp32(dt)): `(rate - last) / self.dt` (lee_position_controller.py:509) on CUDA multiplies by the
                                  fp32 reciprocal of the Python scalar (BinaryDivTrueKernel.cu) */
    /* reset distributions (hideandseek.py:283-313) */
    float drone_xy_lo[2], drone_xy_hi[2], target_xy_lo[2], target_xy_hi[2];
    float z_lo, z_hi;
    float rpy_lo[3], rpy_hi[3];
    /* fixed placements for HNS_INIT_EVAL (xy only) / HNS_INIT_SCENARIO (hideandseek.py:480-531,633-682) */
    float fixed_drone_pos[HNS_MAX_AGENTS + 1][3];
    float fixed_target_pos[3];
    float fixed_cyl_pos[HNS_MAX_CYLINDERS][3];
    int32_t fixed_cyl_active;  /* HNS_INIT_SCENARIO: number of active cylinders */
    int32_t tp_use_obstacles;  /* task.use_obstacles: the predictor's frame also holds [x, y, cylinder_size] of every cylinder slot
                                  (hideandseek.py:808-816); 0 = the reference's default */
    int32_t pid_reset_on_reset;/* 0 = the reference: `_reset_idx` (hideandseek.py:609-723) never touches the body-rate controller; its integrator and
                                  last body rate are cleared only through `reset_pid` at the next step (buffers.reset_pid).  1 = hns_reset also zeroes
                                  pid_integ / pid_last_rate of the envs it resets (a fresh controller per episode; rounds 1-3 of this build) */
    int32_t stats_stride;      /* floats between consecutive rows of buffers.stats: 0 = num_envs (a [HNS_NUM_STATS, E] array of its own); a larger
                                  value lets an env over a SLICE of a bigger batch address its columns of that batch's array in place (the Python
                                  env steps the two halves of its batch on two streams when the predictor is on) */
    int32_t reset_extra_step;  /* 1 = the reference: `_reset_idx` ends with one `sim.step()` of the WHOLE scene (hideandseek.py:722-723) — every drone of
                                  every env (reset or not) integrates one dt with no rotor force (gravity + damping), every evader moves one dt with
                                  the velocity it holds; then the observation of all envs is recomputed (isaac_env.py:221).  0 = no extra step */
    int32_t action_input;      /* hns_action_input: what `action` of hns_step holds (below) */
    /* contact response (ABI 6; NOT the reference's PhysX contacts — an opt-in model, DESIGN.md §A5, described below) */
    int32_t contact_response;  /* 0 = off (the default: bodies pass through cylinders and each other, as every earlier build); 1 = on */
    float contact_drone_radius;   /* r_d: task.contact_drone_radius (0.05) */
    float contact_target_radius;  /* r_t: task.contact_target_radius (0.05, the reference's evader sphere, hideandseek.py:544-551) */
    float contact_dd;          /* D   = fp32(2 r_d): distance of two pursuers in contact */
    float contact_dd2;         /* D2  = fp32(D*D) */
    float contact_rd;          /* Rd  = fp32(cylinder_size + r_d): pursuer <-> cylinder axis in contact */
    float contact_rd2;         /* Rd2 = fp32(Rd*Rd) */
    float contact_rt;          /* Rt  = fp32(cylinder_size + r_t): evader <-> cylinder axis in contact */
    float contact_rt2;         /* Rt2 = fp32(Rt*Rt) */
    int32_t contact_pad[7];    /* zero: the nine contact words padded to one 64-byte line, so that every field the device parameter block
                                  holds behind the config keeps its place within a scalar-cache line */
} hns_cfg;

/*
 * Contact response (cfg.contact_response = 1; a documented model, not PhysX — DESIGN.md §A5).  Runs inside hns_step after the
 * integrator (ground clamp included) and before anything reads S_{t+1}; inelastic, frictionless, cylinders of infinite mass,
 * pursuers of equal mass, fp32 without FMA, correctly rounded sqrt and division.  p, v: integrated position / velocity.
 *   1. pursuer <-> pursuer, one Jacobi pass: for pursuer a, peers j != a ascending: d = p_a - p_j, d2 = (dx*dx + dy*dy) + dz*dz;
 *      if d2 < D2 && d2 > 0: r = sqrt(d2), inv = 1/r, n = d*inv, cp += ((D - r)*0.5f)*n,
 *      vn = ((va.x-vj.x)*n.x + (va.y-vj.y)*n.y) + (va.z-vj.z)*n.z, if vn < 0: cv += (-(vn*0.5f))*n.  Then p_a += cp, v_a += cv (cp, cv from 0).
 *   2. pursuer <-> cylinder, slots ascending, active slots (!(cz < 0)) with p.z < cylinder_height: dx = px - cx, dy = py - cy,
 *      d2 = dx*dx + dy*dy; if d2 < Rd2 && d2 > 0: r = sqrt(d2), n = (dx, dy)*(1/r), px = cx + n.x*Rd, py = cy + n.y*Rd,
 *      vn = vx*n.x + vy*n.y, if vn < 0: vx -= vn*n.x, vy -= vn*n.y.
 *   3. the integrator's ground clamp again (cfg.ground_clamp).
 *   4. evader <-> cylinder: stage 2 on the evader's new position with Rt / Rt2, position only (target_vel stays the policy's velocity).
 * Not modelled: pursuer <-> evader (capture happens far earlier), arena walls and ceiling (no colliders in the reference), friction,
 * restitution, the reset's extra physics step.  hns_create refuses it with num_targets = 2.
 */

/*
 * Two-evader extension (num_targets = 2; NOT in the reference — BASELINE config 5 "6-pursuer/2-evader"):
 * each evader runs the reference's potential-field policy (hideandseek.py:1067-1141) on its own against all
 * pursuers, the arena and the cylinders (evaders ignore each other); line of sight, detection and masking
 * are evaluated per evader; the distance reward refers to the NEAREST evader, the catch reward to ANY
 * evader captured by any pursuer; `blocked` counts steps in which no pursuer sees either evader.  Shapes:
 * target_pos / target_vel [E,2,3]; obs_self / state_drones rows have 24 values = the reference's 20, the
 * relative position of evader 1, one zero; detect[e] is a bit mask (bit k = evader k detected); task vectors
 * are [drones | evader 0 | evader 1 | cylinders].  The predictor (hns_tp_*) runs the SAME network once per evader: unit u = 2 e + j
 * sees evader j's position / velocity under detection bit j; history / pred / groundtruth / tp_done are [2E, ...] (unit-major), the rows
 * have 24 + 6F values = [the reference's 20 + 3F row for evader 0 | relative position of evader 1, 0 | drone - predicted evader 1 (3F)].
 */
/* Device buffers, caller-owned.  Shapes in brackets; E,A,C,k as in hns_cfg. */
typedef struct hns_buffers {
    /* persistent state, updated in place */
    float *drone_state;    /* [E,A,13] pos3 quat4 linvel3 angvel3, world frame == info.drone_state */
    float *throttle;       /* [E,A,4]  rotor throttle, multirotor.py:216 */
    float *pid_integ;      /* [E,A,4]  xyz + pad, lee_position_controller.py:497-502 */
    float *pid_last_rate;  /* [E,A,4]  xyz + the pursuer's line-of-sight flag(s) in the state the buffers hold: 1 = the line to the evader
                            *          is blocked by a cylinder (+2 = to the second evader).  Derived state: written by step and reset
                            *          from the observation pass (hideandseek.py:786), read by the next step as the evader policy's
                            *          test (:1080) — same positions, same result; hns_set_state recomputes it from what it uploads. */
    float *prev_action;    /* [E,A,4]  == info.prev_action (ctbr of the last step) */
    float *target_pos;     /* [E,3]    evader position ([E,2,3] with num_targets = 2) */
    float *target_vel;     /* [E,3]    evader linear velocity set this step (hideandseek.py:741) */
    float *cylinders;      /* [E,C,3]  z<0 => inactive */
    float *progress;       /* [E]      float step counter, isaac_env.py:142-147 */
    float *stats;          /* [HNS_NUM_STATS,E] */
    /* per-step outputs */
    float *obs_self;       /* [E,A,20]       agents.observation.state_self */
    float *obs_others;     /* [E,A,A-1,3]    agents.observation.state_others (unused when A==1) */
    float *obs_cylinders;  /* [E,A,k,5]      agents.observation.cylinders == agents.state.cylinders */
    float *state_drones;   /* [E,A,20]       agents.state.state_drones; may be NULL if !write_critic_state */
    float *reward;         /* [E,A]          agents.reward */
    float *action_error;   /* [E,A]          stats.action_error_order1 (transforms.py:441) */
    uint8_t *done;         /* [E]            bool */
    uint8_t *detect;       /* [E]            bool, nullable: broadcast_detect (hideandseek.py:791), used by the TP_net input */
    /* failure detection (nullable): one sticky word, OR-ed by hns_step on the device, never cleared by the library.
     * bit 0: some pursuer's new rigid state is not finite; bit 1: some evader's new position; bit 2: some reward.
     * "Not finite" is decided on the left-to-right fp32 sum s of the values concerned: (s - s) != 0. */
    uint32_t *nonfinite;   /* [1] */
    /* optional outputs (nullable): the two extra keys PIDRateController._inv_call leaves on the tensordict (transforms.py:456-457) */
    float *ctbr;           /* [E,A,4]        controller output (roll, pitch, yaw command, thrust), lee_position_controller.py:548 */
    float *target_rate;    /* [E,A,4]        target body rate in deg/s (x, y, z, 0), transforms.py:447 */
    /* optional INPUT of hns_step (nullable): `reset_pid = tensordict['done']` (transforms.py:449-454 -> lee_position_controller.py:497-502) —
     * envs whose byte is non-zero start the step with pid_integ = pid_last_rate = 0.  It is read at the very beginning of the step and may ALIAS
     * `done` (written at its very end): the step then consumes the `done` its predecessor (or a reset, which clears it) left — what the root `done`
     * of a stepped tensordict holds in the reference's collector / rollout loops.  NULL = never reset through the step. */
    const uint8_t *reset_pid; /* [E] */
} hns_buffers;

/*
 * Hover task (BASELINE config 1, reference omni_drones/envs/single/hover.py): one Crazyflie per env,
 * 20-dim observation, position/heading/uprightness reward.  Plumbing-scale (tens of envs), so the
 * entry points are stateless: cfg (drone + sim fields of hns_cfg; num_agents = 1) and buffers per call.
 */
#define HNS_HOVER_NUM_STATS 39  /* hover.py:238-278, spec order */
#define HNS_HOVER_NUM_ACC 12    /* *_episode accumulators and last_* values, hover.py:150-155,313-320 */
typedef struct hns_hover_cfg {
    float reward_distance_scale, reward_v_scale, reward_acc_scale, reward_jerk_scale;
    float linear_vel_max, linear_acc_max;
    float alpha;                /* 0.8, hover.py:148 */
    float target_pos[3];        /* (0,0,1), hover.py:146 */
    float target_heading[3];    /* quat_axis(target_rot, 0) with target rpy = 0 -> (1,0,0), hover.py:301-303 */
    float pos_lo[3], pos_hi[3]; /* hover.py:129-132 */
    float rpy_lo[3], rpy_hi[3]; /* hover.py:137-140 */
} hns_hover_cfg;
typedef struct hns_hover_buffers {
    float *drone_state;   /* [E,1,13] */
    float *throttle, *pid_integ, *pid_last_rate, *prev_action;   /* [E,1,4] */
    float *progress;      /* [E] */
    float *stats;         /* [HNS_HOVER_NUM_STATS,E] */
    float *acc;           /* [HNS_HOVER_NUM_ACC,E] */
    float *obs;           /* [E,1,20] */
    float *reward;        /* [E,1] */
    uint8_t *done;        /* [E] */
} hns_hover_buffers;
/* One Hover step = PIDRateController._inv_call + Hover._pre_sim_step + integrator + _compute_state_and_obs
 * + _compute_reward_and_done (hover.py:322-523).  `cfg` supplies num_envs, max_episode_length, dt and the
 * drone/controller/integrator constants. */
int hns_hover_step(const hns_cfg *cfg, const hns_hover_cfg *hover, const hns_hover_buffers *buffers,
                   const float *action, void *stream);
/* Hover._reset_idx (hover.py:285-320) for the masked envs (NULL = all) + their observation. */
int hns_hover_reset(const hns_cfg *cfg, const hns_hover_cfg *hover, const hns_hover_buffers *buffers,
                    const uint8_t *reset_mask, uint64_t seed, uint32_t epoch, void *stream);

typedef struct hns_env hns_env;

/* Validate cfg, select the kernel specialisation, allocate nothing on the device.  The env belongs to the HIP
 * device that is current at this call: bind buffers of that device and launch with it current. */
int hns_create(const hns_cfg *cfg, hns_env **out);
void hns_destroy(hns_env *env);

/* Attach caller-owned device buffers (may be called again to re-point).  Host pointers and memory of another
 * GPU are refused here (HNS_ERR_INVALID_ARG) rather than faulting in a kernel; alignment is checked too. */
int hns_bind(hns_env *env, const hns_buffers *buffers);

/* One environment step for all E envs.  `action` = raw policy output [E,A,4] (pre-tanh) — or, with cfg.action_input =
 * HNS_ACTION_MOTOR, the rotor commands of the caller's own controller transform (hns_action_input above) —
 * device pointer.  `stream` is a hipStream_t (NULL = default stream).  Asynchronous. */
int hns_step(hns_env *env, const float *action, void *stream);

/* Reset the envs whose reset_mask byte is non-zero (NULL = all) and recompute their
 * observation.  `reset_mask` is a device pointer [E] (e.g. buffers.done).  Random draws come
 * from Philox4x32-10 keyed by (seed, global env index, reset epoch); the epoch is a host
 * counter advanced by every call.  Asynchronous. */
int hns_reset(hns_env *env, const uint8_t *reset_mask, uint64_t seed, void *stream);

/* envgen reset (hideandseek_envgen.py:875-902): like hns_reset, but the masked envs with index >=
 * task_first take their placement from `tasks` (device pointer, [E, 3A+3+3C] rows = drone positions,
 * evader position, cylinder positions — the reference's task vector; [E, 3A+6+3C] with both evaders'
 * positions in the two-evader extension) instead of sampling it;
 * orientations are still drawn from the Philox stream.  Masked envs < task_first reset as in hns_reset and
 * their rows of `tasks` are WRITTEN: the placement as sampled, before the extra physics step of
 * cfg.reset_extra_step (the reference archives `tasks_unif` as sampled, :883-895, and steps the scene
 * afterwards, :1013).  Rows of envs that are not masked are left alone. */
int hns_reset_tasks(hns_env *env, const uint8_t *reset_mask, float *tasks, int32_t task_first, uint64_t seed,
                    void *stream);

/* Extension, not in the reference: planar ray-fan range sensor on the bound state.
 * out: device pointer [E,A,num_rays]; ray r of a pursuer points along its horizontal heading rotated by
 * 2*pi*r/num_rays; range = distance to the first active cylinder or the arena wall, clamped to max_range. */
int hns_raycast(hns_env *env, int num_rays, float max_range, float *out, void *stream);

/*
 * Trajectory predictor in the observation (reference default `algo.use_TP_net: 1`).
 * Replaces the TP branch of HideAndSeek._compute_state_and_obs (hideandseek.py:805-854,871-880)
 * incl. the TP_net forward (learning/mappo.py:572-589: LSTM(I -> 64, 1 layer, zero initial state)
 * + Linear(64 -> 3F) + tanh) evaluated on a T-frame history, I = 7 + 3A (+ 3C with cfg.tp_use_obstacles):
 *   frame = [progress, evader pos (masked), evader vel (masked), pursuer positions]   (:815-820)
 *           + [x, y, cylinder_size] of every cylinder slot with task.use_obstacles     (:808-816)
 * I <= 80 (five 16-wide operand chunks): every shape the step kernels take (7 pursuers + 16 cylinder slots = 76 values).
 * The parameters are the caller's tensors in PyTorch layouts (the learner trains them,
 * scripts/train.py:180).  They are converted into a matrix-core operand image (`packed`) by
 * hns_tp_refresh: call it after every parameter update (hns_tp_bind schedules one).
 */
#define HNS_TP_HIDDEN 64           /* TP_net.hidden_dim, mappo.py:576 */
typedef struct hns_tp_buffers {
    const float *w_ih;        /* [4*64, I]   lstm.weight_ih_l0, gate order i,f,g,o */
    const float *w_hh;        /* [4*64, 64]  lstm.weight_hh_l0 */
    const float *b_ih;        /* [4*64]      lstm.bias_ih_l0 */
    const float *b_hh;        /* [4*64]      lstm.bias_hh_l0 */
    const float *w_fc;        /* [3F, 64]    fc.weight */
    const float *b_fc;        /* [3F]        fc.bias */
    void *packed;             /* [hns_tp_packed_bytes()] scratch, 16-byte aligned: operand image of the parameters */
    /* U = E units, or 2E with num_targets = 2 (unit 2 e + j = evader j of env e: the two-evader extension above) */
    float *history;           /* [U,T,I]  state: the sliding window == agents.TP.TP_input, oldest frame first */
    float *pred;              /* [U,F,3]  out: predicted evader positions, arena units (hideandseek.py:834-836) */
    float *obs_self;          /* [E,A,20+3F] out: agents.observation.state_self rows (:846-854); [E,A,24+6F] with two evaders */
    float *state_drones;      /* [E,A,20+3F] out, nullable: agents.state.state_drones (:873-880); [E,A,24+6F] with two evaders */
    float *groundtruth;       /* [U,3]    out: agents.TP.TP_groundtruth (:839-842) */
    uint8_t *tp_done;         /* [U]      out: agents.TP.TP_done (:838) */
} hns_tp_buffers;
size_t hns_tp_packed_bytes(void);
/* history_step T in [1,16], future_step F in [1,10]; max_episode_length <= 60000 (fp16-split operands). */
int hns_tp_bind(hns_env *env, const hns_tp_buffers *buffers, int32_t history_step, int32_t future_step);
/* Re-read the parameters (after an optimiser step / load_state_dict): one small launch on `stream`. */
int hns_tp_refresh(hns_env *env, void *stream);
/* Run after hns_step / hns_reset on the same stream: appends the frame of the bound step buffers to
 * the window (fill_history != 0: the window is filled with this frame, as the reference does on its
 * first call, hideandseek.py:825-828), evaluates TP_net, writes the 20+3F-value rows.  One launch; the kernel's workgroups serve 128, 64 or 32 units
 * depending on the batch size (small batches: more, shorter workgroups — the results do not depend on it; HNS_TP_TILES=1|2|4 forces one, A/B measurements). */
int hns_tp_observe(hns_env *env, int32_t fill_history, void *stream);

/*
 * Adaptive Environment Generator, device side (reference GenBuffer,
 * omni_drones/envs/hide_and_seek/hideandseek_envgen.py:209-377).
 */
/* Farthest-point sampling (replaces dgl.geometry.farthest_point_sampler, :291-304): out_idx[0] = start,
 * out_idx[r] = arg-max over all points of the minimum squared distance to out_idx[0..r-1] (ties -> lower
 * index).  points [n,d] fp32, out_idx [k] int32, scratch [hns_fps_scratch_bytes()] — device pointers.
 * One persistent launch (<= one workgroup per CU).  The XCD-local kernel (up to 36 coordinates, 131 072 points) accepts up to eight samples per
 * exchange — exactly those sequential sampling would select next, so out_idx does not depend on it.  If a workgroup never shows up the kernel gives up
 * instead of hanging: the first 8 bytes of scratch are then non-zero (check after synchronising). */
size_t hns_fps_scratch_bytes(void);
int hns_fps(const float *points, int32_t n, int32_t d, int32_t k, int32_t start, int32_t *out_idx, void *scratch, void *stream);
/* samplenearby (:316-370) with the grid sanity check (:187-207): tasks_out[t] = a random history entry,
 * pursuers / evader jittered by U(-1,1)*expand_step per coordinate (cylinders by {-1,0,1} cells when
 * expand_cylinders), clipped to the task bounds (:320-333); up to 10 attempts, then the entry itself.
 * history [n_hist, 3(A+1+C)], tasks_out [n_tasks, 3(A+1+C)] (3(A+2+C) with two evaders, both jittered like
 * pursuers): device pointers; Philox stream (seed, task). */
int hns_perturb_tasks(hns_env *env, const float *history, int32_t n_hist, float *tasks_out, int32_t n_tasks,
                      int32_t expand_cylinders, float expand_step, uint64_t seed, void *stream);

/* Curriculum hook (hideandseek.py:1012-1015): change the evader speed. */
int hns_set_v_prey(hns_env *env, float v_prey);
/* Smoothness schedule hook (hideandseek.py:988-991). */
int hns_set_smoothness_coef(hns_env *env, float coef);
/* Reset epoch (for checkpoint/resume and tests). */
int hns_set_reset_epoch(hns_env *env, uint32_t epoch);
uint32_t hns_get_reset_epoch(const hns_env *env);

/* Fixture injection / read-back for parity tests and checkpoints (the reference's counterpart is the
 * PhysX tensor view API, omni_drones/views/rigid_prim_view.py:61-118): `host` holds HOST pointers with the
 * shapes of hns_buffers; null fields are skipped; copies are asynchronous on `stream` (synchronise before
 * reading what hns_get_state wrote).  Equivalent to the caller copying into / out of its own bound buffers.
 * `host->stats` is always this handle's dense [HNS_NUM_STATS, num_envs]; for a handle over a slice of a larger batch
 * (cfg.stats_stride > num_envs) its columns of every device row are copied (one pitched copy). */
int hns_set_state(hns_env *env, const hns_buffers *host, void *stream);
int hns_get_state(hns_env *env, const hns_buffers *host, void *stream);
/* Recomputes the derived part of the state (the line-of-sight column of pid_last_rate, see hns_buffers) from drone_state, target_pos and
 * cylinders as the bound buffers hold them.  For callers that write positions into those buffers themselves instead of going through
 * hns_reset / hns_set_state (a checkpoint restored with tensor copies); hns_set_state runs it on what it uploads. */
int hns_refresh_derived_state(hns_env *env, void *stream);

/* Kernel timing: hns_enable_timing(env, n) times every n-th hns_step launch with a start / stop hipEvent pair bound
 * to that dispatch (hipExtLaunchKernelGGL: the timestamps of the kernel itself, on the launch stream; n = 0
 * disables; not for use inside a stream capture).  hns_step_kernel_ms returns the average device time (ms)
 * of the sampled launches since the last call (synchronises on the last sample); <0 if none. */
int hns_enable_timing(hns_env *env, int every_n);
float hns_step_kernel_ms(hns_env *env, int *num_launches);
/* Region timing (bench.py's roofline): ONE start event recorded on `stream` by hns_region_begin, one stop event by hns_region_end — no
 * per-launch host cost in between; hns_region_ms waits for the stop event and returns the device time between the two (ms; <0 without a
 * complete pair).  Divided by the launches in between it is the step kernel's duration INCLUDING the gap to its successor. */
int hns_region_begin(hns_env *env, void *stream);
int hns_region_end(hns_env *env, void *stream);
float hns_region_ms(hns_env *env);
/* Measurement yardstick (SURVEY §8d "achievable with a device copy kernel"): dst[i] = src[i] over `bytes` (a multiple of 16, both 16-byte
 * aligned device pointers) as 16-byte loads / stores, one float4 per thread.  Not part of the environment. */
int hns_copy_f4(void *dst, const void *src, size_t bytes, void *stream);

/* Measurement: the shader clock the chip is running at.  One wave spins for `ticks` periods of the constant 100 MHz clock and writes out[0] = shader-clock
 * cycles elapsed, out[1] = 100 MHz ticks elapsed (device pointer, 2 x uint64): MHz = 100 * out[0] / out[1].  MI355X clocks to its power budget; bench.py
 * reports this before and after its timed region.  Not part of the environment. */
int hns_clock_probe(unsigned long long *out, uint32_t ticks, void *stream);

/* Diagnostics: attach a device buffer of [num_waves, 16] uint64 (num_waves = ceil(E/64)*(A+1); ceil(E/64)*(2A+1) when hns_step_mapping() is 1);
 * lane 0 of every wave of the step kernel then stamps the shader clock at up to 16 phase boundaries (NULL detaches). */
int hns_set_phase_profile(hns_env *env, unsigned long long *device_buf);

/* Which mapping of the step kernel serves this env: 0 = 64-env tiles of A + 1 waves (batches that fill the chip), 1 = the small-batch mapping
 * (2 A + 1 waves per tile: a helper wave per pursuer wave; one evader, E % 64 == 0, obs_max_cylinder <= 4, at most two tiles per compute
 * unit — one with four and more pursuers).  Same buffers, bit for bit, either way; chosen by hns_create (the environment variable HNS_STEP_MAPPING=tile|small overrides it
 * where the shape allows both — A/B measurements and tests; HNS_STEP_PRIO=0|1 likewise overrides whether the tile mapping's pursuer waves
 * start at a raised issue priority, which hns_create decides from the shape and has no effect on any result). */
int hns_step_mapping(const hns_env *env);

/* Diagnostics: the kernel instantiations hns_create chose for this env, by name, in the form tools/kernel_resources.py prints them (argument
 * list, return type and "hns::" stripped, e.g. "hns_step_v4_kernel<3, 1, false, 4, false, 8, false>"): `step` the step kernel, `step_prof` its
 * phase-stamped twin (empty when the env has none), `reset` the reset kernel — each a host buffer of `cap` bytes; *prio_boost (may be NULL) =
 * whether the tile mapping's pursuer waves start at a raised priority.  Returns 1 when the stamped twin serves the next step (a phase-profile
 * buffer is attached and a twin exists), 0 when the plain step kernel does; HNS_ERR_INVALID_ARG when a name does not fit or a kernel handle is
 * not an exported symbol of this library. */
int hns_selected_kernels(const hns_env *env, char *step, char *step_prof, char *reset, int cap, int32_t *prio_boost);

/* The per-rollout moments of the data-parallel advantage normalisation (learning/mappo.py:391-396 made data-parallel; sharding.py) in ONE launch:
 * out[0..4] = [sum v, sum v^2, n, sum s, m] in fp64 over `values` [n] fp32 and `success` [m] fp32 (m may be 0: success NULL) — device
 * pointers; one workgroup, fixed summation order (the same inputs give the same bits on every run). */
int hns_moments(const float *values, int64_t n, const float *success, int64_t m, double *out, void *stream);
/* The same launch with ValueNorm1's batch moments riding along (learning/utils/valuenorm.py:83-91: `input_vector.mean()`, `(input_vector**2).mean()` over the
 * rollout's returns, mappo.py:398-399) — SURVEY §8(e)(3): out[0..7] = [sum adv, sum adv^2, n, sum success, m, sum ret, sum ret^2, n_returns]. */
int hns_rollout_moments(const float *advantages, int64_t n, const float *success, int64_t m, const float *returns, int64_t n_returns, double *out, void *stream);

/* The rollout boundary (learning/utils/gae.py:27-75 driven by learning/mappo.py:370-402), two launches in one stream:
 * hns_gae: GAE over reward / value fp32 [n, t, k] (HNS_GAE_BATCH_MAJOR: compute_gae) or [t, n, k] (HNS_GAE_TIME_MAJOR: compute_gae_), done [.., kd] in the
 * same layout with kd = 1 (broadcast over k) or k, as bytes (bool / uint8: HNS_GAE_DONE_U8) or fp32; next_value [n, k].  scale / shift: both NULL, or two
 * device fp32 scalars every value read (next_value included) is first mapped through, v * scale + shift (ValueNorm1.denormalize: sqrt(var), mean).
 * Writes advantages and returns (= advantages + value) in reward's layout, bit for bit the reference's fp32 statements.  With `moments` (device, 8 fp64)
 * it also writes the rank's row of the moment table (sharding.MOMENT_DIM): [sum adv, sum adv^2, n t k, sum success, m, sum ret, sum ret^2, n t k]
 * (success [m] fp32, m may be 0), deterministically, through `workspace` (device, HNS_GAE_WORKSPACE_DOUBLES fp64) and a second one-workgroup launch.
 * No host synchronisation and no allocation: legal inside a stream capture. */
#define HNS_GAE_BATCH_MAJOR 0
#define HNS_GAE_TIME_MAJOR 1
#define HNS_GAE_DONE_U8 0
#define HNS_GAE_DONE_F32 1
#define HNS_GAE_WORKSPACE_DOUBLES 20480
int hns_gae(const float *reward, const float *value, const void *done, const float *next_value, int64_t n, int64_t t, int64_t k, int64_t kd,
            int32_t layout, int32_t done_dtype, double gamma, double lambda, const float *scale, const float *shift, const float *success, int64_t m,
            float *advantages, float *returns, double *moments, double *workspace, void *stream);
/* In place, ONE launch: advantages[i] = (advantages[i] - *adv_mean) / *adv_den, returns[i] = (returns[i] - *ret_mean) / *ret_scale (device fp32
 * scalars: mean.to(f32) and std.to(f32) + eps from the gathered table; ValueNorm1's mean and sqrt(var) after its update).  Either group (array, n,
 * two scalars) may be left out with NULL scalars. */
int hns_rollout_normalise(float *advantages, int64_t n_adv, const float *adv_mean, const float *adv_den, float *returns, int64_t n_ret,
                          const float *ret_mean, const float *ret_scale, void *stream);

/*
 * The trajectory predictor's training step (learning/mappo.py:252-268 driven by :405-441): loss and gradients of one minibatch
 * and torch.optim.Adam's update, on the device, in PyTorch layouts.  No host synchronisation and no allocation: legal inside a stream capture.
 */
typedef struct hns_tp_params {             /* TP_net's parameters (hns_tp_buffers' first six fields) */
    const float *w_ih, *w_hh, *b_ih, *b_hh, *w_fc, *b_fc;
} hns_tp_params;
typedef struct hns_tp_grads {              /* their gradients, same shapes; b_ih and b_hh receive the same values */
    float *w_ih, *w_hh, *b_ih, *b_hh, *w_fc, *b_fc;
} hns_tp_grads;
/* Bytes of device workspace hns_tp_train_grad needs: a partial-gradient row per workgroup (at most 256 of them), independent of T and of B
 * beyond 4 096 sequences; 0 for an invalid shape. */
size_t hns_tp_train_workspace_bytes(int64_t batch, int32_t input_dim, int32_t future_step);
/* loss = mean((tanh(W_fc h_T + b_fc) - y)^2) over [batch, 3F] (nn.MSELoss) for an LSTM(input_dim -> 64) from a zero state, and its gradients.
 * x: [num_envs, num_steps, T, I] fp32 with element (e, s, t, i) at e stride_env + s stride_step + t I + i (each [T, I] block contiguous);
 * y: [num_envs num_steps, 3F] fp32; index: [batch] int64 rows of the flattened [num_envs num_steps] (NULL: rows 0 .. batch - 1; an index
 * outside the rows contributes nothing — callers check the range).  loss: one device fp32.  T in [1, 16], I in [1, 80], F in [1, 10],
 * batch >= 1.  Two launches; deterministic (per-workgroup partials, fixed-order sums). */
int hns_tp_train_grad(const hns_tp_params *params, const float *x, int64_t num_envs, int64_t num_steps, int64_t stride_env, int64_t stride_step,
                      int32_t history_step, int32_t input_dim, const float *y, const int64_t *index, int64_t batch, int32_t future_step,
                      const hns_tp_grads *grads, float *loss, void *workspace, size_t workspace_bytes, void *stream);
typedef struct hns_tp_adam_tensor {
    float *param;
    const float *grad;
    float *exp_avg, *exp_avg_sq;
    int64_t numel;
} hns_tp_adam_tensor;
/* torch.optim.Adam (amsgrad off, weight decay 0) over 1 to 8 tensors: hns_adam_clipped (below) without a norm, so one Adam launch and the bump
 * of the counter, in one stream.  `step`: the device-resident fp32 step counter (torch's state['step']), read and bumped on the device. */
int hns_tp_adam(const hns_tp_adam_tensor *tensors, int32_t count, float *step, double lr, double beta1, double beta2, double eps, void *stream);

/*
 * The MAPPO policy's forward pass (learning/mappo.py:221-250 with cfg/algo/mappo.yaml's defaults: shared actor, critic on the observation, no rnn,
 * no tanh): per (env, agent) row the actor's PartialAttentionEncoder + DiagGaussian (loc, a sample or the mode, its log_prob) and
 * the critic's encoder + v_out.  embed_dim 128, one head, dim_feedforward 128.  No host synchronisation and no allocation: legal inside a stream
 * capture.
 */
#define HNS_POLICY_MAX_SELF_DIM 96
#define HNS_POLICY_DETERMINISTIC 1         /* action = loc (the distribution's mode) */
#define HNS_POLICY_VALUE_ONLY 2            /* the critic alone: value (train_op's next_value) */
typedef struct hns_policy_net {            /* one network's parameters, fp32 in PyTorch layouts (device) */
    const float *embed_self_w, *embed_self_b;         /* [128, D], [128] */
    const float *embed_others_w, *embed_others_b;     /* [128, 3], [128]; NULL with one pursuer (no state_others key) */
    const float *embed_cyl_w, *embed_cyl_b;           /* [128, 5], [128] */
    const float *ln_w, *ln_b;                         /* SplitEmbedding's LayerNorm(128) */
    const float *in_proj_w, *in_proj_b;               /* [384, 128], [384]: q, k, v */
    const float *out_proj_w, *out_proj_b;             /* [128, 128], [128] */
    const float *linear1_w, *linear1_b, *linear2_w, *linear2_b;   /* [128, 128], [128] each */
    const float *norm1_w, *norm1_b, *norm2_w, *norm2_b;
    const float *head_w, *head_b;                     /* actor fc_mean [4, 128], [4]; critic v_out [1, 128], [1] */
    const float *log_std;                             /* actor [4]; ignored for the critic */
} hns_policy_net;
typedef struct hns_policy_io {
    const float *obs_self;                 /* [E, A, D]: element (e, a, i) at e s[0] + a s[1] + i */
    const float *obs_others;               /* [E, A, A - 1, 3]: (e, a, j, i) at e s[0] + a s[1] + j s[2] + i; NULL when A = 1 */
    const float *obs_cylinders;            /* [E, A, K, 5] likewise */
    int64_t self_stride[2], others_stride[3], cyl_stride[3];
    const float *eps;                      /* [E, A, 4] contiguous standard-normal noise, or NULL: Philox4x32-10 + Box-Muller in the kernel */
    float *action;                         /* [E, A, 4] contiguous */
    float *loc;                            /* [E, A, 4] contiguous, or NULL */
    float *log_prob;                       /* [E, A] (Normal.log_prob summed over the 4 dims) */
    float *value;                          /* [E, A] (the critic's normalised value) */
} hns_policy_io;
/* Bytes of the packed image of both networks (actor, then critic) for self_dim D in [1, 96]; 0 otherwise. */
size_t hns_policy_packed_bytes(int32_t self_dim);
/* Builds the packed image on the device from the parameter tensors (ONE launch): call it again after the parameters change. */
int hns_policy_pack(const hns_policy_net *actor, const hns_policy_net *critic, int32_t self_dim, int32_t num_agents, void *packed, void *stream);
/* The forward pass of num_envs x num_agents rows (num_agents in [1, 7], num_cylinders in [1, 16]).  flags: HNS_POLICY_DETERMINISTIC,
 * HNS_POLICY_VALUE_ONLY (action / log_prob / loc untouched).  When the call samples without io->eps, the noise of row r is Philox4x32-10 with
 * key `seed` and counter (*counter, r), and a second launch bumps the device uint64 *counter, so every call (and every replay of a captured
 * graph) draws fresh noise.  Deterministic: the same inputs give the same bits. */
int hns_policy_forward(const void *packed, int32_t self_dim, int64_t num_envs, int32_t num_agents, int32_t num_cylinders, const hns_policy_io *io,
                       int32_t flags, uint64_t seed, uint64_t *counter, void *stream);
/* The actor alone, the mode of the distribution (evaluation): ONE encoder pass over the actor image (the first half of
 * `packed`), io->action[row * 4 + o] = loc[o] for every row and nothing else.  The critic image, io->eps and the Philox call counter are never
 * read, io->log_prob / io->value / io->loc are ignored (NULL is fine; non-NULL is left untouched).  `action` is bit for bit what
 * hns_policy_forward with HNS_POLICY_DETERMINISTIC writes there.  Refused before any launch, as the forward refuses them: a NULL or misaligned
 * packed image / io, a shape out of range, a missing or misaligned observation, a negative stride, a missing or misaligned action. */
int hns_policy_act(const void *packed, int32_t self_dim, int64_t num_envs, int32_t num_agents, int32_t num_cylinders, const hns_policy_io *io,
                   void *stream);
/*
 * One actor per agent (cfg/algo/mappo.yaml's share_actor: false, mappo.py:148-152, :243-246): the reference stacks the actors'
 * parameters over the agents and vmaps the actor over the agent axis; the critic stays shared.  `actors`: a hns_policy_net whose every tensor is
 * the stacked one, [A, ...] in its PyTorch layout and contiguous, so agent a's slice is a hns_policy_net of its own.  The entries above keep
 * serving the shared actor alone and are unchanged.
 *
 * hns_policy_packed_agents_bytes: bytes of the image of num_agents actors followed by ONE critic, each hns_policy_pack's image of one network
 * (hns_policy_packed_bytes / 2 bytes); 0 for self_dim outside [1, 96] or num_agents outside [1, 7].
 * hns_policy_pack_agents: ONE launch builds that image (16-byte aligned); call it again after the parameters change.  num_agents is the number
 * of actors (and, as for hns_policy_pack, > 1 says the networks have the state_others embedding).  Refused before the launch, as
 * hns_policy_pack refuses: self_dim or num_agents out of range, a NULL or misaligned image, a NULL or misaligned parameter pointer, a missing
 * state_others embedding with num_agents > 1, actors without log_std.
 * hns_policy_forward_agents: hns_policy_forward's arguments, flags, outputs, output layouts ([E, A, ...]), noise scheme and refusals (all
 * before any launch, in its order) on that image, and its launch count: ONE launch, and the bump of the counter when the call samples without
 * io->eps.  A workgroup's 32 rows are 32 consecutive envs of ONE agent: the actor pass reads that agent's image, the critic pass the shared
 * one.  Row (e, a) keeps its number e A + a — outputs, eps and the Philox counter (*counter, e A + a) — and its arithmetic, which does not
 * depend on the rows it shares a tile with: for every agent a, row (e, a) is bit for bit what hns_policy_forward writes for that row on
 * hns_policy_pack's image of (agent a's slice, critic).  Deterministic: fixed-order sums, no atomics.
 * hns_policy_act_agents: hns_policy_act on that image in the same tiles (ONE launch, the actor pass alone; its refusals, before the launch):
 * bit for bit hns_policy_forward_agents' action with HNS_POLICY_DETERMINISTIC.
 */
size_t hns_policy_packed_agents_bytes(int32_t self_dim, int32_t num_agents);
int hns_policy_pack_agents(const hns_policy_net *actors, const hns_policy_net *critic, int32_t self_dim, int32_t num_agents, void *packed, void *stream);
int hns_policy_forward_agents(const void *packed, int32_t self_dim, int64_t num_envs, int32_t num_agents, int32_t num_cylinders, const hns_policy_io *io,
                              int32_t flags, uint64_t seed, uint64_t *counter, void *stream);
int hns_policy_act_agents(const void *packed, int32_t self_dim, int64_t num_envs, int32_t num_agents, int32_t num_cylinders, const hns_policy_io *io,
                          void *stream);
/*
 * The centralised critic (cfg/algo/mappo.yaml's critic_input: state; make_critic(centralized=True), mappo.py:165-181, :553-566, :644-660;
 * hns_amd.policy.CentralCriticDevicePolicy) beside the shared actor.  The critic is ONE row per env: a PartialAttentionEncoder
 * over the state spec — the A rows of state_drones through ONE Linear(D, 128), then the K cylinder rows through Linear(5, 128); token 0 (drone
 * 0) is the query — and v_out = Linear(128, A): value[e, a] = v_out.weight[a] . feat[e] + v_out.bias[a].  The entries above are unchanged.
 *
 * hns_policy_packed_central_bytes: bytes of the image [the shared actor's, the centralised critic's]; 0 for self_dim outside [1, 96] or
 * num_agents outside [1, 7].
 * hns_policy_pack_central: ONE launch builds that image (16-byte aligned); call it again after the parameters change.  Its first
 * hns_policy_packed_bytes / 2 bytes are byte for byte the actor half of hns_policy_pack's image, so hns_policy_act serves this image
 * unchanged.  `critic`: embed_self_w / embed_self_b are the state_drones embedding, embed_others_* must be NULL (the state has no such key),
 * head_w is [A, 128] and head_b [A] with A = num_agents.  Refused before the launch: what hns_policy_pack refuses, and a critic with a
 * state_others embedding.
 * hns_policy_central_forward: hns_policy_forward's arguments, flags, outputs, output layouts, noise scheme and launch count (ONE launch, and
 * the bump of the counter when the call samples without io->eps) with `state`, what the critic reads.  The grid is ceil(E A / 32) actor
 * workgroups — tiles of 32 (env, agent) rows as hns_policy_forward's, whose action, log_prob and loc of every row are bit for bit
 * hns_policy_forward's for the same actor, eps or (seed, *counter, row) — followed by ceil(E / 32) critic workgroups, tiles of 32 envs, which
 * write io->value[e A + a] for a < A.  With one agent and `state` = the observation's rows, value is bit for bit hns_policy_forward's for the
 * same 20 tensors.  HNS_POLICY_VALUE_ONLY launches the critic workgroups alone: the observation pointers are not read (NULL is fine) and
 * action / log_prob / loc are untouched.  Refused before any launch, in hns_policy_forward's order: a NULL or misaligned packed image / io, a
 * shape out of range, an unknown flag, (unless value-only) a missing or misaligned observation or a negative stride, a NULL state or a NULL or
 * misaligned pointer or a negative stride in it, then the outputs as hns_policy_forward.  Deterministic: fixed-order sums, no atomics.
 * (Named hns_policy_central_*, not hns_policy_forward_*: the eight hns_policy_forward* / hns_policy_act* entries are the four policy classes'
 * table, keyed (agents, rnn, act), and this one takes a further argument.)
 */
typedef struct hns_policy_state {
    const float *state_drones;             /* [E, A, D]: element (e, a, i) at e s[0] + a s[1] + i */
    const float *cylinders;                /* [E, K, 5]: (e, k, i) at e s[0] + k s[1] + i.  s[0] = A K 5 reads agent 0's rows of a contiguous
                                            * obs_cylinders [E, A, K, 5] in place */
    int64_t drones_stride[2], cyl_stride[2];
} hns_policy_state;
size_t hns_policy_packed_central_bytes(int32_t self_dim, int32_t num_agents);
int hns_policy_pack_central(const hns_policy_net *actor, const hns_policy_net *critic, int32_t self_dim, int32_t num_agents, void *packed, void *stream);
int hns_policy_central_forward(const void *packed, int32_t self_dim, int64_t num_envs, int32_t num_agents, int32_t num_cylinders,
                               const hns_policy_io *io, const hns_policy_state *state, int32_t flags, uint64_t seed, uint64_t *counter, void *stream);
/*
 * One actor per agent beside the centralised critic (share_actor: false WITH critic_input: state — heterogeneous actors under one critic over
 * the joint state; hns_amd.policy.PerAgentCentralCriticDevicePolicy).  The entries above are unchanged.
 *
 * hns_policy_packed_central_agents_bytes: bytes of the image [num_agents actors, the centralised critic]: num_agents times
 * hns_policy_packed_bytes / 2, then the central critic's image as it lies behind hns_policy_pack_central's actor; 0 for self_dim outside
 * [1, 96] or num_agents outside [1, 7].
 * hns_policy_pack_central_agents: ONE launch builds that image (16-byte aligned); call it again after the parameters change.  `actors` is the
 * stacked actor as hns_policy_pack_agents takes it (every tensor [A, ...], contiguous; the agents' slices are formed on the host the same
 * way), `critic` the centralised critic as hns_policy_pack_central takes it (embed_others_* NULL, head_w [A, 128], head_b [A]).  The first
 * num_agents actor images are byte for byte the first num_agents images hns_policy_pack_agents writes, so hns_policy_act_agents serves this
 * image unchanged; the central image behind them is byte for byte the one hns_policy_pack_central writes behind its actor.  Refused before
 * the launch, in this order: self_dim or num_agents out of range, a NULL or misaligned image, what hns_policy_pack_agents refuses of
 * `actors` (a NULL or misaligned parameter pointer, a missing state_others embedding with num_agents > 1, no log_std), what
 * hns_policy_pack_central refuses of `critic` (a NULL or misaligned parameter pointer, then a state_others embedding).
 * hns_policy_central_forward_agents: hns_policy_central_forward's arguments, flags, outputs, output layouts, noise scheme, launch count (ONE
 * launch, and the bump of the counter when the call samples without io->eps) and refusals (all before any launch, in its order) on that
 * image.  The grid is ceil(E / 32) tiles of 32 envs times A + 1 ranges: range a < A is agent a's — the actor pass of
 * hns_policy_forward_agents on agent a's image, row (e, a) keeping its number e A + a — and range A the critic's, the critic workgroups of
 * hns_policy_central_forward.  For every row (e, a), action, log_prob and loc are bit for bit hns_policy_forward_agents' for the same stacked
 * actor, eps or (seed, *counter, row); value is bit for bit hns_policy_central_forward's for the same critic and state.
 * HNS_POLICY_VALUE_ONLY launches the critic's range alone: the observation pointers are not read (NULL is fine) and action / log_prob / loc
 * are untouched.  Deterministic: fixed-order sums, no atomics.
 */
size_t hns_policy_packed_central_agents_bytes(int32_t self_dim, int32_t num_agents);
int hns_policy_pack_central_agents(const hns_policy_net *actors, const hns_policy_net *critic, int32_t self_dim, int32_t num_agents, void *packed,
                                   void *stream);
int hns_policy_central_forward_agents(const void *packed, int32_t self_dim, int64_t num_envs, int32_t num_agents, int32_t num_cylinders,
                                      const hns_policy_io *io, const hns_policy_state *state, int32_t flags, uint64_t seed, uint64_t *counter,
                                      void *stream);

/*
 * The MAPPO critic's update (learning/mappo.py:326-352 on make_critic's network at the defaults: critic_input obs, no rnn): value
 * loss, explained variance and every parameter's gradient of one minibatch, then clip_grad_norm_ and torch.optim.Adam's update, on the device, in
 * PyTorch layouts.  No host synchronisation and no allocation: legal inside a stream capture.  Deterministic: fixed-order sums, no float atomics.
 */
#define HNS_CRITIC_LOSS_HUBER 0            /* nn.HuberLoss(delta = huber_delta) */
#define HNS_CRITIC_LOSS_MSE 1              /* nn.MSELoss() */
typedef struct hns_policy_grads {          /* one network's gradients: hns_policy_net's fields and shapes, writable (log_std: the actor's; unused by the critic) */
    float *embed_self_w, *embed_self_b, *embed_others_w, *embed_others_b, *embed_cyl_w, *embed_cyl_b, *ln_w, *ln_b, *in_proj_w, *in_proj_b;
    float *out_proj_w, *out_proj_b, *linear1_w, *linear1_b, *linear2_w, *linear2_b, *norm1_w, *norm1_b, *norm2_w, *norm2_b, *head_w, *head_b, *log_std;
} hns_policy_grads;
typedef struct hns_critic_batch {          /* a minibatch of make_dataset_naive (seq_len 1) read in place from the rollout */
    const float *obs_self;                 /* [N, T, A, D]: element (n, t, a, i) at n s[0] + t s[1] + a s[2] + i */
    const float *obs_others;               /* [N, T, A, A - 1, 3]: (n, t, a, j, i) at n s[0] + t s[1] + a s[2] + j s[3] + i; NULL when A = 1 */
    const float *obs_cylinders;            /* [N, T, A, K, 5] likewise */
    int64_t self_stride[3], others_stride[4], cyl_stride[4];
    int64_t num_envs, num_steps;           /* N, T: env-step e of the flattened [N T] is (e / T, e % T) */
    const int64_t *index;                  /* [batch] env-steps, or NULL: env-steps 0 .. batch - 1; an index outside [0, N T) contributes nothing */
    int64_t batch;                         /* env-steps in the minibatch; each contributes its A agent rows */
    const float *b_values, *b_returns;     /* [N T, A] contiguous */
} hns_critic_batch;
/* Bytes of device workspace for a minibatch of `rows` = batch x num_agents rows; 0 for an invalid shape.  Per row: the staged operand pairs of
 * the six weight gradients, 12 x 512 bytes, and the row's share of its 32-row tile's two partial rows of LayerNorm / head / embedding
 * gradients, (2 308 + 128 self_dim) x 4 / 16 bytes (1.7 KB at self_dim 35, 3.6 KB at 96); beside them the packed operand image (0.8 MB) and
 * at most 48 x 6 weight-gradient partials (19 MB).  213 MB at 24 576 rows and self_dim 35 (151 + 42 + 20), 6.2 GB at 786 432 rows. */
size_t hns_critic_train_workspace_bytes(int64_t rows, int32_t self_dim, int32_t num_agents, int32_t num_cylinders);
/* values = critic(obs); value_loss = max(mean loss(b_returns, values), mean loss(b_returns, b_values + clamp(values - b_values, +-clip_param)))
 * — the max of two means: one branch for the whole minibatch, both by halves at an exact tie, as torch's backward; explained_var =
 * 1 - mse(values, b_returns) / var(b_returns) (unbiased); grads: d value_loss / d parameter for each of the critic's 22 tensors (`critic`: live
 * fp32 tensors in PyTorch layouts, 16-byte aligned; in_proj_b's k third receives zeros: the softmax cancels it); grad_norm: their total 2-norm.
 * value_loss, explained_var, grad_norm: one device fp32 each; values: [batch, A] or NULL; workspace: 256-byte aligned.  self_dim in [1, 96],
 * num_agents in [1, 7], num_cylinders in [1, 16], batch >= 1.  Seven launches in one stream. */
int hns_critic_train_grad(const hns_policy_net *critic, const hns_critic_batch *batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders,
                          float clip_param, int32_t loss_kind, float huber_delta, const hns_policy_grads *grads, float *value_loss,
                          float *explained_var, float *grad_norm, float *values, void *workspace, size_t workspace_bytes, void *stream);
/* The centralised critic's update (critic_input: state; the network of hns_policy_central_forward; hns_amd.critic_train.update_critic_central;
 * DESIGN.md §7.20): hns_critic_train_grad's arguments, outputs, scalars, launches (seven) and refusals on hns_critic_batch REINTERPRETED:
 * obs_self is state_drones [N, T, A, D] — token j of an env-step's row at j self_stride[2] —, obs_others must be NULL (as the critic's
 * embed_others_*: refused after the hyper-parameters), obs_cylinders is read at agent index 0 (cyl_stride[2] is ignored; cyl_stride[3] steps
 * the K rows), b_values / b_returns / values stay [.., A].  A tile is 32 env-steps; a row's A values come from head_w [A, 128] and head_b [A] on
 * its one feature vector; the means are over the batch x A values.  d head_w / d head_b come from the row's A value gradients, d embed_self_*
 * sum over all A drone tokens (the query's through its key / value path and its residual path), there are no state_others gradients.  With
 * one agent every output is bit for bit hns_critic_train_grad's on the same tensors.  hns_critic_train_central_workspace_bytes takes `batch`
 * (env-steps, not batch x num_agents). */
size_t hns_critic_train_central_workspace_bytes(int64_t batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders);
int hns_critic_train_grad_central(const hns_policy_net *critic, const hns_critic_batch *batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders,
                                  float clip_param, int32_t loss_kind, float huber_delta, const hns_policy_grads *grads, float *value_loss,
                                  float *explained_var, float *grad_norm, float *values, void *workspace, size_t workspace_bytes, void *stream);
typedef struct hns_adam_tensor {
    float *param, *grad, *exp_avg, *exp_avg_sq;
    int64_t numel;
} hns_adam_tensor;
/* clip_grad_norm_ and torch.optim.Adam over ANY number of tensors with ONE bump of the device step counter: every gradient is multiplied by
 * min(max_norm / (*total_norm + 1e-6), 1) in place (torch's statements: the reciprocal, times max_norm, clamped), then Adam (amsgrad off, weight
 * decay 0) in the single-tensor statement order of torch's CPU kernels with step = *step + 1: m = fma(1 - b1, g - m, m); v = fma((1 - b2) g, g, v b2);
 * denom = sqrt(v) / f32(sqrt(1 - b2^step)) + f32(eps); p = p + (f32(-lr / (1 - b1^step)) m) / denom.  *step is bumped after the last tensor (one
 * launch per 64 tensors, then the bump).  total_norm NULL or max_norm = +inf: no clipping.  A data-parallel caller all-reduces the gradient
 * buckets that the *_train_grad_global entries (below) filled and hands this call hns_grad_norm's device scalar over the summed bucket. */
int hns_adam_clipped(const hns_adam_tensor *tensors, int32_t count, float *step, const float *total_norm, double max_norm, double lr, double beta1,
                     double beta2, double eps, void *stream);

/*
 * The MAPPO actor's update (learning/mappo.py:271-324 on make_ppo_actor's network at the defaults: share_actor, no tanh, no rnn, DiagGaussian over
 * a 4-dim action): the clipped PPO surrogate, the entropy bonus and every parameter's gradient of one minibatch; the step itself is
 * hns_adam_clipped over the 23 tensors.  Same properties as the critic's call: one stream, no host synchronisation, no allocation, capturable,
 * fixed-order sums and no float atomics.
 */
typedef struct hns_actor_batch {           /* hns_critic_batch's observation / index part, then the actor's per-row data */
    const float *obs_self, *obs_others, *obs_cylinders;
    int64_t self_stride[3], others_stride[4], cyl_stride[4];
    int64_t num_envs, num_steps;
    const int64_t *index;
    int64_t batch;
    const float *action;                   /* [N T, A, 4] contiguous: the stored actions */
    const float *log_probs_old;            /* [N T, A] contiguous */
    const float *advantages;               /* [N T, A] contiguous */
} hns_actor_batch;
/* Bytes of device workspace for a minibatch of `rows` = batch x num_agents rows; 0 for an invalid shape.  The critic's workspace with a tile's
 * partial rows 388 floats longer (three more head rows, log_std) and 22 fp64 loss partials per tile instead of 5. */
size_t hns_actor_train_workspace_bytes(int64_t rows, int32_t self_dim, int32_t num_agents, int32_t num_cylinders);
/* Per row: mu = fc_mean(encoder(obs)), logp = sum_i Normal(mu_i, exp(log_std_i)).log_prob(action_i), r = exp(logp - log_probs_old);
 * policy_loss = -mean(min(r adv, clamp(r, 1 - clip_param, 1 + clip_param) adv) 4); entropy: the mean of the distribution's entropy (the same for
 * every row); grads: d (policy_loss - entropy_coef entropy) / d parameter for each of the actor's 23 tensors (16-byte aligned live fp32 tensors in
 * PyTorch layouts; in_proj_b's k third receives zeros) — the backward weight of min and clamp is per row: 1 inside the clip (bounds included),
 * outside 1 where the unclipped surrogate is the smaller and 0 otherwise; ess = mean over agents of exp(2 logsumexp_batch(r) - logsumexp_batch(2 r))
 * / batch (of the ratio itself, as the reference writes it); grad_norm: the total 2-norm.  policy_loss, entropy, ess, grad_norm: one device fp32
 * each; log_probs: [batch, A] or NULL, receives logp.  Six launches in one stream: pack, ONE pass over the tiles (forward, loss partials,
 * backward), the scalars, weight gradients, reduce, norm. */
int hns_actor_train_grad(const hns_policy_net *actor, const hns_actor_batch *batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders,
                         double clip_param, double entropy_coef, const hns_policy_grads *grads, float *policy_loss, float *entropy, float *ess,
                         float *grad_norm, float *log_probs, void *workspace, size_t workspace_bytes, void *stream);
/* The actor's update with one actor per agent (share_actor: false: MAPPOPolicy.update_actor's else branch, mappo.py:288-291) on
 * one minibatch of `batch` env-steps x A agents.  `actors`, `grads`: the STACKED tensors ([A, ...] in PyTorch layouts, contiguous, 16-byte
 * aligned; every slice is then aligned too) and their gradients in the same layouts.  Agent a's rows run on agent a's slice.  The loss is the
 * reference's: policy_loss = -mean over all batch A rows of min(surr1, surr2) 4 (every row carries 1 / (batch A), as above); entropy: the mean
 * over the same rows, that is the mean over the agents of each agent's entropy, so each agent's d log_std takes -entropy_coef / A once; ess as
 * above (it is per agent over the batch already); grads: agent a's slice is the gradient of the whole loss with respect to agent a's parameters
 * (only its rows contribute; in_proj_b's k third receives zeros per agent); grad_norm: the total 2-norm over ALL agents' gradients
 * (clip_grad_norm_ over the stacked tensors).  The step is hns_adam_clipped over the 23 stacked tensors.  log_probs [batch, A] (or NULL) is bit
 * for bit what hns_actor_train_grad writes for row (b, a) with agent a's slice as the actor.
 * Six launches in one stream, the pipeline above for all agents together: pack (A images), ONE pass over the tiles, the scalars, weight
 * gradients, reduce (each agent's partials into its slice), ONE norm.  A tile is 32 minibatch positions of ONE agent and the tiles are numbered
 * agent-major, each agent's count padded to whole row ranges of the weight-gradient kernel (rows that are not live), so no range holds rows of
 * two agents.  Refused before any launch, as hns_actor_train_grad refuses and in its order: a NULL pointer, a shape out of range (self_dim in
 * [1, 96], num_agents in [1, 7], num_cylinders in [1, 16], batch >= 1), a negative or non-finite clip_param, a non-finite entropy_coef, a NULL or
 * misaligned parameter or gradient, a missing or misaligned observation, a negative stride, missing or misaligned action / log_probs_old /
 * advantages, a misaligned index, output or workspace, a workspace below hns_actor_train_agents_workspace_bytes(batch x num_agents, ...) (0 for
 * an invalid shape or rows that are no multiple of num_agents).  The workspace is the caller's: nothing is allocated, so it can be cached and
 * the call captured.  Deterministic: every sum has a fixed order, no float atomics. */
size_t hns_actor_train_agents_workspace_bytes(int64_t rows, int32_t self_dim, int32_t num_agents, int32_t num_cylinders);
int hns_actor_train_grad_agents(const hns_policy_net *actors, const hns_actor_batch *batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders,
                                double clip_param, double entropy_coef, const hns_policy_grads *grads, float *policy_loss, float *entropy, float *ess,
                                float *grad_norm, float *log_probs, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The data-parallel learner's entries (hns_amd.learner.DeviceLearner(group=)): W ranks, each holding a part of a minibatch,
 * perform ONE update on the union.  Per minibatch the critic runs hns_critic_train_sums, an all-reduce (SUM) of the five fp64 values,
 * hns_critic_train_grad_global, an all-reduce (SUM) of the gradient bucket, hns_grad_norm, hns_adam_clipped; the actor runs
 * hns_actor_train_grad_global, the bucket's all-reduce, hns_grad_norm, hns_adam_clipped.  The kernels, workspaces, refusals and properties (one
 * stream, no host synchronisation, no allocation, capturable, fixed-order sums) are those of hns_critic_train_grad / hns_actor_train_grad;
 * with one rank (global_rows = batch x num_agents, entropy_share 1) every output has the bits of those calls.
 *
 * hns_critic_train_sums: pack, forward, and the SUMMING half of the loss launch — values as hns_critic_train_grad writes them and
 * sums[0 .. 5) = sum loss(v - ret), sum loss(clipped - ret), sum (v - ret)^2, sum ret, sum ret^2 over this rank's rows, fp64, added in exactly
 * the order hns_critic_train_grad adds its tile partials.  sums: device, 8-byte aligned.  No gradients.  Three launches.
 */
int hns_critic_train_sums(const hns_policy_net *critic, const hns_critic_batch *batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders,
                          float clip_param, int32_t loss_kind, float huber_delta, double *sums, float *values, void *workspace, size_t workspace_bytes,
                          void *stream);
/* hns_critic_train_grad's arguments, then `sums` (the five values of ALL ranks' rows: the all-reduced output of hns_critic_train_sums) and
 * `global_rows` (their row count, >= batch x num_agents).  The DECIDING half of the loss launch forms value_loss, explained_var and the branch
 * weights of the max from `sums` with n = global_rows — one decision for the union, the same on every rank — and the backward pass scales each
 * row by f32(1 / global_rows), so the ranks' gradients ADD UP to the union's.  It packs the operand image again (the call stands alone: the
 * workspace need not be the one hns_critic_train_sums used) and does not run the forward launch: `values` is not written (it is
 * hns_critic_train_sums' output; the parameter keeps the two argument lists parallel).  grad_norm may be NULL: the norm of one rank's part
 * means nothing, and the launch is skipped.  Refused as hns_critic_train_grad refuses, plus NULL or misaligned sums, global_rows < rows. */
int hns_critic_train_grad_global(const hns_policy_net *critic, const hns_critic_batch *batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders,
                                 float clip_param, int32_t loss_kind, float huber_delta, const hns_policy_grads *grads, float *value_loss,
                                 float *explained_var, float *grad_norm, float *values, void *workspace, size_t workspace_bytes, void *stream,
                                 const double *sums, int64_t global_rows);
/* hns_actor_train_grad's arguments, then `global_rows` (all ranks' rows of the minibatch, >= batch x num_agents) and `entropy_share`.  Each row's
 * backward weight is scaled by f32(1 / global_rows); policy_loss = -4 sum_local min(..) / global_rows is this rank's SHARE (the shares add up to
 * the union's loss); the entropy term's constant gradient joins d log_std as -entropy_coef x entropy_share (1 / world, so a SUM over the ranks
 * counts it once); entropy is the same on every rank; ess stays this rank's own (a diagnostic).  grad_norm may be NULL (launch skipped).
 * Refused as hns_actor_train_grad refuses, plus global_rows < rows and a non-finite entropy_share. */
int hns_actor_train_grad_global(const hns_policy_net *actor, const hns_actor_batch *batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders,
                                double clip_param, double entropy_coef, const hns_policy_grads *grads, float *policy_loss, float *entropy, float *ess,
                                float *grad_norm, float *log_probs, void *workspace, size_t workspace_bytes, void *stream, int64_t global_rows,
                                double entropy_share);
/* hns_actor_train_grad_agents' arguments, then `global_rows` and `entropy_share`: one rank's part of a data-parallel update of one actor per
 * agent (hns_amd.learner.DataParallelPerAgentLearner).  It is to hns_actor_train_grad_agents what hns_actor_train_grad_global
 * is to hns_actor_train_grad, on that entry's launches, plan, tiles and workspace (hns_actor_train_agents_workspace_bytes): every row's backward
 * weight carries f32(1 / global_rows); policy_loss = -4 sum_local min(..) / global_rows is this rank's SHARE; each agent's d log_std takes
 * (-entropy_coef x entropy_share) / A, formed in that order, so a share of 1 leaves the local constant and a SUM over W ranks with share 1 / W
 * counts the entropy term once; entropy (the mean over the agents) is the same on every rank; ess stays this rank's own.  grad_norm may be NULL:
 * the norm launch is skipped (five launches).  Order of every sum: hns_actor_train_grad_agents' — the tiles agent-major and padded to whole row
 * ranges, the loss kernel's tile partials in its fixed order with n = global_rows, each agent's weight-gradient partials in split order, its
 * tile partials in tile order.  With one rank (global_rows = batch x num_agents, entropy_share 1) every output has hns_actor_train_grad_agents'
 * bits.  Refused as that entry refuses and in its order (grad_norm excepted), plus, after clip_param and entropy_coef, global_rows < batch x
 * num_agents and a non-finite entropy_share. */
int hns_actor_train_grad_agents_global(const hns_policy_net *actors, const hns_actor_batch *batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders,
                                       double clip_param, double entropy_coef, const hns_policy_grads *grads, float *policy_loss, float *entropy, float *ess,
                                       float *grad_norm, float *log_probs, void *workspace, size_t workspace_bytes, void *stream, int64_t global_rows,
                                       double entropy_share);
/*
 * The PartialAttentionEncoder alone as a differentiable op (hns_amd.encoder): the forward pass gives the 128 features of every
 * (env-step, agent) row of a minibatch, the backward pass takes d features and gives the gradients of the encoder's 20 parameter tensors, so any
 * head, loss, optimiser or schedule can be written on top of it (torch.autograd, or any other caller).  The kernels are the updates' tile kernel
 * without a head and without a loss; the backward pass recomputes its tile's forward pass, so nothing is kept between the two calls.  `net`:
 * hns_policy_net, whose head_w, head_b and log_std are ignored (NULL is fine); `batch`: hns_critic_batch, whose b_values and b_returns are ignored
 * (NULL is fine).  features / dfeatures: fp32 [batch x num_agents, 128] row-major, 16-byte aligned, row = minibatch position x num_agents + agent
 * (the row order of hns_critic_train_grad's `values`).  A row whose index lies outside [0, N T) contributes nothing: its feature row is not
 * written, its dfeatures row is not read.  Properties of both calls: one stream, no host synchronisation, no allocation, fixed-order sums, no
 * float atomics, the same inputs give the same bits.  Refused before any launch, in hns_critic_train_grad's order: shape, NULL or misaligned
 * parameters (and gradients), observation pointers, strides, a NULL or misaligned features / dfeatures, index, workspace.
 *
 * hns_encoder_workspace_bytes: bytes of device workspace for `rows` = batch x num_agents rows (backward != 0: hns_encoder_backward's); 0 for an
 * invalid shape.  Forward: the packed operand image alone (0.8 MB).  Backward: hns_critic_train_workspace_bytes without the branch weights and
 * the loss partials.
 * hns_encoder_forward: two launches (pack, tiles).
 * hns_encoder_backward: each of the 20 encoder tensors of `grads` is WRITTEN (not accumulated) in its PyTorch layout with the gradient of
 * sum(features x dfeatures): dfeatures is used as given, no 1 / n.  in_proj_b's k third receives zeros; the state_others embedding is written only
 * when num_agents > 1; the head fields of `grads` are ignored.  Four launches (pack, tiles, weight gradients, reduce); no gradient norm.
 */
size_t hns_encoder_workspace_bytes(int64_t rows, int32_t self_dim, int32_t num_agents, int32_t num_cylinders, int32_t backward);
int hns_encoder_forward(const hns_policy_net *net, const hns_critic_batch *batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders,
                        float *features, void *workspace, size_t workspace_bytes, void *stream);
int hns_encoder_backward(const hns_policy_net *net, const hns_critic_batch *batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders,
                         const float *dfeatures, const hns_policy_grads *grads, void *workspace, size_t workspace_bytes, void *stream);
/*
 * The encoder op on the STACKED tensors (the encoder of one recurrent actor per agent: share_actor: false with actor.rnn):
 * hns_encoder_forward / hns_encoder_backward with a hns_policy_net / hns_policy_grads whose every encoder tensor is stacked over the agents
 * ([A, ...], contiguous, as hns_actor_train_grad_agents takes them; the head fields are ignored): agent a's rows run on slice a, and agent a's
 * slice of every gradient is the sum over its own rows (in_proj_b's k third receives zeros per agent).  features / dfeatures keep the shared
 * op's layout, [batch x num_agents, 128] with row = position x num_agents + agent, so the GRU op reads and writes them in place; a row's
 * features are bit for bit hns_encoder_forward's with slice a.  The pack, the tiles (32 minibatch positions of ONE agent, numbered agent-major,
 * each agent's count padded to whole row ranges of the weight-gradient kernel), the weight-gradient launch and the order of every sum are
 * hns_actor_train_grad_agents'; the reduce writes each agent's partials into its slice; no norm.  The forward pass launches the agents' live
 * tiles alone.  Properties: one stream, no allocation, no host synchronisation, fixed-order sums, no float atomics, capturable.  Refusals:
 * hns_encoder_forward's / hns_encoder_backward's, in their order.  hns_encoder_agents_workspace_bytes: as hns_encoder_workspace_bytes (A packed
 * images forward); 0 for an invalid shape and for `rows` that are no multiple of num_agents.
 */
size_t hns_encoder_agents_workspace_bytes(int64_t rows, int32_t self_dim, int32_t num_agents, int32_t num_cylinders, int32_t backward);
int hns_encoder_forward_agents(const hns_policy_net *nets, const hns_critic_batch *batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders,
                               float *features, void *workspace, size_t workspace_bytes, void *stream);
int hns_encoder_backward_agents(const hns_policy_net *nets, const hns_critic_batch *batch, int32_t self_dim, int32_t num_agents, int32_t num_cylinders,
                                const float *dfeatures, const hns_policy_grads *grads, void *workspace, size_t workspace_bytes, void *stream);
/*
 * The recurrent block of the reference's rnn heads as a differentiable op (hns_amd.rnn): modules/rnn.py's GRU — an nn.GRUCell
 * stepped over the sequence, the carried state multiplied by 1 - is_init before every step, LayerNorm(h + x) behind it — with input size =
 * hidden size = 128 (the reference builds it on the encoder's 128 features).  For t = 0 .. L - 1, per sequence s:
 *     h <- h (1 - is_init[s, t])
 *     r = sigmoid(W_ir x_t + b_ir + W_hr h + b_hr),  z = sigmoid(W_iz x_t + b_iz + W_hz h + b_hz),  n = tanh(W_in x_t + b_in + r (W_hn h + b_hn))
 *     h <- (1 - z) n + z h,   out_t = LayerNorm(h + x_t) (eps 1e-5, biased variance),   h_last = h after step L - 1.
 * Parameters in nn.GRUCell's / nn.LayerNorm's layouts (gate order r, z, n), every pointer 16-byte aligned.  Sequences have a two-level index,
 * s = b inner + a, so that the encoder op's [B L A, 128] features are read in place as [B, A, L, 128] (x_stride = {L A 128, 128, A 128}) and dx
 * lands in the order hns_encoder_backward reads; out, dout and dx have x's strides (multiples of 4 floats, >= 0; the 128 values contiguous).
 * Properties of both calls: one stream, no host synchronisation, no allocation, fixed-order sums, no float atomics, the same inputs give the
 * same bits; the workspace is used from scratch.  A sequence's results do not depend on the other sequences of the call, and one call over L
 * steps gives the bits of L one-step calls chained through h_last -> h0.
 * Refused before any launch: a NULL struct, a NULL or misaligned (16 bytes) parameter, gradient, x, out, h_last, dout or dx; a misaligned h0,
 * h_hist, dh_last or dh0; steps outside [1, HNS_GRU_MAX_STEPS]; outer or inner < 1 (or outer x inner x steps >= 2^40); a negative stride or one
 * that is no multiple of 4; hns_gru_backward without h_hist; a workspace that is NULL, not 256-byte aligned or shorter than the size function's.
 *
 * hns_gru_workspace_bytes: bytes of device workspace for `seqs` sequences of `steps` steps; the forward pass needs none (0, and takes a NULL
 * workspace); backward != 0: the gate gradients ([seqs steps, 512] fp32) and the partial sums; 0 for an invalid shape too.
 * hns_gru_forward: one launch.  h_hist (may be NULL): h after every step, [S, L, 128] — the one activation the backward pass needs.
 * hns_gru_backward: three launches (sweep, weight gradients, reduce).  WRITES (does not accumulate) the six parameter gradients of
 * sum(out x dout) + sum(h_last x dh_last) (dh_last NULL: zeros) in their PyTorch layouts, dx, and dh0 when it is not NULL; the gates are
 * recomputed from x, h0 and h_hist.  dh0 of a sequence with is_init[s, 0] = 1 is zero.
 */
#define HNS_GRU_HIDDEN 128     /* input size = hidden size */
#define HNS_GRU_MAX_STEPS 64   /* the reference asserts train_seq_len <= train_every (64) */
typedef struct hns_gru_net { const float *weight_ih, *weight_hh, *bias_ih, *bias_hh, *ln_w, *ln_b; } hns_gru_net;   /* [384,128] x2, [384] x2, [128] x2 */
typedef struct hns_gru_grads { float *weight_ih, *weight_hh, *bias_ih, *bias_hh, *ln_w, *ln_b; } hns_gru_grads;
typedef struct hns_gru_seq {
    const float *x;            /* element (b, a, t, i) at b x_stride[0] + a x_stride[1] + t x_stride[2] + i: sequence s = b * inner + a */
    int64_t x_stride[3];
    int64_t outer, inner;      /* B, A: S = B * A sequences (inner = 1 for a plain [S, L, 128]) */
    int32_t steps;             /* L in [1, HNS_GRU_MAX_STEPS] */
    const float *h0;           /* [S, 128] contiguous, or NULL: zeros */
    const uint8_t *is_init;    /* [S, L] contiguous, or NULL: none */
} hns_gru_seq;
size_t hns_gru_workspace_bytes(int64_t seqs, int32_t steps, int32_t backward);
int hns_gru_forward(const hns_gru_net *net, const hns_gru_seq *seq, float *out, float *h_last, float *h_hist, void *workspace, size_t workspace_bytes,
                    void *stream);
int hns_gru_backward(const hns_gru_net *net, const hns_gru_seq *seq, const float *h_hist, const float *dout, const float *dh_last,
                     const hns_gru_grads *grads, float *dx, float *dh0, void *workspace, size_t workspace_bytes, void *stream);
/*
 * One GRU per agent (the stacked actor of share_actor: false with actor.rnn; hns_amd.rnn with stacked parameters):
 * hns_gru_forward / hns_gru_backward with a hns_gru_net / hns_gru_grads whose every tensor is stacked over `inner` = A agents
 * ([A, 384, 128] x2, [A, 384] x2, [A, 128] x2, contiguous): sequence s = b inner + a runs on slice a, and agent a's slice of every gradient
 * is the sum over its own sequences.  x, out, dout, dx, h0, is_init, h_hist, h_last and dh0 keep the layouts and the index order above.
 * Per sequence the arithmetic and its order are hns_gru_forward's and hns_gru_backward's: out, h_last, h_hist, dx and dh0 of sequence (b, a)
 * are bit for bit those of the shared entries called with slice a.
 * The division of the work is a function of the shape alone.  Sweeps: a tile is 16 sequences of ONE agent (b = 16 i .. 16 i + 15 at fixed
 * a), tpa = ceil(outer / 16) tiles per agent; the grid has A gpa workgroups, gpa = min(tpa, floor(256 / A)); workgroup g belongs to agent
 * g / gpa for the whole launch and runs that agent's tiles g % gpa, g % gpa + gpa, ...  Weight gradients: the gate-gradient workspace is
 * numbered agent-major, row (a, b L + t), each agent's outer L rows padded to spa row ranges of tps 32-row tiles (t = ceil(outer L / 32),
 * tps = ceil(t / floor(256 / A)), spa = ceil(t / tps)), so no range holds two agents; the padding rows are neither written nor read.  Sums:
 * a weight-gradient partial adds its range's rows in index order; agent a's gradient value is the fp64 sum of its spa range partials in index
 * order (the LayerNorm's: of its gpa workgroups' partial rows, each the workgroup's tiles in the order it ran them), rounded once.
 * Refusals: hns_gru_forward's / hns_gru_backward's, in their order, and behind the shape checks `inner` outside [1, HNS_MAX_AGENTS].
 * hns_gru_agents_workspace_bytes: as hns_gru_workspace_bytes for `outer` x `inner` sequences (0 forward, and for an invalid shape).
 */
size_t hns_gru_agents_workspace_bytes(int64_t outer, int64_t inner, int32_t steps, int32_t backward);
int hns_gru_forward_agents(const hns_gru_net *nets, const hns_gru_seq *seq, float *out, float *h_last, float *h_hist, void *workspace,
                           size_t workspace_bytes, void *stream);
int hns_gru_backward_agents(const hns_gru_net *nets, const hns_gru_seq *seq, const float *h_hist, const float *dout, const float *dh_last,
                            const hns_gru_grads *grads, float *dx, float *dh0, void *workspace, size_t workspace_bytes, void *stream);
/*
 * The recurrent policy's forward pass (actor.rnn / critic.rnn: the GRU block above behind each encoder; hns_amd.policy.RecurrentDevicePolicy;
 * DESIGN.md §7.12): ONE launch per call runs encoder -> one GRU step -> head for both networks, the state carried by the caller on the device.
 * Per (env e, agent a) row and per network:
 *     f = the encoder's output, exactly hns_policy_forward's encoder on the same packed image
 *     h = is_init[e] ? 0 : h_in[e, a]          (h_in (1 - is_init) for finite h_in; a flagged row's h_in is not read, so NaN there is harmless)
 *     the GRU cell as stated for hns_gru_forward, one step, with x_t = f;   h_out[e, a] = h
 *     y = LayerNorm(h + f) (eps 1e-5, biased variance)
 *     the head on y: the actor's fc_mean, the sample or the mode and its log_prob; the critic's v_out.
 * is_init is an ENV-level flag (uint8 [E], NULL: none) that holds for all of the env's agents (the reference's expand_right).  h_in: [E, A, 128]
 * fp32 contiguous or NULL for zeros; h_out [E, A, 128].  h_out may be h_in (in place): a workgroup reads its rows' state before it writes
 * them, and touches no other rows.  HNS_POLICY_DETERMINISTIC and HNS_POLICY_VALUE_ONLY as for hns_policy_forward; with value-only, action /
 * log_prob / loc and actor_h_out are untouched and actor_h_in is not read.  Noise, seed and counter: hns_policy_forward's scheme, bump included.
 * Summation order (NOT hns_gru_forward's: the two agree to fp32 rounding, not bit for bit): each gate pre-activation starts from its bias
 * (b_ir + b_hr and b_iz + b_hz rounded once when the image is packed; b_in; b_hn), then takes the 128 products with f, then the 128 products
 * with h, as v_mfma_f32_16x16x4_f32 steps of four k each, k ascending within a step's quarter (k = 4 s + kq); r = 1 / (1 + exp(-a_r)), likewise
 * z; n = tanh(a_in + r a_hn); h' = (1 - z) n + z h without contraction; LayerNorm as the encoder's (two-pass, 1 / sqrt(var + eps)).
 * Properties: no host synchronisation, no allocation, capturable; the same inputs give the same bits; a row's results do not depend on the
 * other rows of the call.  Refused before any launch, in hns_policy_forward's order with, after the packed image / io / shape: a NULL or
 * misaligned (16 bytes) rnn_packed, a NULL or misaligned (8 bytes) rio; and last: a missing or misaligned (16 bytes) critic_h_out (actor_h_out too unless
 * value-only), a misaligned h_in.
 *
 * hns_policy_rnn_pack: ONE launch builds the GRUs' packed image (hns_policy_rnn_packed_bytes() bytes, 16-byte aligned; separate from
 * hns_policy_pack's, which is unchanged) from the two networks' tensors: call it again after they change.
 */
typedef struct hns_policy_rnn_io {
    const float *actor_h_in, *critic_h_in;     /* [E, A, 128] contiguous, 16-byte aligned, or NULL: zeros */
    float *actor_h_out, *critic_h_out;         /* [E, A, 128]; may alias the matching h_in */
    const uint8_t *is_init;                    /* [E] or NULL */
} hns_policy_rnn_io;
size_t hns_policy_rnn_packed_bytes(void);
int hns_policy_rnn_pack(const hns_gru_net *actor_rnn, const hns_gru_net *critic_rnn, void *rnn_packed, void *stream);
int hns_policy_forward_rnn(const void *packed, const void *rnn_packed, int32_t self_dim, int64_t num_envs, int32_t num_agents, int32_t num_cylinders,
                           const hns_policy_io *io, const hns_policy_rnn_io *rio, int32_t flags, uint64_t seed, uint64_t *counter, void *stream);
/* The recurrent actor alone, the mode of the distribution (recurrent evaluation; hns_amd.policy.RecurrentDevicePolicy.act_step; DESIGN.md
 * §7.13): ONE launch runs the actor half of hns_policy_forward_rnn — the encoder over the actor image (the first half of `packed`), one GRU
 * step on the actor's GRU image (the first half of `rnn_packed`), LayerNorm(h' + f), fc_mean — and writes io->action[row * 4 + o] = loc[o] and
 * rio->actor_h_out[row] = h' for every row, and nothing else.  Never read or written: the critic half of `packed`, the critic half of
 * `rnn_packed`, io->eps, the Philox call counter, io->log_prob / io->value / io->loc, rio->critic_h_in / rio->critic_h_out (NULL is fine for
 * all of these; non-NULL is left untouched).  `action` and `actor_h_out` are bit for bit what hns_policy_forward_rnn with
 * HNS_POLICY_DETERMINISTIC writes there for the same inputs: the same device functions in the same order, no other summation order.
 * rio->actor_h_in: [E, A, 128] or NULL for zeros; rio->is_init: uint8 [E] or NULL, the env-level flag (a flagged row's h_in is not read, so NaN
 * there is harmless); actor_h_out may be actor_h_in (in place).  Properties: no host synchronisation, no allocation, capturable; the same
 * inputs give the same bits; a row's results do not depend on the other rows of the call.  Refused before the launch, in this order: a NULL or
 * misaligned packed image / io and a shape out of range (as hns_policy_act); a NULL or misaligned rnn_packed (16 bytes) or rio (8 bytes); a
 * missing or misaligned observation, a negative stride; a missing or misaligned action; a missing or misaligned (16 bytes) actor_h_out; a
 * misaligned (16 bytes) actor_h_in. */
int hns_policy_act_rnn(const void *packed, const void *rnn_packed, int32_t self_dim, int64_t num_envs, int32_t num_agents, int32_t num_cylinders,
                       const hns_policy_io *io, const hns_policy_rnn_io *rio, void *stream);
/*
 * One RECURRENT actor per agent (share_actor: false with actor.rnn / critic.rnn; hns_amd.policy.PerAgentRecurrentDevicePolicy; DESIGN.md
 * §7.17): the reference stacks the actor's parameters — its GRU's among them — over the agents and vmaps the actor over the agent axis
 * (mappo.py:148-152, :243-246, :281-284); the critic and the critic's GRU stay shared.  `packed` is hns_policy_pack_agents' image (A actor
 * images, then the critic's); `rnn_packed` the image below.  The entries above keep their behaviour.
 *
 * hns_policy_rnn_packed_agents_bytes: bytes of num_agents actor-GRU images followed by ONE critic-GRU image, each one network's half of
 * hns_policy_rnn_pack's image (hns_policy_rnn_packed_bytes() / 2 bytes); 0 for num_agents outside [1, 7].
 * hns_policy_rnn_pack_agents: ONE launch builds that image (16-byte aligned); call it again after the tensors change.  `actor_rnns`: a
 * hns_gru_net whose every tensor is the stacked one ([A, 384, 128] x2, [A, 384] x2, [A, 128] x2, contiguous), so agent a's slice is a
 * hns_gru_net of its own; `critic_rnn` as for hns_policy_rnn_pack.  Image a (a < A) is byte for byte the actor half of hns_policy_rnn_pack's
 * image of (agent a's slice, critic_rnn) — the pre-added b_ir + b_hr and b_iz + b_hz included — and image A its critic half.  Refused before
 * the launch: num_agents out of range, then what hns_policy_rnn_pack refuses (a NULL or misaligned image, a NULL network, a NULL or
 * misaligned tensor pointer).
 * hns_policy_forward_rnn_agents: hns_policy_forward_rnn's arguments, flags, outputs, layouts ([E, A, ...]; the states [E, A, 128]), noise
 * scheme (the Philox counter of row e A + a is the call counter and e A + a; the bump after a sampling call without io->eps), in-place rule
 * (h_out may be h_in) and refusals in its order, all before any launch.  ONE launch (plus the bump): a workgroup is 32 consecutive envs of ONE
 * agent, its actor pass reads that agent's two images, its critic pass the shared two; a tile's state rows lie A 512 bytes apart.  The
 * per-row arithmetic is hns_policy_forward_rnn's and a row's results do not depend on the rows it shares a tile with: for every agent a,
 * every output of row (e, a) — action, loc, log_prob, value, actor_h_out, critic_h_out — is bit for bit what hns_policy_forward_rnn writes
 * for that row on hns_policy_pack's and hns_policy_rnn_pack's images of (agent a's slices, critic).  Deterministic: fixed-order sums, no
 * atomics; no host synchronisation, no allocation, capturable.
 * hns_policy_act_rnn_agents: hns_policy_act_rnn on those images in the same tiles (ONE launch, the actor half alone; its arguments and its
 * refusals, before the launch): bit for bit hns_policy_forward_rnn_agents' action and actor_h_out with HNS_POLICY_DETERMINISTIC; nothing
 * else is read or written.
 */
size_t hns_policy_rnn_packed_agents_bytes(int32_t num_agents);
int hns_policy_rnn_pack_agents(const hns_gru_net *actor_rnns, const hns_gru_net *critic_rnn, int32_t num_agents, void *rnn_packed, void *stream);
int hns_policy_forward_rnn_agents(const void *packed, const void *rnn_packed, int32_t self_dim, int64_t num_envs, int32_t num_agents,
                                  int32_t num_cylinders, const hns_policy_io *io, const hns_policy_rnn_io *rio, int32_t flags, uint64_t seed,
                                  uint64_t *counter, void *stream);
int hns_policy_act_rnn_agents(const void *packed, const void *rnn_packed, int32_t self_dim, int64_t num_envs, int32_t num_agents, int32_t num_cylinders,
                              const hns_policy_io *io, const hns_policy_rnn_io *rio, void *stream);
/*
 * The head and the loss of a recurrent update over hns_gru_forward's output, forward and backward (hns_amd.rnn_train): what a
 * recurrent learner runs between hns_gru_forward and hns_gru_backward.  A minibatch is B segments x L steps x A agents; row (b, t, a), row index
 * (b L + t) A + a, reads the 128 values at y + b y_stride[0] + a y_stride[1] + t y_stride[2] (hns_gru_seq.x_stride's three strides: the op's
 * [B, A, L, 128] view of [B L A, 128] is {L A 128, 128, A 128}, a plain [S, L, 128] is {L 128, 0, 128} with inner 1) and its per-row data at
 * env-step e = segment[b] L + t of the rollout's contiguous [N T, A(, 4)] arrays, i.e. element e A + a.  segment: int64 [B] ids into the
 * flattened [N, T / L], NULL for 0 .. B - 1; num_segments = N T / L.  A segment id outside [0, num_segments) contributes nothing (the
 * convention of hns_critic_batch.index): its per-row data is not read, its L A rows of dy are written as zeros, it is left out of every sum, and
 * n stays B L A.  y and dy are addressed by b alone: nothing is read or written out of bounds through a bad id.  dy has y's strides.
 * Properties of both entries: one stream, no host synchronisation, no allocation, capturable; no float atomics; the same inputs give the same
 * bits; the workspace is used from scratch (it may be dirty).  Order of every sum: a workgroup is 32 row groups of 8 lanes and takes TRIPS of 32
 * consecutive rows; with G = min(ceil(B L A / 32), 512) workgroups, workgroup w takes trips w, w + G, ...; a row group adds its rows trip after
 * trip (head-gradient products in fp32, loss terms in fp64), the workgroup's partial is its 32 row groups added in index order in fp64 (in the
 * workspace), and the G partials are added in index order in fp64 and rounded once to fp32.  A row's 128-wide dot product is, per lane g of
 * its group, the fmaf chain over features 4 g + 32 i + u (i, then u, ascending), then s += s[lane ^ 1], [lane ^ 2], [lane ^ 4].
 * Refused before any launch, with the error string set: a NULL rows struct; outer < 1, inner outside [1, 7], steps outside
 * [1, HNS_GRU_MAX_STEPS]; a NULL or misaligned pointer (16 bytes for y, dy and the head's tensors; 8 for segment; 4 for the per-row arrays, the
 * gradients and the scalars); a negative y stride or one that is no multiple of 4; a negative num_segments; a bad clip_param / loss_kind /
 * huber_delta; a workspace that is NULL, not 256-byte aligned or shorter than the size function's bytes (which are 0 for an invalid shape).
 *
 * hns_rnn_actor_head_grad: fc_mean (head_w [4, 128], head_b [4]) and log_std [4] on y.  Per row mu = W y + b, logp (formed in fp64 from the
 * fp32 mu) and the ratio r as hns_actor_train_grad states them; the backward weight of min and clamp is that entry's: 1 inside the clip
 * (bounds included), outside 1 where the unclipped surrogate is the smaller and 0 otherwise.  dy: the gradient of policy_loss - entropy_coef
 * entropy with respect to y; d_head_w [4, 128], d_head_b [4], d_log_std [4]: WRITTEN (not accumulated), PyTorch layouts;
 * policy_loss = -4 mean(min(r adv, clamp(r) adv)); entropy; ess as the reference writes it for [B, L, A, 1] ratios: the mean over the L A
 * (step, agent) columns of exp(2 logsumexp_b(r) - logsumexp_b(2 r)), divided by B; log_probs: [B, L, A] or NULL.  Three launches.
 * hns_rnn_critic_head_grad: v_out (head_w [1, 128], head_b [1]).  hns_critic_train_grad's statements: value_loss = max(mean loss(b_returns, v),
 * mean loss(b_returns, b_values + clamp(v - b_values, +-clip_param))), one branch for the whole minibatch, both by halves at an exact tie;
 * explained_var = 1 - mse(v, b_returns) / var(b_returns) (unbiased); values: [B, L, A] or NULL.  y is read twice (values and sums, then dy after
 * the decision).  Four launches.
 */
typedef struct hns_rnn_rows {
    const float *y;            /* row (b, t, a) at y + b y_stride[0] + a y_stride[1] + t y_stride[2], 128 contiguous values */
    int64_t y_stride[3];
    int64_t outer, inner;      /* B segments, A agents */
    int32_t steps;             /* L in [1, HNS_GRU_MAX_STEPS] */
    const int64_t *segment;    /* [B] ids into the flattened [N, T / L], or NULL: 0 .. B - 1 */
    int64_t num_segments;      /* N T / L */
} hns_rnn_rows;
size_t hns_rnn_actor_head_workspace_bytes(int64_t outer, int32_t inner, int32_t steps);
size_t hns_rnn_critic_head_workspace_bytes(int64_t outer, int32_t inner, int32_t steps);
int hns_rnn_actor_head_grad(const float *head_w, const float *head_b, const float *log_std, const hns_rnn_rows *rows, const float *action,
                            const float *log_probs_old, const float *advantages, double clip_param, double entropy_coef, float *dy, float *d_head_w,
                            float *d_head_b, float *d_log_std, float *policy_loss, float *entropy, float *ess, float *log_probs, void *workspace,
                            size_t workspace_bytes, void *stream);
int hns_rnn_critic_head_grad(const float *head_w, const float *head_b, const hns_rnn_rows *rows, const float *b_values, const float *b_returns,
                             float clip_param, int32_t loss_kind, float huber_delta, float *dy, float *d_head_w, float *d_head_b, float *value_loss,
                             float *explained_var, float *values, void *workspace, size_t workspace_bytes, void *stream);
/*
 * One head per agent (the stacked actor of share_actor: false with actor.rnn; hns_amd.rnn_train.policy_loss_and_grad_rnn_per_agent; DESIGN.md
 * §7.18): hns_rnn_actor_head_grad with head_w [A, 4, 128], head_b [A, 4] and log_std [A, 4] (A = rows->inner, contiguous) and their gradients
 * stacked the same way; row (b, t, a) runs on slice a, and agent a's slices of the gradients are the sums over its own rows.  policy_loss =
 * -4 mean over ALL B L A rows of min(..) (every row's backward weight carries 1 / (B L A)); entropy = the mean over the agents of each agent's
 * entropy, so each agent's d_log_std takes -entropy_coef / A once; ess is hns_rnn_actor_head_grad's (its columns are per agent).  The
 * dead-segment rule, the geometry struct, the log_probs layout, the ESS launch, the properties and the refusals are hns_rnn_actor_head_grad's;
 * dy and log_probs of row (b, t, a) are bit for bit those of hns_rnn_actor_head_grad with agent a's head over all rows.
 * Order of every sum (a function of the shape alone): the rows kernel runs A gpa workgroups, gpa = min(ceil(B L / 32), floor(512 / A));
 * workgroup w belongs to agent w / gpa and takes trips w % gpa, w % gpa + gpa, ... of that agent's B L positions p = b L + t, 32 consecutive
 * positions to a trip; a row group adds its rows trip after trip (head-gradient products in fp32, loss terms in fp64), the workgroup's partial
 * is its 32 row groups added in index order in fp64; agent a's gradient values add its gpa partials in index order in fp64, rounded once; the
 * loss sum adds all A gpa partials in workgroup order (agent-major); the entropy adds each agent's four terms in index order, then the agents
 * in index order, and divides by A.  hns_rnn_actor_head_agents_workspace_bytes: the bytes for that plan (0 for an invalid shape).
 */
size_t hns_rnn_actor_head_agents_workspace_bytes(int64_t outer, int32_t inner, int32_t steps);
int hns_rnn_actor_head_grad_agents(const float *head_w, const float *head_b, const float *log_std, const hns_rnn_rows *rows, const float *action,
                                   const float *log_probs_old, const float *advantages, double clip_param, double entropy_coef, float *dy,
                                   float *d_head_w, float *d_head_b, float *d_log_std, float *policy_loss, float *entropy, float *ess, float *log_probs,
                                   void *workspace, size_t workspace_bytes, void *stream);
/*
 * The global forms of the two head entries: one rank's part of a data-parallel recurrent update over the union of W ranks' minibatches
 * (they mirror hns_critic_train_sums, hns_critic_train_grad_global and hns_actor_train_grad_global).  Rows, geometry, the
 * dead-segment rule, the order of every sum, the workspace's alignment and size functions and the properties are those above.  With one rank —
 * global_rows = B L A, entropy_share = 1, sums = the call's own hns_rnn_critic_head_sums output — every output has the local entries' bits.
 *
 * hns_rnn_critic_head_sums: the values pass and the sum of its G workgroup partials, no dy and no gradient.  sums[0 .. 5) (device memory,
 * 8-byte aligned): sum loss(v - ret), sum loss(clipped - ret), sum (v - ret)^2, sum ret, sum ret^2 in fp64 over THIS call's live rows, the
 * partials added in the order hns_rnn_critic_head_grad adds them.  values: [B, L, A] or NULL.  Two launches.
 * hns_rnn_critic_head_grad_global: sums are the five values of ALL ranks' rows (the caller added them), global_rows the union's row count.
 * The decision is hns_rnn_critic_head_grad's rule with n = global_rows on the sums given — value_loss, explained_var and the branch weights
 * are the union's, the same on every rank — and dv is scaled by f32(1 / global_rows), so the ranks' dy-driven gradients and head gradients add
 * up to the union's.  The call stands alone: v is recomputed from y into this call's workspace (y is read twice, as in the local entry);
 * `values` is not written.  Four launches.
 * hns_rnn_actor_head_grad_global: every row's backward weight is scaled by f32(1 / global_rows); policy_loss = -4 sum_local min(..) /
 * global_rows, this rank's SHARE (the shares add up to the union's loss); d_log_std takes -entropy_coef entropy_share (1 / W: a SUM over the
 * ranks counts the entropy term once); entropy is the same on every rank; ess stays this call's own, over its own B segments (a diagnostic).
 * Refused as the local entries refuse, and: NULL or misaligned (8 bytes) sums; global_rows < B L A; an entropy_share that is not finite.
 */
int hns_rnn_critic_head_sums(const float *head_w, const float *head_b, const hns_rnn_rows *rows, const float *b_values, const float *b_returns,
                             float clip_param, int32_t loss_kind, float huber_delta, double *sums, float *values, void *workspace, size_t workspace_bytes,
                             void *stream);
int hns_rnn_critic_head_grad_global(const float *head_w, const float *head_b, const hns_rnn_rows *rows, const float *b_values, const float *b_returns,
                                    float clip_param, int32_t loss_kind, float huber_delta, float *dy, float *d_head_w, float *d_head_b,
                                    float *value_loss, float *explained_var, float *values, void *workspace, size_t workspace_bytes, void *stream,
                                    const double *sums, int64_t global_rows);
int hns_rnn_actor_head_grad_global(const float *head_w, const float *head_b, const float *log_std, const hns_rnn_rows *rows, const float *action,
                                   const float *log_probs_old, const float *advantages, double clip_param, double entropy_coef, float *dy,
                                   float *d_head_w, float *d_head_b, float *d_log_std, float *policy_loss, float *entropy, float *ess, float *log_probs,
                                   void *workspace, size_t workspace_bytes, void *stream, int64_t global_rows, double entropy_share);
/* The global form of hns_rnn_actor_head_grad_agents (one head per agent, data-parallel: hns_amd.learner.DataParallelPerAgentRecurrentLearner;
 * DESIGN.md §7.19): that entry's arguments, launches, order of every sum and workspace (hns_rnn_actor_head_agents_workspace_bytes), with
 * hns_rnn_actor_head_grad_global's scalars.  Every row's backward weight is scaled by f32(1 / global_rows); policy_loss = -4 sum_local min(..) /
 * global_rows is this rank's SHARE; each agent's d_log_std takes (-entropy_coef entropy_share) / A, the product formed first, so a share of 1
 * leaves the local constant; entropy is the same on every rank; ess stays this call's own.  The dead-segment rule is unchanged and n stays
 * global_rows.  With global_rows = B L A and entropy_share = 1 every output (dy, the three gradients, the scalars, log_probs) has
 * hns_rnn_actor_head_grad_agents' bits.  Refused as that entry refuses and in its order, then global_rows < B L A and an entropy_share that is
 * not finite (both before the workspace is looked at). */
int hns_rnn_actor_head_grad_agents_global(const float *head_w, const float *head_b, const float *log_std, const hns_rnn_rows *rows, const float *action,
                                          const float *log_probs_old, const float *advantages, double clip_param, double entropy_coef, float *dy,
                                          float *d_head_w, float *d_head_b, float *d_log_std, float *policy_loss, float *entropy, float *ess,
                                          float *log_probs, void *workspace, size_t workspace_bytes, void *stream, int64_t global_rows,
                                          double entropy_share);
/* The 2-norm of one flat fp32 gradient bucket: norm[0] = f32(sqrt(sum_i flat[i]^2)), in this order (tests/dp_reference.py restates it in numpy):
 * the bucket is cut into quads of four consecutive floats, the last one short by numel % 4 values that count as 0 (nothing past numel is
 * read); G = clamp(ceil(quads / 1024), 1, 64) workgroups of 256 threads, T = 256 G; thread t of the grid adds, for q = t, t + T, t + 2 T, ...,
 * ((x x + y y) + z z) + w w of quad q in fp64 (each product exact) to its sum; within a workgroup each wave of 64 runs the butterfly
 * s += s[lane ^ o] for o = 32, 16, 8, 4, 2, 1 and the four waves add in index order to the workgroup's partial (fp64, in `workspace`); a second
 * launch adds the G partials in index order and rounds the fp64 square root once.  An entry of 3e19 squares to 9e38 without overflow.  Two
 * launches in one stream; no atomics, no allocation, no host synchronisation, capturable; the same inputs give the same bits.  Refused before
 * any launch: a NULL or misaligned pointer (flat 16 bytes, norm 4, workspace 8), numel < 1, a workspace shorter than the size function's
 * bytes (numel < 1: 0). */
size_t hns_grad_norm_workspace_bytes(long long numel);
int hns_grad_norm(const float *flat, long long numel, float *norm, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The info row of MAPPOPolicy.train_op (learning/mappo.py:463-472): the means over the minibatches of the scalars the updates wrote
 * into `table` ([minibatches, columns] fp32, contiguous; hns_amd.learner hands the two *_train_grad calls pointers into its rows), then
 * action_norm = mean over the rows of sqrt(sum_i a_i^2), row r's element i at action[r action_stride[0] + i action_stride[1]] (strides in
 * elements, >= 0; float4 loads where act_dim is 4, the element stride 1 and every row 16-byte aligned).  out [columns + 1]: column c's fp64 sum in
 * row order divided by `minibatches` and rounded once to fp32, then action_norm: per-workgroup fp64 partials in `workspace`, summed in index
 * order by one workgroup, divided by `rows`, rounded once.  Two launches in one stream; no allocation, no host synchronisation, no float
 * atomics, capturable; the same inputs give the same bits.  Refused before any launch: a NULL or misaligned pointer (fp32 arrays 4-byte,
 * workspace 8-byte aligned), rows < 1, act_dim outside [1, 8], minibatches < 1, columns outside [1, 16], a negative stride, a workspace
 * shorter than the size function's bytes (rows < 1: 0).
 */
size_t hns_learner_info_workspace_bytes(long long rows);
int hns_learner_info(const float *action, const int64_t action_stride[2], long long rows, int act_dim, const float *table, int minibatches,
                     int columns, float *out, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The rollout collector's per-step store (hns_amd.collector): ONE launch copies up to 16 per-env rows into time slot `slot` of
 * their batch-major storage — segment s takes env e's row_bytes contiguous bytes at src + e src_stride and writes them at
 * dst + e dst_stride + slot row_bytes, for e in [0, num_envs).  A tensor without a slot axis (the last step's next observation) is stored with
 * num_slots = 1, slot = 0.  The segments travel by value in the kernel arguments (no device-side table, no allocation); each is copied in
 * the widest of 16-, 4- and 1-byte units that src, dst, both strides and row_bytes are all multiples of.  Nothing outside the target rows
 * is written.  One launch in one stream; no host synchronisation, capturable.  Refused before any launch: NULL segments, count outside
 * [1, 16], num_envs < 1, num_slots < 1, slot outside [0, num_slots), a NULL src or dst, row_bytes outside [1, 2^20], src_stride < row_bytes,
 * dst_stride < num_slots row_bytes, num_envs dst_stride (or num_envs src_stride) past int64.  Sources and destinations must not overlap.
 */
#define HNS_ROLLOUT_MAX_SEGMENTS 16
typedef struct hns_rollout_segment {
    const void *src;   /* env e's row: row_bytes contiguous bytes at src + e * src_stride */
    void *dst;         /* storage base: env e, slot t at dst + e * dst_stride + t * row_bytes */
    int64_t src_stride, dst_stride, row_bytes;   /* in bytes */
} hns_rollout_segment;
int hns_rollout_store(const hns_rollout_segment *segments, int32_t count, int64_t num_envs, int64_t slot, int64_t num_slots, void *stream);

/*
 * The evaluator's statistic means (hns_amd.evaluator): for each of `count` rows the mean, over the envs e in [0, num_envs) with
 * mask[e] != 0 (every env when mask is NULL), of the values src[e * stride] that are not NaN — torch.nanmean restricted to the mask.
 * used[i]: the values that entered row i's mean; used[count]: the masked envs.  A row with no value entering gives NaN; +-inf propagates as in
 * IEEE addition.  The rows travel by value in the kernel arguments; one 256-thread workgroup per row sums its elements tid, tid + 256, ... in
 * fp64 in that order, joins the partials in a fixed-order tree, divides once and rounds once to fp32: no atomics, the same inputs give the same
 * bits.  For num_envs <= 2^20: |mean - exact| <= 2^-24 |exact| + 2^-33 mean|x|.  One launch in one stream; no allocation, no host
 * synchronisation, capturable.  Refused before the launch: NULL rows, mean or used, count outside [1, 64], num_envs < 1, a NULL src, a
 * misaligned src / mean (4 bytes) or used (8 bytes), a stride < 1 (or one with num_envs * stride * 4 past int64).
 */
#define HNS_EVAL_MAX_ROWS 64
typedef struct hns_eval_row {
    const float *src;   /* element e of the row is src[e * stride] */
    int64_t stride;     /* in elements, >= 1 */
} hns_eval_row;
int hns_eval_means(const hns_eval_row *rows, int32_t count, int64_t num_envs, const uint8_t *mask, float *mean, int64_t *used, void *stream);

int hns_abi_version(void);
size_t hns_cfg_size(void);  /* sizeof(hns_cfg) the library was built with (binding self-check) */
const char *hns_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* HNS_H_ */
