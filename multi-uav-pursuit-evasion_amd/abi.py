"""ctypes mirror of include/hns.h and loader of the HIP shared library (libhns.so).

The product path has no CPU fallback: `load_library()` raises if the HIP extension has not
been built (`python -c "import __graft_entry__ as g; g.build()"`).
"""
import ctypes as C
import os

HNS_ABI_VERSION = 8
HNS_MAX_AGENTS = 7
HNS_MAX_CYLINDERS = 16
HNS_NUM_STATS = 24
HNS_SELF_DIM = 20

HNS_INIT_RANDOM, HNS_INIT_EVAL, HNS_INIT_SCENARIO = 0, 1, 2
HNS_ACTION_POLICY, HNS_ACTION_MOTOR = 0, 1      # hns_action_input

# row order of hns_buffers.stats == stats_spec order (reference hideandseek.py:400-425)
STAT_NAMES = [
    "success", "collision", "blocked", "distance_reward", "distance_predicted_reward",
    "speed_reward", "collision_reward", "collision_wall", "collision_cylinder", "collision_drone",
    "detect_reward", "catch_reward", "smoothness_reward", "smoothness_mean", "smoothness_max",
    "first_capture_step", "sum_detect_step", "return", "action_error_order1_mean",
    "action_error_order1_max", "target_predicted_error", "distance_threshold_L", "out_of_arena",
    "smoothness_coef",
]
assert len(STAT_NAMES) == HNS_NUM_STATS

_f = C.c_float
_i = C.c_int32


class HnsCfg(C.Structure):
    _fields_ = [
        ("abi_version", _i), ("num_envs", _i), ("num_agents", _i), ("num_cylinders", _i),
        ("obs_max_cylinder", _i), ("max_episode_length", _i), ("use_deployment", _i),
        ("fixed_yaw", _i), ("ground_clamp", _i), ("write_critic_state", _i), ("init_mode", _i),
        ("cyl_min_num", _i), ("cyl_fixed_num", _i), ("grid_num", _i), ("env_index_offset", _i),
        ("num_targets", _i),
        ("dt", _f), ("gravity", _f),
        ("arena_size", _f), ("max_height", _f), ("cylinder_size", _f), ("cylinder_height", _f),
        ("catch_radius", _f), ("drone_detect_radius", _f), ("target_detect_radius", _f),
        ("collision_radius", _f), ("v_drone", _f), ("v_prey", _f),
        ("dist_reward_coef", _f), ("catch_reward_coef", _f), ("detect_reward_coef", _f),
        ("collision_coef", _f), ("speed_coef", _f), ("smoothness_coef", _f),
        ("mask_value", _f), ("invalid_z", _f), ("grid_size", _f), ("arena_sq", _f),
        ("coll_drone_dist", _f), ("boundary", _f),
        ("mass", _f), ("inertia", _f * 3), ("kf", _f * 4), ("km", _f * 4), ("rotor_dir", _f * 4),
        ("rotor_px", _f * 4), ("rotor_py", _f * 4), ("tau_up", _f), ("tau_down", _f),
        ("max_thrust_ratio", _f), ("target_clip", _f), ("hover_throttle", _f),
        ("pid_kp", _f * 3), ("pid_ki", _f * 3), ("pid_kd", _f * 3), ("pid_ilimit", _f * 3),
        ("pid_outlimit", _f),
        ("lin_damp_factor", _f), ("ang_damp_factor", _f), ("max_ang_vel", _f), ("inv_mass", _f), ("inv_inertia", _f * 3), ("inv_num_agents", _f),
        ("inv_max_episode_length", _f), ("max_lin_vel", _f), ("inv_dt", _f),
        ("drone_xy_lo", _f * 2), ("drone_xy_hi", _f * 2), ("target_xy_lo", _f * 2),
        ("target_xy_hi", _f * 2), ("z_lo", _f), ("z_hi", _f), ("rpy_lo", _f * 3), ("rpy_hi", _f * 3),
        ("fixed_drone_pos", (_f * 3) * (HNS_MAX_AGENTS + 1)), ("fixed_target_pos", _f * 3),
        ("fixed_cyl_pos", (_f * 3) * HNS_MAX_CYLINDERS), ("fixed_cyl_active", _i), ("tp_use_obstacles", _i),
        ("pid_reset_on_reset", _i), ("stats_stride", _i), ("reset_extra_step", _i), ("action_input", _i),
        # contact response (include/hns.h; off by default): the switch, the two radii, the derived fp32 constants, padding to 64 bytes
        ("contact_response", _i), ("contact_drone_radius", _f), ("contact_target_radius", _f),
        ("contact_dd", _f), ("contact_dd2", _f), ("contact_rd", _f), ("contact_rd2", _f), ("contact_rt", _f), ("contact_rt2", _f),
        ("contact_pad", _i * 7),
    ]

    def copy(self):
        out = HnsCfg()
        C.memmove(C.byref(out), C.byref(self), C.sizeof(HnsCfg))
        return out


_fp = C.c_void_p  # device (or, for the oracle, host) pointers travel as integers

BUFFER_FIELDS = [
    "drone_state", "throttle", "pid_integ", "pid_last_rate", "prev_action", "target_pos",
    "target_vel", "cylinders", "progress", "stats", "obs_self", "obs_others", "obs_cylinders",
    "state_drones", "reward", "action_error", "done", "detect", "nonfinite", "ctbr", "target_rate", "reset_pid",
]
# nullable fields: ctbr / target_rate are bound only with task.publish_ctbr (transforms.py:456-457); reset_pid is an INPUT that may alias
# `done` (include/hns.h) and is never allocated by buffer_shapes
OPTIONAL_BUFFER_FIELDS = ("ctbr", "target_rate", "reset_pid")


class HnsBuffers(C.Structure):
    _fields_ = [(name, _fp) for name in BUFFER_FIELDS]


def self_dim(num_targets=1):
    """Values per state_self / state_drones row: the reference's 20; 24 with the two-evader extension."""
    return 24 if num_targets == 2 else HNS_SELF_DIM


def buffer_shapes(E, A, Cn, K, num_targets=1, publish_ctbr=False):
    """Shape (and dtype name) of every hns_buffers field (the optional ones only when asked for)."""
    tgt = (E, 2, 3) if num_targets == 2 else (E, 3)
    D = self_dim(num_targets)
    extra = {"ctbr": ((E, A, 4), "float32"), "target_rate": ((E, A, 4), "float32")} if publish_ctbr else {}
    return {**_required_buffer_shapes(E, A, Cn, K, tgt, D), **extra}


def _required_buffer_shapes(E, A, Cn, K, tgt, D):
    return {
        "drone_state": ((E, A, 13), "float32"), "throttle": ((E, A, 4), "float32"),
        "pid_integ": ((E, A, 4), "float32"), "pid_last_rate": ((E, A, 4), "float32"),
        "prev_action": ((E, A, 4), "float32"), "target_pos": (tgt, "float32"),
        "target_vel": (tgt, "float32"), "cylinders": ((E, Cn, 3), "float32"),
        "progress": ((E,), "float32"), "stats": ((HNS_NUM_STATS, E), "float32"),
        "obs_self": ((E, A, D), "float32"), "obs_others": ((E, A, max(A - 1, 0), 3), "float32"),
        "obs_cylinders": ((E, A, K, 5), "float32"), "state_drones": ((E, A, D), "float32"),
        "reward": ((E, A), "float32"), "action_error": ((E, A), "float32"), "done": ((E,), "uint8"),
        "detect": ((E,), "uint8"), "nonfinite": ((1,), "int32"),
    }


HNS_HOVER_NUM_STATS = 39
HNS_HOVER_NUM_ACC = 12
HOVER_STAT_NAMES = [
    "return", "pos_bonus", "head_bonus", "reward_pos", "reward_up", "reward_vel", "reward_acc", "reward_jerk",
    "episode_len", "pos_error", "heading_alignment", "uprightness", "action_smoothness", "linear_v_max",
    "angular_v_max", "linear_a_max", "angular_a_max", "linear_jerk_max", "angular_jerk_max", "linear_v_mean",
    "angular_v_mean", "linear_a_mean", "angular_a_mean", "linear_jerk_mean", "angular_jerk_mean", "motor1",
    "motor2", "motor3", "motor4", "cmd_r", "cmd_p", "cmd_y", "cmd_thrust", "target_r_rate", "target_p_rate",
    "target_y_rate", "real_r_rate", "real_p_rate", "real_y_rate",
]
assert len(HOVER_STAT_NAMES) == HNS_HOVER_NUM_STATS


class HnsHoverCfg(C.Structure):
    _fields_ = [("reward_distance_scale", _f), ("reward_v_scale", _f), ("reward_acc_scale", _f), ("reward_jerk_scale", _f),
                ("linear_vel_max", _f), ("linear_acc_max", _f), ("alpha", _f), ("target_pos", _f * 3),
                ("target_heading", _f * 3), ("pos_lo", _f * 3), ("pos_hi", _f * 3), ("rpy_lo", _f * 3), ("rpy_hi", _f * 3)]


HOVER_BUFFER_FIELDS = ["drone_state", "throttle", "pid_integ", "pid_last_rate", "prev_action", "progress", "stats",
                       "acc", "obs", "reward", "done"]


class HnsHoverBuffers(C.Structure):
    _fields_ = [(name, _fp) for name in HOVER_BUFFER_FIELDS]


def hover_buffer_shapes(E):
    return {"drone_state": ((E, 1, 13), "float32"), "throttle": ((E, 1, 4), "float32"), "pid_integ": ((E, 1, 4), "float32"),
            "pid_last_rate": ((E, 1, 4), "float32"), "prev_action": ((E, 1, 4), "float32"), "progress": ((E,), "float32"),
            "stats": ((HNS_HOVER_NUM_STATS, E), "float32"), "acc": ((HNS_HOVER_NUM_ACC, E), "float32"),
            "obs": ((E, 1, HNS_SELF_DIM), "float32"), "reward": ((E, 1), "float32"), "done": ((E,), "uint8")}


HNS_GAE_BATCH_MAJOR, HNS_GAE_TIME_MAJOR = 0, 1        # hns_gae layouts: [N, T, K] (compute_gae) / [T, N, K] (compute_gae_)
HNS_GAE_DONE_U8, HNS_GAE_DONE_F32 = 0, 1              # hns_gae done dtypes: bool / uint8 bytes, fp32
HNS_GAE_WORKSPACE_DOUBLES = 20480                     # fp64 scratch hns_gae needs for its moment row
HNS_OK, HNS_ERR_INVALID_ARG, HNS_ERR_NOT_BOUND, HNS_ERR_DEVICE, HNS_ERR_NO_DEVICE, HNS_ERR_CONFIG = 0, -1, -2, -3, -4, -5

# ---- trajectory predictor (include/hns.h: hns_tp_buffers) ------------------------------------------------
HNS_TP_HIDDEN = 64
TP_PACKED_BYTES = 16 * (8 * 2 * (5 + 4) * 64 + 2 * 4 * 64 + 256 // 4 + 32 // 4)      # hns_tp_packed_bytes(): the predictor's operand image at five frame chunks
TP_WEIGHT_FIELDS = ["w_ih", "w_hh", "b_ih", "b_hh", "w_fc", "b_fc"]
TP_BUFFER_FIELDS = TP_WEIGHT_FIELDS + ["packed", "history", "pred", "obs_self", "state_drones", "groundtruth", "tp_done"]
# hns_tp_buffers weight field -> TP_net.state_dict() key (learning/mappo.py:572-589)
TP_STATE_DICT_KEYS = {"w_ih": "lstm.weight_ih_l0", "w_hh": "lstm.weight_hh_l0", "b_ih": "lstm.bias_ih_l0",
                      "b_hh": "lstm.bias_hh_l0", "w_fc": "fc.weight", "b_fc": "fc.bias"}


class HnsTpBuffers(C.Structure):
    _fields_ = [(name, _fp) for name in TP_BUFFER_FIELDS]


class HnsTpParams(C.Structure):           # hns_tp_params / hns_tp_grads: the six weight pointers
    _fields_ = [(name, _fp) for name in TP_WEIGHT_FIELDS]


def tp_frame_dim(A, C=0, use_obstacles=False):
    """Width of one predictor frame (hideandseek.py:808-820)."""
    return 7 + 3 * A + (3 * C if use_obstacles else 0)


def tp_buffer_shapes(E, A, T, F, I=None, num_targets=1):
    """Two evaders (extension): the predictor runs once per (env, evader) unit — window, prediction, ground truth and done flag are
    [E * 2, ...] (unit 2 e + j), rows carry both predictions (24 + 6F values)."""
    NT = 2 if num_targets == 2 else 1
    I, D = (7 + 3 * A if I is None else I), self_dim(NT) + 3 * F * NT
    U = E * NT
    return {"w_ih": ((4 * HNS_TP_HIDDEN, I), "float32"), "w_hh": ((4 * HNS_TP_HIDDEN, HNS_TP_HIDDEN), "float32"),
            "b_ih": ((4 * HNS_TP_HIDDEN,), "float32"), "b_hh": ((4 * HNS_TP_HIDDEN,), "float32"),
            "w_fc": ((3 * F, HNS_TP_HIDDEN), "float32"), "b_fc": ((3 * F,), "float32"),
            "packed": ((TP_PACKED_BYTES,), "uint8"), "history": ((U, T, I), "float32"), "pred": ((U, F, 3), "float32"), "obs_self": ((E, A, D), "float32"),
            "state_drones": ((E, A, D), "float32"), "groundtruth": ((U, 3), "float32"), "tp_done": ((U,), "uint8")}


# the MAPPO policy's forward pass (include/hns.h: hns_policy_*; hns_amd.policy)
HNS_POLICY_MAX_SELF_DIM = 96
HNS_POLICY_DETERMINISTIC, HNS_POLICY_VALUE_ONLY = 1, 2
POLICY_NET_FIELDS = ["embed_self_w", "embed_self_b", "embed_others_w", "embed_others_b", "embed_cyl_w", "embed_cyl_b", "ln_w", "ln_b",
                     "in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b", "linear1_w", "linear1_b", "linear2_w", "linear2_b",
                     "norm1_w", "norm1_b", "norm2_w", "norm2_b", "head_w", "head_b", "log_std"]


class HnsPolicyNet(C.Structure):
    _fields_ = [(f, _fp) for f in POLICY_NET_FIELDS]


class HnsPolicyIo(C.Structure):
    _fields_ = [("obs_self", _fp), ("obs_others", _fp), ("obs_cylinders", _fp), ("self_stride", C.c_int64 * 2), ("others_stride", C.c_int64 * 3),
                ("cyl_stride", C.c_int64 * 3), ("eps", _fp), ("action", _fp), ("loc", _fp), ("log_prob", _fp), ("value", _fp)]


class HnsPolicyState(C.Structure):         # hns_policy_state (hns_policy_central_forward; hns_amd.policy.CentralCriticDevicePolicy)
    _fields_ = [("state_drones", _fp), ("cylinders", _fp), ("drones_stride", C.c_int64 * 2), ("cyl_stride", C.c_int64 * 2)]


# the MAPPO critic's update (include/hns.h: hns_critic_train_grad, hns_adam_clipped; hns_amd.critic_train)
HNS_CRITIC_LOSS_HUBER, HNS_CRITIC_LOSS_MSE = 0, 1


# hns_critic_batch's and hns_actor_batch's observation / index part (hns_amd.policy_train fills it), in front of each update's per-row pointers
TRAIN_BATCH_FIELDS = [("obs_self", _fp), ("obs_others", _fp), ("obs_cylinders", _fp), ("self_stride", C.c_int64 * 3), ("others_stride", C.c_int64 * 4),
                      ("cyl_stride", C.c_int64 * 4), ("num_envs", C.c_int64), ("num_steps", C.c_int64), ("index", _fp), ("batch", C.c_int64)]


class HnsCriticBatch(C.Structure):
    _fields_ = TRAIN_BATCH_FIELDS + [("b_values", _fp), ("b_returns", _fp)]


class HnsActorBatch(C.Structure):         # the MAPPO actor's update (include/hns.h: hns_actor_train_grad; hns_amd.actor_train)
    _fields_ = TRAIN_BATCH_FIELDS + [("action", _fp), ("log_probs_old", _fp), ("advantages", _fp)]


class HnsAdamTensor(C.Structure):          # hns_adam_tensor, and hns_tp_adam_tensor (the same layout: csrc/hns_adam.hip asserts it)
    _fields_ = [("param", _fp), ("grad", _fp), ("exp_avg", _fp), ("exp_avg_sq", _fp), ("numel", C.c_int64)]


HnsTpAdamTensor = HnsAdamTensor

HNS_ROLLOUT_MAX_SEGMENTS = 16


class HnsRolloutSegment(C.Structure):      # hns_rollout_segment (hns_rollout_store; hns_amd.collector): strides and row length in bytes
    _fields_ = [("src", _fp), ("dst", _fp), ("src_stride", C.c_int64), ("dst_stride", C.c_int64), ("row_bytes", C.c_int64)]


HNS_EVAL_MAX_ROWS = 64


class HnsEvalRow(C.Structure):             # hns_eval_row (hns_eval_means; hns_amd.evaluator): the stride in elements
    _fields_ = [("src", _fp), ("stride", C.c_int64)]


# the GRU as a differentiable op (include/hns.h: hns_gru_*; hns_amd.rnn)
HNS_GRU_HIDDEN = 128
HNS_GRU_MAX_STEPS = 64
GRU_NET_FIELDS = ["weight_ih", "weight_hh", "bias_ih", "bias_hh", "ln_w", "ln_b"]


class HnsGruNet(C.Structure):              # hns_gru_net / hns_gru_grads: the six parameter pointers
    _fields_ = [(f, _fp) for f in GRU_NET_FIELDS]


class HnsGruSeq(C.Structure):
    _fields_ = [("x", _fp), ("x_stride", C.c_int64 * 3), ("outer", C.c_int64), ("inner", C.c_int64), ("steps", C.c_int32), ("h0", _fp), ("is_init", _fp)]


class HnsRnnRows(C.Structure):             # hns_rnn_rows (hns_rnn_actor_head_grad / hns_rnn_critic_head_grad; hns_amd.rnn_train)
    _fields_ = [("y", _fp), ("y_stride", C.c_int64 * 3), ("outer", C.c_int64), ("inner", C.c_int64), ("steps", C.c_int32), ("segment", _fp),
                ("num_segments", C.c_int64)]


class HnsPolicyRnnIo(C.Structure):         # hns_policy_rnn_io (hns_policy_forward_rnn; hns_amd.policy.RecurrentDevicePolicy)
    _fields_ = [("actor_h_in", _fp), ("critic_h_in", _fp), ("actor_h_out", _fp), ("critic_h_out", _fp), ("is_init", _fp)]


_LIB = None
LIB_NAME = "libhns.so"


def library_path():
    """In-tree libhns.so; HNS_LIBRARY names another build of the same ABI (A/B measurement builds, tools/build_variant.sh)."""
    return os.environ.get("HNS_LIBRARY") or os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)


def load_library():
    """dlopen the HIP extension and declare its C-ABI. Raises if it is not built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: the HIP extension is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
            "There is no CPU fallback for the product path.")
    lib = C.CDLL(path)
    lib.hns_create.argtypes = [C.POINTER(HnsCfg), C.POINTER(C.c_void_p)]
    lib.hns_create.restype = C.c_int
    lib.hns_destroy.argtypes = [C.c_void_p]
    lib.hns_destroy.restype = None
    lib.hns_bind.argtypes = [C.c_void_p, C.POINTER(HnsBuffers)]
    lib.hns_bind.restype = C.c_int
    lib.hns_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hns_step.restype = C.c_int
    lib.hns_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.hns_reset.restype = C.c_int
    lib.hns_reset_tasks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p]
    lib.hns_reset_tasks.restype = C.c_int
    lib.hns_raycast.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
    lib.hns_raycast.restype = C.c_int
    lib.hns_set_v_prey.argtypes = [C.c_void_p, C.c_float]
    lib.hns_set_v_prey.restype = C.c_int
    lib.hns_set_smoothness_coef.argtypes = [C.c_void_p, C.c_float]
    lib.hns_set_smoothness_coef.restype = C.c_int
    lib.hns_set_reset_epoch.argtypes = [C.c_void_p, C.c_uint32]
    lib.hns_set_reset_epoch.restype = C.c_int
    lib.hns_get_reset_epoch.argtypes = [C.c_void_p]
    lib.hns_get_reset_epoch.restype = C.c_uint32
    lib.hns_enable_timing.argtypes = [C.c_void_p, C.c_int]
    lib.hns_enable_timing.restype = C.c_int
    lib.hns_step_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.hns_step_kernel_ms.restype = C.c_float
    lib.hns_region_begin.argtypes = [C.c_void_p, C.c_void_p]
    lib.hns_region_begin.restype = C.c_int
    lib.hns_region_end.argtypes = [C.c_void_p, C.c_void_p]
    lib.hns_region_end.restype = C.c_int
    lib.hns_region_ms.argtypes = [C.c_void_p]
    lib.hns_region_ms.restype = C.c_float
    lib.hns_moments.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.hns_moments.restype = C.c_int
    lib.hns_rollout_moments.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.hns_rollout_moments.restype = C.c_int
    lib.hns_gae.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                            C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hns_gae.restype = C.c_int
    lib.hns_rollout_normalise.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hns_rollout_normalise.restype = C.c_int
    lib.hns_clock_probe.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    lib.hns_clock_probe.restype = C.c_int
    lib.hns_copy_f4.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.hns_copy_f4.restype = C.c_int
    lib.hns_set_phase_profile.argtypes = [C.c_void_p, C.c_void_p]
    lib.hns_set_phase_profile.restype = C.c_int
    lib.hns_step_mapping.argtypes = [C.c_void_p]
    lib.hns_step_mapping.restype = C.c_int
    lib.hns_selected_kernels.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_int32)]
    lib.hns_selected_kernels.restype = C.c_int
    lib.hns_hover_step.argtypes = [C.POINTER(HnsCfg), C.POINTER(HnsHoverCfg), C.POINTER(HnsHoverBuffers), C.c_void_p, C.c_void_p]
    lib.hns_hover_step.restype = C.c_int
    lib.hns_hover_reset.argtypes = [C.POINTER(HnsCfg), C.POINTER(HnsHoverCfg), C.POINTER(HnsHoverBuffers), C.c_void_p,
                                    C.c_uint64, C.c_uint32, C.c_void_p]
    lib.hns_hover_reset.restype = C.c_int
    lib.hns_tp_bind.argtypes = [C.c_void_p, C.POINTER(HnsTpBuffers), C.c_int32, C.c_int32]
    lib.hns_tp_bind.restype = C.c_int
    lib.hns_tp_refresh.argtypes = [C.c_void_p, C.c_void_p]
    lib.hns_tp_refresh.restype = C.c_int
    lib.hns_tp_packed_bytes.argtypes = []
    lib.hns_tp_packed_bytes.restype = C.c_size_t
    lib.hns_tp_observe.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.hns_tp_observe.restype = C.c_int
    lib.hns_tp_train_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32]
    lib.hns_tp_train_workspace_bytes.restype = C.c_size_t
    lib.hns_tp_train_grad.argtypes = [C.POINTER(HnsTpParams), C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                      C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(HnsTpParams), C.c_void_p, C.c_void_p, C.c_size_t,
                                      C.c_void_p]
    lib.hns_tp_train_grad.restype = C.c_int
    lib.hns_tp_adam.argtypes = [C.POINTER(HnsTpAdamTensor), C.c_int32, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p]
    lib.hns_tp_adam.restype = C.c_int
    lib.hns_policy_packed_bytes.argtypes = [C.c_int32]
    lib.hns_policy_packed_bytes.restype = C.c_size_t
    lib.hns_policy_pack.argtypes = [C.POINTER(HnsPolicyNet), C.POINTER(HnsPolicyNet), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.hns_policy_pack.restype = C.c_int
    lib.hns_policy_forward.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(HnsPolicyIo), C.c_int32, C.c_uint64,
                                       C.c_void_p, C.c_void_p]
    lib.hns_policy_forward.restype = C.c_int
    lib.hns_policy_act.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(HnsPolicyIo), C.c_void_p]
    lib.hns_policy_act.restype = C.c_int
    # one actor per agent (include/hns.h; hns_amd.policy.PerAgentDevicePolicy, actor_train.policy_loss_and_grad_per_agent)
    lib.hns_policy_packed_agents_bytes.argtypes = [C.c_int32, C.c_int32]
    lib.hns_policy_packed_agents_bytes.restype = C.c_size_t
    lib.hns_policy_pack_agents.argtypes = lib.hns_policy_pack.argtypes
    lib.hns_policy_pack_agents.restype = C.c_int
    lib.hns_policy_forward_agents.argtypes = lib.hns_policy_forward.argtypes
    lib.hns_policy_forward_agents.restype = C.c_int
    lib.hns_policy_act_agents.argtypes = lib.hns_policy_act.argtypes
    lib.hns_policy_act_agents.restype = C.c_int
    # the centralised critic (include/hns.h; hns_amd.policy.CentralCriticDevicePolicy, critic_train.update_critic_central)
    lib.hns_policy_packed_central_bytes.argtypes = [C.c_int32, C.c_int32]
    lib.hns_policy_packed_central_bytes.restype = C.c_size_t
    lib.hns_policy_pack_central.argtypes = lib.hns_policy_pack.argtypes
    lib.hns_policy_pack_central.restype = C.c_int
    lib.hns_policy_central_forward.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(HnsPolicyIo), C.POINTER(HnsPolicyState),
                                               C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.hns_policy_central_forward.restype = C.c_int
    # one actor per agent beside the centralised critic (include/hns.h; hns_amd.policy.PerAgentCentralCriticDevicePolicy)
    lib.hns_policy_packed_central_agents_bytes.argtypes = [C.c_int32, C.c_int32]
    lib.hns_policy_packed_central_agents_bytes.restype = C.c_size_t
    lib.hns_policy_pack_central_agents.argtypes = lib.hns_policy_pack.argtypes
    lib.hns_policy_pack_central_agents.restype = C.c_int
    lib.hns_policy_central_forward_agents.argtypes = lib.hns_policy_central_forward.argtypes
    lib.hns_policy_central_forward_agents.restype = C.c_int
    lib.hns_critic_train_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32]
    lib.hns_critic_train_workspace_bytes.restype = C.c_size_t
    lib.hns_critic_train_grad.argtypes = [C.POINTER(HnsPolicyNet), C.POINTER(HnsCriticBatch), C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32,
                                          C.c_float, C.POINTER(HnsPolicyNet), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                          C.c_void_p]
    lib.hns_critic_train_grad.restype = C.c_int
    lib.hns_critic_train_central_workspace_bytes.argtypes = lib.hns_critic_train_workspace_bytes.argtypes
    lib.hns_critic_train_central_workspace_bytes.restype = C.c_size_t
    lib.hns_critic_train_grad_central.argtypes = lib.hns_critic_train_grad.argtypes
    lib.hns_critic_train_grad_central.restype = C.c_int
    lib.hns_actor_train_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32]
    lib.hns_actor_train_workspace_bytes.restype = C.c_size_t
    lib.hns_actor_train_grad.argtypes = [C.POINTER(HnsPolicyNet), C.POINTER(HnsActorBatch), C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                         C.POINTER(HnsPolicyNet), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.c_void_p]
    lib.hns_actor_train_grad.restype = C.c_int
    lib.hns_actor_train_agents_workspace_bytes.argtypes = lib.hns_actor_train_workspace_bytes.argtypes
    lib.hns_actor_train_agents_workspace_bytes.restype = C.c_size_t
    lib.hns_actor_train_grad_agents.argtypes = lib.hns_actor_train_grad.argtypes
    lib.hns_actor_train_grad_agents.restype = C.c_int
    # the data-parallel learner's entries (include/hns.h)
    lib.hns_critic_train_sums.argtypes = [C.POINTER(HnsPolicyNet), C.POINTER(HnsCriticBatch), C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32,
                                          C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.hns_critic_train_sums.restype = C.c_int
    lib.hns_critic_train_grad_global.argtypes = lib.hns_critic_train_grad.argtypes + [C.c_void_p, C.c_int64]
    lib.hns_critic_train_grad_global.restype = C.c_int
    lib.hns_actor_train_grad_global.argtypes = lib.hns_actor_train_grad.argtypes + [C.c_int64, C.c_double]
    lib.hns_actor_train_grad_global.restype = C.c_int
    lib.hns_actor_train_grad_agents_global.argtypes = lib.hns_actor_train_grad_global.argtypes     # one actor per agent, data-parallel
    lib.hns_actor_train_grad_agents_global.restype = C.c_int
    # the encoder as a differentiable op (include/hns.h; hns_amd.encoder)
    lib.hns_encoder_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.hns_encoder_workspace_bytes.restype = C.c_size_t
    lib.hns_encoder_forward.argtypes = [C.POINTER(HnsPolicyNet), C.POINTER(HnsCriticBatch), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                        C.c_size_t, C.c_void_p]
    lib.hns_encoder_forward.restype = C.c_int
    lib.hns_encoder_backward.argtypes = [C.POINTER(HnsPolicyNet), C.POINTER(HnsCriticBatch), C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                         C.POINTER(HnsPolicyNet), C.c_void_p, C.c_size_t, C.c_void_p]
    lib.hns_encoder_backward.restype = C.c_int
    # the encoder op on the stacked tensors
    lib.hns_encoder_agents_workspace_bytes.argtypes = lib.hns_encoder_workspace_bytes.argtypes
    lib.hns_encoder_agents_workspace_bytes.restype = C.c_size_t
    lib.hns_encoder_forward_agents.argtypes = lib.hns_encoder_forward.argtypes
    lib.hns_encoder_forward_agents.restype = C.c_int
    lib.hns_encoder_backward_agents.argtypes = lib.hns_encoder_backward.argtypes
    lib.hns_encoder_backward_agents.restype = C.c_int
    # the GRU as a differentiable op (include/hns.h; hns_amd.rnn)
    lib.hns_gru_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32]
    lib.hns_gru_workspace_bytes.restype = C.c_size_t
    lib.hns_gru_forward.argtypes = [C.POINTER(HnsGruNet), C.POINTER(HnsGruSeq), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.hns_gru_forward.restype = C.c_int
    lib.hns_gru_backward.argtypes = [C.POINTER(HnsGruNet), C.POINTER(HnsGruSeq), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(HnsGruNet), C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.hns_gru_backward.restype = C.c_int
    # one GRU per agent: the same calls on tensors stacked over seq.inner
    lib.hns_gru_agents_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int32, C.c_int32]
    lib.hns_gru_agents_workspace_bytes.restype = C.c_size_t
    lib.hns_gru_forward_agents.argtypes = lib.hns_gru_forward.argtypes
    lib.hns_gru_forward_agents.restype = C.c_int
    lib.hns_gru_backward_agents.argtypes = lib.hns_gru_backward.argtypes
    lib.hns_gru_backward_agents.restype = C.c_int
    # the recurrent update's head and loss (include/hns.h; hns_amd.rnn_train)
    for fn in (lib.hns_rnn_actor_head_workspace_bytes, lib.hns_rnn_critic_head_workspace_bytes, lib.hns_rnn_actor_head_agents_workspace_bytes):
        fn.argtypes = [C.c_int64, C.c_int32, C.c_int32]
        fn.restype = C.c_size_t
    lib.hns_rnn_actor_head_grad.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(HnsRnnRows), C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                            C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_size_t, C.c_void_p]
    lib.hns_rnn_actor_head_grad.restype = C.c_int
    lib.hns_rnn_actor_head_grad_agents.argtypes = lib.hns_rnn_actor_head_grad.argtypes          # one head per agent
    lib.hns_rnn_actor_head_grad_agents.restype = C.c_int
    lib.hns_rnn_critic_head_grad.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(HnsRnnRows), C.c_void_p, C.c_void_p, C.c_float, C.c_int32, C.c_float,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.hns_rnn_critic_head_grad.restype = C.c_int
    # their global forms: the local entries' arguments, then (sums, global_rows) / (global_rows, entropy_share)
    lib.hns_rnn_critic_head_sums.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(HnsRnnRows), C.c_void_p, C.c_void_p, C.c_float, C.c_int32, C.c_float,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.hns_rnn_critic_head_sums.restype = C.c_int
    lib.hns_rnn_critic_head_grad_global.argtypes = lib.hns_rnn_critic_head_grad.argtypes + [C.c_void_p, C.c_int64]
    lib.hns_rnn_critic_head_grad_global.restype = C.c_int
    lib.hns_rnn_actor_head_grad_global.argtypes = lib.hns_rnn_actor_head_grad.argtypes + [C.c_int64, C.c_double]
    lib.hns_rnn_actor_head_grad_global.restype = C.c_int
    lib.hns_rnn_actor_head_grad_agents_global.argtypes = lib.hns_rnn_actor_head_grad_global.argtypes   # one head per agent, data-parallel (§7.19)
    lib.hns_rnn_actor_head_grad_agents_global.restype = C.c_int
    lib.hns_grad_norm_workspace_bytes.argtypes = [C.c_longlong]
    lib.hns_grad_norm_workspace_bytes.restype = C.c_size_t
    lib.hns_grad_norm.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.hns_grad_norm.restype = C.c_int
    lib.hns_adam_clipped.argtypes = [C.POINTER(HnsAdamTensor), C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double,
                                     C.c_double, C.c_void_p]
    lib.hns_adam_clipped.restype = C.c_int
    lib.hns_learner_info_workspace_bytes.argtypes = [C.c_longlong]
    lib.hns_learner_info_workspace_bytes.restype = C.c_size_t
    lib.hns_learner_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_size_t, C.c_void_p]
    lib.hns_learner_info.restype = C.c_int
    lib.hns_policy_rnn_packed_bytes.argtypes = []
    lib.hns_policy_rnn_packed_bytes.restype = C.c_size_t
    lib.hns_policy_rnn_pack.argtypes = [C.POINTER(HnsGruNet), C.POINTER(HnsGruNet), C.c_void_p, C.c_void_p]
    lib.hns_policy_rnn_pack.restype = C.c_int
    lib.hns_policy_forward_rnn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(HnsPolicyIo),
                                           C.POINTER(HnsPolicyRnnIo), C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.hns_policy_forward_rnn.restype = C.c_int
    lib.hns_policy_act_rnn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(HnsPolicyIo),
                                       C.POINTER(HnsPolicyRnnIo), C.c_void_p]
    lib.hns_policy_act_rnn.restype = C.c_int
    lib.hns_policy_rnn_packed_agents_bytes.argtypes = [C.c_int32]
    lib.hns_policy_rnn_packed_agents_bytes.restype = C.c_size_t
    lib.hns_policy_rnn_pack_agents.argtypes = [C.POINTER(HnsGruNet), C.POINTER(HnsGruNet), C.c_int32, C.c_void_p, C.c_void_p]
    lib.hns_policy_rnn_pack_agents.restype = C.c_int
    lib.hns_policy_forward_rnn_agents.argtypes = lib.hns_policy_forward_rnn.argtypes
    lib.hns_policy_forward_rnn_agents.restype = C.c_int
    lib.hns_policy_act_rnn_agents.argtypes = lib.hns_policy_act_rnn.argtypes
    lib.hns_policy_act_rnn_agents.restype = C.c_int
    lib.hns_rollout_store.argtypes = [C.POINTER(HnsRolloutSegment), C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]
    lib.hns_rollout_store.restype = C.c_int
    lib.hns_eval_means.argtypes = [C.POINTER(HnsEvalRow), C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hns_eval_means.restype = C.c_int
    lib.hns_set_state.argtypes = [C.c_void_p, C.POINTER(HnsBuffers), C.c_void_p]
    lib.hns_set_state.restype = C.c_int
    lib.hns_get_state.argtypes = [C.c_void_p, C.POINTER(HnsBuffers), C.c_void_p]
    lib.hns_get_state.restype = C.c_int
    lib.hns_refresh_derived_state.argtypes = [C.c_void_p, C.c_void_p]
    lib.hns_refresh_derived_state.restype = C.c_int
    lib.hns_fps_scratch_bytes.argtypes = []
    lib.hns_fps_scratch_bytes.restype = C.c_size_t
    lib.hns_fps.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hns_fps.restype = C.c_int
    lib.hns_perturb_tasks.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_uint64, C.c_void_p]
    lib.hns_perturb_tasks.restype = C.c_int
    lib.hns_abi_version.argtypes = []
    lib.hns_abi_version.restype = C.c_int
    lib.hns_cfg_size.argtypes = []
    lib.hns_cfg_size.restype = C.c_size_t
    lib.hns_last_error.argtypes = []
    lib.hns_last_error.restype = C.c_char_p
    if lib.hns_abi_version() != HNS_ABI_VERSION:
        raise RuntimeError("libhns.so ABI version mismatch")
    if lib.hns_tp_packed_bytes() != TP_PACKED_BYTES:
        raise RuntimeError("hns_tp_packed_bytes() differs from abi.TP_PACKED_BYTES")
    if lib.hns_cfg_size() != C.sizeof(HnsCfg):
        raise RuntimeError("hns_cfg layout mismatch between include/hns.h and abi.py")
    _LIB = lib
    return lib


def check(rc, what):
    """Raise with hns_last_error's text unless `rc` is HNS_OK."""
    if rc != HNS_OK:
        raise RuntimeError(f"{what} failed ({rc}): {load_library().hns_last_error().decode()}")


EXPORTED_SYMBOLS = [
    "hns_create", "hns_destroy", "hns_bind", "hns_step", "hns_reset", "hns_reset_tasks", "hns_raycast", "hns_set_v_prey",
    "hns_set_smoothness_coef", "hns_set_reset_epoch", "hns_get_reset_epoch", "hns_enable_timing",
    "hns_step_kernel_ms", "hns_region_begin", "hns_region_end", "hns_region_ms", "hns_copy_f4", "hns_moments", "hns_rollout_moments", "hns_gae", "hns_rollout_normalise", "hns_clock_probe", "hns_set_phase_profile", "hns_step_mapping", "hns_selected_kernels", "hns_set_state", "hns_get_state", "hns_refresh_derived_state", "hns_fps", "hns_fps_scratch_bytes", "hns_perturb_tasks", "hns_tp_bind", "hns_tp_refresh", "hns_tp_packed_bytes", "hns_tp_observe", "hns_tp_train_workspace_bytes", "hns_tp_train_grad", "hns_tp_adam", "hns_policy_packed_bytes", "hns_policy_pack", "hns_policy_forward", "hns_policy_act", "hns_critic_train_workspace_bytes", "hns_critic_train_grad", "hns_actor_train_workspace_bytes", "hns_actor_train_grad", "hns_critic_train_sums", "hns_critic_train_grad_global", "hns_actor_train_grad_global", "hns_grad_norm_workspace_bytes", "hns_grad_norm", "hns_adam_clipped", "hns_learner_info_workspace_bytes", "hns_learner_info", "hns_rollout_store", "hns_eval_means", "hns_encoder_workspace_bytes", "hns_encoder_forward", "hns_encoder_backward", "hns_gru_workspace_bytes", "hns_gru_forward", "hns_gru_backward", "hns_policy_rnn_packed_bytes", "hns_policy_rnn_pack", "hns_policy_forward_rnn", "hns_policy_act_rnn", "hns_rnn_actor_head_workspace_bytes", "hns_rnn_critic_head_workspace_bytes", "hns_rnn_actor_head_grad", "hns_rnn_critic_head_grad", "hns_rnn_critic_head_sums", "hns_rnn_critic_head_grad_global", "hns_rnn_actor_head_grad_global", "hns_policy_packed_agents_bytes", "hns_policy_pack_agents", "hns_policy_forward_agents", "hns_policy_act_agents", "hns_actor_train_agents_workspace_bytes", "hns_actor_train_grad_agents", "hns_policy_rnn_packed_agents_bytes", "hns_policy_rnn_pack_agents", "hns_policy_forward_rnn_agents", "hns_policy_act_rnn_agents", "hns_gru_agents_workspace_bytes", "hns_gru_forward_agents", "hns_gru_backward_agents", "hns_encoder_agents_workspace_bytes", "hns_encoder_forward_agents", "hns_encoder_backward_agents", "hns_rnn_actor_head_agents_workspace_bytes", "hns_rnn_actor_head_grad_agents", "hns_actor_train_grad_agents_global", "hns_rnn_actor_head_grad_agents_global", "hns_policy_packed_central_bytes", "hns_policy_pack_central", "hns_policy_central_forward", "hns_critic_train_central_workspace_bytes", "hns_critic_train_grad_central", "hns_policy_packed_central_agents_bytes", "hns_policy_pack_central_agents", "hns_policy_central_forward_agents", "hns_hover_step", "hns_hover_reset", "hns_abi_version", "hns_cfg_size", "hns_last_error",
]
