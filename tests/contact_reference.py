"""numpy float32 restatement of the contact response (include/hns.h) and the composed reference step the HIP contact kernel is
checked against (test infrastructure, imported by tests/test_contact_reference.py and tests/test_hip_contact.py).

Every operation is one IEEE fp32 operation in the order the model states (numpy float32 arrays: no FMA, correctly rounded sqrt and /), so the
stages match the kernel bit for bit.  The composed step:
  1. the CPU oracle's step with the contact response off, on a copy of the state, with max_episode_length = 2^30 (nothing in front of the reward
     reads it, and the statistics rows the step writes before the reward stay un-divided);
  2. the contact stages on its drone_state and target_pos;
  3. observation, line of sight, reward, done and statistics recomputed on that state by the oracle's obs_reward, from the statistics as they
     stood before the reward (action error rows and out_of_arena from step 1, everything else from the state the step started at).
The throttle difference the reward statistics need comes from the oracle's controller and rotor stages on the starting state."""
import numpy as np

import hns_oracle as O
from hns_amd import abi

f32 = np.float32
ST = {n: i for i, n in enumerate(abi.STAT_NAMES)}
PRE_REWARD_ROWS = (ST["action_error_order1_mean"], ST["action_error_order1_max"], ST["out_of_arena"])


def constants(cfg):
    return {k: f32(getattr(cfg, "contact_" + k)) for k in ("dd", "dd2", "rd", "rd2", "rt", "rt2")}


def pursuer_pairs(cfg, p, v):
    """Stage 1: one Jacobi pass.  p, v: [E, A, 3] float32 (integrated).  Returns new arrays."""
    k = constants(cfg)
    D, D2 = k["dd"], k["dd2"]
    E, A, _ = p.shape
    pn, vn_ = p.copy(), v.copy()
    with np.errstate(all="ignore"):
        for a in range(A):
            cp, cv = np.zeros((E, 3), f32), np.zeros((E, 3), f32)
            for j in range(A):
                if j == a:
                    continue
                d = p[:, a] - p[:, j]
                d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                m = (d2 < D2) & (d2 > f32(0))
                r = np.sqrt(np.where(m, d2, f32(1)))
                inv = f32(1) / r
                n = d * inv[:, None]
                h = (D - r) * f32(0.5)
                cp = np.where(m[:, None], cp + h[:, None] * n, cp)
                dv = v[:, a] - v[:, j]
                vn = (dv[:, 0] * n[:, 0] + dv[:, 1] * n[:, 1]) + dv[:, 2] * n[:, 2]
                g = -(vn * f32(0.5))
                cv = np.where((m & (vn < f32(0)))[:, None], cv + g[:, None] * n, cv)
            pn[:, a] = p[:, a] + cp
            vn_[:, a] = v[:, a] + cv
    return pn, vn_


def cylinders(cfg, p, v, cyl, R, R2):
    """Stages 2 / 4: bodies p [N, 3] (v [N, 3] or None: position only) against their cylinder rows cyl [N, C, 3].  Returns new arrays."""
    p = p.copy()
    v = None if v is None else v.copy()
    ch = f32(cfg.cylinder_height)
    with np.errstate(all="ignore"):
        for k in range(cyl.shape[1]):
            cx, cy, cz = cyl[:, k, 0], cyl[:, k, 1], cyl[:, k, 2]
            dx, dy = p[:, 0] - cx, p[:, 1] - cy
            d2 = dx * dx + dy * dy
            m = ~(cz < f32(0)) & (p[:, 2] < ch) & (d2 < R2) & (d2 > f32(0))
            r = np.sqrt(np.where(m, d2, f32(1)))
            inv = f32(1) / r
            nx, ny = dx * inv, dy * inv
            p[:, 0] = np.where(m, cx + nx * R, p[:, 0])
            p[:, 1] = np.where(m, cy + ny * R, p[:, 1])
            if v is not None:
                vn = v[:, 0] * nx + v[:, 1] * ny
                mv = m & (vn < f32(0))
                v[:, 0] = np.where(mv, v[:, 0] - vn * nx, v[:, 0])
                v[:, 1] = np.where(mv, v[:, 1] - vn * ny, v[:, 1])
    return p, v


def ground(cfg, p, v):
    """Stage 3: the integrator's ground clamp again."""
    if not cfg.ground_clamp:
        return p, v
    p, v = p.copy(), v.copy()
    m = p[..., 2] < f32(0)
    p[..., 2] = np.where(m, f32(0), p[..., 2])
    v[..., 2] = np.where(m & (v[..., 2] < f32(0)), f32(0), v[..., 2])
    return p, v


def contact_stages(cfg, drone_state, target_pos, cyl):
    """Stages 1-4 on S_{t+1} as the integrator left it.  Returns (drone_state, target_pos), new arrays."""
    k = constants(cfg)
    E, A, _ = drone_state.shape
    ds = drone_state.copy()
    p, v = pursuer_pairs(cfg, ds[..., 0:3], ds[..., 7:10])
    cylA = np.repeat(cyl, A, axis=0)
    p2, v2 = cylinders(cfg, p.reshape(E * A, 3), v.reshape(E * A, 3), cylA, k["rd"], k["rd2"])
    p, v = ground(cfg, p2.reshape(E, A, 3), v2.reshape(E, A, 3))
    ds[..., 0:3], ds[..., 7:10] = p, v
    tp, _ = cylinders(cfg, target_pos.reshape(E, 3), None, cyl, k["rt"], k["rt2"])
    return ds, tp.reshape(target_pos.shape)


def identity(cfg, drone_state, target_pos, cyl):
    return drone_state.copy(), target_pos.copy()


def throttle_difference(cfg, arrs, action):
    """[E, A] throttle difference of the rotor stage on the state the step starts at (hideandseek.py:735-737 statistics input)."""
    E, A = cfg.num_envs, cfg.num_agents
    ds = arrs["drone_state"].reshape(E * A, 13)
    if cfg.action_input == abi.HNS_ACTION_MOTOR:
        cmd = np.asarray(action, f32).reshape(E * A, 4)
    else:
        if "reset_pid" in arrs:
            rp = arrs["reset_pid"]
        else:
            rp = None if cfg.pid_reset_on_reset else arrs["done"]
        mask = None if rp is None else np.repeat(np.asarray(rp, np.uint8), A)
        out = O.ctbr_pid(cfg, np.asarray(action, f32).reshape(E * A, 4), ds[:, 3:7], ds[:, 10:13], mask,
                         arrs["prev_action"].reshape(E * A, 4), arrs["pid_integ"].reshape(E * A, 4)[:, :3],
                         arrs["pid_last_rate"].reshape(E * A, 4)[:, :3])
        cmd = out["cmd"]
    _, _, _, td = O.rotor(cfg, cmd, arrs["throttle"].reshape(E * A, 4))
    return td.reshape(E, A)


def _nonfinite_bits(ds, tp, reward):
    bad = 0
    s = ds[..., 0].copy()
    for i in range(1, 13):
        s = s + ds[..., i]
    with np.errstate(all="ignore"):
        if ((s - s) != 0).any():
            bad |= 1
        t = (tp[:, 0] + tp[:, 1]) + tp[:, 2]
        if ((t - t) != 0).any():
            bad |= 2
        r = reward[:, 0].copy()
        for a in range(1, reward.shape[1]):
            r = r + reward[:, a]
        if ((r - r) != 0).any():
            bad |= 4
    return bad


def composed_step(cfg, arrs, action, stages=contact_stages):
    """One step with the contact response, in place on `arrs` (the oracle's buffers), as the HIP contact kernel computes it."""
    assert cfg.num_targets != 2
    start = {k: (v.copy() if v is not None else None) for k, v in arrs.items()}
    td = throttle_difference(cfg, start, action)
    big = cfg.copy()
    big.max_episode_length = 1 << 30
    O.step(big, arrs, action)                                     # contact off; `arrs` now holds S_{t+1} before contact
    ds, tp = stages(cfg, arrs["drone_state"], arrs["target_pos"], arrs["cylinders"])
    arrs["drone_state"][:] = ds
    arrs["target_pos"][:] = tp
    stats = start["stats"].copy()
    for r in PRE_REWARD_ROWS:
        stats[r] = arrs["stats"][r]
    arrs["stats"][:] = stats
    critic = arrs["state_drones"].copy()
    blocked, bdet, _ = O.obs_reward(cfg, arrs, thr_diff=td, do_reward=True)
    if not cfg.write_critic_state:
        arrs["state_drones"][:] = critic
    arrs["pid_last_rate"][..., 3] = blocked.astype(f32)
    if arrs.get("detect") is not None:
        arrs["detect"][:] = bdet.astype(np.uint8)
    arrs["nonfinite"][:] = start["nonfinite"] | _nonfinite_bits(arrs["drone_state"], arrs["target_pos"], arrs["reward"])
