"""The contact response's CPU restatement (tests/contact_reference.py): the composed step is the oracle's step when the contact stages are the
identity, the stages keep their promises on constructed scenes, and the configuration carries the model's constants (include/hns.h).
CPU only."""
import os

import numpy as np
import pytest

import contact_reference as CR
import hns_oracle as O
from hns_amd import abi, config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _cfg(E, A, C, max_len=9, **task):
    cyl = {"max_num": C, "obs_max_cylinder": 3, "min_num": min(4, C)}
    cyl.update(task.pop("cylinder", {}))
    return config.resolve_hns_cfg(config.make_cfg({"num_agents": A, "cylinder": cyl, "env": {"num_envs": E, "max_episode_length": max_len}, **task}))


def _same(a, b, what):
    for k in a:
        if a[k] is None:
            continue
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: buffer {k}")


IDENTITY_CASES = [
    dict(E=40, A=3, C=8),
    dict(E=33, A=1, C=5),
    dict(E=20, A=7, C=16, cylinder={"min_num": 16}),
    dict(E=24, A=3, C=5, cylinder={"fixed_num": 0}),
    dict(E=30, A=3, C=8, action_input="motor"),
    dict(E=16, A=4, C=6, use_deployment=1, init_smoothness_coef=2.0, pid_reset="on_reset"),
]


@pytest.mark.parametrize("case", IDENTITY_CASES, ids=lambda c: f"A{c['A']}C{c['C']}" + ("motor" if "action_input" in c else ""))
def test_composed_step_with_identity_stages_is_the_oracle_step(case):
    case = dict(case)
    c = _cfg(case.pop("E"), case.pop("A"), case.pop("C"), **case)
    E, A = c.num_envs, c.num_agents
    ref = O.alloc_buffers(c)
    O.reset(c, ref, None, 77, 0)
    mine = {k: v.copy() for k, v in ref.items()}
    rng = np.random.default_rng(3)
    fired = False
    for t in range(20):
        if c.action_input == abi.HNS_ACTION_MOTOR:
            act = rng.random((E, A, 4), dtype=np.float32) * 2 - 1
            ae = rng.random((E, A), dtype=np.float32)
            ref["action_error"][:] = ae
            mine["action_error"][:] = ae
        else:
            act = (rng.standard_normal((E, A, 4)) * 0.8).astype(np.float32)
        O.step(c, ref, act)
        CR.composed_step(c, mine, act, stages=CR.identity)
        _same(ref, mine, f"step {t}")
        if ref["done"].any():
            fired = True
            mask = ref["done"].copy()
            O.reset(c, ref, mask, 77, t + 1)
            O.reset(c, mine, mask, 77, t + 1)
    assert fired


def _rd(c):
    return CR.constants(c)


def test_isolated_cylinder_contact_ends_outside_and_not_inward():
    c = _cfg(1, 1, 5)
    k = _rd(c)
    rng = np.random.default_rng(5)
    n = 4000
    cyl = np.zeros((n, 5, 3), f32)
    cyl[:, :, 2] = -20.0                                                     # inactive slots
    cyl[:, 2] = [0.1, -0.2, 0.6]
    ang = rng.uniform(0, 2 * np.pi, n)
    rad = rng.uniform(0.0, 0.2, n)
    p = np.stack([0.1 + rad * np.cos(ang), -0.2 + rad * np.sin(ang), rng.uniform(0.0, 1.1, n)], -1).astype(f32)
    v = rng.uniform(-2, 2, (n, 3)).astype(f32)
    p2, v2 = CR.cylinders(c, p, v, cyl, k["rd"], k["rd2"])
    dx, dy = p2[:, 0] - f32(0.1), p2[:, 1] - f32(-0.2)
    dxy = np.sqrt(dx.astype(np.float64) ** 2 + dy.astype(np.float64) ** 2)
    inside = rad < float(k["rd"])
    assert inside.sum() > 1000
    assert (dxy[inside] >= float(k["rd"]) - 1e-6).all()
    radial = (v2[:, 0] * dx + v2[:, 1] * dy) / dxy
    assert (radial[inside] >= -1e-6).all()
    assert np.array_equal(p2[~inside], p[~inside]) and np.array_equal(v2[~inside], v[~inside])
    above = p.copy()
    above[:, 2] = f32(c.cylinder_height) + 0.01                              # above the top: no contact
    p3, _ = CR.cylinders(c, above, v, cyl, k["rd"], k["rd2"])
    assert np.array_equal(p3, above)


def test_isolated_pair_ends_in_contact_conserving_momentum():
    c = _cfg(1, 2, 5)
    k = _rd(c)
    rng = np.random.default_rng(8)
    n = 4000
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sep = rng.uniform(0.01, 0.099, n)
    p = np.zeros((n, 2, 3), f32)
    p[:, 0] = rng.uniform(-0.5, 0.5, (n, 3))
    p[:, 1] = p[:, 0] + (d * sep[:, None]).astype(f32)
    v = rng.uniform(-2, 2, (n, 2, 3)).astype(f32)
    p2, v2 = CR.pursuer_pairs(c, p, v)
    dist = np.linalg.norm(p2[:, 0].astype(np.float64) - p2[:, 1], axis=1)
    assert np.abs(dist - float(k["dd"])).max() < 1e-6
    nrm = (p2[:, 0].astype(np.float64) - p2[:, 1]) / dist[:, None]
    dv = v2[:, 0].astype(np.float64) - v2[:, 1]
    rel = (dv * nrm).sum(1)
    assert (rel >= -1e-6 * np.maximum(1.0, np.linalg.norm(dv, axis=1))).all()   # (fp32 rounding of velocities up to ~4 m/s)
    assert np.abs(v2.sum(1).astype(np.float64) - v.sum(1)).max() < 1e-6
    ke = lambda w: (w.astype(np.float64) ** 2).sum((1, 2))                  # noqa: E731
    assert (ke(v2) <= ke(v) + 1e-6).all()


def test_bodies_far_from_everything_are_untouched():
    c = _cfg(50, 3, 8)
    arrs = O.alloc_buffers(c)
    O.reset(c, arrs, None, 3, 0)
    ds, tp = arrs["drone_state"].copy(), arrs["target_pos"].copy()
    ds[..., 0:3] = [[0.0, 0.0, 0.5], [0.5, 0.0, 0.5], [0.0, 0.5, 0.5]]
    tp[:] = [-0.5, -0.5, 0.5]
    arrs["cylinders"][:] = [5.0, 5.0, 0.6]
    ds2, tp2 = CR.contact_stages(c, ds, tp, arrs["cylinders"])
    assert np.array_equal(ds2, ds) and np.array_equal(tp2, tp)


def test_task_file_loads_and_two_evaders_are_refused():
    path = os.path.join(ROOT, "cfg", "task", "HideAndSeek_hip_contact.yaml")
    cfg = config.load_cfg(path)
    assert cfg.task.contact_response == 1 and cfg.task.action_transform == "none"
    c = config.resolve_hns_cfg(cfg, num_envs=64)
    assert c.contact_response == 1 and c.action_input == abi.HNS_ACTION_POLICY
    base = config.resolve_hns_cfg(config.load_cfg(os.path.join(ROOT, "cfg", "task", "HideAndSeek_hip.yaml")), num_envs=64)
    assert base.contact_response == 0
    with pytest.raises(ValueError, match="two-evader"):
        config.load_cfg(path, num_targets=2)
    with pytest.raises(ValueError, match="contact_response"):
        config.make_cfg({"contact_response": 2})
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            config.make_cfg({"contact_response": 1, "contact_drone_radius": bad})
        with pytest.raises(ValueError):
            config.make_cfg({"contact_response": 1, "contact_target_radius": bad})


def test_hns_cfg_carries_the_derived_constants():
    c = _cfg(8, 3, 5, contact_response=1, contact_drone_radius=0.05, contact_target_radius=0.07)
    assert c.contact_response == 1
    assert f32(c.contact_drone_radius) == f32(0.05) and f32(c.contact_target_radius) == f32(0.07)
    D = f32(2 * 0.05)
    Rd, Rt = f32(0.1 + 0.05), f32(0.1 + 0.07)
    assert f32(c.contact_dd) == D and f32(c.contact_dd2) == f32(D * D)
    assert f32(c.contact_rd) == Rd and f32(c.contact_rd2) == f32(Rd * Rd)
    assert f32(c.contact_rt) == Rt and f32(c.contact_rt2) == f32(Rt * Rt)
    assert list(c.contact_pad) == [0] * 7
    off = _cfg(8, 3, 5)
    assert off.contact_response == 0
    # the defaults keep every contact a penalised one (hideandseek.py:961-985)
    assert float(off.contact_rd) - 0.1 < float(off.collision_radius) and float(off.contact_dd) < 2 * float(off.collision_radius)
