"""The contact response on the GPU (task.contact_response = 1; include/hns.h): the HIP contact kernels against the composed CPU
reference (tests/contact_reference.py) bit for bit on every buffer, in scenes dense with contacts, over episode boundaries; the model's
properties; kernel choice and refusals; graph capture and snapshot resume."""
import ctypes as C

import numpy as np
import pytest
import torch

import contact_reference as CR
import hns_oracle as O
from hns_amd import abi, config

pytestmark = pytest.mark.gpu
f32 = np.float32


def make_env(E, A, C_, max_len=40, K=3, contact=1, **task):
    from hns_amd.env import HideAndSeek
    cyl = {"max_num": C_, "obs_max_cylinder": K, "min_num": min(4, C_)}
    cyl.update(task.pop("cylinder", {}))
    cfg = config.make_cfg({"num_agents": A, "cylinder": cyl, "env": {"num_envs": E, "max_episode_length": max_len},
                           "contact_response": contact, **task})
    return HideAndSeek(cfg, headless=True, write_critic_state=True)


def assert_same(host, dev, what=""):
    for k in host:
        if host[k] is None or (k == "state_drones" and not host[k].size):
            continue
        np.testing.assert_array_equal(host[k], dev[k], err_msg=f"{what}: buffer {k}")


def dense_scene(st, rng):
    """Pursuer 0 next to or inside the annulus of an active cylinder, pursuer 1 next to or inside pursuer 0's contact sphere, the others
    near them, the evader next to or inside another cylinder's annulus; velocities toward each other."""
    ds, cyl = st["drone_state"], st["cylinders"]
    E, A, _ = ds.shape
    act = cyl[..., 2] >= 0
    k0 = np.where(act.any(1), np.argmax(act * rng.random(act.shape), 1), -1)
    k1 = np.where(act.any(1), np.argmax(act * rng.random(act.shape), 1), -1)
    ang = rng.uniform(0, 2 * np.pi, E)
    rad = rng.uniform(0.05, 0.22, E)
    base = np.where((k0 >= 0)[:, None], cyl[np.arange(E), np.maximum(k0, 0), :2], rng.uniform(-0.5, 0.5, (E, 2)))
    p0 = np.stack([base[:, 0] + rad * np.cos(ang), base[:, 1] + rad * np.sin(ang), rng.uniform(0.05, 1.0, E)], -1)
    ds[:, 0, 0:3] = p0
    for a in range(1, A):
        d = rng.standard_normal((E, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        ds[:, a, 0:3] = ds[:, a - 1, 0:3] + d * rng.uniform(0.02, 0.14, (E, 1))
    ds[..., 2] = np.clip(ds[..., 2], 0.0, 1.1)
    ds[..., 7:10] = rng.uniform(-1.0, 1.0, (E, A, 3))
    ds[:, 0, 7:9] = (base - p0[:, :2]) * 5.0                                  # pursuer 0 flies into its cylinder
    tb = np.where((k1 >= 0)[:, None], cyl[np.arange(E), np.maximum(k1, 0), :2], rng.uniform(-0.5, 0.5, (E, 2)))
    ang = rng.uniform(0, 2 * np.pi, E)
    rad = rng.uniform(0.05, 0.2, E)
    st["target_pos"][:] = np.stack([tb[:, 0] + rad * np.cos(ang), tb[:, 1] + rad * np.sin(ang), rng.uniform(0.1, 1.0, E)], -1)
    return st


def run_parity(env, steps=200, seed=0, motor=False, inject_every=50):
    c = env.hcfg
    O.set_threads(8 if c.num_envs > 1024 else 1)
    env.set_seed(100 + seed)
    env.reset()
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    E, A = env.num_envs, env.num_agents
    host = None
    for t in range(steps):
        if t % inject_every == 0:
            st = dense_scene(env.export_state(), rng)
            env.import_state(st)
            host = env.export_state()
        if motor:                                                           # rotor commands + the controller transform's keys (include/hns.h)
            from hns_amd.tensordict_shim import TensorDict
            action = torch.rand(E, A, 4, generator=g) * 2 - 1
            pa, ae = torch.rand(E, A, 4, generator=g) * 2 - 1, torch.rand(E, A, generator=g)
            dev = lambda x: x.to(env.device)                                # noqa: E731
            env.step(TensorDict({"agents": {"action": dev(action)}, "info": {"prev_action": dev(pa)}, "stats": {"action_error_order1": dev(ae)},
                                 "done": dev(torch.from_numpy(host["done"].astype(bool))[:, None])}, env.batch_size))
            host["prev_action"][:], host["action_error"][:] = pa.numpy(), ae.numpy()
        else:
            action = torch.randn(E, A, 4, generator=g) * 0.7
            env.step(env.rand_step_input(action.to(env.device)))
        CR.composed_step(c, host, action.numpy())
        assert_same(host, env.export_state(), f"step {t}")
        if host["done"].any():
            mask = host["done"].copy()
            if t % 2:
                mask[::3] = 0
            td = env.rand_step_input()
            td.set("_reset", torch.as_tensor(mask.astype(bool), device=env.device))
            epoch = env.reset_epoch
            env.reset(td)
            O.reset(c, host, mask, env.seed, epoch)
            assert_same(host, env.export_state(), f"reset after step {t}")
    return host


PARITY_CASES = [
    dict(E=256, A=3, C_=8, cylinder={"min_num": 8}),          # tuned, CS = 8
    dict(E=128, A=3, C_=6),                                   # tuned, CS = 0
    dict(E=300, A=3, C_=8),                                   # ragged: generic
    dict(E=128, A=3, C_=8, K=5),                              # wide k: generic
    dict(E=130, A=3, C_=8, action_input="motor"),             # motor input: generic
    dict(E=128, A=7, C_=8, cylinder={"min_num": 8}),          # seven pursuers, CS = 8
    dict(E=65, A=7, C_=12, K=4),                              # seven pursuers, ragged
    dict(E=128, A=1, C_=5),                                   # one pursuer, CS = 5
    dict(E=128, A=3, C_=6, use_random_cylinder=0, scenario_flag="narrow_gap"),   # HNS_INIT_SCENARIO placement
    dict(E=2048, A=3, C_=5),                                  # the reference's default batch: tile mapping (the small one has no contact stages)
]


@pytest.mark.parametrize("case", PARITY_CASES, ids=lambda c: f"E{c['E']}A{c['A']}C{c['C_']}K{c.get('K', 3)}" + ("motor" if "action_input" in c else ""))
def test_contact_kernel_matches_composed_reference(case):
    case = dict(case)
    env = make_env(**case)
    assert env.hcfg.contact_response == 1 and env.step_mapping == "tile"
    run_parity(env, steps=200, motor=case.get("action_input") == "motor")


def test_step_mapping_with_contact(monkeypatch):
    monkeypatch.delenv("HNS_STEP_MAPPING", raising=False)
    assert make_env(E=2048, A=3, C_=5).step_mapping == "tile"
    assert make_env(E=2048, A=3, C_=5, contact=0).step_mapping == "small"
    monkeypatch.setenv("HNS_STEP_MAPPING", "small")
    assert make_env(E=2048, A=3, C_=5).step_mapping == "tile"


def test_two_evaders_with_contact_are_refused():
    with pytest.raises(ValueError, match="two-evader"):
        config.make_cfg({"num_targets": 2, "contact_response": 1})
    c = config.resolve_hns_cfg(config.make_cfg({"num_targets": 2, "env": {"num_envs": 64}}))
    c.contact_response = 1                                                  # past the Python check: the C ABI refuses it too
    lib = abi.load_library()
    h = C.c_void_p()
    assert lib.hns_create(C.byref(c), C.byref(h)) == -1 and not h.value
    c.contact_response, c.num_targets, c.contact_dd = 1, 1, 0.0
    assert lib.hns_create(C.byref(c), C.byref(h)) == -1 and not h.value


def _isolated(env, rng, kind):
    st = env.export_state()
    E = env.num_envs
    ds, cyl = st["drone_state"], st["cylinders"]
    cyl[..., 2] = -20.0
    if kind == "cylinder":
        cyl[:, 0] = [0.0, 0.0, 0.6]
        ang = rng.uniform(0, 2 * np.pi, E)
        rad = rng.uniform(0.05, 0.25, E)
        ds[:, 0, 0:3] = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(0.2, 1.0, E)], -1)
        ds[:, 0, 7:9] = -ds[:, 0, 0:2] * 8.0                                 # straight at the axis
    else:
        ds[:, 0, 0:3] = rng.uniform(-0.3, 0.3, (E, 3)) + [0, 0, 0.6]
        d = rng.standard_normal((E, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        ds[:, 1, 0:3] = ds[:, 0, 0:3] + d * rng.uniform(0.03, 0.2, (E, 1))
        ds[:, 0, 7:10] = d * 2.0                                             # toward each other
        ds[:, 1, 7:10] = -d * 2.0
    st["target_pos"][:] = [-0.7, -0.7, 0.5]
    env.import_state(st)


@pytest.mark.parametrize("kind", ["cylinder", "pair"])
def test_contact_properties_on_gpu(kind):
    """Isolated contacts, 300 steps of flight (full collective thrust every other step) into a cylinder / into each other.  Every step starts a
    contact-off twin from the same state with the same action: an env made contact in that step iff the two results differ."""
    A = 1 if kind == "cylinder" else 2
    on, off = (make_env(E=4096, A=A, C_=5, max_len=10 ** 6, contact=x) for x in (1, 0))
    on.set_seed(9)
    on.reset()
    rng = np.random.default_rng(4)
    k = CR.constants(on.hcfg)
    full = torch.zeros(on.num_envs, A, 4, device=on.device)
    full[..., 3] = 4.0
    touched = 0
    for t in range(300):
        if t % 30 == 0:
            _isolated(on, rng, kind)
        off.import_state(on.export_state())
        act = full if t % 2 else torch.randn(on.num_envs, A, 4, device=on.device)
        on.step(on.rand_step_input(act))
        off.step(off.rand_step_input(act))
        ds = on.export_state()["drone_state"].astype(np.float64)
        hit = (on.export_state()["drone_state"] != off.export_state()["drone_state"]).any((1, 2))
        if kind == "cylinder":
            p, v = ds[:, 0, 0:3], ds[:, 0, 7:10]
            below = p[:, 2] < float(on.hcfg.cylinder_height)
            dxy = np.hypot(p[:, 0], p[:, 1])
            assert (dxy[below] >= float(k["rd"]) - 1e-6).all(), f"step {t}: a pursuer inside the cylinder's contact annulus"
            radial = (p[:, 0] * v[:, 0] + p[:, 1] * v[:, 1]) / dxy
            assert (radial[hit] >= -1e-5).all(), f"step {t}: inward velocity after a contact"
            assert (np.abs(dxy[hit] - float(k["rd"])) < 1e-5).all(), f"step {t}: a contact that did not end on the annulus"
        else:
            d = ds[:, 0, 0:3] - ds[:, 1, 0:3]
            dist = np.linalg.norm(d, axis=1)
            free = ~(ds[:, :, 2] <= 0.0).any(1)                                 # (the ground clamp may move what stage 1 put together)
            assert (dist[free] >= float(k["dd"]) - 1e-6).all(), f"step {t}: a pair closer than the contact distance"
            hit &= free
            rel = ((ds[:, 0, 7:10] - ds[:, 1, 7:10]) * d).sum(1) / dist
            assert (rel[hit] >= -1e-5).all(), f"step {t}: approaching after a contact"
            assert (np.abs(dist[hit] - float(k["dd"])) < 1e-6).all(), f"step {t}: a contact that did not end at the contact distance"
        touched += int(hit.sum())
    assert touched > 1000


def test_one_step_energy_does_not_grow():
    on, off = make_env(E=4096, A=3, C_=8, cylinder={"min_num": 8}), make_env(E=4096, A=3, C_=8, cylinder={"min_num": 8}, contact=0)
    on.set_seed(2)
    on.reset()
    rng = np.random.default_rng(2)
    g = torch.Generator().manual_seed(2)
    for rep in range(5):
        st = dense_scene(on.export_state(), rng)
        on.import_state(st)
        off.import_state(st)
        act = (torch.randn(4096, 3, 4, generator=g) * 0.7).to(on.device)
        on.step(on.rand_step_input(act))
        off.step(off.rand_step_input(act))
        ke = lambda e: (e.export_state()["drone_state"][..., 7:10].astype(np.float64) ** 2).sum((1, 2))   # noqa: E731
        k_on, k_off = ke(on), ke(off)
        assert (k_on <= k_off * (1 + 1e-6) + 1e-9).all()
        assert (k_on < k_off).sum() > 100


def test_far_from_everything_contact_changes_nothing():
    on, off = make_env(E=2048, A=3, C_=5), make_env(E=2048, A=3, C_=5, contact=0)
    on.set_seed(6)
    on.reset()
    st = on.export_state()
    st["drone_state"][..., 0:3] = [[0.4, 0.0, 0.6], [-0.3, 0.4, 0.6], [-0.3, -0.4, 0.6]]
    st["drone_state"][..., 7:13] = 0.0
    st["target_pos"][:] = [0.0, 0.0, 0.6]
    st["cylinders"][:] = [3.0, 3.0, 0.6]
    on.import_state(st)
    off.import_state(st)
    g = torch.Generator().manual_seed(6)
    for t in range(10):
        act = (torch.randn(2048, 3, 4, generator=g) * 0.3).to(on.device)
        on.step(on.rand_step_input(act))
        off.step(off.rand_step_input(act))
    assert_same(off.export_state(), on.export_state(), "contact on vs off, far from everything")


def test_graph_replay_with_contact():
    E, A, steps, replays = 4096, 3, 4, 3
    envs = [make_env(E, A, 8, max_len=1000) for _ in range(2)]
    rng = np.random.default_rng(1)
    for env in envs:
        env.set_seed(5)
        env.reset()
    st = dense_scene(envs[0].export_state(), rng)
    for env in envs:
        env.import_state(st)
    act = torch.randn(E, A, 4, device=envs[0].device)
    eager, graphed = envs
    for _ in range(steps * replays):
        assert eager._lib.hns_step(eager._env, act.data_ptr(), eager._stream()) == 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            for _ in range(steps):
                assert graphed._lib.hns_step(graphed._env, act.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for _ in range(replays):
        graph.replay()
    torch.cuda.synchronize()
    a, b = eager.export_state(), graphed.export_state()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_snapshot_resume_with_contact(tmp_path):
    a = make_env(200, 3, 8, max_len=7)
    a.set_seed(5)
    a.reset()
    a.import_state(dense_scene(a.export_state(), np.random.default_rng(3)))
    g = torch.Generator().manual_seed(1)
    acts = [torch.randn(200, 3, 4, generator=g) for _ in range(12)]
    for t in range(5):
        a.step(a.rand_step_input(acts[t].to(a.device)))
    a.save_state(str(tmp_path / "snap.npz"))
    b = make_env(200, 3, 8, max_len=7)
    b.load_state(str(tmp_path / "snap.npz"))
    for env in (a, b):
        for t in range(5, 12):
            td = env.step(env.rand_step_input(acts[t].to(env.device)))
            if bool(td[("next", "done")].any()):
                r = env.rand_step_input()
                r.set("_reset", td[("next", "done")].squeeze(-1))
                env.reset(r)
    assert_same(a.export_state(), b.export_state(), "resumed")
