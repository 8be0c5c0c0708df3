"""GPU parity of the trajectory-predictor path (hns_tp_observe) through the C ABI.

HIP vs the C oracle: the window (TP_input), TP_groundtruth and TP_done bit for bit; the predicted
positions and the 35-value rows within 1e-5 (north-star tolerance: the kernel evaluates the
products as two-term fp16 splits on the matrix cores and its sigmoid/tanh on the transcendental
unit; the oracle is plain fp32 + libm).  HIP vs the reference golden (its own TP_net, 14 consecutive calls) within 1e-5, and
the env class against a plain-torch fp32 LSTM."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hns_oracle as O
from hns_amd import abi, config
from hns_amd.env import HideAndSeek
from tp_reference import TPObservation

TOL = 1e-5


def _env(E, A, Cn=5, max_len=40, use_obstacles=0, **kw):
    cfg = config.make_cfg({"num_agents": A, "use_obstacles": use_obstacles, "cylinder": {"max_num": Cn, "min_num": min(3, Cn)},
                           "env": {"num_envs": E, "max_episode_length": max_len}}, algo={"use_TP_net": 1, **kw})
    env = HideAndSeek(cfg)
    env.set_seed(3)
    return env


def _host_tp(env):
    """Host copies of the predictor's buffers + weights, for the oracle."""
    tpa = {k: v.cpu().numpy().copy() for k, v in env._tp_bufs.items() if k != "packed"}
    tpa["packed"] = np.zeros(16, np.uint8)               # unused by the oracle
    sd = env.TP.state_dict()
    for f, key in abi.TP_STATE_DICT_KEYS.items():
        tpa[f] = sd[key].detach().cpu().numpy().copy()
    return tpa


@pytest.mark.parametrize("E,A,obst", [(48, 3, 0), (300, 1, 0), (257, 2, 0), (1000, 4, 0), (130, 6, 0), (65536, 3, 0),
                                      (24001, 3, 0),                # one-chunk frames: 1 / 2 / 4 column tiles per workgroup by batch size (here 2, ragged)
                                      (200, 3, 1), (70, 1, 1),      # obst: task.use_obstacles, cylinders in the frame
                                      (300, 6, 12), (260, 6, 16), (129, 7, 16)])   # obst > 1: that many cylinder slots: frames of 61, 73 and 76 values
def test_tp_observe_matches_oracle(E, A, obst):
    O.set_threads(16 if E > 4096 else 1)                    # (65536, 3): BASELINE config 3 at full size
    Cn = obst if obst > 1 else 5
    env = _env(E, A, Cn=Cn, critic_input="state", use_obstacles=min(obst, 1))
    assert env._tp_bufs["history"].shape == (E, 10, 7 + 3 * A + 3 * Cn * min(obst, 1))
    torch.manual_seed(E + A)
    with torch.no_grad():
        for prm in env.TP.parameters():                     # larger than the default init: gates leave the linear range
            prm.mul_(3.0)
    env.reset()
    host = env.export_state()
    tpa = _host_tp(env)
    tpa["history"][:] = 0
    O.tp_observe(env.hcfg, host, tpa, fill=True)
    err = 0.0
    for t in range(14 if E <= 4096 else 4):
        dev = {k: v.cpu().numpy() for k, v in env._tp_bufs.items()}
        err = max(err, float(np.abs(dev["pred"] - tpa["pred"]).max()))
        assert np.array_equal(dev["history"], tpa["history"]), f"window differs at call {t}"
        assert np.array_equal(dev["groundtruth"], tpa["groundtruth"])
        assert np.array_equal(dev["tp_done"], tpa["tp_done"])
        np.testing.assert_allclose(dev["pred"], tpa["pred"], rtol=0, atol=TOL)
        np.testing.assert_allclose(dev["obs_self"], tpa["obs_self"], rtol=0, atol=TOL)
        np.testing.assert_allclose(dev["state_drones"], tpa["state_drones"], rtol=0, atol=TOL)
        act = torch.randn(E, A, 4, device=env.device)
        env.step(env.rand_step_input(act))
        host = env.export_state()                           # the step itself is covered by test_hip_parity
        O.tp_observe(env.hcfg, host, tpa, fill=False)
    assert np.abs(tpa["pred"]).max() > 0.05
    print(f"E={E} A={A}: max |pred_hip - pred_oracle| = {err:.2e}")


@pytest.mark.parametrize("shape", [("4133", "3", "0", "5"), ("1500", "6", "0", "5"), ("1100", "3", "1", "8"), ("900", "7", "1", "16")])
def test_tp_tiles_per_workgroup_do_not_change_a_bit(shape):
    """The weight-stationary kernel serves small batches with 1 or 2 column tiles per workgroup instead of 4 (csrc/hns_tp.hip: ws_envs; picked by batch
    size, HNS_TP_TILES forces one): the tile arithmetic does not depend on it — predictions, rows and window after 12 steps of a ragged batch are the same
    bytes for every tile count (one process each: the override is read once per process).  Shapes (units, pursuers, obstacles in the frame, cylinder slots):
    frames of one, two, three and five chunks — at these batch sizes the library picks one tile (what the oracle comparisons of this file run), so the forced
    four-tile launches are what covers the wide-frame four-tile kernels and their late frame emission."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    digests = {}
    for tiles in ("auto", "1", "2", "4"):
        env = dict(os.environ, HNS_TP_TILES_DIGEST_ONLY="1")
        env.pop("HNS_TP_TILES", None)
        if tiles != "auto":
            env["HNS_TP_TILES"] = tiles
        if tiles == "2" and shape[1:] != ("3", "0", "5"):
            continue                                        # two-tile workgroups: one-chunk frames only
        out = subprocess.run([sys.executable, os.path.join(root, "tools", "tp_tiles.py"), "--child", *shape], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        digests[tiles] = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])["digest"]
    assert len(set(digests.values())) == 1, digests


@pytest.mark.parametrize("T", [13, 14, 15, 16])
def test_tp_widest_frames_and_longest_windows(T):
    """Five-chunk frames (7 pursuers, 16 cylinders in the frame: 76 values) with the longest windows: one-tile workgroups hold the WHOLE window's operands in
    LDS, which fits 14 frames of this width (160 KB) — beyond that hns_tp_observe falls back to four-tile workgroups.  Both against the oracle, in one
    process and in this order (the LDS attribute of an instantiation is set once per device: the first launch must ask for the largest window it can serve)."""
    cfg = config.make_cfg({"num_agents": 7, "use_obstacles": 1, "cylinder": {"max_num": 16, "min_num": 3}, "history_step": T, "future_predcition_step": 5,
                           "env": {"num_envs": 96, "max_episode_length": 40}}, algo={"use_TP_net": 1})
    O.set_threads(1)
    env = HideAndSeek(cfg)
    env.set_seed(T)
    env.reset()
    assert env._tp_bufs["history"].shape == (96, T, 76)
    tpa = _host_tp(env)
    tpa["history"][:] = 0
    O.tp_observe(env.hcfg, env.export_state(), tpa, fill=True)
    for t in range(T + 3):
        dev = {k: v.cpu().numpy() for k, v in env._tp_bufs.items()}
        assert np.array_equal(dev["history"], tpa["history"]), f"window differs at call {t}"
        np.testing.assert_allclose(dev["pred"], tpa["pred"], rtol=0, atol=TOL)
        np.testing.assert_allclose(dev["obs_self"], tpa["obs_self"], rtol=0, atol=TOL)
        env.step(env.rand_step_input(torch.randn(96, 7, 4, device=env.device)))
        O.tp_observe(env.hcfg, env.export_state(), tpa, fill=False)


def test_tp_rows_without_critic_state_and_lazy_state():
    env = _env(200, 3)                                       # critic_input: obs -> state_drones pointer is NULL
    env.reset()
    td = env.step(env.rand_step_input())
    nxt = td["next"]
    ss = nxt[("agents", "observation", "state_self")]
    sd = nxt[("agents", "state")]["state_drones"]
    assert ss.shape == (200, 3, 1, 35) and sd.shape == (200, 3, 35)
    rpos = env._bufs["drone_state"][..., :3] - env._bufs["target_pos"].unsqueeze(1)
    assert torch.equal(sd[..., :3], rpos) and torch.equal(sd[..., 3:], ss[:, :, 0, 3:])
    assert nxt[("agents", "TP", "TP_input")].shape == (200, 10, 16)
    assert nxt[("agents", "TP", "TP_done")].dtype == torch.bool


def test_tp_env_matches_torch_lstm():
    """The env's rows against the plain-torch composition (torch.nn.LSTM fp32 on the same device)."""
    E, A = 512, 3
    env = _env(E, A, critic_input="state")
    ref = TPObservation(env.TP, A, float(env.hcfg.arena_size), float(env.hcfg.max_height), env.max_episode_length)
    env.reset()
    b = env._bufs
    for t in range(13):
        ss, sd, tp = ref(b["obs_self"], b["drone_state"][..., :3], b["target_pos"], b["target_vel"], env.progress_buf, b["detect"])
        tb = env._tp_bufs
        assert torch.equal(tp["TP_input"], tb["history"])
        torch.testing.assert_close(ss, tb["obs_self"], rtol=0, atol=TOL)
        torch.testing.assert_close(sd, tb["state_drones"], rtol=0, atol=TOL)
        torch.testing.assert_close(tp["TP_groundtruth"], tb["groundtruth"], rtol=0, atol=1e-6)
        assert torch.equal(tp["TP_done"][:, 0], tb["tp_done"].bool())
        env.step(env.rand_step_input(torch.randn(E, A, 4, device=env.device)))


@pytest.mark.parametrize("name", ["g_tp_obs", "g_tp_obs_a6", "g_tp_obs_obst", "g_tp_obs_obst_c8"])
def test_tp_matches_reference_golden(golden, name):
    """hns_tp_observe fed with the golden's states (obs rows from the oracle's observation pass) against
    the reference's own `_compute_state_and_obs` + TP_net outputs."""
    g = golden(name)
    E, A, Cn, T, max_len = (int(x) for x in g["meta"])
    obst = int(g["use_obstacles"]) if "use_obstacles" in g else 0          # task.use_obstacles: cylinders in the frame
    cfg = config.make_cfg({"num_agents": A, "drone_detect_radius": 0.9, "use_obstacles": obst, "cylinder": {"max_num": Cn, "min_num": 4},
                           "env": {"num_envs": E, "max_episode_length": max_len}}, algo={"use_TP_net": 1, "critic_input": "state"})
    env = HideAndSeek(cfg)
    env.TP.load_state_dict({k: torch.from_numpy(g["w_" + k.replace(".", "_")]) for k in env.TP.state_dict()})
    c = env.hcfg
    arrs = O.alloc_buffers(c)
    arrs["cylinders"][:] = g["cyl"]
    for t in range(T):
        arrs["drone_state"][..., 0:3], arrs["drone_state"][..., 3:7], arrs["drone_state"][..., 7:13] = g["pos"][t], g["rot"][t], g["vel"][t]
        arrs["throttle"][:] = g["throttle"][t]
        arrs["target_pos"][:] = g["tpos"][t][:, 0]
        arrs["target_vel"][:] = g["tvel"][t][:, 0]
        arrs["progress"][:] = g["progress"][t]
        _, bdet, _ = O.obs_reward(c, arrs)
        arrs["detect"][:] = bdet
        env.import_state(arrs)
        env._tp_observe()
        tb = {k: v.cpu().numpy() for k, v in env._tp_bufs.items()}
        np.testing.assert_allclose(tb["history"], g["TP_input"][t], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(tb["obs_self"], g["state_self"][t][:, :, 0], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(tb["state_drones"], g["state_drones"][t], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(tb["groundtruth"], g["TP_groundtruth"][t], rtol=1e-6, atol=1e-6)
        assert (tb["tp_done"].astype(bool) == g["TP_done"][t][:, 0]).all()


def test_tp_sees_in_place_weight_updates_and_rebinds():
    env = _env(64, 3)
    env.reset()
    p0 = env._tp_bufs["pred"].clone()
    with torch.no_grad():
        env.TP.fc.bias.add_(0.5)                             # in-place optimiser-style update: same storage
    env._tp_observe()
    assert not torch.equal(p0, env._tp_bufs["pred"])
    ptrs = env._tp_weight_ptrs
    env.TP.fc.bias = torch.nn.Parameter(env.TP.fc.bias.detach().clone())   # swapped tensor -> re-bind
    env._tp_observe()
    assert env._tp_weight_ptrs != ptrs


def test_tp_bind_errors():
    env = _env(64, 3)
    lib = env._lib
    tb = abi.HnsTpBuffers()
    assert lib.hns_tp_bind(env._env, C.byref(tb), 10, 5) == abi.HNS_ERR_INVALID_ARG
    assert lib.hns_tp_bind(env._env, None, 10, 5) == abi.HNS_ERR_INVALID_ARG
    env2 = HideAndSeek(config.make_cfg({"env": {"num_envs": 64}}))
    assert lib.hns_tp_observe(env2._env, 1, None) == abi.HNS_ERR_NOT_BOUND
    assert b"hns_tp_bind" in lib.hns_last_error()
    assert lib.hns_tp_refresh(env2._env, None) == abi.HNS_ERR_NOT_BOUND
    # the frame holds `progress`: episodes longer than the fp16-split operands can represent are refused
    long_env = HideAndSeek(config.make_cfg({"env": {"num_envs": 64, "max_episode_length": 100000}}, algo={"use_TP_net": 1}))
    with pytest.raises(Exception, match="max_episode_length"):
        long_env.reset()


def test_tp_snapshot_resume(tmp_path):
    """save_state / load_state carry the predictor's window: a resumed run reproduces the rows bit for bit."""
    E, A = 200, 3
    env = _env(E, A)
    env.reset()
    g = torch.Generator(device="cpu").manual_seed(1)
    acts = [torch.randn(E, A, 4, generator=g).to(env.device) for _ in range(8)]
    for a in acts[:5]:
        env.step(env.rand_step_input(a))
    path = str(tmp_path / "snap.npz")
    env.save_state(path)
    for a in acts[5:]:
        env.step(env.rand_step_input(a))
    want = {k: v.clone() for k, v in env._tp_bufs.items() if k != "packed"}
    want_obs = env._bufs["obs_self"].clone()
    env2 = _env(E, A)
    env2.TP.load_state_dict(env.TP.state_dict())
    env2.reset()
    env2.load_state(path)
    for a in acts[5:]:
        env2.step(env2.rand_step_input(a))
    assert torch.equal(env2._bufs["obs_self"], want_obs)
    for k, v in want.items():
        assert torch.equal(env2._tp_bufs[k], v), k


def test_load_policy_checkpoint(tmp_path):
    """The "TP" entry of a reference MAPPO checkpoint (mappo.py:477-484) drives the predictor after loading."""
    a, b = _env(64, 3), _env(64, 3)
    with torch.no_grad():
        for prm in a.TP.parameters():
            prm.mul_(2.5)
    ckpt = {"TP": {k: v.detach().cpu() for k, v in a.TP.state_dict().items()}, "critic": {}, "actor_params": None, "value_normalizer": {}}
    path = tmp_path / "checkpoint_final.pt"
    torch.save(ckpt, path)
    for env in (a, b):
        env.reset()
    b.load_policy_checkpoint(str(path))
    act = torch.randn(64, 3, 4, device=a.device)
    for _ in range(3):
        a.step(a.rand_step_input(act))
        b.step(b.rand_step_input(act))
    torch.testing.assert_close(a._tp_bufs["pred"], b._tp_bufs["pred"], rtol=0, atol=0)
    assert float(a._tp_bufs["pred"].abs().max()) > 0


def test_tp_saturated_gates_stay_finite():
    """Parameters 20x the default init drive the gate pre-activations far into saturation (|z| ~ 100: exp2 overflows
    to inf / underflows to 0 inside the sigmoids): everything stays finite.  With such gains the recurrence amplifies
    last-bit differences (plain fp32 against fp64 is off by 5e-6 on one golden window already, tests/test_tp_accuracy.py),
    so HIP and oracle are compared on the bulk (median) and with a loose bound on the tail."""
    E, A = 256, 3
    env = _env(E, A, critic_input="state")
    with torch.no_grad():
        for prm in env.TP.parameters():
            prm.mul_(20.0)
    env.reset()
    host = env.export_state()
    tpa = _host_tp(env)
    tpa["history"][:] = 0
    O.tp_observe(env.hcfg, host, tpa, fill=True)
    for t in range(6):
        dev = {k: v.cpu().numpy() for k, v in env._tp_bufs.items()}
        assert np.isfinite(dev["pred"]).all() and np.isfinite(dev["obs_self"]).all()
        diff = np.abs(dev["pred"] - tpa["pred"])
        assert np.median(diff) < 1e-6 and diff.max() < 5e-3, (float(np.median(diff)), float(diff.max()))
        env.step(env.rand_step_input(torch.randn(E, A, 4, device=env.device)))
        host = env.export_state()
        O.tp_observe(env.hcfg, host, tpa, fill=False)
    assert np.abs(tpa["pred"]).max() > 0.3


def _draw_tp_case(seed):
    r = np.random.RandomState(7000 + seed)
    A = int(r.randint(1, 8))
    obst = int(r.rand() < 0.5)
    Cn = int(r.randint(1, 17))
    E = int(r.choice([1, 31, 64, 100, 128, 129, 192, 257, 384, 500]))
    task = {"num_agents": A, "num_targets": 2 if r.rand() < 0.3 else 1, "use_obstacles": obst, "cylinder": {"max_num": Cn, "min_num": int(r.randint(0, Cn + 1)), "obs_max_cylinder": min(3, Cn)},
            "env": {"num_envs": E, "max_episode_length": int(r.choice([8, 40, 800]))}, "history_step": int(r.randint(1, 17)),
            "future_predcition_step": int(r.randint(1, 11)), "drone_detect_radius": float(r.choice([0.7, 100.0]))}
    return task, E, A, float(r.choice([1.0, 2.0, 3.0]))


@pytest.mark.parametrize("seed", list(range(int(os.environ.get("HNS_FUZZ_TP_SEEDS", 60)))))
def test_tp_random_configuration_matches_oracle(seed):
    """Seeded sweep over frame widths (1-5 operand chunks, both kernels), window lengths, horizons and batch sizes: window, ground
    truth and flags exact, predictions and rows within 1e-5 of the oracle's fp32 LSTM."""
    task, E, A, scale = _draw_tp_case(seed)
    for _ in range(20):
        try:
            cfg = config.make_cfg(task, algo={"use_TP_net": 1})
            config.resolve_hns_cfg(cfg)
            break
        except ValueError:                                  # the placement grid does not hold the bodies: fewer cylinder slots
            task["cylinder"]["max_num"] = max(1, task["cylinder"]["max_num"] - 2)
            task["cylinder"]["min_num"] = min(task["cylinder"]["min_num"], task["cylinder"]["max_num"])
            task["cylinder"]["obs_max_cylinder"] = min(3, task["cylinder"]["max_num"])
    O.set_threads(1)
    env = HideAndSeek(cfg)
    env.set_seed(seed)
    torch.manual_seed(seed)
    with torch.no_grad():
        for prm in env.TP.parameters():
            prm.mul_(scale)
    env.reset()
    tpa = _host_tp(env)
    tpa["history"][:] = 0
    O.tp_observe(env.hcfg, env.export_state(), tpa, fill=True)
    for t in range(12):
        dev = {k: v.cpu().numpy() for k, v in env._tp_bufs.items()}
        what = f"seed {seed} {task} call {t}"
        assert np.array_equal(dev["history"], tpa["history"]), what
        assert np.array_equal(dev["groundtruth"], tpa["groundtruth"]), what
        assert np.array_equal(dev["tp_done"], tpa["tp_done"]), what
        np.testing.assert_allclose(dev["pred"], tpa["pred"], rtol=0, atol=TOL, err_msg=what)
        np.testing.assert_allclose(dev["obs_self"], tpa["obs_self"], rtol=0, atol=TOL, err_msg=what)
        env.step(env.rand_step_input(torch.randn(E, A, 4, device=env.device)))
        O.tp_observe(env.hcfg, env.export_state(), tpa, fill=False)
        done = env._bufs["done"].bool()
        if bool(done.any()) and t % 3 != 2:                  # masked reset: the window is not reset per env, the new frame is appended (hideandseek.py:825-830)
            td = env.rand_step_input()
            td.set("_reset", done.clone())
            env.reset(td)
            O.tp_observe(env.hcfg, env.export_state(), tpa, fill=False)


@pytest.mark.parametrize("E,A,NT", [(256, 3, 1), (384, 6, 1), (256, 3, 2)])
def test_step_and_predictor_as_two_half_batches_on_two_streams(E, A, NT):
    """task.tp_overlap: the halves [0, E/2) and [E/2, E) stepped by two handles over slices of the same buffers, on two streams
    between a fork and a join event, leave every buffer — step state, statistics (a [24, E] array addressed with the whole batch's row stride),
    the predictor's window, predictions and rows — bit-identical to the whole batch on one stream, across a masked reset, a curriculum change of
    the evader's speed and an in-place parameter update."""
    def make(overlap):
        cfg = config.make_cfg({"num_agents": A, "num_targets": NT, "tp_overlap": overlap, "cylinder": {"max_num": 5, "min_num": 3},
                               "env": {"num_envs": E, "max_episode_length": 9}}, algo={"use_TP_net": 1, "critic_input": "state"})
        env = HideAndSeek(cfg)
        env.set_seed(11)
        torch.manual_seed(5)
        for p_ in env.TP.parameters():
            torch.nn.init.uniform_(p_, -0.3, 0.3)
        env.reset()
        return env
    whole, split = make(0), make(1)
    assert whole._halves is None and split._halves is not None and int(split._halves[1].cfg.stats_stride) == E
    g = torch.Generator(device="cpu").manual_seed(1)
    for t in range(14):
        a = torch.randn(E, A, 4, generator=g).to(whole.device)
        for env in (whole, split):
            env.step(env.rand_step_input(a.clone()))
        if t == 8:                                         # every env done: reset two thirds of them
            mask = torch.zeros(E, 1, dtype=torch.bool, device=whole.device)
            mask[::3] = True
            mask[1::3] = True
            for env in (whole, split):
                from hns_amd.tensordict_shim import TensorDict
                env.reset(TensorDict({"_reset": mask.clone()}, [E]))
        if t == 4:
            for env in (whole, split):
                env.v_prey = 1.1
                for h in env._handles():
                    env._check(env._lib.hns_set_v_prey(h, C.c_float(1.1)), "hns_set_v_prey")
        if t == 10:
            for env in (whole, split):
                with torch.no_grad():
                    env.TP.fc.bias.add_(0.05)                # version counter moves: every handle's image is re-packed
    a, b = whole.export_state(), split.export_state()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{k} differs between the whole batch and the two half batches"
    for k in ("history", "pred", "obs_self", "state_drones", "groundtruth", "tp_done"):
        assert torch.equal(whole._tp_bufs[k], split._tp_bufs[k]), f"predictor buffer {k} differs"
    assert whole.check_finite() and split.check_finite()


def test_get_set_state_of_a_half_batch_handle_copies_its_stats_columns():
    """hns_get_state / hns_set_state on a handle over a SLICE of a larger batch (stats rows strided by the owner's env count) used to
    skip `stats` silently; now the handle's columns of every row travel as one pitched copy, the other half's columns stay untouched."""
    E, A = 256, 3
    cfg = config.make_cfg({"num_agents": A, "tp_overlap": 1, "cylinder": {"max_num": 5, "min_num": 3}, "env": {"num_envs": E, "max_episode_length": 9}},
                          algo={"use_TP_net": 1})
    env = HideAndSeek(cfg)
    env.set_seed(2)
    env.reset()
    for _ in range(3):
        env.step(env.rand_step_input())
    torch.cuda.synchronize()
    whole = env._bufs["stats"].cpu().numpy().copy()                       # [24, E]
    h = E // 2
    for i, hv in enumerate(env._halves):
        got = np.full((whole.shape[0], h), np.nan, np.float32)
        hb = abi.HnsBuffers()
        hb.stats = got.ctypes.data
        assert env._lib.hns_get_state(hv.env, C.byref(hb), env._stream()) == 0, env._lib.hns_last_error()
        torch.cuda.synchronize()
        assert np.array_equal(got, whole[:, i * h:(i + 1) * h])
    new = np.random.default_rng(0).random((whole.shape[0], h), dtype=np.float32)
    hb = abi.HnsBuffers()
    hb.stats = new.ctypes.data
    assert env._lib.hns_set_state(env._halves[1].env, C.byref(hb), env._stream()) == 0, env._lib.hns_last_error()
    torch.cuda.synchronize()
    after = env._bufs["stats"].cpu().numpy()
    assert np.array_equal(after[:, h:], new) and np.array_equal(after[:, :h], whole[:, :h])
