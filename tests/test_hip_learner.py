"""hns_amd.learner.DeviceLearner and hns_learner_info on an MI355X.

Bit identity, no tolerance: one train_op on the device equals the same blocks driven by hand through the package's public calls with
per-call workspaces and their own result tensors (tests/learner_cases.py) — parameters, Adam state, ValueNorm1, info row — which covers the
cached workspaces, the out= pointers into the table and the index path at once; a learner whose workspaces regrow and shrink in use equals a
fresh one.  The predictor's inputs use TP_done all ones: the reference's `view(batch, -1, ...)` of the selected windows (mappo.py:419)
needs the same count in every env.

hns_learner_info: action_norm against fp64 numpy on the same fp32 actions under the project's rule, e_hip <= 8 max(e_torch32,
2^-24 |ref64|); the column means equal float32(fp64 row-order sum / M) bit for bit.  The PPO loop runs under torch's sync debug mode
"error": no host synchronisation.

Device against the CPU path, one train_op from one start over the same minibatch rows (one epoch of two minibatches, so that no ratio is
re-rolled by more than one earlier update): per tensor e_device <= 8 max(e_cpu32, 2^-24 max|p64|), errors as max-abs against the fp64
train_op of tests/learner_f64_reference.py, which first asserts in fp64 that no row lies within 1e-3 of the PPO clip's or the value clip's
bounds (log_probs_old is the fp64 log-probability minus a delta outside the band around log 1.1 / -log 0.9, as test_hip_actor_train.py).
Measured on an MI355X: worst ratio over the 54 tensors 6.64 (critic out_proj.bias: e_device 1.6e-8, e_cpu32 2.4e-9 — a first Adam step divides each gradient by its own magnitude, so a small gradient's rounding shows in full), then 3.27 (the predictor's weight_ih), 2.36, 2.24, 2.01; the rest below 2."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import actor_update_reference as U
import learner_cases as LC
import learner_f64_reference as F64
from hns_amd import abi, learner

pytestmark = pytest.mark.gpu

BAR = 8.0
A = 3


def _cfg(**kw):
    cfg = copy.deepcopy(LC.CFG)
    cfg.update(kw)
    return cfg


def _check_info(info, hand):
    for k in learner.COLUMNS + ("advantages_mean", "advantages_std", "value_running_mean", "TP_loss"):
        assert np.float32(info[f"drone/{k}"]).tobytes() == np.float32(hand[k]).tobytes(), (k, info[f"drone/{k}"], hand[k])
    ref = hand["action_norm_f64"]                                # (the accuracy gate of action_norm is the test below; here: one rounding)
    assert abs(info["drone/action_norm"] - ref) <= BAR * 2.0 ** -24 * abs(ref)


@pytest.mark.parametrize("N, T, minibatches", [(8, 8, 2), (5, 7, 4)])
def test_train_op_on_the_device_is_the_hand_driven_sequence_bit_for_bit(N, T, minibatches):
    """[8, 8, 3] in 2 minibatches of 32 env-steps: 96 rows, three 32-row tiles; [5, 7, 3] in 4: 35 env-steps, 8 per minibatch (24 rows: a
    partial tile), 3 dropped."""
    cfg = _cfg(num_minibatches=minibatches)
    cpu = LC.make_state(A, 31)
    ro = LC.to_device(LC.make_rollout(cpu, N, T, A, 32), "cuda")
    hand_state = LC.clone_state(cpu, "cuda")
    opts = LC.hand_optimisers(hand_state, cfg)
    hand = LC.hand_train_op(hand_state, opts, ro, torch.Generator(device="cuda").manual_seed(5), cfg)
    state = LC.clone_state(cpu, "cuda")
    L = LC.make_learner(state, cfg, seed=5)
    info = L.train_op(LC.as_tensordict(ro))
    torch.cuda.synchronize()
    LC.assert_same_state(LC.state_tensors(state, LC.learner_opts(L)), LC.state_tensors(hand_state, opts), "device train_op against the hand sequence")
    _check_info(info, hand)
    assert set(L._ws) == {"actor", "critic", "info"}
    steps = 2 * minibatches
    assert float(L.actor_opt.state[next(iter(state["actor"].values()))]["step"]) == steps


def test_a_learner_whose_workspaces_regrow_equals_a_fresh_one():
    """small rollout, a larger one (both update workspaces regrow), the small one again (the larger buffers are reused): before each call a
    fresh learner is started from the same state (parameters, optimisers, ValueNorm1, generator seed); after it both hold the same bits."""
    cfg = _cfg(num_minibatches=2)
    cpu = LC.make_state(A, 41)
    small, large = (LC.to_device(LC.make_rollout(cpu, n, 8, A, 42 + n), "cuda") for n in (4, 16))
    state = LC.clone_state(cpu, "cuda")
    L = LC.make_learner(state, cfg, seed=0)
    sizes = []
    for step, ro in enumerate((small, large, small)):
        fresh_state = LC.clone_state(state)
        F = LC.make_learner(fresh_state, cfg, seed=0)
        F.load_state_dict(copy.deepcopy(L.state_dict()))
        L.generator.manual_seed(100 + step)
        F.generator.manual_seed(100 + step)
        a, b = L.train_rollout(**ro), F.train_rollout(**ro)
        torch.cuda.synchronize()
        assert a == b, step
        LC.assert_same_state(LC.state_tensors(state, LC.learner_opts(L)), LC.state_tensors(fresh_state, LC.learner_opts(F)), f"call {step}")
        sizes.append({k: (v.numel(), v.data_ptr()) for k, v in L._ws.items()})
    assert sizes[1]["actor"][0] > sizes[0]["actor"][0] and sizes[1]["critic"][0] > sizes[0]["critic"][0]
    assert sizes[2]["actor"] == sizes[1]["actor"] and sizes[2]["critic"] == sizes[1]["critic"]        # reused, not reallocated
    L.release()
    assert L._ws == {}


def _info(action2d, table):
    lib = abi.load_library()
    rows, d = action2d.shape
    nbytes = lib.hns_learner_info_workspace_bytes(rows)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.full((table.shape[1] + 1,), float("nan"), device="cuda")
    rc = lib.hns_learner_info(action2d.data_ptr(), (C.c_int64 * 2)(action2d.stride(0), action2d.stride(1)), rows, d, table.data_ptr(), table.shape[0],
                              table.shape[1], out.data_ptr(), ws.data_ptr(), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.hns_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("layout", ["dim4", "dim4_strided", "dim1", "dim8"])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 8 * 8 * 3, 2049])
def test_action_norm_against_fp64(rows, layout):
    """rows: one, around a wave, the [8, 8, 3] rollout, one past a workgroup's share of 2 048 (two partials).  dim4: contiguous, float4
    loads; dim4_strided: columns 1..4 of a [rows, 7] tensor (row stride 7, rows not 16-byte aligned): scalar loads."""
    g = torch.Generator().manual_seed(rows)
    d = {"dim4": 4, "dim4_strided": 4, "dim1": 1, "dim8": 8}[layout]
    if layout == "dim4_strided":
        a = (torch.randn(rows, 7, generator=g) * 1.5).cuda()[:, 1:5]
        assert a.stride(0) == 7 and a.data_ptr() % 16 != 0
    else:
        a = (torch.randn(rows, d, generator=g) * 1.5).cuda()
        assert a.data_ptr() % 16 == 0
    table = torch.zeros(1, 1, device="cuda")
    out = _info(a, table)
    a32 = a.cpu()
    a64 = a32.double().numpy()
    ref = float(np.sqrt((a64 * a64).sum(-1)).mean())
    e_32 = abs(float(a32.norm(dim=-1).mean()) - ref)
    e_hip = abs(float(out[1]) - ref)
    bound = max(e_32, 2.0 ** -24 * abs(ref))
    print(f"  action_norm rows {rows} {layout}: e_hip {e_hip:.3e} e_32 {e_32:.3e} ref {ref:.6f} ratio {e_hip / bound:.2f}")
    assert e_hip <= BAR * bound
    assert out[0] == 0.0
    assert np.array_equal(out, _info(a, table))                 # two calls: the same bits


@pytest.mark.parametrize("columns", [1, 8, 16])
@pytest.mark.parametrize("M", [1, 2, 64])
def test_column_means_are_the_fp64_row_order_sum_rounded_once(M, columns):
    g = torch.Generator().manual_seed(M * 100 + columns)
    table = torch.randn(M, columns, generator=g) * torch.logspace(-3, 3, columns)       # magnitudes from 1e-3 to 1e3 across the columns
    out = _info(torch.ones(5, 4, device="cuda"), table.cuda())
    want = np.array([LC._mean32(table[:, c].tolist()) for c in range(columns)], np.float32)
    assert out[:columns].tobytes() == want.tobytes()
    assert out[columns] == 2.0                                   # |(1, 1, 1, 1)|


def test_the_ppo_loop_makes_no_host_synchronisation():
    """torch's sync debug mode "error" around the PPO loop (not around update_tp's selected-count read or the final copy): the loop completes.
    Skipped where the installed torch does not offer the mode on this device."""
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("torch.cuda.set_sync_debug_mode is not available in this torch")
    try:
        torch.cuda.set_sync_debug_mode("error")
        torch.cuda.set_sync_debug_mode("default")
    except Exception as e:                                       # noqa: BLE001
        pytest.skip(f"the sync debug mode cannot be set on this build: {e}")
    cfg = _cfg(num_minibatches=2)
    cpu = LC.make_state(A, 51)
    ro = LC.to_device(LC.make_rollout(cpu, 8, 8, A, 52), "cuda")
    L = LC.make_learner(LC.clone_state(cpu, "cuda"), cfg, seed=1)
    L.train_rollout(**ro)                                        # first call: .grad tensors, optimiser state and workspaces are allocated
    loop, ran = L._ppo_loop, []

    def guarded(*a):
        torch.cuda.set_sync_debug_mode("error")
        try:
            loop(*a)
            ran.append(True)
        finally:
            torch.cuda.set_sync_debug_mode("default")

    L._ppo_loop = guarded
    info = L.train_rollout(**ro)
    assert ran == [True] and np.isfinite(list(info.values())).all()


def fp64_gate_case(lpo_seed=65):
    """(cfg, start state, CPU rollout) of the device-against-CPU gate: [8, 8, 3], one epoch of two minibatches of 32 env-steps, log_probs_old
    off the clip.  lpo_seed: 65 is the first seed from 63 on at which the fp64 train_op keeps every ratio of BOTH minibatches 1e-3 off the
    clip's bounds (63 and 64 leave one ratio of the second minibatch, moved by the first update, 1.7e-4 and 4.4e-4 from a bound)."""
    N, T = 8, 8
    cfg = _cfg(ppo_epochs=1, num_minibatches=2)
    start = LC.make_state(A, 61)
    ro = LC.make_rollout(start, N, T, A, 62)
    actor = {k: v.detach().numpy() for k, v in start["actor"].items()}
    flat = lambda t: t.reshape(N * T, *t.shape[2:])             # noqa: E731
    obs = F64.obs_dict(flat(ro["obs_self"]), flat(ro["obs_others"]), flat(ro["obs_cylinders"]))
    logp = U.new_log_probs(actor, obs, flat(ro["action"]).numpy())
    ro["log_probs"] = torch.from_numpy(U.make_old_log_probs(logp, lpo_seed)).reshape(N, T, A, 1)
    return cfg, start, ro


def run_with_fixed_rows(monkeypatch, cfg, start, ro, device, seed=7):
    """One train_op on `device` with every permutation drawn from a CPU generator (the two devices' generators differ); returns the changed
    tensors and the index rows in the order drawn."""
    gen, rows = torch.Generator().manual_seed(seed), []

    def draw(n, m, dev, generator=None):
        perm = torch.randperm((n // m) * m, generator=gen).reshape(m, -1)
        rows.extend(perm.tolist())
        return perm.to(dev)

    monkeypatch.setattr(learner.tp_train, "minibatches", draw)
    state = LC.clone_state(start, device)
    LC.make_learner(state, cfg, seed=0).train_rollout(**LC.to_device(ro, device))
    none = {"actor": None, "critic": None, "tp": None}
    return {k: v.detach().cpu().double().numpy() for k, v in LC.state_tensors(state, none).items()}, rows


def gate_ratios(p64, cpu, dev):
    out = {}
    for k, ref in p64.items():
        e_dev, e_cpu = float(np.abs(dev[k] - ref).max()), float(np.abs(cpu[k] - ref).max())
        bound = max(e_cpu, 2.0 ** -24 * float(np.abs(ref).max()))
        out[k] = (e_dev, e_cpu, bound, e_dev / bound if bound > 0 else (0.0 if e_dev == 0 else float("inf")))
    return out


def test_one_train_op_on_the_device_against_the_cpu_path_under_the_fp64_bar(monkeypatch):
    """Measured on an MI355X (e_device / max(e_cpu32, 2^-24 max|p64|)): worst 6.64 on critic out_proj.bias, 3.27 on the predictor's weight_ih,
    every other of the 54 tensors at most 2.36; the actor's in_proj_bias has e_cpu32 2.8e-4 (autograd noise on the k third, whose true gradient
    is zero, through Adam's first step) where the device writes exact zeros."""
    cfg, start, ro = fp64_gate_case()
    cpu, rows = run_with_fixed_rows(monkeypatch, cfg, start, ro, "cpu")
    dev, rows_dev = run_with_fixed_rows(monkeypatch, cfg, start, ro, "cuda")
    assert rows == rows_dev and [len(r) for r in rows] == [12, 12, 32, 32]
    p64 = F64.train_op64(start, ro, cfg, rows[:2], rows[2:])
    assert set(p64) == set(cpu) == set(dev)
    ratios = gate_ratios(p64, cpu, dev)
    for k, (e_dev, e_cpu, bound, r) in ratios.items():
        print(f"  {k}: e_device {e_dev:.3e} e_cpu32 {e_cpu:.3e} max|p64| {np.abs(p64[k]).max():.3e} ratio {r:.2f}")
    print("  worst:", max(ratios.items(), key=lambda kv: kv[1][3]))
    bad = [f"{k}: e_device {v[0]:.3e} > {BAR} x {v[2]:.3e} (ratio {v[3]:.2f})" for k, v in ratios.items() if not v[3] <= BAR]
    assert not bad, "; ".join(bad)
