"""The data-parallel per-agent update's device entries on an MI355X: hns_actor_train_grad_agents_global,
hns_rnn_actor_head_grad_agents_global, the `*_per_agent_global` functions over them, learner.DataParallelPerAgentLearner and
learner.DataParallelPerAgentRecurrentLearner.  The cases: tests/dp_per_agent_cases.py; the CPU part: tests/test_dp_per_agent_learner.py.

  one-rank bits        global_rows = the call's own rows and entropy_share 1 give the LOCAL per-agent entry's bits in every output — the
                       stacked gradients, the scalars, log_probs (dy too for the recurrent entry) — whatever the workspace held:
                       plain (A, K, D; batch): (1, 1, 1; 1); (3, 5, 35; 33), a second tile with one live row; (3, 5, 35; 513), the smallest
                       batch at which ct_plan_agents gives A 3 two tiles per weight-gradient row range and a padding tile (asserted from
                       the restated plan: 512 still has one);
                       recurrent B x L x A: 1 x 1 x 1; 5 x 4 x 3; 11 x 3 x 7 (33 positions an agent: a second trip of one row); 172 x 16 x 6
                       (2 752 positions > 32 floor(512 / 6) = 2 720: past one trip of an agent's workgroups), through the op's strided view
                       and the contiguous layout of y, guard runs around dy.
  two emulated ranks   plain: batch 5 + 11 and 1 + 512 (A 3); recurrent: B 5 + 11 (L 4, A 3) and 1 + 171 (L 16, A 6), once more with a dead
                       segment in part 1 (n stays global_rows, the reference rescaled); entropy_share 1/2 each.  The summed gradients (each
                       stacked tensor per agent slice) and the summed policy_loss shares meet the gate e <= 8 max(e_32, 2^-24 max|ref_64|)
                       against fp64 autograd over the union; entropy is bit-equal on both parts; off the clip asserted first in fp64.
                       At 1 + 512 the data is per_agent_cases' (3, 5, 35; 520, 513), whose agent 0's d fc_mean.bias slice the LOCAL
                       device path misses torch's e_32 with (DESIGN-open-items.md, item 14: the row arithmetic's and fp32 summation's
                       error over 513 rows, 8.57 against the bar of 8): that slice alone is gated, as tests/test_hip_per_agent_edges.py
                       gates it, against the local device path's own error on the same rows in place of e_32.
  refusals             on the new names: global_rows < rows, a NaN and an infinite entropy_share, a NULL required pointer — an error code,
                       hns_last_error names the entry, every output keeps its fill.
  learner              a one-rank gloo group (file store) against the group-less per-agent learner, held to what the existing
                       data-parallel tests hold their classes to: DataParallelPerAgentLearner as test_hip_dp_learner.py holds
                       DeviceLearner(group=) — max_grad_norm above every norm, parameters, Adam states and ValueNorm1 bit-identical, the
                       two gradient-norm columns within ONE unit in the last place (the local entry's norm and hns_grad_norm add in
                       another order), every other info value identical; DataParallelPerAgentRecurrentLearner as
                       test_hip_dp_rnn_learner.py holds its class — BIT IDENTITY throughout (both sides take the bucket's norm).
                       Two real ranks on one card over gloo (tests/dp_per_agent_learner_job.py, one child process a rank, each under its
                       own time limit, 2 processes with the GPU open; nothing is started after a child that ends abnormally): the ranks
                       end bit-identical with equal info rows, for both classes.

Recorded on an MI355X: the file's 28 tests take 13.0 s; the worst ratio e / max(e_32, 2^-24 max|ref_64|) per case: plain 5 + 11 1.99,
plain 1 + 512 3.67 (encoder.linear2.bias of agent 0), recurrent 5 + 11 1.59, 1 + 171 2.59, the dead segment 2.01; agent 0's d fc_mean.bias
at 1 + 512: e 4.003e-08 for the summed two-part gradient, the local device path's own error to every printed digit."""
import copy
import ctypes as C
import json
import os
import queue
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import actor_per_agent_reference as UA
import dp_per_agent_cases as DC
import dp_reference as DR
import dp_rnn_reference as DU
import learner_cases as LC
import per_agent_cases as PC
import rnn_update_reference as U
import test_hip_rnn_train as TR
from hns_amd import abi, learner
from hns_amd import actor_train as AT
from hns_amd import policy_train as PT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 128
GUARD, FILL = 64, -7.5
_dev = TR._dev


# ---------------------------------------------------------------------------------------------------------------- the plain entry
def _plain_case(A, K, D, S, B, seed):
    import test_hip_per_agent as THP
    return THP._case(S, A, K, D, seed, B=B)


def _plain_call(data, index=None, glob=None, workspace=None, bucket=False, **kw):
    """policy_loss_and_grad_per_agent (glob None) or its _global form (glob = (global_rows, entropy_share)) on `data` with `index`."""
    actors, obs, action, lpo, adv, idx = data
    idx = idx if index is None else index
    live = {k: torch.as_tensor(v.copy()).cuda() for k, v in actors.items()}
    d = lambda x: torch.as_tensor(np.ascontiguousarray(x)).cuda() if x is not None else None       # noqa: E731
    args = (live, d(obs["state_self"]), d(obs.get("state_others")), d(obs["cylinders"]), d(action), d(lpo), d(adv), d(idx))
    if glob is None:
        out = AT.policy_loss_and_grad_per_agent(*args, workspace=workspace, **kw)
    else:
        out = AT.policy_loss_and_grad_per_agent_global(*args, workspace=workspace, global_rows=glob[0], entropy_share=glob[1],
                                                       bucket=PT.GradBucket(live) if bucket else None, **kw)
    torch.cuda.synchronize()
    return live, out


PLAIN_SHAPES = [(1, 1, 1, 3, 1), (3, 5, 35, 40, 33), (3, 5, 35, 520, 513)]          # (A, K, D, S, B)


@pytest.mark.parametrize("A, K, D, S, B", PLAIN_SHAPES)
def test_one_rank_plain_global_entry_has_the_local_entrys_bits(A, K, D, S, B):
    if B == 513:                                                 # read from the plan: the first batch past one row range for A = 3
        assert PC.agents_plan(513, 3) == (17, 2, 9, 1, 54) and PC.agents_plan(512, 3)[1] == 1
    if B == 33:
        assert PC.agents_plan(33, 3)[0] == 2                     # a second tile, of one live row
    data = PC.edge_case((A, K, D, S, B)) if B == 513 else _plain_case(A, K, D, S, B, 500 + A + S)
    nbytes = abi.load_library().hns_actor_train_agents_workspace_bytes(B * A, D, A, K)
    assert nbytes > 0
    filled = lambda byte: torch.full((nbytes,), byte, dtype=torch.uint8, device="cuda")           # noqa: E731
    loc, want = _plain_call(data)
    for byte, bucket in ((0x7F, False), (0xFF, True)):
        glo, got = _plain_call(data, glob=(B * A, 1.0), workspace=filled(byte), bucket=bucket)
        for k in loc:
            assert LC.bits_equal(glo[k].grad, loc[k].grad), k
        for n in ("policy_loss", "entropy", "ess", "log_probs"):
            assert LC.bits_equal(getattr(got, n), getattr(want, n)), n
        if bucket:                                               # hns_grad_norm over the bucket: another order of the same sum
            assert DR.ulps(float(got.grad_norm), float(want.grad_norm)) <= 1, (float(got.grad_norm), float(want.grad_norm))
        else:
            assert got.grad_norm is None                         # no bucket: the entry's norm launch is skipped and nothing stands in for it


# case -> the ONE slice gated against the local device path's own error (the docstring; tests/test_hip_per_agent_edges.py: SHARED_YARDSTICK)
LOCAL_YARDSTICK = {513: ("act_dist.fc_mean.bias", 0)}


@pytest.mark.parametrize("sizes", [(5, 11), (1, 512)])
def test_two_emulated_plain_ranks_meet_the_gate_over_the_union(sizes):
    A, B = 3, sum(sizes)
    data = PC.edge_case((3, 5, 35, 520, 513)) if B == 513 else _plain_case(3, 5, 35, 40, B, 543)
    actors, obs, action, lpo, adv, index = data
    r64, r32 = (UA.loss_and_grad(actors, obs, action, lpo, adv, index, dtype=dt) for dt in (torch.float64, torch.float32))
    DC.plain_preconditions(r64, r32)
    parts = [_plain_call(data, index=idx, glob=(B * A, 0.5)) for idx in (index[:sizes[0]], index[sizes[0]:])]
    (l0, o0), (l1, o1) = parts
    assert LC.bits_equal(o0.entropy, o1.entropy)
    grads = {k: (l0[k].grad + l1[k].grad).cpu().double().numpy() for k in l0}       # the all-reduce: one fp32 addition per entry
    yard = {}
    if B in LOCAL_YARDSTICK:
        name, a = LOCAL_YARDSTICK[B]
        loc, _ = _plain_call(data)
        yard[f"{name}[{a}]"] = loc[name].grad[a].cpu().double().numpy() - r64["grads"][name][a]
        print(f"  {name}[{a}]: gated against the local device path's own error, {np.abs(yard[f'{name}[{a}]']).max():.3e}, printed below as e_32")
    items = [(f"{k}[{a}]", grads[k][a], r64["grads"][k][a], r32["grads"][k][a]) for k in grads for a in range(A)]
    items = [(n, g, r, r + yard[n] if n in yard else b) for n, g, r, b in items]
    items += [("policy_loss", float(o0.policy_loss) + float(o1.policy_loss), r64["policy_loss"], r32["policy_loss"]),
              ("entropy", float(o0.entropy), r64["entropy"], r32["entropy"]),
              ("log_probs", torch.cat([o0.log_probs, o1.log_probs]).cpu().double().numpy(), r64["log_probs"], r32["log_probs"])]
    worst, bad = U.gate(f"plain {sizes[0]}+{sizes[1]}", items)
    assert not bad, "; ".join(bad)


# ---------------------------------------------------------------------------------------------------------------- the recurrent entry
class ACall(TR.Call):
    """TR.Call on a stacked head case with the two per-agent entries; dy lies between two guard runs."""

    def _guarded_dy(self):
        n = self.B * self.L * self.A * H
        buf = torch.full((n + 2 * GUARD,), FILL, device="cuda")
        body = buf[GUARD:GUARD + n]
        dy = body.view(self.B, self.A, self.L, H) if self.y.is_contiguous() else body.view(self.B, self.L, self.A, H).transpose(1, 2)
        assert dy.data_ptr() % 16 == 0
        return buf, dy

    def agents(self, glob=None, fill=0x7F):
        lib = abi.load_library()
        nb = lib.hns_rnn_actor_head_agents_workspace_bytes(self.B, self.A, self.L)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda").fill_(fill)
        buf, dy = self._guarded_dy()
        A = self.A
        o = {"d_head_w": torch.empty(A, 4, H, device="cuda"), "d_head_b": torch.empty(A, 4, device="cuda"), "d_log_std": torch.empty(A, 4, device="cuda"),
             "scal": torch.empty(3, device="cuda"), "log_probs": torch.full((self.B, self.L, A), float("nan"), device="cuda")}
        h, r, rows = self.head, self.rows, self.struct()
        entry = lib.hns_rnn_actor_head_grad_agents if glob is None else lib.hns_rnn_actor_head_grad_agents_global
        more = () if glob is None else (int(glob[0]), float(glob[1]))
        rc = entry(h["head_w"].data_ptr(), h["head_b"].data_ptr(), h["log_std"].data_ptr(), C.byref(rows), r["action"].data_ptr(),
                   r["log_probs_old"].data_ptr(), r["advantages"].data_ptr(), 0.1, 1e-3, dy.data_ptr(), o["d_head_w"].data_ptr(), o["d_head_b"].data_ptr(),
                   o["d_log_std"].data_ptr(), o["scal"][0:].data_ptr(), o["scal"][1:].data_ptr(), o["scal"][2:].data_ptr(), o["log_probs"].data_ptr(),
                   ws.data_ptr(), nb, None, *more)
        abi.check(rc, entry.__name__)
        torch.cuda.synchronize()
        n = self.B * self.L * A * H
        assert (buf[:GUARD] == FILL).all() and (buf[GUARD + n:] == FILL).all(), "a guard row was written"
        s = o.pop("scal").cpu().numpy()
        out = {k: v.cpu().numpy() for k, v in o.items()}
        out.update(dy=dy.transpose(1, 2).cpu().numpy(), policy_loss=s[0], entropy=s[1], ess=s[2])
        return out


RNN_SHAPES = [(1, 1, 1), (5, 4, 3), (11, 3, 7), (172, 16, 6)]
_CASES = {}


def _head_case(B, L, A, seed=None):
    key = (B, L, A, seed)
    if key not in _CASES:
        _CASES[key] = DC.stacked_head_case(B, L, A, 10 * B + L + A if seed is None else seed)
    return _CASES[key]


@pytest.mark.parametrize("B,L,A", RNN_SHAPES)
@pytest.mark.parametrize("strided", [True, False])
def test_one_rank_recurrent_global_entry_has_the_local_entrys_bits(B, L, A, strided):
    gpa = min(-(-B * L // TR.R_ROWS), TR.G_MAX // A)             # csrc/hns_rnn_train.hip: rt_groups_per_agent
    assert (B * L > TR.R_ROWS * gpa) == (B == 172) and ((B, L, A) != (172, 16, 6) or (B * L, TR.R_ROWS * (TR.G_MAX // A)) == (2752, 2720))
    assert (B, L, A) != (11, 3, 7) or B * L == TR.R_ROWS + 1     # a second trip that holds one row
    k = ACall(_head_case(B, L, A), strided=strided)
    want = k.agents(fill=0x00)
    for fill in (0x7F, 0xFF):
        got = k.agents(glob=(B * L * A, 1.0), fill=fill)
        for n in TR.ACTOR_OUT:
            assert got[n].shape == want[n].shape and got[n].tobytes() == want[n].tobytes(), f"{B}x{L}x{A} {n} differs from the local entry"


def _two_parts(c, sizes, dead=None):
    parts, ids = DU.split(c, sizes), DU.segment_ids(sizes)
    B = sum(sizes)
    rows = int(np.prod(c["y"].shape[:3]))
    calls = []
    for r, (p, seg) in enumerate(zip(parts, ids)):
        seg = seg.copy()
        if dead is not None and dead[0] == r:
            seg[dead[1]] = B + 3
        calls.append(ACall(p, segment=seg, nseg=B))
    a = [k.agents(glob=(rows, 0.5)) for k in calls]
    add = lambda x, y: (x.astype(np.float32) + y.astype(np.float32))      # noqa: E731  (the all-reduce: one fp32 addition per entry)
    out = {"dy": np.concatenate([x["dy"] for x in a]), "log_probs": np.concatenate([x["log_probs"] for x in a]),
           "policy_loss": np.float64(a[0]["policy_loss"]) + np.float64(a[1]["policy_loss"]), "entropy": a[0]["entropy"]}
    out.update({n: add(a[0][n], a[1][n]) for n in ("d_head_w", "d_head_b", "d_log_std")})
    assert a[0]["entropy"].tobytes() == a[1]["entropy"].tobytes()
    return out


NAMES = ("dy", "d_head_w", "d_head_b", "d_log_std", "policy_loss", "entropy")


@pytest.mark.parametrize("sizes,L,A", [((5, 11), 4, 3), ((1, 171), 16, 6)])
def test_two_emulated_recurrent_ranks_meet_the_gate_over_the_union(sizes, L, A):
    c = _head_case(sum(sizes), L, A) if sum(sizes) == 172 else _head_case(sum(sizes), L, A, 2024)
    a64, a32 = DC.stacked_head_autograd(c, torch.float64), DC.stacked_head_autograd(c, torch.float32)
    DC.assert_off_the_clip(a64, a32)
    out = _two_parts(c, sizes)
    worst, bad = U.gate(f"{sizes[0]}+{sizes[1]}", DC.head_items("", out, a64, a32, NAMES + ("log_probs",), A))
    assert not bad, "; ".join(bad)


def test_a_dead_segment_in_part_1_leaves_n_at_global_rows():
    sizes, L, A = (5, 11), 4, 3
    c = _head_case(sum(sizes), L, A, 2024)
    rows = sum(sizes) * L * A
    dead_b = sizes[0] + 4                                        # segment 4 of part 1
    keep = [b for b in range(sum(sizes)) if b != dead_b]
    a64, a32 = (DC.stacked_head_autograd(c, dt, keep=keep, global_rows=rows) for dt in (torch.float64, torch.float32))
    DC.assert_off_the_clip(a64, a32)
    out = _two_parts(c, sizes, dead=(1, 4))
    assert not out["dy"][dead_b].any() and np.isnan(out["log_probs"][dead_b]).all()         # a dead row's log_probs are not written
    out["log_probs"] = out["log_probs"][keep]
    worst, bad = U.gate("dead segment", DC.head_items("", out, a64, a32, NAMES + ("log_probs",), A))
    assert not bad, "; ".join(bad)


# ---------------------------------------------------------------------------------------------------------------- refusals
REFUSALS = ("global_rows_short", "nan_share", "inf_share", "null_policy_loss")


@pytest.mark.parametrize("what", REFUSALS)
def test_the_plain_entry_refuses_with_an_error_and_writes_nothing(what):
    lib = abi.load_library()
    A, K, D, S, B = 3, 5, 35, 8, 5
    actors, obs, action, lpo, adv, index = _plain_case(A, K, D, S, B, 77)
    live = {k: torch.as_tensor(v.copy()).cuda() for k, v in actors.items()}
    p = AT.actor_parameters_per_agent(live)
    for t in p.values():
        t.grad = torch.full_like(t, FILL)
    d = lambda x: torch.as_tensor(np.ascontiguousarray(x)).cuda()           # noqa: E731
    xs, xo, xc = PT.as_rollout(d(obs["state_self"]), d(obs["state_others"]), d(obs["cylinders"]))
    act, old, ad, idx = d(action), d(lpo), d(adv), d(index)
    shape = PT.validate("actor", {k: v[0] for k, v in p.items()}, xs, xo, xc, (("action", act, 4), ("log_probs_old", old, 1), ("advantages", ad, 1)), idx, True)
    scal_in = torch.full((4,), FILL, device="cuda")
    net, grd, b, ws, nbytes, scal, _, st = PT.prepare_call("actor", p, xs, xo, xc, idx, shape, lib.hns_actor_train_agents_workspace_bytes, None, scal_in, 4,
                                                           abi.HnsActorBatch)
    b.action, b.log_probs_old, b.advantages = act.data_ptr(), old.data_ptr(), ad.data_ptr()
    logp = torch.full((B, A, 1), FILL, device="cuda")
    arg = dict(n=B * A, share=1.0, loss=scal[0:].data_ptr())
    if what == "global_rows_short":
        arg["n"] = B * A - 1
    elif what == "nan_share":
        arg["share"] = float("nan")
    elif what == "inf_share":
        arg["share"] = float("inf")
    else:
        arg["loss"] = None
    rc = lib.hns_actor_train_grad_agents_global(C.byref(net), C.byref(b), D, A, K, 0.1, 1e-3, C.byref(grd), arg["loss"], scal[1:].data_ptr(), scal[2:].data_ptr(),
                                                None, logp.data_ptr(), ws.data_ptr(), nbytes, st, arg["n"], arg["share"])
    assert rc != 0 and lib.hns_last_error().decode().startswith("hns_actor_train_grad_agents_global:"), (what, lib.hns_last_error())
    torch.cuda.synchronize()
    assert (scal == FILL).all() and (logp == FILL).all() and all(bool((t.grad == FILL).all()) for t in p.values()), what


@pytest.mark.parametrize("what", REFUSALS)
def test_the_recurrent_entry_refuses_with_an_error_and_writes_nothing(what):
    lib = abi.load_library()
    B, L, A = 3, 5, 2
    k = ACall(_head_case(B, L, A, 9))
    rows_n = B * L * A
    fill = lambda *s: torch.full(s, FILL, device="cuda")         # noqa: E731
    nb = lib.hns_rnn_actor_head_agents_workspace_bytes(B, A, L)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    pad = fill(rows_n * H)
    dy = pad.view(B, L, A, H).transpose(1, 2)
    outs = [fill(A, 4, H), fill(A, 4), fill(A, 4), fill(4), fill(B, L, A)]
    arg = dict(n=rows_n, share=1.0, loss=outs[3].data_ptr())
    if what == "global_rows_short":
        arg["n"] = rows_n - 1
    elif what == "nan_share":
        arg["share"] = float("nan")
    elif what == "inf_share":
        arg["share"] = float("inf")
    else:
        arg["loss"] = None
    h, r, rows = k.head, k.rows, k.struct()
    rc = lib.hns_rnn_actor_head_grad_agents_global(h["head_w"].data_ptr(), h["head_b"].data_ptr(), h["log_std"].data_ptr(), C.byref(rows), r["action"].data_ptr(),
                                                   r["log_probs_old"].data_ptr(), r["advantages"].data_ptr(), 0.1, 1e-3, dy.data_ptr(), outs[0].data_ptr(),
                                                   outs[1].data_ptr(), outs[2].data_ptr(), arg["loss"], outs[3][1:].data_ptr(), outs[3][2:].data_ptr(),
                                                   outs[4].data_ptr(), ws.data_ptr(), nb, None, arg["n"], arg["share"])
    assert rc != 0 and lib.hns_last_error().decode().startswith("hns_rnn_actor_head_grad_agents_global:"), (what, lib.hns_last_error())
    torch.cuda.synchronize()
    for t in (pad, *outs):
        assert (t == FILL).all(), what


# ---------------------------------------------------------------------------------------------------------------- the learners
@pytest.fixture
def one_rank_group(tmp_path):
    import torch.distributed as dist
    assert not dist.is_initialized()
    dist.init_process_group("gloo", rank=0, world_size=1, store=dist.FileStore(str(tmp_path / "store"), 1))
    yield dist.group.WORLD
    dist.destroy_process_group()


def test_a_one_rank_group_trains_as_the_per_agent_learner_without_one(one_rank_group):
    """DeviceLearner(group=)'s rule (tests/test_hip_dp_learner.py): max_grad_norm above every norm, everything bit-identical but the two
    gradient-norm columns, which lie within one unit in the last place."""
    cfg = copy.deepcopy(DC.CFG_PLAIN)
    cfg.update(max_grad_norm=1e9)
    cpu = DC.plain_state(DC.A, 61)
    ro = DC.to_device(DC.plain_rollout(cpu, 8, 8, DC.A, 62), "cuda")
    runs = []
    for group in (None, one_rank_group):
        state = PC.clone_state(cpu, "cuda")
        args = dict(tp_net=state["tp"], value_normalizer=state["vn"], generator=torch.Generator(device="cuda").manual_seed(9))
        lrn = learner.PerAgentDeviceLearner(state["actor"], state["critic"], cfg, **args) if group is None else \
            learner.DataParallelPerAgentLearner(state["actor"], state["critic"], cfg, group=group, **args)
        info = lrn.train_rollout(**ro)
        torch.cuda.synchronize()
        runs.append((LC.state_tensors(state, LC.learner_opts(lrn)), info))
    LC.assert_same_state(runs[1][0], runs[0][0], "a one-rank group against no group")
    plain, grouped = runs[0][1], runs[1][1]
    assert set(plain) == set(grouped) == {f"drone/{k}" for k in learner.INFO_KEYS}
    for k in plain:
        if k.endswith("_grad_norm"):
            assert DR.ulps(plain[k], grouped[k]) <= 1, (k, plain[k], grouped[k])
        else:
            assert plain[k] == grouped[k] and np.isfinite(plain[k]), (k, plain[k], grouped[k])


def test_a_one_rank_group_trains_as_the_recurrent_per_agent_learner_without_one(one_rank_group):
    """DataParallelRecurrentLearner's rule (tests/test_hip_dp_rnn_learner.py): bit identity of the info row and of every tensor."""
    actor, critic = DC.rnn_nets(DC.A, 900)
    kw, rk = (DC.to_device(x, "cuda") for x in DC.rnn_rollout(5, DC.T, DC.A, DC.L, 70))
    runs = []
    for group in (None, one_rank_group):
        a, c = ({k: v.clone().cuda() for k, v in p.items()} for p in (actor, critic))
        args = dict(tp_net=DC.predictor(DC.A, 41).cuda(), value_normalizer=learner.ValueNorm1().cuda(), generator=torch.Generator(device="cuda").manual_seed(7))
        lrn = learner.PerAgentRecurrentDeviceLearner(a, c, DC.CFG_RNN, **args) if group is None else \
            learner.DataParallelPerAgentRecurrentLearner(a, c, DC.CFG_RNN, group=group, **args)
        info = lrn.train_rollout(**kw, **rk)
        torch.cuda.synchronize()
        runs.append((info, DC.rnn_snapshot(lrn)))
    (i0, s0), (i1, s1) = runs
    assert list(i0) == list(i1) == [f"drone/{k}" for k in learner.INFO_KEYS]
    for k in i0:
        assert np.float32(i0[k]) == np.float32(i1[k]) and np.isfinite(i0[k]), (k, i0[k], i1[k])
    assert len(s0) == len(s1) and all(torch.equal(x, y) for x, y in zip(s0, s1))
    assert not torch.equal(s0[0], next(iter(actor.values())).cuda())                           # the parameters moved


@pytest.mark.timeout(400)
@pytest.mark.parametrize("which", ["plain", "rnn"])
def test_two_ranks_on_one_gpu_over_gloo(tmp_path, which):
    """tests/dp_per_agent_learner_job.py, one child process a rank, each under its own time limit; both ranks share cuda:0 and the
    collectives run over gloo — a correctness run.  The parent stops at the first non-zero status.  The ranks end with one sha256 over their
    stacked actor, critic, predictor, Adam states and ValueNorm1, and with equal info rows."""
    job = os.path.join(ROOT, "tests", "dp_per_agent_learner_job.py")
    logs = [open(tmp_path / f"rank{r}.log", "w+") for r in range(2)]
    procs = [subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, job, "--which", which, "--rank", str(r), "--world", "2", "--store",
                               str(tmp_path / "store"), "--out", str(tmp_path)], stdout=logs[r], stderr=subprocess.STDOUT, cwd=ROOT) for r in range(2)]
    done, status = queue.Queue(), [None, None]
    waiters = [threading.Thread(target=lambda r=r, p=p: done.put((r, p.wait())), daemon=True) for r, p in enumerate(procs)]
    for w in waiters:
        w.start()
    try:
        for _ in procs:
            r, code = done.get(timeout=300)                      # (the children end under their own time limits first)
            status[r] = code
            if code != 0:
                break                                            # nothing goes on after a failed rank
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
            p.wait()

    def tail(r):
        logs[r].seek(0)
        return logs[r].read()[-3000:]
    assert status == [0, 0], f"statuses {status}\nrank 0:\n{tail(0)}\nrank 1:\n{tail(1)}"
    reps = [json.load(open(tmp_path / f"rank{r}.json")) for r in range(2)]
    assert reps[0]["digest"] == reps[1]["digest"] and reps[0]["start"] == reps[1]["start"] != reps[0]["digest"]
    assert reps[0]["infos"] == reps[1]["infos"] and len(reps[0]["infos"]) == 2
    assert [r["envs"] for r in reps] == [3, 5]                   # unequal shards
    for info in reps[0]["infos"]:
        assert list(info) == [f"drone/{k}" for k in learner.INFO_KEYS] and all(np.isfinite(v) for v in info.values()), info
