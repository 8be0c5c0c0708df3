"""The recurrent update with one actor per agent on an MI355X (hns_amd.rnn_train.policy_loss_and_grad_rnn_per_agent /
update_actor_rnn_per_agent, learner.PerAgentRecurrentDeviceLearner: hns_encoder_*_agents -> hns_gru_*_agents ->
hns_rnn_actor_head_grad_agents -> one bucket, one norm, one ClippedAdam step over the 29 stacked tensors).  The cases, their
plans, what each reaches, the seed table and the teeth of the gate: tests/per_agent_rnn_update_cases.py, tests/test_per_agent_rnn_train.py.

  (a) per row and per sequence, bit for bit against the SHARED entries called with agent a's slices, for every agent a and every case: the
      encoder's features of rows (p, a); the GRU's out, h_last and h_hist, and dx and dh0, of sequences (b, a); the head's dy and log_probs of
      rows (., ., a).  These follow from the shared entries' row and sequence independence, and all of them hold.
  (b) the gate: every case, rnn_update_reference.gate unchanged (bar 8: e <= 8 max(e_32, 2^-24 max|ref_64|)) on every stacked gradient tensor
      AND every agent's slice of it, every scalar, log_probs and grad_norm, the preconditions asserted first.
  (c) composition: update_actor_rnn_per_agent's gradients and scalars within the gate and its step against the CPU path's; a cached workspace
      reused across two calls of different B gives the bits of fresh ones; an out-of-range segment id contributes nothing;
      PerAgentRecurrentDeviceLearner.train_rollout against the hand-driven device sequence bit for bit at N 8, T 32, L 16, A 3, 2 minibatches,
      1 epoch, predictor off; the parameters change for every agent; two agents with identical slices and rows end with identical slices;
      examples/per_agent_recurrent.py --learner trains the configuration end to end, the first minibatch's ratio 1 up to rounding.

Worst ratio per case, recorded on an MI355X (RATIOS, printed by test_report_ratios):
    default 1.77   second-tile 1.97   widest 1.58   longest 1.27   one-step 1.85   one-segment 2.37   second-trip 1.47   bad-id 1.36
The file's wall time on an MI355X: 8.4 s for its first 20 tests, the fp64 and fp32 flows on the host included; the slowest 2.5 s (second-trip)."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import per_agent_rnn_update_cases as PC
import rnn_update_reference as U
from hns_amd import abi, encoder, gae, learner, rnn, rnn_train
from hns_amd import policy as P
from hns_amd import policy_train as PT

pytestmark = pytest.mark.gpu

H = 128
RATIOS = {}


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _same_bits(x, y, rows=None):
    assert set(x) == set(y)
    for k in x:
        a, b = (x[k][rows], y[k][rows]) if rows is not None and k == "log_probs" else (x[k], y[k])
        assert np.array_equal(a, b), k


# ---------------------------------------------------------------------------------------------------------------- (a) bit for bit per op
def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _head(entry, query, hw, hb, ls, y, seg, NS, rows, dims):
    """One head entry on y [B, A, L, 128] (a view): (dy with y's layout as [B, L, A, 128], log_probs [B, L, A])."""
    B, L, A = dims
    nbytes = query(B, A, L)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dy = torch.zeros(B * L, A, H, device="cuda")
    g = [torch.empty_like(t) for t in (hw, hb, ls)]
    scal = torch.empty(3, device="cuda")
    logp = torch.empty(B, L, A, device="cuda")
    r = rnn_train._rows_struct(y, seg, NS)
    rc = entry(hw.data_ptr(), hb.data_ptr(), ls.data_ptr(), C.byref(r), *(t.data_ptr() for t in rows), 0.1, 1e-3, dy.data_ptr(), *(t.data_ptr() for t in g),
               scal[0:].data_ptr(), scal[1:].data_ptr(), scal[2:].data_ptr(), logp.data_ptr(), ws.data_ptr(), nbytes, _stream())
    abi.check(rc, entry.__name__)
    return dy.view(B, L, A, H), logp


@pytest.mark.parametrize("tag", PC.TAGS)
def test_rows_and_sequences_equal_the_shared_entries_on_agent_slices_bit_for_bit(tag):
    b = PC.refs(tag)
    A, K, D, N, T, L, B = b.case
    lib = abi.load_library()
    live = {k: _dev(v) for k, v in b.net.items()}
    net = rnn_train.network_parameters(live, True, stacked=True)
    xs, xo, xc = PT.as_rollout(_dev(b.obs["state_self"]), _dev(b.obs["state_others"]) if A > 1 else None, _dev(b.obs["cylinders"]))
    shape = PT.validate("actor", P.agent_slice(net.encoder, 0), xs, xo, xc, (), None, False)
    seg, NS = _dev(b.seg), N * (T // L)
    index = rnn_train._step_index(seg, L)
    state, is_init = _dev(b.state), _dev(b.is_init)
    h0, flags = rnn_train._gathered(state, is_init, seg, NS, A, L)
    rows = [_dev(r) for r in b.rows]
    g = torch.Generator(device="cuda").manual_seed(5)
    dout = (torch.randn(B * L, A, H, device="cuda", generator=g) * 0.1).view(B, L, A, H).transpose(1, 2)
    # the stacked entries
    feats = encoder.device_forward(net.encoder, xs, xo, xc, index, shape)                          # [B L, A, 128]
    x4 = feats.view(B, L, A, H).transpose(1, 2)
    y, h_last, hist = rnn.device_forward(net.gru, x4, h0, flags, True)
    _, dx, dh0 = rnn.device_backward(net.gru, x4, h0, flags, hist, dout, None, True)
    dy, logp = _head(lib.hns_rnn_actor_head_grad_agents, lib.hns_rnn_actor_head_agents_workspace_bytes, net.head["head_w"], net.head["head_b"],
                     net.head["log_std"], y, seg, NS, rows, (B, L, A))
    torch.cuda.synchronize()
    for a in range(A):
        f1 = encoder.device_forward(P.agent_slice(net.encoder, a), xs, xo, xc, index, shape)
        assert torch.equal(f1[:, a], feats[:, a]), f"features of agent {a}"
        y1, hl1, hist1 = rnn.device_forward(P.agent_slice(net.gru, a), x4, h0, flags, True)
        assert torch.equal(y1[:, a], y[:, a]) and torch.equal(hl1.view(B, A, H)[:, a], h_last.view(B, A, H)[:, a]), f"GRU forward of agent {a}"
        assert torch.equal(hist1.view(B, A, L, H)[:, a], hist.view(B, A, L, H)[:, a]), f"h_hist of agent {a}"
        _, dx1, dh1 = rnn.device_backward(P.agent_slice(net.gru, a), x4, h0, flags, hist1, dout, None, True)
        assert torch.equal(dx1[:, a], dx[:, a]) and torch.equal(dh1.view(B, A, H)[:, a], dh0.view(B, A, H)[:, a]), f"GRU backward of agent {a}"
        # the shared head with agent a's head over ALL rows, on the stacked entries' y
        dy1, logp1 = _head(lib.hns_rnn_actor_head_grad, lib.hns_rnn_actor_head_workspace_bytes, *(net.head[k][a] for k in ("head_w", "head_b", "log_std")),
                           y, seg, NS, rows, (B, L, A))
        assert torch.equal(dy1[:, :, a], dy[:, :, a]) and torch.equal(logp1[:, :, a], logp[:, :, a]), f"head of agent {a}"


# ---------------------------------------------------------------------------------------------------------------- (b) the gate
@pytest.mark.parametrize("tag", PC.TAGS)
def test_the_composed_update_against_the_independent_per_agent_flow(tag):
    b = PC.refs(tag)
    bad = PC.preconditions(b)
    assert not bad, bad
    out = PC.outputs(b, *PC.call(b, _dev))
    worst, bad = U.gate(tag, PC.items(b, out))
    RATIOS[tag] = worst
    assert not bad, f"{tag}: " + "; ".join(bad)


# ---------------------------------------------------------------------------------------------------------------- (c) composition
def test_update_actor_rnn_per_agent_steps_as_the_cpu_path_does():
    """One update on the device and on the CPU from the same parameters: the gradients and scalars within the gate; every agent's parameters
    change; and the stepped parameters agree to 2 lr — Adam's first step moves a value by lr g / (|g| + eps), at most lr, so two first steps
    on gradients of any two signs differ by at most 2 lr."""
    b = PC.refs("default")
    lr, got = 5e-4, {}
    for name, to in (("cpu", lambda v: torch.as_tensor(np.asarray(v)).clone()), ("cuda", _dev)):
        live = {k: to(v) for k, v in b.net.items()}
        opt = rnn_train.make_optimizer_per_agent(live, {"share_actor": False, "actor": {"lr": lr}})
        info = rnn_train.update_actor_rnn_per_agent(live, to(b.obs["state_self"]), to(b.obs["state_others"]), to(b.obs["cylinders"]), to(b.state),
                                                    to(b.is_init), *(to(r) for r in b.rows), opt, segment=to(b.seg), seq_len=b.case.L,
                                                    cfg={"entropy_coef": 1e-3})
        got[name] = (live, info)
    live, info = got["cuda"]
    res = rnn_train.ActorLoss(info["policy_loss"], info["entropy"], info["ESS"], info["actor_grad_norm"], _dev(b.s64["log_probs"]).unsqueeze(-1))
    out = PC.outputs(b, live, res)
    worst, bad = U.gate("update", [it for it in PC.items(b, out) if it[0] != "log_probs"])
    assert not bad, "; ".join(bad)
    for k, v in b.net.items():
        new, cpu = live[k].cpu().numpy(), got["cpu"][0][k].numpy()
        for a in range(b.case.A):
            assert not np.array_equal(new[a], v[a]), (k, a)
        assert np.abs(new - cpu).max() <= 2 * lr * (1 + 1e-6), k


def test_a_cached_workspace_reused_at_another_batch_gives_the_bits_of_fresh_ones():
    b, big = PC.refs("default"), PC.refs("second-tile")
    assert big.case.B > b.case.B and PC.plan(big.case)["gru_bytes"] > PC.plan(b.case)["gru_bytes"]
    live = {k: _dev(v) for k, v in b.net.items()}
    bucket = rnn_train.make_bucket(live, True, stacked=True)
    fresh = PC.outputs(b, *PC.call(b, _dev, live=live, bucket=bucket, workspace=rnn_train.RnnWorkspace()))
    ws = rnn_train.RnnWorkspace()
    big_fresh = PC.outputs(big, *PC.call(big, _dev, workspace=rnn_train.RnnWorkspace()))
    big_first = PC.outputs(big, *PC.call(big, _dev, workspace=ws))
    sizes = {k: t.numel() for k, t in ws._t.items()}
    dirty = PC.outputs(b, *PC.call(b, _dev, live=live, bucket=bucket, workspace=ws))
    assert sizes == {k: t.numel() for k, t in ws._t.items()} and len(sizes) >= 8       # nothing regrew: slices of the larger buffers
    small = rnn_train.RnnWorkspace()
    PC.call(b, _dev, workspace=small)
    regrown = PC.outputs(big, *PC.call(big, _dev, workspace=small))                    # ... and a workspace that regrows
    _same_bits(fresh, dirty)
    _same_bits(big_fresh, big_first)
    _same_bits(big_fresh, regrown)


def test_an_out_of_range_segment_id_contributes_nothing():
    b = PC.refs("default")
    B, NS = b.case.B, PC.plan(b.case)["segments"]
    import rnn_update_cases as RC
    bad_at = next(i for i in range(4, B) if b.seg[i] not in (0, RC.flagged_segment(b.case)))
    keep = np.array([i for i in range(B) if i != bad_at])
    r64, r32 = PC.rescaled_flow(b, keep, torch.float64), PC.rescaled_flow(b, keep, torch.float32)
    kept = b._replace(g64=r64[0], s64=r64[1], g32=r32[0], s32=r32[1])
    assert not PC.preconditions(kept)
    outs = []
    for bad_id in (-1, NS + 7):
        seg = b.seg.copy()
        seg[bad_at] = bad_id
        outs.append(PC.outputs(b, *PC.call(b, _dev, seg=seg, check_index=False)))
    _same_bits(*outs, rows=keep)
    worst, bad = U.gate("bad-id", PC.items(kept, outs[0], rows=keep))
    RATIOS["bad-id"] = worst
    assert not bad, "; ".join(bad)


def _to(x, dev):
    if torch.is_tensor(x):
        return x.to(dev)
    if isinstance(x, (tuple, list)):
        return tuple(_to(v, dev) for v in x)
    return x


def _learner(actor, critic, seed):
    a, c = ({k: v.clone().cuda() for k, v in p.items()} for p in (actor, critic))
    return learner.PerAgentRecurrentDeviceLearner(a, c, PC.LEARNER_CFG, value_normalizer=learner.ValueNorm1().cuda(),
                                                  generator=torch.Generator(device="cuda").manual_seed(seed))


def _snapshot(lrn):
    out = [v.detach().clone() for v in (*lrn.actor.values(), *lrn.critic.values())]
    for opt in (lrn.actor_opt, lrn.critic_opt):
        for st in opt.state_dict()["state"].values():
            out += [st["step"].clone().cuda(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
    vn = lrn.value_normalizer
    return out + [vn.running_mean.clone(), vn.running_mean_sq.clone(), vn.debiasing_term.clone()]


def _by_hand(lrn, kw, rk):
    """train_rollout's blocks through the public calls, every workspace allocated by the call that needs it."""
    xs, xo, xc = kw["obs_self"], kw["obs_others"], kw["obs_cylinders"]
    N, T = kw["reward"].shape[:2]
    L, M = lrn.train_seq_len, lrn.num_minibatches
    nv = lrn.policy.forward(*kw["next_obs_last"], critic_state=rk["last_critic_rnn_state"], is_init=rk["last_is_init"], value_only=True).value
    adv, ret, _, (am, asd) = gae.rollout_targets(kw["reward"], kw["done"].unsqueeze(-1), kw["state_value"], nv, lrn.gamma, lrn.gae_lambda,
                                                 value_normalizer=lrn.value_normalizer, normalize_advantages=True, return_moments=True)
    table = torch.empty(lrn.ppo_epochs * M, len(learner.COLUMNS), device="cuda")
    m = 0
    for _ in range(lrn.ppo_epochs):
        perm = torch.randperm((N * (T // L) // M) * M, device="cuda", generator=lrn.generator).reshape(M, -1)
        for idx in perm:
            rnn_train.update_actor_rnn_per_agent(lrn.actor, xs, xo, xc, rk["actor_rnn_state"], rk["is_init"], kw["action"], kw["log_probs"], adv,
                                                 lrn.actor_opt, segment=idx, cfg=lrn.cfg, out=table[m, :4])
            rnn_train.update_critic_rnn(lrn.critic, xs, xo, xc, rk["critic_rnn_state"], rk["is_init"], kw["state_value"], ret, lrn.critic_opt,
                                        segment=idx, cfg=lrn.cfg, out=table[m, 4:])
            m += 1
    head = lrn._info_row(kw["action"], table).tolist()
    info = dict(zip(learner.COLUMNS + ("action_norm",), head))
    info["advantages_mean"], info["advantages_std"] = float(am), float(asd)
    info["value_running_mean"] = float(lrn.value_normalizer.running_mean.mean())
    return {f"drone/{k}": info[k] for k in learner.INFO_KEYS if k in info}


def test_train_rollout_equals_the_hand_driven_device_calls_bit_for_bit():
    case = PC.Case(3, 5, 35, 8, 32, 16, 8)
    actor, critic, kw, rk = PC.learner_rollout(case, 900)
    kw, rk = {k: _to(v, "cuda") for k, v in kw.items()}, {k: _to(v, "cuda") for k, v in rk.items()}
    a, b = _learner(actor, critic, 7), _learner(actor, critic, 7)
    assert isinstance(a.policy, P.PerAgentRecurrentDevicePolicy) and a.ppo_epochs == 1 and a.num_minibatches == 2 and not a.use_tp
    loop = a._ppo_loop

    def guarded(*args, **kwargs):                                # a host synchronisation inside the PPO loop raises
        torch.cuda.set_sync_debug_mode("error")
        try:
            return loop(*args, **kwargs)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    a._ppo_loop = guarded
    ia, ib = a.train_rollout(**kw, **rk), _by_hand(b, kw, rk)
    assert list(ia) == list(ib) and len(ia) >= len(learner.COLUMNS) + 3
    for k in ia:
        assert np.float32(ia[k]) == np.float32(ib[k]) and np.isfinite(ia[k]), (k, ia[k], ib[k])
    sa, sb = _snapshot(a), _snapshot(b)
    assert len(sa) == len(sb) and all(torch.equal(x, y) for x, y in zip(sa, sb))
    for k, v in actor.items():                                   # the parameters moved, for every agent
        for ag in range(case.A):
            assert not torch.equal(a.actor[k][ag].cpu(), v[ag]), (k, ag)


def test_two_agents_with_identical_slices_and_rows_end_with_identical_slices():
    b = PC.refs("second-tile")
    net = {k: v.copy() for k, v in b.net.items()}
    for v in net.values():
        v[1] = v[0]
    twin = lambda x: np.concatenate([x[:, :, :1], x[:, :, :1], x[:, :, 2:]], 2)       # noqa: E731  agent 1's rows := agent 0's
    obs = {k: twin(v) for k, v in b.obs.items()}
    live = {k: _dev(v) for k, v in net.items()}
    opt = rnn_train.make_optimizer_per_agent(live, {"share_actor": False})
    rnn_train.update_actor_rnn_per_agent(live, _dev(obs["state_self"]), _dev(obs["state_others"]), _dev(obs["cylinders"]), _dev(twin(b.state)),
                                         _dev(b.is_init), *(_dev(twin(r)) for r in b.rows), opt, segment=_dev(b.seg), seq_len=b.case.L)
    for k, v in live.items():
        assert torch.equal(v[0], v[1]), k
        assert not torch.equal(v[0], v[2]) and not np.array_equal(v[0].cpu().numpy(), net[k][0]), k
        assert torch.equal(v.grad[0], v.grad[1]), k


def test_the_example_trains_the_configuration_through_the_learner():
    """The first minibatch's new log-probabilities against the stored ones before any step: the same kernels' arithmetic in another
    summation order (the policy step's fused GRU against the GRU op), so |ratio - 1| is fp32 rounding of a log-probability of order 10:
    asked below 1e-4 (recurrent_policy.py reports the same figure for the shared actor)."""
    script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "per_agent_recurrent.py")
    run = subprocess.run([sys.executable, script, "--envs", "64", "--steps", "16", "--seq-len", "8", "--learner", "--updates", "1"], capture_output=True,
                         text=True, timeout=240)
    assert run.returncode == 0, run.stdout + run.stderr
    first = next(ln for ln in run.stdout.splitlines() if ln.startswith("first minibatch, before any step"))
    assert float(re.search(r"= ([0-9.e+-]+)$", first).group(1)) < 1e-4, first
    for it in (0, 1):
        line = next(ln for ln in run.stdout.splitlines() if ln.startswith(f"rollout {it}: "))
        for k in learner.INFO_KEYS:
            assert f"{k} " in line, (k, line)
    assert "bit for bit the first's" in run.stdout


def test_report_ratios():
    for tag, worst in sorted(RATIOS.items()):
        print(f"worst ratio {tag}: {worst:.2f}")
    assert all(math.isfinite(w) for w in RATIOS.values())
