"""The composed recurrent update on an MI355X past one tile of each of its ops (hns_amd.rnn_train.policy_loss_and_grad_rnn /
value_loss_and_grad_rnn: encoder op -> GRU op -> head entry -> GRU backward -> encoder backward through one RnnWorkspace)
against rnn_update_reference.flow, fp64 autograd of the reference's statements.  The cases, what each reaches and why its seed was chosen:
tests/rnn_update_cases.py; their plans, well-posedness and the teeth of this gate (six plan-limited defects that fail it on the cases below and
are invisible at test_hip_rnn_train.py's 5-segment shape): tests/test_rnn_update_edges.py.

  * the gate: every case x {actor, critic}, U.gate unchanged (bar 8: e <= 8 max(e_32, 2^-24 max|ref_64|)) on every gradient tensor, every
    scalar, log_probs / values and grad_norm, the preconditions asserted first;
  * workspaces: at `default` and `encoder-ranges` the same bits from a fresh RnnWorkspace, from one that `longest` used just before (every
    buffer larger and dirty) and from the call repeated, one gradient bucket serving the three;
  * a bad id: `default` with one id replaced by -1 and by NS + 7 (check_index=False) gives the same bits, and passes the gate against the flow on
    the kept segments rescaled to n = B L A (rnn_update_cases.rescaled_flow);
  * the one-rank global form at `encoder-ranges`: the actor with global_rows = its own rows and entropy_share 1, the critic through
    value_loss_sums_rnn -> value_loss_and_grad_rnn(sums=, global_rows=, forward=), bit for bit the local calls;
  * RecurrentDeviceLearner.train_rollout at [24 envs, 32 steps, 3 agents], L 16, 2 epochs x 2 minibatches of 24 segments (72 sequences, five
    GRU tiles), predictor on, on the device against the same call on CPU tensors.

Worst ratio per case (RATIOS, printed by test_report_ratios), recorded on an MI355X:
    default 0.94 / 2.00   encoder-ranges 1.78 / 2.25   longest 0.90 / 1.83   widest 1.13 / 1.88   (actor / critic)
    second-trips 1.74 / 1.50   ess-columns 1.06 / 1.59   one-step 1.45 / 3.03   one-segment 1.09 / 1.47   bad-id 1.01 / 2.21
The file's wall time on an MI355X: 11.7 s for the 26 tests, the fp64 and fp32 flows on the host included; the slowest test 2.2 s (second-trips)."""
import math

import numpy as np
import pytest
import torch

import rnn_update_cases as RC
import rnn_update_reference as U
from hns_amd import rnn_train

pytestmark = pytest.mark.gpu

RATIOS = {}
NETS = [True, False]
net_id = lambda actor: "actor" if actor else "critic"           # noqa: E731


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _same_bits(x, y, rows=None):
    """Every output of RC.outputs equal bit for bit (rows: the minibatch positions of log_probs / values that are compared)."""
    assert set(x) == set(y)
    for k in x:
        a, b = (x[k][rows], y[k][rows]) if rows is not None and k in ("log_probs", "values") else (x[k], y[k])
        assert np.array_equal(a, b), k


# ---------------------------------------------------------------------------------------------------------------- the gate
@pytest.mark.parametrize("actor", NETS, ids=net_id)
@pytest.mark.parametrize("tag", RC.TAGS)
def test_the_composed_update_against_the_independent_flow(tag, actor):
    b = RC.refs(tag, actor)
    bad, _ = RC.preconditions(b)
    assert not bad, bad
    out = RC.outputs(b, *RC.call(b, _dev))
    name = f"{tag}-{net_id(actor)}"
    worst, bad = U.gate(name, RC.items(b, out))
    RATIOS[name] = worst
    assert not bad, f"{name}: " + "; ".join(bad)


# ---------------------------------------------------------------------------------------------------------------- workspaces
@pytest.mark.parametrize("actor", NETS, ids=net_id)
@pytest.mark.parametrize("tag", ["default", "encoder-ranges"])
def test_same_bits_from_a_fresh_a_larger_dirty_and_a_reused_workspace(tag, actor):
    b, big = RC.refs(tag, actor), RC.refs("longest", actor)
    p, q = RC.plan(b.case), RC.plan(big.case)
    for k in ("rows", "seqs", "gru_bytes", "enc_bytes", "actor_head_bytes", "critic_head_bytes"):
        assert q[k] > p[k], k                                    # every buffer of `longest` is the larger one
    live = {k: _dev(v) for k, v in b.net.items()}
    bucket = rnn_train.make_bucket(live, actor)
    fresh = RC.outputs(b, *RC.call(b, _dev, live=live, bucket=bucket, workspace=rnn_train.RnnWorkspace()))
    ws = rnn_train.RnnWorkspace()
    RC.call(big, _dev, workspace=ws)
    sizes = {k: t.numel() for k, t in ws._t.items()}
    dirty = RC.outputs(b, *RC.call(b, _dev, live=live, bucket=bucket, workspace=ws))
    assert sizes == {k: t.numel() for k, t in ws._t.items()} and len(sizes) >= 8     # nothing regrew: slices of the larger buffers
    again = RC.outputs(b, *RC.call(b, _dev, live=live, bucket=bucket, workspace=ws))
    _same_bits(fresh, dirty)
    _same_bits(fresh, again)
    assert not U.gate(tag, RC.items(b, dirty), verbose=False)[1]


# ---------------------------------------------------------------------------------------------------------------- a bad id
@pytest.mark.parametrize("actor", NETS, ids=net_id)
def test_an_out_of_range_id_in_the_composed_call_contributes_nothing(actor):
    b = RC.refs("default", actor)
    B, NS = b.case.B, RC.plan(b.case)["segments"]
    bad_at = next(i for i in range(4, B) if b.seg[i] not in (0, RC.flagged_segment(b.case)))   # the kept segments still hold both flagged ones
    keep = np.array([i for i in range(B) if i != bad_at])
    r64, r32 = RC.rescaled_flow(b, keep, torch.float64), RC.rescaled_flow(b, keep, torch.float32)
    kept = b._replace(g64=r64[0], s64=r64[1], g32=r32[0], s32=r32[1])
    bad, _ = RC.preconditions(kept)
    assert not bad, bad
    outs = []
    for bad_id in (-1, NS + 7):
        seg = b.seg.copy()
        seg[bad_at] = bad_id
        outs.append(RC.outputs(b, *RC.call(b, _dev, seg=seg, check_index=False)))
    _same_bits(*outs, rows=keep)
    name = f"bad-id-{net_id(actor)}"
    worst, bad = U.gate(name, RC.items(kept, outs[0], rows=keep))
    RATIOS[name] = worst
    assert not bad, f"{name}: " + "; ".join(bad)


# ---------------------------------------------------------------------------------------------------------------- the one-rank global form
def test_the_actors_global_entry_over_its_own_rows_gives_the_local_bits():
    b = RC.refs("encoder-ranges", True)
    live = {k: _dev(v) for k, v in b.net.items()}
    bucket = rnn_train.make_bucket(live, True)
    local = RC.outputs(b, *RC.call(b, _dev, live=live, bucket=bucket))
    glob = RC.outputs(b, *RC.call(b, _dev, live=live, bucket=bucket, global_rows=RC.plan(b.case)["rows"], entropy_share=1.0))
    _same_bits(local, glob)


def test_the_critics_sums_and_global_entry_over_its_own_rows_give_the_local_bits():
    b = RC.refs("encoder-ranges", False)
    live = {k: _dev(v) for k, v in b.net.items()}
    bucket = rnn_train.make_bucket(live, False)
    local = RC.outputs(b, *RC.call(b, _dev, live=live, bucket=bucket))
    obs = (_dev(b.obs["state_self"]), _dev(b.obs["state_others"]), _dev(b.obs["cylinders"]))
    args = (live, *obs, _dev(b.state), _dev(b.is_init), *(_dev(r) for r in b.rows))
    kw = dict(segment=_dev(b.seg), seq_len=b.case.L, workspace=rnn_train.RnnWorkspace())
    half = rnn_train.value_loss_sums_rnn(*args, **kw)
    res = rnn_train.value_loss_and_grad_rnn(*args, **kw, bucket=bucket, sums=half.sums, global_rows=RC.plan(b.case)["rows"], forward=half.forward)
    assert res.values is None
    glob = RC.outputs(b, live, res._replace(values=half.values))
    _same_bits(local, glob)


# ---------------------------------------------------------------------------------------------------------------- the learner
def test_the_learner_on_the_device_agrees_with_the_cpu_path_on_the_info_row(monkeypatch):
    """One RecurrentDeviceLearner.train_rollout at [24, 32, 3], L 16, on CPU tensors and on the device, from the same parameters and the
    same rollout (collected once on the CPU: test_hip_rnn_learner._rollout), every permutation — the predictor's and the segments' — drawn
    from ONE CPU generator (the two devices' generators differ).  The bound is
    test_hip_per_agent.py::test_the_device_agrees_with_the_cpu_path_on_the_info_row's, with its reason: every scalar of the row is a mean over
    the 4 updates of numbers the update gate holds to fp32's error at equal parameters; after a step the two sides' parameters differ by Adam
    steps on gradients that differ at fp32's error, which is second order for the scalars — |device - cpu| <= 1e-4 max(1, |cpu|), two decades
    above fp32's error over such means and two below a change that matters.
    Measured on an MI355X: the largest difference 2.4e-7 (actor_grad_norm 2.643), the others at most 3.0e-8, seven of twelve entries equal."""
    import test_hip_rnn_learner as TL
    from hns_amd import learner
    N, T = 24, 32
    params, kw, rk = TL._rollout(N, T)
    M = TL.CFG["num_minibatches"]
    assert (N * (T // TL.L)) // M == 24 and RC.plan(RC.Case(3, 5, 35, N, T, TL.L, 24))["gru_tiles"] == 5
    infos = {}
    for device in ("cpu", "cuda"):
        gen = torch.Generator().manual_seed(7)
        monkeypatch.setattr(learner.tp_train, "minibatches", lambda n, m, dev, generator=None: torch.randperm((n // m) * m, generator=gen).reshape(m, -1).to(dev))
        actor, critic = ({k: v.clone().to(device) for k, v in p.items()} for p in params)
        lrn = learner.RecurrentDeviceLearner(actor, critic, TL.CFG, tp_net=U.predictor(3, 41).to(device), value_normalizer=learner.ValueNorm1().to(device))
        infos[device] = lrn.train_rollout(**{k: TL._to(v, device) for k, v in kw.items()}, **{k: TL._to(v, device) for k, v in rk.items()})
    assert set(infos["cpu"]) == set(infos["cuda"]) == {f"drone/{k}" for k in learner.INFO_KEYS}
    bad = []
    for k, c in infos["cpu"].items():
        d = infos["cuda"][k]
        print(f"  {k}: cpu {c:.7g} device {d:.7g} |diff| {abs(d - c):.2e}")
        if not abs(d - c) <= 1e-4 * max(1.0, abs(c)):
            bad.append(k)
    assert not bad, bad


def test_report_ratios():
    for tag, worst in sorted(RATIOS.items()):
        print(f"worst ratio {tag}: {worst:.2f}")
    assert all(math.isfinite(w) for w in RATIOS.values())
