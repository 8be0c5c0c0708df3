"""The data-parallel per-agent learners on the CPU (learner.DataParallelPerAgentLearner, learner.DataParallelPerAgentRecurrentLearner, the
`*_per_agent_global` functions of actor_train and rnn_train): two gloo ranks perform ONE update of one actor per agent per
minibatch on the union of their minibatches.  The device entries: tests/test_hip_dp_per_agent.py.  The cases: tests/dp_per_agent_cases.py.

One spawn of two workers runs every case and hands numpy results to the tests:
  learner   both classes: 3 and 5 envs x 8 steps, A 3, 2 cylinders, 2 epochs x 2 minibatches, predictor on, L 4 for the recurrent class
            (global_rows 96 in both); rank 1 starts from OTHER weights and, in the second rollout, its TP_done selects no window.  After two
            train_rollouts the ranks' stacked parameters, Adam states, ValueNorm1 and info rows are bit-identical.
  grads     both forms: the first minibatch through the `*_per_agent_global` calls with group=, each rank's units the first minibatch of its
            own permutation.  The all-reduced gradients (each stacked tensor AND each agent's slice), the summed policy_loss shares, the
            entropy and every row of log_probs meet the gate e <= 8 max(e_32, 2^-24 max|ref_64|) against the fp64 per-agent flow over the
            union (actor_per_agent_reference.loss_and_grad / per_agent_rnn_update_cases.flow); off the clip by 1e-3 in fp64 and fp32 on the
            same side of it are asserted on the union first.  The entropy term separately: with entropy_coef 0 and 0.3 the summed d log_std
            differ by -0.3 / A per agent — once, not W times (to 16 fp32 roundings of the larger gradient: each side is a sum whose last
            addition alone rounds differently).
  refusals  ranks that disagree on the number of agents or on train_seq_len, a rank with fewer units than minibatches: ValueError on every
            rank before the updates, on a group with a 20 s timeout, so a collective entered by one rank alone shows as an error.
  The two local learners given group= still raise NotImplementedError and name the new classes.
In this process: a missing group= raises ValueError; the two local rnn_train functions still raise and name the new ones; with one rank
(global_rows = own rows, entropy_share 1) the CPU path has the bits of the group-less CPU path."""
import datetime
import os
import sys
import traceback

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _paths():
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import hns_amd  # noqa: F401


def _np(ts):
    return [t.detach().cpu().numpy().copy() for t in ts]


def _case_learner_plain(rank):
    import dp_per_agent_cases as DC
    from hns_amd import learner
    N = DC.ENVS[rank]
    state = DC.plain_state(DC.A, 51 + 10 * rank)                 # other weights on every rank, until the broadcast
    first = [v.detach().clone() for v in state["actor"].values()]
    lrn = learner.DataParallelPerAgentLearner(state["actor"], state["critic"], DC.CFG_PLAIN, tp_net=state["tp"], value_normalizer=state["vn"],
                                              generator=torch.Generator().manual_seed(100 + rank), group="world")
    start = _np(state["actor"].values())
    moved = not all(torch.equal(a, b) for a, b in zip(first, state["actor"].values()))
    infos = []
    for it in range(2):
        ro = DC.plain_rollout(state, N, DC.T, DC.A, 60 + rank + 10 * it, tp_windows=not (it == 1 and rank == 1))
        infos.append(lrn.train_rollout(**ro))
    return {"start": start, "moved_at_start": moved, "infos": infos, "state": _np(DC.plain_snapshot(state, lrn)), "updates": lrn.n_updates,
            "bucket": [tuple(v.shape) for v in lrn.actor_bucket.views]}


def _case_learner_rnn(rank):
    import dp_per_agent_cases as DC
    from hns_amd import learner
    N = DC.ENVS[rank]
    actor, critic = DC.rnn_nets(DC.A, 900 + 10 * rank)
    first = [v.clone() for v in actor.values()]
    lrn = learner.DataParallelPerAgentRecurrentLearner(actor, critic, DC.CFG_RNN, tp_net=DC.predictor(DC.A, 41 + rank), value_normalizer=learner.ValueNorm1(),
                                                       generator=torch.Generator().manual_seed(100 + rank), group="world")
    start = _np(actor.values())
    moved = not all(torch.equal(a, b) for a, b in zip(first, actor.values()))
    infos = []
    for it in range(2):
        kw, rk = DC.rnn_rollout(N, DC.T, DC.A, DC.L, 70 + rank + 10 * it, tp_windows=not (it == 1 and rank == 1))
        infos.append(lrn.train_rollout(**kw, **rk))
    return {"start": start, "moved_at_start": moved, "infos": infos, "state": _np(DC.rnn_snapshot(lrn)), "updates": lrn.n_updates,
            "bucket": [tuple(v.shape) for v in lrn.actor_bucket.views]}


def _case_grads(rank):
    import dp_per_agent_cases as DC
    from hns_amd import actor_train as AT
    from hns_amd import policy_train as PT
    from hns_amd import rnn_train
    out = {}
    data = DC.plain_union()
    part = DC.plain_part(data, rank)
    assert part[-1].numel() * DC.A < DC.GLOBAL_ROWS
    for coef in (1e-3, 0.0, 0.3):
        live = {k: torch.as_tensor(v.copy()) for k, v in data[0].items()}
        res = AT.policy_loss_and_grad_per_agent_global(live, *part[:6], part[6], entropy_coef=coef, global_rows=DC.GLOBAL_ROWS, entropy_share=0.5,
                                                       group=dist.group.WORLD, bucket=PT.GradBucket(live))
        out[("plain", coef)] = {"grads": {k: v.grad.numpy().copy() for k, v in live.items()}, "policy_loss": float(res.policy_loss),
                                "entropy": float(res.entropy), "grad_norm": float(res.grad_norm), "log_probs": res.log_probs.numpy().copy()}
    b, local = DC.rnn_union()
    part = DC.rnn_part(b, local, rank)
    for coef in (1e-3, 0.0, 0.3):
        live = {k: torch.as_tensor(np.asarray(v)).clone() for k, v in b.net.items()}
        res = rnn_train.policy_loss_and_grad_rnn_per_agent_global(live, *part[:8], segment=part[8], seq_len=DC.L, entropy_coef=coef,
                                                                  global_rows=DC.GLOBAL_ROWS, entropy_share=0.5, group=dist.group.WORLD,
                                                                  bucket=rnn_train.make_bucket(live, True, stacked=True))
        out[("rnn", coef)] = {"grads": {k: v.grad.numpy().copy() for k, v in live.items()}, "policy_loss": float(res.policy_loss),
                              "entropy": float(res.entropy), "grad_norm": float(res.grad_norm), "log_probs": res.log_probs.squeeze(-1).numpy().copy()}
    return out


def _case_refusals(rank):
    import dp_per_agent_cases as DC
    from hns_amd import learner
    group = dist.new_group(ranks=[0, 1], backend="gloo", timeout=datetime.timedelta(seconds=20))
    out = {}

    def run(name, lrn, params, rollout):
        before = _np(params)
        try:
            lrn.train_rollout(**rollout)
            out[name] = ("no error", "")
        except Exception as e:                                   # noqa: BLE001  (the type is what the test asserts)
            out[name] = (type(e).__name__, str(e))
        probe = torch.ones(1)
        dist.all_reduce(probe, group=group)                      # the ranks are still in step: nobody waits in a collective of the refused call
        out[name] += (float(probe), all(np.array_equal(a, b) for a, b in zip(before, _np(params))) and lrn.n_updates == 0)

    off = dict(DC.CFG_PLAIN, use_TP_net=0)
    # (the stacked tensors have 3 agents on both ranks — the construction broadcast needs one shape; rank 1's ROLLOUT holds 2 agents)
    for name, agents, n, steps in (("plain-agents", (3, 2)[rank], 2, DC.T), ("plain-short", 3, 2 - rank, (DC.T, 1)[rank])):
        state = DC.plain_state(3, 51)
        lrn = learner.DataParallelPerAgentLearner(state["actor"], state["critic"], off, value_normalizer=state["vn"], group=group)
        ro = {k: v for k, v in DC.plain_rollout(state, n, steps, agents, 5).items() if k != "tp"}
        run(name, lrn, list(state["actor"].values()), ro)
    for name, agents, n, steps, seq in (("rnn-agents", (3, 2)[rank], 2, DC.T, DC.L), ("rnn-seq_len", 3, 2, DC.T, (4, 2)[rank]),
                                        ("rnn-short", 3, 2 - rank, (DC.T, DC.L)[rank], DC.L)):
        cfg = dict(DC.CFG_RNN, use_TP_net=0, actor={"rnn": {"train_seq_len": seq}}, critic={"rnn": {"train_seq_len": seq}})
        actor, critic = DC.rnn_nets(3, 900)
        lrn = learner.DataParallelPerAgentRecurrentLearner(actor, critic, cfg, value_normalizer=learner.ValueNorm1(), group=group)
        kw, rk = DC.rnn_rollout(n, steps, agents, seq, 7)
        run(name, lrn, list(actor.values()), {**{k: v for k, v in kw.items() if k != "tp"}, **rk})
    return out


def _case_parents_refuse(rank):
    import dp_per_agent_cases as DC
    from hns_amd import learner
    out = {}
    state = DC.plain_state(3, 51)
    actor, critic = DC.rnn_nets(3, 900)
    for name, make in (("plain", lambda: learner.PerAgentDeviceLearner(state["actor"], state["critic"], DC.CFG_PLAIN, group="world")),
                       ("rnn", lambda: learner.PerAgentRecurrentDeviceLearner(actor, critic, DC.CFG_RNN, group="world"))):
        try:
            make()
            out[name] = ("no error", "")
        except Exception as e:                                   # noqa: BLE001
            out[name] = (type(e).__name__, str(e))
    return out


def _worker(rank, world, port, q):
    _paths()
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    torch.set_num_threads(2)
    out = {}
    try:
        for name, fn in (("plain", _case_learner_plain), ("rnn", _case_learner_rnn), ("grads", _case_grads), ("refusals", _case_refusals),
                         ("parents", _case_parents_refuse)):
            out[name] = fn(rank)
    except Exception:                                            # noqa: BLE001
        out["error"] = traceback.format_exc()
    q.put((rank, out))
    if "error" not in out:
        dist.monitored_barrier()      # gloo's CPU barrier: dist.barrier() probes for an accelerator, which opens the GPU in every rank of a CPU job
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 39600 + os.getpid() % 2000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    outs = [o for _, o in sorted((q.get(timeout=240) for _ in range(2)), key=lambda x: x[0])]
    for p in procs:
        p.join(timeout=60)
    for o in outs:
        assert "error" not in o, o["error"]
    assert all(p.exitcode == 0 for p in procs)
    return outs


def _same_bits(a, b):
    assert len(a) == len(b)
    bad = [i for i, (x, y) in enumerate(zip(a, b)) if x.tobytes() != y.tobytes() or x.shape != y.shape]
    assert not bad, f"{len(bad)} of {len(a)} tensors differ between the ranks: {bad[:8]}"


@pytest.mark.timeout(300)
@pytest.mark.parametrize("which, tensors", [("plain", 23), ("rnn", 29)])
def test_two_ranks_end_bit_identical_after_two_rollouts(ranks, which, tensors):
    _paths()
    from hns_amd import learner
    r0, r1 = ranks[0][which], ranks[1][which]
    assert r1["moved_at_start"] and not r0["moved_at_start"]     # rank 1's other weights were replaced by rank 0's at construction
    _same_bits(r0["start"], r1["start"])
    _same_bits(r0["state"], r1["state"])                         # stacked parameters, Adam moments and step counts, ValueNorm1
    assert r0["updates"] == r1["updates"] == 2
    # the bucket that is all-reduced lies behind the STACKED tensors (plain: in the mapping's order, which is the optimiser's; recurrent: in
    # network_parameters' order — encoder, GRU, head)
    shapes = [a.shape for a in r0["start"]]
    assert len(r0["bucket"]) == tensors and all(s[0] == 3 for s in r0["bucket"]) and sorted(r0["bucket"]) == sorted(shapes)
    assert which == "rnn" or r0["bucket"] == shapes
    for i0, i1 in zip(r0["infos"], r1["infos"]):
        assert i0 == i1 and list(i0) == [f"drone/{k}" for k in learner.INFO_KEYS], (i0, i1)
        assert all(np.isfinite(v) for v in i0.values()), i0
    moved = [not np.array_equal(a, b) for a, b in zip(r0["start"], r0["state"])]
    assert all(moved), "a stacked tensor did not move"
    assert r0["infos"][1]["drone/TP_loss"] > 0                   # the second rollout: rank 1 selected no window and stepped with the others


def _union_refs(which):
    import dp_per_agent_cases as DC
    import per_agent_rnn_update_cases as PCR
    if which == "plain":
        data = DC.plain_union()
        r64, r32 = DC.plain_refs(data)
        DC.plain_preconditions(r64, r32)
        assert len(data[6]) * DC.A == DC.GLOBAL_ROWS == 96 and len(set(data[6].tolist())) == len(data[6])
        names = list(data[0])
        ref = lambda r: ({k: r["grads"][k] for k in names}, r)   # noqa: E731
        return names, ref(r64), ref(r32)
    b, _ = DC.rnn_union()
    bad = PCR.preconditions(b)
    assert not bad, bad
    assert len(b.seg) * DC.L * DC.A == DC.GLOBAL_ROWS == 96 and len(set(b.seg.tolist())) == len(b.seg)
    return list(b.net), (b.g64, b.s64), (b.g32, b.s32)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("which", ["plain", "rnn"])
def test_the_first_minibatchs_gradients_meet_the_gate_over_the_union(ranks, which):
    _paths()
    import dp_per_agent_cases as DC
    import rnn_update_reference as U
    names, (g64, s64), (g32, s32) = _union_refs(which)
    r0, r1 = ranks[0]["grads"][(which, 1e-3)], ranks[1]["grads"][(which, 1e-3)]
    for k in names:
        assert r0["grads"][k].tobytes() == r1["grads"][k].tobytes(), k              # the all-reduced gradient: one on both ranks
    assert r0["grad_norm"] == r1["grad_norm"] and r0["entropy"] == r1["entropy"]
    items = []
    for k in names:
        items.append((k, r0["grads"][k], g64[k], g32[k]))
        items += [(f"{k}[{a}]", r0["grads"][k][a], g64[k][a], g32[k][a]) for a in range(DC.A)]
    logp = np.concatenate([r0["log_probs"], r1["log_probs"]])
    items += [("grad_norm", r0["grad_norm"], s64["grad_norm"], s32["grad_norm"]),
              ("policy_loss", r0["policy_loss"] + r1["policy_loss"], s64["policy_loss"], s32["policy_loss"]),          # the shares add up
              ("entropy", r0["entropy"], s64["entropy"], s32["entropy"]),
              ("log_probs", logp, np.asarray(s64["log_probs"]).reshape(logp.shape), np.asarray(s32["log_probs"]).reshape(logp.shape))]
    worst, bad = U.gate(f"union {which}", items)
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("which", ["plain", "rnn"])
def test_the_entropy_term_is_counted_once_over_the_ranks(ranks, which):
    _paths()
    import dp_per_agent_cases as DC
    for r in ranks:                                              # (the summed gradient: the same on both ranks)
        g0, g3 = (r["grads"][(which, c)]["grads"]["act_dist.log_std"].astype(np.float64) for c in (0.0, 0.3))
        assert g0.shape == (DC.A, 4)
        tol = 16 * 2.0 ** -24 * max(np.abs(g0).max(), np.abs(g3).max())
        assert np.abs((g3 - g0) - (-0.3 / DC.A)).max() <= tol, (g3 - g0, -0.3 / DC.A, tol)
        assert tol < 0.01 * 0.3 / DC.A                           # (W times, or not at all, is 0.1 off)
        for k, v in r["grads"][(which, 0.0)]["grads"].items():   # nothing else sees the coefficient
            if k != "act_dist.log_std":
                assert v.tobytes() == r["grads"][(which, 0.3)]["grads"][k].tobytes(), k


@pytest.mark.timeout(300)
def test_disagreeing_ranks_are_refused_before_the_updates(ranks):
    for r in ranks:
        for name, word in (("plain-agents", "number of agents differs"), ("plain-short", "fewer env-steps than num_minibatches"),
                           ("rnn-agents", "number of agents differs"), ("rnn-seq_len", "train_seq_len differs"),
                           ("rnn-short", "fewer segments than num_minibatches")):
            kind, text, probe, untouched = r["refusals"][name]
            assert kind == "ValueError" and word in text, (name, kind, text)
            assert probe == 2.0 and untouched, name


def test_the_local_learners_and_functions_still_refuse_and_name_the_new_ones(ranks):
    for r in ranks:
        for which, new in (("plain", "DataParallelPerAgentLearner"), ("rnn", "DataParallelPerAgentRecurrentLearner")):
            kind, text = r["parents"][which]
            assert kind == "NotImplementedError" and "group" in text and new in text, (kind, text)
    _paths()
    import dp_per_agent_cases as DC
    from hns_amd import learner, rnn_train
    state = DC.plain_state(3, 51)
    actor, critic = DC.rnn_nets(3, 900)
    with pytest.raises(ValueError, match="group"):               # ... and the new classes need one
        learner.DataParallelPerAgentLearner(state["actor"], state["critic"], DC.CFG_PLAIN)
    with pytest.raises(ValueError, match="group"):
        learner.DataParallelPerAgentRecurrentLearner(actor, critic, DC.CFG_RNN)
    kw, rk = DC.rnn_rollout(2, DC.T, 3, DC.L, 7)
    args = (actor, kw["obs_self"], kw["obs_others"], kw["obs_cylinders"], rk["actor_rnn_state"], rk["is_init"], kw["action"], kw["log_probs"], kw["reward"])
    opt = rnn_train.make_optimizer_per_agent(actor, {"share_actor": False})
    for extra in ({"global_rows": 96}, {"group": "world"}):
        with pytest.raises(NotImplementedError, match="policy_loss_and_grad_rnn_per_agent_global"):
            rnn_train.policy_loss_and_grad_rnn_per_agent(*args, seq_len=DC.L, **extra)
        with pytest.raises(NotImplementedError, match="update_actor_rnn_per_agent_global"):
            rnn_train.update_actor_rnn_per_agent(*args, opt, seq_len=DC.L, **extra)
    # the new functions' own refusals: an update steps on the bucket's norm over the union
    with pytest.raises(ValueError, match="bucket"):
        rnn_train.update_actor_rnn_per_agent_global(*args, opt, seq_len=DC.L, global_rows=96)
    with pytest.raises(ValueError, match="global_rows"):
        rnn_train.policy_loss_and_grad_rnn_per_agent_global(*args, seq_len=DC.L)


def test_one_rank_on_the_cpu_has_the_bits_of_the_group_less_path():
    _paths()
    import dp_per_agent_cases as DC
    from hns_amd import actor_train as AT
    from hns_amd import policy_train as PT
    from hns_amd import rnn_train
    data = DC.plain_union()
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v))       # noqa: E731
    args = (t(data[1]["state_self"]), t(data[1]["state_others"]), t(data[1]["cylinders"]), t(data[2]), t(data[3]), t(data[4]), t(data[6]))
    n = len(data[6]) * DC.A
    plain, glob = ({k: t(v).clone() for k, v in data[0].items()} for _ in range(2))
    want = AT.policy_loss_and_grad_per_agent(plain, *args, entropy_coef=1e-3)
    got = AT.policy_loss_and_grad_per_agent_global(glob, *args, entropy_coef=1e-3, global_rows=n, entropy_share=1.0, bucket=PT.GradBucket(glob))
    for k in plain:
        assert torch.equal(plain[k].grad, glob[k].grad), k
    for k in ("policy_loss", "ess", "log_probs"):
        assert torch.equal(getattr(want, k), getattr(got, k)), k
    # entropy: the local torch path's fp32 mean over the B A rows depends on B once the agents' entropies differ (at these log_std: 12 and 20
    # env-steps give 0x1.8bad8cp+2, 32 give 0x1.8bad8ep+2), and the data-parallel form must give every rank, whatever its row count, one value.
    # So the global form is held to the statement's exact value — the agents' mean in fp64, rounded once — bit for bit, and the local path
    # to it within the worst-case error of an fp32 sum of n terms, n u |mean|.
    ls64 = t(data[0]["act_dist.log_std"]).double()
    exact = (0.5 + 0.5 * np.log(2 * np.pi) + ls64).sum(-1).mean()
    assert torch.equal(got.entropy, exact.float())
    assert abs(float(want.entropy) - float(exact)) <= n * 2.0 ** -24 * float(exact)
    assert abs(float(got.grad_norm) - float(want.grad_norm)) <= 2.0 ** -22 * float(want.grad_norm)      # (the bucket's norm: another order of the sum)
    with pytest.raises(ValueError, match="global_rows"):
        AT.policy_loss_and_grad_per_agent_global(glob, *args, global_rows=n - 1)
    with pytest.raises(ValueError, match="bucket"):
        AT.update_actor_per_agent_global(glob, *args[:6], AT.make_optimizer_per_agent(glob, {"share_actor": False}), index=args[6], global_rows=n)

    b, _ = DC.rnn_union()
    o = (t(b.obs["state_self"]), t(b.obs["state_others"]), t(b.obs["cylinders"]), t(b.state), t(b.is_init), *(t(r) for r in b.rows))
    seg = t(b.seg)
    n = seg.numel() * DC.L * DC.A
    plain, glob = ({k: t(v).clone() for k, v in b.net.items()} for _ in range(2))
    want = rnn_train.policy_loss_and_grad_rnn_per_agent(plain, *o, segment=seg, seq_len=DC.L, entropy_coef=1e-3)
    got = rnn_train.policy_loss_and_grad_rnn_per_agent_global(glob, *o, segment=seg, seq_len=DC.L, entropy_coef=1e-3, global_rows=n, entropy_share=1.0,
                                                              bucket=rnn_train.make_bucket(glob, True, stacked=True))
    for k in plain:
        assert torch.equal(plain[k].grad, glob[k].grad), k
    for k in ("policy_loss", "entropy", "ess", "log_probs"):
        assert torch.equal(getattr(want, k), getattr(got, k)), k
    assert abs(float(got.grad_norm) - float(want.grad_norm)) <= 2.0 ** -22 * float(want.grad_norm)
    # the restatement with a stacked head: the global form at its own rows is the local one
    y = torch.randn(2, DC.L, DC.A, 128, generator=torch.Generator().manual_seed(3))
    hw, hb, ls = (glob[k].detach() for k in ("act_dist.fc_mean.weight", "act_dist.fc_mean.bias", "act_dist.log_std"))
    rows = (torch.randn(2, DC.L, DC.A, 4, generator=torch.Generator().manual_seed(4)) * 0.3, torch.full((2, DC.L, DC.A), -3.0),
            torch.randn(2, DC.L, DC.A, generator=torch.Generator().manual_seed(5)))
    loc = rnn_train.actor_head(hw, hb, ls, y, *rows, 0.1, 1e-3)
    glo = rnn_train.actor_head(hw, hb, ls, y, *rows, 0.1, 1e-3, global_rows=2 * DC.L * DC.A, entropy_share=1.0)
    for k in loc:
        assert torch.equal(loc[k], glo[k]), k
    half = rnn_train.actor_head(hw, hb, ls, y, *rows, 0.1, 1e-3, global_rows=4 * DC.L * DC.A, entropy_share=0.5)
    assert torch.allclose(half["d_head_w"], loc["d_head_w"] / 2, rtol=1e-6, atol=0) and torch.equal(half["entropy"], loc["entropy"])
