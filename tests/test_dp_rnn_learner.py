"""The data-parallel recurrent learner on the CPU (learner.DataParallelRecurrentLearner, rnn_train's global forms): two gloo
ranks perform ONE recurrent PPO update per minibatch on the union of their minibatches of segments.  The device entries:
tests/test_hip_dp_rnn_learner.py.

One spawn of two workers runs every case (process start-up is most of the time) and hands numpy results to the tests:
  learner   3 and 5 envs x 8 steps of the example's stand-in env, L 4, 3 agents, 2 epochs x 2 minibatches, predictor on; rank 1 starts from
            OTHER weights (the construction broadcast is part of what is tested) and, in the second rollout, its TP_done selects no window.
            After two train_rollouts the ranks' parameters, Adam states, ValueNorm1 and info rows are bit-identical.
  grads     the first minibatch pair of such an update through rnn_train's calls with group=: rollout_case N = 3 + 5, T 8, L 4, A 3, 2
            cylinders, 2 minibatches (3 and 5 segments a rank, global_rows 96), each rank's segments the first minibatch of its own
            permutation.  The all-reduced gradients, the summed policy_loss shares and the union's scalars meet the gate,
            e <= 8 max(e_32, 2^-24 max|ref_64|), against rnn_update_reference.flow in fp64 over the union's segments; every row of log_probs
            and values is compared.  assert_off_the_edges' three conditions are asserted on the union in fp64.
  branch    dp_rnn_reference.branch_flip_case (5 + 11 segments): part 0 alone takes the unclipped branch, the union the clipped one; both ranks'
            dy follows the union's.
  refusals  ranks that disagree on train_seq_len, num_minibatches or the number of agents, a rank with fewer segments than minibatches: ValueError
            on every rank before the updates — on a group with a 20 s timeout, so a collective entered by one rank alone shows as an error.
  RecurrentDeviceLearner(group="world") still raises NotImplementedError and names the new class.
In this process: with one rank (global_rows = own rows, entropy_share 1, own sums) the CPU path has the bits of the group-less CPU path."""
import datetime
import importlib.util
import os
import sys
import traceback

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS, T, L, A, CYL, D, M = (3, 5), 8, 4, 3, 2, 35, 2
S = T // L
GLOBAL_ROWS = sum(n * S // M for n in ENVS) * L * A
CFG = {"ppo_epochs": 2, "num_minibatches": M, "TP_epochs": 1, "use_TP_net": 1, "actor": {"rnn": {"train_seq_len": L}}, "critic": {"rnn": {"train_seq_len": L}}}
FLIP = ((5, 11), 4, 3, 4242)


def _paths():
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import hns_amd  # noqa: F401


def _example():
    spec = importlib.util.spec_from_file_location("recurrent_policy_example", os.path.join(ROOT, "examples", "recurrent_policy.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _np(ts):
    return [t.detach().cpu().numpy().copy() for t in ts]


def _snapshot(lrn):
    """Parameters of the three networks, the three Adam states, ValueNorm1."""
    from hns_amd import tp_train
    out = [v.detach().clone() for v in (*lrn.actor.values(), *lrn.critic.values(), *(tp_train.parameters(lrn.tp_net) if lrn.tp_net is not None else ()))]
    for opt in (lrn.actor_opt, lrn.critic_opt, lrn.tp_opt):
        if opt is not None:
            for st in opt.state_dict()["state"].values():
                out += [st["step"].clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
    vn = lrn.value_normalizer
    return out + ([vn.running_mean.clone(), vn.running_mean_sq.clone(), vn.debiasing_term.clone()] if vn is not None else [])


def _setup(rank, N, seq=L, agents=A, steps=T):
    from hns_amd import collector
    from hns_amd import policy as P
    ex = _example()
    ex.SEQ = seq
    torch.manual_seed(7 * rank)                                  # other weights on every rank, until the broadcast
    env = ex.StandInEnv(N, A=agents, max_episode_length=5)       # episodes end inside the segments: flags in their middle
    env.set_seed(50 + rank)
    actor, critic = ex.Network(env.D, env.A, True, 10 * rank), ex.Network(env.D, env.A, False, 10 * rank + 1)
    pol = P.RecurrentDevicePolicy(actor.names(), critic.names(), seed=rank)
    return actor, critic, pol, collector.DeviceCollector(env, pol, steps, rnn_seq_len=seq)


def _case_learner(rank):
    import rnn_update_reference as U
    from hns_amd import learner
    N = ENVS[rank]
    actor, critic, pol, col = _setup(rank, N)
    first = [v.detach().clone() for v in (*actor.names().values(), *critic.names().values())]
    lrn = learner.DataParallelRecurrentLearner(actor.names(), critic.names(), CFG, tp_net=U.predictor(A, 41 + rank), value_normalizer=learner.ValueNorm1(),
                                               generator=torch.Generator().manual_seed(100 + rank), device_policy=pol, group="world")
    start = _np([*actor.names().values(), *critic.names().values()])
    moved_at_start = not all(torch.equal(a, b) for a, b in zip(first, (*actor.names().values(), *critic.names().values())))
    infos = []
    for it in range(2):
        st = col.collect()
        tp = U.predictor_rollout(N, T, A, 17 + rank + 10 * it)
        if it == 1 and rank == 1:
            tp = (tp[0], tp[1], torch.zeros_like(tp[2]))         # no window selected on this rank
        infos.append(lrn.train_rollout(**st.learner_kwargs(), tp=tp, **st.recurrent_kwargs()))
    return {"start": start, "moved_at_start": moved_at_start, "infos": infos, "state": _np(_snapshot(lrn)), "updates": lrn.n_updates}


def union_case():
    """The union rollout of the `grads` case, its per-row tensors and the ranks' segments (the first minibatch of each rank's permutation)."""
    import rnn_update_reference as U
    from hns_amd import tp_train
    N = sum(ENVS)
    a_net, c_net, obs, states, is_init = U.rollout_case(N, T, A, CYL, D, L, 908)               # (seeds for which the fp64 preconditions hold on the union)
    rows = {"actor": U.per_row_case(True, N, T, A, 31, a_net, obs, states["actor"], is_init, L),
            "critic": U.per_row_case(False, N, T, A, 31, c_net, obs, states["critic"], is_init, L)}
    local = [tp_train.minibatches(n * S, M, torch.device("cpu"), torch.Generator().manual_seed(300 + r))[0].numpy() for r, n in enumerate(ENVS)]
    return a_net, c_net, obs, states, is_init, rows, local


def _case_grads(rank):
    import dp_rnn_reference as DU
    from hns_amd import rnn_train, sharding
    a_net, c_net, obs, states, is_init, rows, local = union_case()
    o, st, fl, pr = DU.split_rollout(obs, states, is_init, rows, ENVS)[rank]
    t = torch.as_tensor
    seg = t(local[rank])
    assert seg.numel() * L * A < GLOBAL_ROWS
    out = {}
    live = {k: t(v).clone() for k, v in a_net.items()}
    res = rnn_train.policy_loss_and_grad_rnn(live, t(o["state_self"]), t(o["state_others"]), t(o["cylinders"]), t(st["actor"]), t(fl), *(t(r) for r in pr["actor"]),
                                             segment=seg, seq_len=L, entropy_coef=1e-3, global_rows=GLOBAL_ROWS, entropy_share=0.5, group=dist.group.WORLD,
                                             bucket=rnn_train.make_bucket(live, True))
    out["actor"] = {"grads": {k: v.grad.numpy().copy() for k, v in live.items()}, "policy_loss": float(res.policy_loss), "entropy": float(res.entropy),
                    "grad_norm": float(res.grad_norm), "log_probs": res.log_probs.squeeze(-1).numpy().copy()}
    live = {k: t(v).clone() for k, v in c_net.items()}
    args = (live, t(o["state_self"]), t(o["state_others"]), t(o["cylinders"]), t(st["critic"]), t(fl), *(t(r) for r in pr["critic"]))
    half = rnn_train.value_loss_sums_rnn(*args, segment=seg, seq_len=L)
    sums = sharding.all_reduce_sum(half.sums.clone(), dist.group.WORLD)
    res = rnn_train.value_loss_and_grad_rnn(*args, segment=seg, seq_len=L, sums=sums, global_rows=GLOBAL_ROWS, group=dist.group.WORLD,
                                            bucket=rnn_train.make_bucket(live, False), forward=half.forward)
    out["critic"] = {"grads": {k: v.grad.numpy().copy() for k, v in live.items()}, "value_loss": float(res.value_loss),
                     "explained_var": float(res.explained_var), "grad_norm": float(res.grad_norm), "values": half.values.squeeze(-1).numpy().copy()}
    return out


def _case_branch(rank):
    import dp_rnn_reference as DU
    from hns_amd import rnn_train, sharding
    c, parts = DU.branch_flip_case(*FLIP)
    p = {k: torch.as_tensor(v) for k, v in parts[rank].items()}
    rows = float(np.prod(c["y"].shape[:3]))
    out = {}
    for how in ("global", "per_rank"):
        own, _ = rnn_train.critic_head_sums(p["v_w"], p["v_b"], p["y"], p["b_values"], p["b_returns"], 0.1)
        sums = sharding.all_reduce_sum(own.clone(), dist.group.WORLD) if how == "global" else own     # per_rank: each rank decides on its own sums
        res = rnn_train.critic_head(p["v_w"], p["v_b"], p["y"], p["b_values"], p["b_returns"], 0.1, sums=sums, global_rows=rows)
        out[how] = {k: res[k].numpy().copy() for k in ("dy", "d_head_w", "d_head_b", "value_loss", "explained_var")}
    return out


def _case_refusals(rank):
    from hns_amd import learner
    group = dist.new_group(ranks=[0, 1], backend="gloo", timeout=datetime.timedelta(seconds=20))
    out = {}
    cases = (("seq_len", dict(seq=(4, 2)[rank]), CFG),
             ("minibatches", {}, dict(CFG, num_minibatches=1 + rank)),
             ("agents", dict(agents=(3, 2)[rank]), CFG),
             ("short", dict(steps=(8, 4)[rank]) if rank else {}, CFG))
    for name, kw, cfg in cases:
        seq = kw.get("seq", L)
        cfg = dict(cfg, use_TP_net=0, actor={"rnn": {"train_seq_len": seq}}, critic={"rnn": {"train_seq_len": seq}})
        actor, critic, pol, col = _setup(0, 1 if name == "short" and rank else 2, **kw)
        lrn = learner.DataParallelRecurrentLearner(actor.names(), critic.names(), cfg, value_normalizer=learner.ValueNorm1(), device_policy=pol, group=group)
        st = col.collect()
        before = _np([*actor.names().values(), *critic.names().values()])
        try:
            lrn.train_rollout(**st.learner_kwargs(), **st.recurrent_kwargs())
            out[name] = ("no error", "")
        except Exception as e:                                   # noqa: BLE001  (the type is what the test asserts)
            out[name] = (type(e).__name__, str(e))
        after = _np([*actor.names().values(), *critic.names().values()])
        probe = torch.ones(1)
        dist.all_reduce(probe, group=group)                      # the ranks are still in step: nobody waits in a collective of the refused call
        out[name] += (float(probe), all(np.array_equal(a, b) for a, b in zip(before, after)) and lrn.n_updates == 0)
    return out


def _case_parent_refuses(rank):
    from hns_amd import learner
    actor, critic, pol, _ = _setup(0, 2)
    try:
        learner.RecurrentDeviceLearner(actor.names(), critic.names(), CFG, device_policy=pol, group="world")
        return ("no error", "")
    except Exception as e:                                       # noqa: BLE001
        return (type(e).__name__, str(e))


def _worker(rank, world, port, q):
    _paths()
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    torch.set_num_threads(2)
    out = {}
    try:
        for name, fn in (("learner", _case_learner), ("grads", _case_grads), ("branch", _case_branch), ("refusals", _case_refusals),
                         ("parent", _case_parent_refuses)):
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
    port = 37500 + os.getpid() % 2000
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
def test_two_ranks_end_bit_identical_after_two_rollouts(ranks):
    r0, r1 = ranks[0]["learner"], ranks[1]["learner"]
    assert r1["moved_at_start"] and not r0["moved_at_start"]     # rank 1's other weights were replaced by rank 0's at construction
    _same_bits(r0["start"], r1["start"])
    _same_bits(r0["state"], r1["state"])                         # parameters, Adam moments and step counts, ValueNorm1
    assert r0["updates"] == r1["updates"] == 2
    from hns_amd import learner
    for i0, i1 in zip(r0["infos"], r1["infos"]):
        assert i0 == i1 and list(i0) == [f"drone/{k}" for k in learner.INFO_KEYS], (i0, i1)
        assert all(np.isfinite(v) for v in i0.values()), i0
    moved = [not np.array_equal(a, b) for a, b in zip(r0["start"], r0["state"])]
    assert all(moved), "a parameter did not move"
    # the second rollout: rank 1 selected no window, and stepped its predictor with the others (its tensors are rank 0's, above)
    assert r0["infos"][1]["drone/TP_loss"] > 0


@pytest.mark.timeout(300)
def test_the_first_minibatch_pairs_gradients_meet_the_gate_over_the_union(ranks):
    _paths()
    import dp_rnn_reference as DU
    import rnn_update_reference as U
    a_net, c_net, obs, states, is_init, rows, local = union_case()
    seg = DU.union_segments(local, ENVS, S)
    assert len(seg) * L * A == GLOBAL_ROWS == 96 and len(set(seg.tolist())) == len(seg)
    for word, net in (("actor", a_net), ("critic", c_net)):
        actor = word == "actor"
        g64, s64 = U.flow(net, actor, obs, states[word], is_init, rows[word], seg, L, torch.float64)
        g32, s32 = U.flow(net, actor, obs, states[word], is_init, rows[word], seg, L, torch.float32)
        r0, r1 = ranks[0]["grads"][word], ranks[1]["grads"][word]
        for k in net:
            assert r0["grads"][k].tobytes() == r1["grads"][k].tobytes(), k          # the all-reduced gradient: one on both ranks
        assert r0["grad_norm"] == r1["grad_norm"]
        items = [(k, r0["grads"][k], g64[k], g32[k]) for k in net] + [("grad_norm", r0["grad_norm"], s64["grad_norm"], s32["grad_norm"])]
        if actor:
            d = np.minimum(np.abs(s64["ratio"] - 0.9), np.abs(s64["ratio"] - 1.1))
            assert d.min() >= U.MARGIN and np.array_equal(s64["w"], s32["w"])
            assert r0["entropy"] == r1["entropy"]
            items += [("policy_loss", r0["policy_loss"] + r1["policy_loss"], s64["policy_loss"], s32["policy_loss"]),       # the shares add up
                      ("entropy", r0["entropy"], s64["entropy"], s32["entropy"]),
                      ("log_probs", np.concatenate([r0["log_probs"], r1["log_probs"]]), s64["log_probs"], s32["log_probs"])]
        else:
            assert float(s64["dist"]) >= U.MARGIN and abs(float(s64["l_orig"] - s64["l_clip"])) >= 1e-3 * float(s64["value_loss"])
            assert (r0["value_loss"], r0["explained_var"]) == (r1["value_loss"], r1["explained_var"])
            items += [("value_loss", r0["value_loss"], s64["value_loss"], s32["value_loss"]),
                      ("explained_var", r0["explained_var"], s64["explained_var"], s32["explained_var"]),
                      ("values", np.concatenate([r0["values"], r1["values"]]), s64["values"], s32["values"])]
        worst, bad = U.gate(f"union {word}", items)
        assert not bad, "; ".join(bad)


@pytest.mark.timeout(300)
def test_the_branch_of_the_max_is_the_unions_on_both_ranks(ranks):
    _paths()
    import dp_rnn_reference as DU
    import rnn_update_reference as U
    c, parts = DU.branch_flip_case(*FLIP)
    DU.assert_branch_precondition(c, parts)
    c64, c32 = U.critic_head_autograd(c, torch.float64), U.critic_head_autograd(c, torch.float32)
    g = [ranks[r]["branch"]["global"] for r in range(2)]
    assert g[0]["value_loss"].tobytes() == g[1]["value_loss"].tobytes() and g[0]["explained_var"].tobytes() == g[1]["explained_var"].tobytes()
    items = [("dy", np.concatenate([g[0]["dy"], g[1]["dy"]]), c64["dy"], c32["dy"])]
    items += [(k, g[0][k] + g[1][k], c64[k], c32[k]) for k in ("d_head_w", "d_head_b")]
    items += [(k, g[0][k], c64[k], c32[k]) for k in ("value_loss", "explained_var")]
    worst, bad = U.gate("branch flip", items)
    assert not bad, "; ".join(bad)
    # rank 0 deciding on its own sums takes its rows down the other branch: far outside the bar
    B0 = FLIP[0][0]
    wrong = ranks[0]["branch"]["per_rank"]["dy"]
    worst, bad = U.gate("per-rank decision", [("dy", wrong, c64["dy"][:B0], c32["dy"][:B0])], verbose=False)
    assert worst > U.BAR, worst


@pytest.mark.timeout(300)
def test_disagreeing_ranks_are_refused_before_the_updates(ranks):
    for r in ranks:
        for name, word in (("seq_len", "train_seq_len differs"), ("minibatches", "num_minibatches differs"), ("agents", "number of agents differs"),
                           ("short", "fewer segments than num_minibatches")):
            kind, text, probe, untouched = r["refusals"][name]
            assert kind == "ValueError" and word in text, (name, kind, text)
            assert probe == 2.0 and untouched, name


def test_the_recurrent_learner_itself_still_refuses_a_group(ranks):
    for r in ranks:
        kind, text = r["parent"]
        assert kind == "NotImplementedError" and "group" in text and "DataParallelRecurrentLearner" in text, (kind, text)
    _paths()
    from hns_amd import learner
    actor, critic, pol, _ = _setup(0, 2)
    with pytest.raises(ValueError, match="group"):               # ... and the new class needs one
        learner.DataParallelRecurrentLearner(actor.names(), critic.names(), CFG, device_policy=pol)


def test_one_rank_on_the_cpu_has_the_bits_of_the_group_less_path():
    _paths()
    from hns_amd import rnn_train
    a_net, c_net, obs, states, is_init, rows, local = union_case()
    t = torch.as_tensor
    seg = t(np.array([4, 0, 5, 2, 1], np.int64))
    n = seg.numel() * L * A
    o = (t(obs["state_self"]), t(obs["state_others"]), t(obs["cylinders"]))
    plain, glob = ({k: t(v).clone() for k, v in a_net.items()} for _ in range(2))
    args = (t(states["actor"]), t(is_init), *(t(r) for r in rows["actor"]))
    want = rnn_train.policy_loss_and_grad_rnn(plain, *o, *args, segment=seg, seq_len=L)
    got = rnn_train.policy_loss_and_grad_rnn(glob, *o, *args, segment=seg, seq_len=L, global_rows=n, entropy_share=1.0, bucket=rnn_train.make_bucket(glob, True))
    for k in plain:
        assert torch.equal(plain[k].grad, glob[k].grad), k
    for k in ("policy_loss", "entropy", "ess", "log_probs"):
        assert torch.equal(getattr(want, k), getattr(got, k)), k
    assert abs(float(got.grad_norm) - float(want.grad_norm)) <= 2.0 ** -22 * float(want.grad_norm)      # (the bucket's norm: another order of the sum)
    plain, glob = ({k: t(v).clone() for k, v in c_net.items()} for _ in range(2))
    args = (t(states["critic"]), t(is_init), *(t(r) for r in rows["critic"]))
    want = rnn_train.value_loss_and_grad_rnn(plain, *o, *args, segment=seg, seq_len=L)
    half = rnn_train.value_loss_sums_rnn(glob, *o, *args, segment=seg, seq_len=L)
    got = rnn_train.value_loss_and_grad_rnn(glob, *o, *args, segment=seg, seq_len=L, sums=half.sums, global_rows=n, forward=half.forward,
                                            bucket=rnn_train.make_bucket(glob, False))
    again = {k: t(v).clone() for k, v in c_net.items()}          # ... and without the forward state: a second encoder and GRU pass, the same bits
    rnn_train.value_loss_and_grad_rnn(again, *o, *args, segment=seg, seq_len=L, sums=half.sums, global_rows=n, bucket=rnn_train.make_bucket(again, False))
    for k in plain:
        assert torch.equal(plain[k].grad, glob[k].grad) and torch.equal(plain[k].grad, again[k].grad), k
    assert torch.equal(want.value_loss, got.value_loss) and torch.equal(want.explained_var, got.explained_var)
    assert torch.equal(want.values, half.values) and torch.equal(want.values, got.values)
    # the refusals of the data-parallel arguments
    with pytest.raises(ValueError, match="global_rows"):
        rnn_train.value_loss_and_grad_rnn(glob, *o, *args, segment=seg, seq_len=L, sums=half.sums, global_rows=n - 1)
    with pytest.raises(ValueError, match="bucket"):
        rnn_train.update_critic_rnn(glob, *o, *args, rnn_train.make_optimizer(glob, None, actor=False), segment=seg, seq_len=L, global_rows=n, sums=half.sums)
    with pytest.raises(ValueError, match="sums"):
        rnn_train.update_critic_rnn(glob, *o, *args, rnn_train.make_optimizer(glob, None, actor=False), segment=seg, seq_len=L, global_rows=n,
                                    bucket=rnn_train.make_bucket(glob, False))
    with pytest.raises(ValueError, match="travel together"):
        rnn_train.value_loss_and_grad_rnn(glob, *o, *args, segment=seg, seq_len=L, global_rows=n)
