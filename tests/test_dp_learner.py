"""The data-parallel learner on the CPU: two gloo ranks perform ONE PPO update on the union of their minibatches.

One spawn of two workers runs every case (process start-up is most of the time) and hands numpy results to the tests:
  union     6 + 4 envs x 8 steps of one synthetic rollout (unequal shards), 3 pursuers, K 5, D 20, one epoch, one minibatch, predictor on;
            rank 1 starts from OTHER weights, so the construction broadcast is part of what is tested.  The ranks end bit-identical; the
            all-reduced actor and critic gradients meet the update tests' bar against fp64 autograd over the union minibatch.
  branch    returns and old values such that rank 0 alone takes the unclipped branch of the max and the union the clipped one.
  tp        one rank's TP_done selects no window.
  refusals  unequal num_minibatches; a rank with fewer env-steps than minibatches — on a group with a 20 s timeout, so a collective entered
            by one rank alone shows as an error, not a hang.
The bar, BAR and e_32 are test_hip_critic_train.py's (tests/dp_reference.py)."""
import copy
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
A, D, T = 3, 20, 8
SHARDS = (slice(0, 6), slice(6, 10))
UNION_CFG = {"ppo_epochs": 1, "num_minibatches": 1, "max_grad_norm": 1e9}     # the clip inactive: .grad holds the all-reduced gradient unscaled


def _paths():
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import hns_amd  # noqa: F401
    import learner_cases as LC
    LC.D = D                                                     # the cases' self_dim (this process only)
    return LC


def _cut(ro, sl):
    cut = lambda t: t[sl].contiguous() if torch.is_tensor(t) else (tuple(cut(x) for x in t) if isinstance(t, tuple) else t)   # noqa: E731
    return {k: cut(v) for k, v in ro.items()}


def _np(d):
    return {k: v.detach().cpu().numpy().copy() for k, v in d.items()}


def _union_start(LC):
    state0 = LC.make_state(A, 21)
    return state0, LC.make_rollout(state0, 10, T, A, 22)


def _case_union(LC, rank):
    from hns_amd import gae, learner
    cfg = dict(LC.CFG, **UNION_CFG)
    state0, ro = _union_start(LC)
    state = LC.make_state(A, 21 + 7 * rank)
    mine = _cut(ro, SHARDS[rank])
    L = learner.DeviceLearner(state["actor"], state["critic"], cfg, tp_net=state["tp"], value_normalizer=state["vn"],
                              generator=torch.Generator().manual_seed(100 + rank), group="world")
    same_start = all(torch.equal(a, b) for a, b in zip(LC.state_tensors(state, {}).values(), LC.state_tensors(state0, {}).values()))
    # the targets as train_rollout is about to form them (its statements on a copy of the normaliser): the fp64 yardstick's inputs
    with torch.no_grad():
        next_value = L.policy.forward(*mine["next_obs_last"], value_only=True).value
    adv, ret, _, _ = gae.rollout_targets(mine["reward"], mine["done"].unsqueeze(-1), mine["state_value"], next_value, cfg["gamma"], cfg["gae_lambda"],
                                         value_normalizer=copy.deepcopy(state["vn"]), normalize_advantages=True, return_moments=True)
    info = L.train_rollout(**mine)
    grads = {f"actor.{k}": v.grad for k, v in state["actor"].items()}
    grads.update({f"critic.{k}": v.grad for k, v in state["critic"].named_parameters()})
    return {"same_start": same_start, "info": info, "state": _np(LC.state_tensors(state, LC.learner_opts(L))), "grads": _np(grads),
            "adv": adv.numpy().copy(), "ret": ret.numpy().copy()}


def _case_branch(LC, rank):
    import dp_reference as DR
    from hns_amd import critic_train as CT
    from hns_amd import policy_train as PT
    from hns_amd import sharding
    critic, obs, bv, ret, sl = DR.branch_flip_case(A=A, D=D)
    rows = bv.shape[0] * A
    t = lambda x: torch.as_tensor(x[sl[rank]])                   # noqa: E731
    args = (t(obs["state_self"]), t(obs["state_others"]), t(obs["cylinders"]), t(bv), t(ret))
    out = {}
    for how in ("global", "per_rank"):
        c = {k: torch.nn.Parameter(torch.as_tensor(v)) for k, v in critic.items()}
        bucket = PT.GradBucket(CT.critic_parameters(c))
        own = CT.value_loss_sums(c, *args).sums
        sums = sharding.all_reduce_sum(own.clone(), dist.group.WORLD) if how == "global" else own     # per_rank: each rank decides on its own sums
        res = CT.value_loss_and_grad(c, *args, sums=sums, global_rows=rows, group=dist.group.WORLD, bucket=bucket)
        out[how] = {"value_loss": float(res.value_loss), "explained_var": float(res.explained_var), "grad_norm": float(res.grad_norm),
                    "grads": _np({k: v.grad for k, v in c.items()})}
    return out


def _case_tp(LC, rank):
    from hns_amd import learner
    cfg = dict(LC.CFG, **UNION_CFG)
    state0 = LC.make_state(A, 31)
    ro = LC.make_rollout(state0, 8, T, A, 32)
    state = LC.clone_state(state0)
    mine = _cut(ro, slice(0, 4) if rank == 0 else slice(4, 8))
    if rank == 1:
        mine["tp"] = (mine["tp"][0], mine["tp"][1], torch.zeros_like(mine["tp"][2]))        # no window selected on this rank
    L = learner.DeviceLearner(state["actor"], state["critic"], cfg, tp_net=state["tp"], value_normalizer=state["vn"],
                              generator=torch.Generator().manual_seed(200 + rank), group="world")
    info = L.train_rollout(**mine)
    return {"info": info, "state": _np(LC.state_tensors(state, LC.learner_opts(L)))}


def _case_refusals(LC, rank):
    from hns_amd import learner
    group = dist.new_group(ranks=[0, 1], backend="gloo", timeout=datetime.timedelta(seconds=20))
    state0 = LC.make_state(A, 41)
    out = {}
    for name, cfg, shape in (("minibatches", dict(LC.CFG, num_minibatches=1 + rank), (2, T)),
                             ("short", dict(LC.CFG, num_minibatches=4), (2, T) if rank == 0 else (1, 2))):
        state = LC.clone_state(state0)
        ro = LC.make_rollout(state0, *shape, A, 42)
        ro.pop("tp")
        L = learner.DeviceLearner(state["actor"], state["critic"], cfg, tp_net=None, value_normalizer=state["vn"], group=group)
        before = _np(LC.state_tensors(state, {}))
        try:
            L.train_rollout(**ro)
            out[name] = ("no error", "")
        except Exception as e:                                   # noqa: BLE001  (the type is what the test asserts)
            out[name] = (type(e).__name__, str(e))
        after = _np(LC.state_tensors(state, {}))
        probe = torch.ones(1)
        dist.all_reduce(probe, group=group)                      # the ranks are still in step: nobody waits in a collective of the refused call
        out[name] += (float(probe), all(np.array_equal(before[k], after[k]) for k in before))
    return out


def _worker(rank, world, port, q):
    LC = _paths()
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    torch.set_num_threads(2)
    out = {}
    try:
        for name, fn in (("union", _case_union), ("branch", _case_branch), ("tp", _case_tp), ("refusals", _case_refusals)):
            out[name] = fn(LC, rank)
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
    port = 35500 + os.getpid() % 2000
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


@pytest.fixture(scope="module")
def cases():
    LC = _paths()
    import dp_reference as DR
    yield LC, DR
    LC.D = 35                                                    # learner_cases' own width, for the modules collected after this one


def _same_bits(a, b):
    assert set(a) == set(b)
    bad = [k for k in a if a[k].tobytes() != b[k].tobytes() or a[k].shape != b[k].shape]
    assert not bad, f"{len(bad)} of {len(a)} tensors differ between the ranks: {bad[:8]}"


@pytest.mark.timeout(300)
def test_two_ranks_perform_the_union_update(ranks, cases):
    LC, DR = cases
    r0, r1 = ranks[0]["union"], ranks[1]["union"]
    assert r0["same_start"] and r1["same_start"]                 # rank 1's other weights were replaced by rank 0's at construction
    _same_bits(r0["state"], r1["state"])                         # parameters, Adam moments and step counts, ValueNorm1
    _same_bits(r0["grads"], r1["grads"])
    assert r0["info"] == r1["info"] and all(np.isfinite(v) for v in r0["info"].values()), (r0["info"], r1["info"])
    # the all-reduced gradients against autograd over the union minibatch (one minibatch: every env-step of both ranks)
    state0, ro = _union_start(LC)
    cfg = dict(LC.CFG, **UNION_CFG)
    S = 10 * T
    flat = lambda t: t.reshape(S, *t.shape[2:])                  # noqa: E731
    obs = DR.obs_dict(flat(ro["obs_self"]), flat(ro["obs_others"]), flat(ro["obs_cylinders"]))
    adv, ret = (np.concatenate([r0[k], r1[k]]).reshape(S, A, 1) for k in ("adv", "ret"))
    actor = {k: v.detach().numpy() for k, v in state0["actor"].items()}
    critic = {k: v.detach().numpy() for k, v in state0["critic"].named_parameters()}
    a64, a32 = DR.actor_refs(actor, obs, flat(ro["action"]).numpy(), flat(ro["log_probs"]).numpy(), adv, clip_param=cfg["clip_param"],
                             entropy_coef=cfg["entropy_coef"])
    c64, c32 = DR.critic_refs(critic, obs, flat(ro["state_value"]).numpy(), ret, clip_param=cfg["clip_param"], loss="huber",
                              huber_delta=float(cfg["critic"]["huber_delta"]))
    got_a = {k[len("actor."):]: v for k, v in r0["grads"].items() if k.startswith("actor.")}
    got_c = {k[len("critic."):]: v for k, v in r0["grads"].items() if k.startswith("critic.")}
    info = r0["info"]
    DR.assert_within_bar("union actor", DR.grad_items(got_a, a64, a32) + [
        ("policy_loss", info["drone/policy_loss"], a64["policy_loss"], a32["policy_loss"]), ("entropy", info["drone/entropy"], a64["entropy"], a32["entropy"]),
        ("grad_norm", info["drone/actor_grad_norm"], a64["grad_norm"], a32["grad_norm"])])
    DR.assert_within_bar("union critic", DR.grad_items(got_c, c64, c32) + [
        ("value_loss", info["drone/value_loss"], c64["value_loss"], c32["value_loss"]),
        ("explained_var", info["drone/explained_var"], c64["explained_var"], c32["explained_var"]),
        ("grad_norm", info["drone/critic_grad_norm"], c64["grad_norm"], c32["grad_norm"])])
    # the predictor: weights 6 / 10 and 4 / 10 of the ranks' means are the union's mean (fp32 means of the same numbers)
    from hns_amd import tp_train
    tp = copy.deepcopy(state0["tp"])
    want = float(tp_train.update_tp(tp, *ro["tp"], LC.FUTURE, 1, 1, 1, tp_train.TPAdam(tp_train.parameters(tp), lr=1e-4)))
    assert abs(info["drone/TP_loss"] - want) <= 1e-6 * abs(want), (info["drone/TP_loss"], want)


@pytest.mark.timeout(300)
def test_the_branch_of_the_max_is_the_unions(ranks, cases):
    _, DR = cases
    critic, obs, bv, ret, sl = DR.branch_flip_case(A=A, D=D)
    DR.assert_branch_precondition(critic, obs, bv, ret, sl)      # rank 0 alone: unclipped; the union: clipped; none near the tie
    c64, c32 = DR.critic_refs(critic, obs, bv, ret)
    g0, g1 = ranks[0]["branch"]["global"], ranks[1]["branch"]["global"]
    _same_bits(g0["grads"], g1["grads"])
    assert (g0["value_loss"], g0["explained_var"], g0["grad_norm"]) == (g1["value_loss"], g1["explained_var"], g1["grad_norm"])
    DR.assert_within_bar("branch flip", DR.grad_items(g0["grads"], c64, c32) + [(k, g0[k], c64[k], c32[k]) for k in ("value_loss", "explained_var", "grad_norm")])
    # each rank deciding on its own sums takes rank 0's rows down the other branch: far outside the bar
    worst = max(DR.ratios(DR.grad_items(ranks[0]["branch"]["per_rank"]["grads"], c64, c32)).values())
    assert worst > DR.BAR, worst


@pytest.mark.timeout(300)
def test_a_rank_without_selected_windows_still_steps_with_the_others(ranks, cases):
    LC, _ = cases
    r0, r1 = ranks[0]["tp"], ranks[1]["tp"]
    _same_bits(r0["state"], r1["state"])
    assert r0["info"] == r1["info"]
    from hns_amd import tp_train
    state0 = LC.make_state(A, 31)
    ro = _cut(LC.make_rollout(state0, 8, T, A, 32), slice(0, 4))     # the union's selected windows are rank 0's
    tp = copy.deepcopy(state0["tp"])
    want = float(tp_train.update_tp(tp, *ro["tp"], LC.FUTURE, 1, 1, 1, tp_train.TPAdam(tp_train.parameters(tp), lr=1e-4)))
    assert abs(r0["info"]["drone/TP_loss"] - want) <= 1e-6 * abs(want), (r0["info"]["drone/TP_loss"], want)
    moved = [k for k, v in r1["state"].items() if k.startswith("tp.") and not np.array_equal(v, state0["tp"].state_dict()[k[3:]].numpy())]
    assert len(moved) == 6                                       # the rank without windows stepped its predictor too


@pytest.mark.timeout(300)
def test_disagreeing_ranks_are_refused_before_the_updates(ranks):
    for r in ranks:
        for name, word in (("minibatches", "num_minibatches differs"), ("short", "fewer env-steps than num_minibatches")):
            kind, text, probe, untouched = r["refusals"][name]
            assert kind == "ValueError" and word in text, (name, kind, text)
            assert probe == 2.0 and untouched
