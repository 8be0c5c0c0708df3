"""The data-parallel learner's device entries on an MI355X: hns_grad_norm, hns_critic_train_sums,
hns_critic_train_grad_global, hns_actor_train_grad_global, DeviceLearner(group=).

  hns_grad_norm            bit for bit the numpy restatement of its documented order (tests/dp_reference.py), at every size where the code takes
                           another path: one value, a short last quad (3, 5, 255, 257, 4099), whole quads (4, 256), more than one workgroup
                           (4099 and the actor's bucket at D = 35), an entry whose square overflows fp32.  Its refusals need no device.
  identity                 with one rank (global_rows = rows, entropy_share 1) the global entries give the bits of the single-rank calls, at
                           33 rows (a full tile and a one-row tile) and at the smallest shape (A 1, K 1, D 1, one env-step), through an index.
  two emulated ranks       one minibatch split 7 + 4 env-steps: sums added, each part's global call, buckets added — against fp64 autograd over
                           the union under the update tests' bar (BAR and e_32: test_hip_critic_train.py's); the branch-flip inputs too.
  DeviceLearner(group=)    a one-rank gloo group in this process against group=None.
  two real ranks           tests/dp_learner_job.py under torch.distributed.run, both ranks on this card over gloo (a correctness run)."""
import copy
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dp_reference as DR
import learner_cases as LC
import test_hip_actor_train as TA
import test_hip_critic_train as TC
from hns_amd import abi
from hns_amd import actor_train as AT
from hns_amd import critic_train as CT
from hns_amd import learner
from hns_amd import policy_train as PT

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _norm_dev(x):
    flat = torch.as_tensor(np.asarray(x, np.float32)).cuda()
    lib = abi.load_library()
    nbytes = lib.hns_grad_norm_workspace_bytes(flat.numel())
    ws, out = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(1, device="cuda")
    assert flat.data_ptr() % 16 == 0 and nbytes >= 8
    abi.check(lib.hns_grad_norm(flat.data_ptr(), flat.numel(), out.data_ptr(), ws.data_ptr(), nbytes, None), "hns_grad_norm")
    torch.cuda.synchronize()
    return np.float32(out.item())


@gpu
@pytest.mark.parametrize("numel", [1, 3, 4, 5, 255, 256, 257, 4099, "actor"])
def test_grad_norm_is_its_documented_order_bit_for_bit(numel):
    if numel == "actor":                                         # the real bucket: the actor's 23 tensors at D = 35, 3 pursuers
        actor, _ = LC.P.random_parameters(35, 3, 1)
        numel = PT.GradBucket([torch.nn.Parameter(v) for v in actor.values()]).flat.numel()
        assert numel % 4 == 0 and 20 < -(-numel // 4096) <= 64      # some 26 workgroups, one stride of the grid
    x = (np.random.default_rng(numel).standard_normal(numel) * 0.3).astype(np.float32)
    got, want = _norm_dev(x), DR.grad_norm(x)
    assert got.tobytes() == want.tobytes(), (numel, got, want)
    assert abs(float(got) - float(np.sqrt((x.astype(np.float64) ** 2).sum()))) <= 2.0 ** -23 * float(got)


@gpu
def test_grad_norm_squares_in_fp64():
    """One entry of 3e19 among small ones: its square, 9e38, is past fp32's largest value; the norm is 3e19 to the last bit of the restatement."""
    x = (np.random.default_rng(7).standard_normal(1027) * 0.3).astype(np.float32)
    x[513] = np.float32(3e19)
    got = _norm_dev(x)
    assert np.isfinite(got) and got.tobytes() == DR.grad_norm(x).tobytes() and abs(float(got) - 3e19) <= 2.0 ** -23 * 3e19


def test_grad_norm_refusals_come_before_any_launch():
    """No device is touched: every refusal returns before the first launch (the pointers are never read)."""
    lib = abi.load_library()
    ok = 4096
    assert lib.hns_grad_norm_workspace_bytes(0) == 0 and lib.hns_grad_norm_workspace_bytes(-3) == 0
    need = lib.hns_grad_norm_workspace_bytes(100000)
    assert need >= 25 * 8 and need % 256 == 0
    for args, word in (((None, 8, ok, ok, 256), "null"), ((ok, 8, None, ok, 256), "null"), ((ok, 8, ok, None, 256), "null"),
                       ((ok + 4, 8, ok, ok, 256), "16-byte"), ((ok, 8, ok + 2, ok, 256), "misaligned"), ((ok, 8, ok, ok + 4, 256), "8-byte"),
                       ((ok, 0, ok, ok, 256), "numel"), ((ok, 100000, ok, ok, need - 1), "workspace shorter")):
        flat, numel, norm, ws, nbytes = args
        assert lib.hns_grad_norm(flat, numel, norm, ws, nbytes, None) != 0, args
        assert word in lib.hns_last_error().decode(), (args, lib.hns_last_error())


def _cuda(x):
    return torch.as_tensor(np.asarray(x)).cuda()


def _critic_args(obs, bv, ret, index):
    return (_cuda(obs["state_self"]), _cuda(obs["state_others"]) if "state_others" in obs else None, _cuda(obs["cylinders"]), _cuda(bv), _cuda(ret),
            _cuda(index) if index is not None else None)


def _actor_args(obs, action, lpo, adv, index):
    return (_cuda(obs["state_self"]), _cuda(obs["state_others"]) if "state_others" in obs else None, _cuda(obs["cylinders"]), _cuda(action), _cuda(lpo),
            _cuda(adv), _cuda(index) if index is not None else None)


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), what


@gpu
@pytest.mark.parametrize("shape", [(3, 5, 35, 11), (1, 1, 1, 1)])
def test_one_rank_global_calls_have_the_bits_of_the_single_rank_calls(shape):
    A, K, D, B = shape
    critic, obs, bv, ret, index = TC._case(16, A, K, D, 900 + A + D, B=B)
    args = _critic_args(obs, bv, ret, index)
    plain = {k: _cuda(v) for k, v in critic.items()}
    want = CT.value_loss_and_grad(plain, *args)
    c = {k: _cuda(v) for k, v in critic.items()}
    bucket = PT.GradBucket(CT.critic_parameters(c))
    s = CT.value_loss_sums(c, *args)
    got = CT.value_loss_and_grad(c, *args, sums=s.sums, global_rows=B * A, bucket=bucket)
    torch.cuda.synchronize()
    assert len(c) == 22 - (2 if A == 1 else 0)
    for k in c:
        _same(c[k].grad, plain[k].grad, k)
    _same(got.value_loss, want.value_loss, "value_loss")
    _same(got.explained_var, want.explained_var, "explained_var")
    _same(s.values, want.values, "values")
    assert DR.ulps(float(got.grad_norm), float(want.grad_norm)) <= 1, (float(got.grad_norm), float(want.grad_norm))
    assert np.float32(got.grad_norm.item()).tobytes() == DR.grad_norm(bucket.flat.cpu().numpy()).tobytes()

    actor, obs, action, lpo, adv, index = TA._case(16, A, K, D, 950 + A + D, B=B)
    args = _actor_args(obs, action, lpo, adv, index)
    plain = {k: _cuda(v) for k, v in actor.items()}
    want = AT.policy_loss_and_grad(plain, *args)
    a = {k: _cuda(v) for k, v in actor.items()}
    bucket = PT.GradBucket(AT.actor_parameters(a))
    got = AT.policy_loss_and_grad(a, *args, global_rows=B * A, entropy_share=1.0, bucket=bucket)
    torch.cuda.synchronize()
    for k in a:
        _same(a[k].grad, plain[k].grad, k)
    for n in ("policy_loss", "entropy", "ess", "log_probs"):
        _same(getattr(got, n), getattr(want, n), n)
    assert DR.ulps(float(got.grad_norm), float(want.grad_norm)) <= 1, (float(got.grad_norm), float(want.grad_norm))


def _two_part_critic(critic, obs, bv, ret, parts, per_rank=False, **kw):
    """Two emulated ranks: sums added (per_rank: each part decides on its own), each part's global call into its own bucket, buckets added."""
    rows = sum(len(p) for p in parts) * obs["state_self"].shape[1]
    nets = [{k: _cuda(v) for k, v in critic.items()} for _ in parts]
    buckets = [PT.GradBucket(CT.critic_parameters(c)) for c in nets]
    args = [_critic_args(obs, bv, ret, np.asarray(p)) for p in parts]
    own = [CT.value_loss_sums(c, *a, **kw).sums for c, a in zip(nets, args)]
    union = own[0] + own[1]                                      # the all-reduce of two ranks: one fp64 addition per value
    outs = [CT.value_loss_and_grad(c, *a, sums=o if per_rank else union, global_rows=rows, bucket=b, **kw) for c, a, o, b in zip(nets, args, own, buckets)]
    buckets[0].flat.add_(buckets[1].flat)
    norm = buckets[0].norm()
    torch.cuda.synchronize()
    return {k: v.grad.cpu().double().numpy() for k, v in nets[0].items()}, outs, float(norm)


@gpu
def test_two_emulated_ranks_meet_the_bar_over_the_union():
    A, K, D, B = 3, 5, 35, 11
    critic, obs, bv, ret, index = TC._case(16, A, K, D, 1001, B=B)
    c64, c32 = DR.critic_refs(critic, {k: v[index] for k, v in obs.items()}, bv[index], ret[index])
    assert abs(c64["l_orig"] - c64["l_clip"]) >= 1e-3 * c64["value_loss"]
    grads, outs, norm = _two_part_critic(critic, obs, bv, ret, (index[:7], index[7:]))
    assert float(outs[0].value_loss) == float(outs[1].value_loss) and float(outs[0].explained_var) == float(outs[1].explained_var)
    DR.assert_within_bar("critic 7 + 4", DR.grad_items(grads, c64, c32) + [("value_loss", float(outs[0].value_loss), c64["value_loss"], c32["value_loss"]),
                                                                          ("explained_var", float(outs[0].explained_var), c64["explained_var"], c32["explained_var"]),
                                                                          ("grad_norm", norm, c64["grad_norm"], c32["grad_norm"])])

    actor, obs, action, lpo, adv, index = TA._case(16, A, K, D, 1002, B=B)
    sub = lambda x: x[index]                                      # noqa: E731
    a64, a32 = DR.actor_refs(actor, {k: sub(v) for k, v in obs.items()}, sub(action), sub(lpo), sub(adv))
    TA.U.assert_off_the_clip(a64, 0.1, need_all=False)
    assert np.array_equal(a64["w"], a32["w"])
    nets = [{k: _cuda(v) for k, v in actor.items()} for _ in range(2)]
    buckets = [PT.GradBucket(AT.actor_parameters(n)) for n in nets]
    outs = [AT.policy_loss_and_grad(n, *_actor_args(obs, action, lpo, adv, part), global_rows=B * A, entropy_share=0.5, bucket=b)
            for n, b, part in zip(nets, buckets, (index[:7], index[7:]))]
    buckets[0].flat.add_(buckets[1].flat)
    norm = float(buckets[0].norm())
    torch.cuda.synchronize()
    grads = {k: v.grad.cpu().double().numpy() for k, v in nets[0].items()}
    loss = float(outs[0].policy_loss.double() + outs[1].policy_loss.double())        # the shares add up to the union's loss
    DR.assert_within_bar("actor 7 + 4", DR.grad_items(grads, a64, a32) + [("policy_loss", loss, a64["policy_loss"], a32["policy_loss"]),
                                                                         ("entropy", float(outs[1].entropy), a64["entropy"], a32["entropy"]),
                                                                         ("grad_norm", norm, a64["grad_norm"], a32["grad_norm"])])


@gpu
def test_the_branch_is_decided_on_the_unions_sums_on_the_device():
    critic, obs, bv, ret, sl = DR.branch_flip_case()
    DR.assert_branch_precondition(critic, obs, bv, ret, sl)
    c64, c32 = DR.critic_refs(critic, obs, bv, ret)
    parts = (np.arange(sl[0].start, sl[0].stop), np.arange(sl[1].start, sl[1].stop))
    grads, outs, norm = _two_part_critic(critic, obs, bv, ret, parts)
    DR.assert_within_bar("branch flip", DR.grad_items(grads, c64, c32) + [("value_loss", float(outs[0].value_loss), c64["value_loss"], c32["value_loss"]),
                                                                         ("explained_var", float(outs[1].explained_var), c64["explained_var"], c32["explained_var"]),
                                                                         ("grad_norm", norm, c64["grad_norm"], c32["grad_norm"])])
    wrong, _, _ = _two_part_critic(critic, obs, bv, ret, parts, per_rank=True)
    assert max(DR.ratios(DR.grad_items(wrong, c64, c32)).values()) > DR.BAR


@pytest.fixture
def one_rank_group(tmp_path):
    import torch.distributed as dist
    assert not dist.is_initialized()
    dist.init_process_group("gloo", rank=0, world_size=1, store=dist.FileStore(str(tmp_path / "store"), 1))
    yield dist.group.WORLD
    dist.destroy_process_group()


@gpu
def test_a_one_rank_group_trains_as_no_group(one_rank_group):
    """2 epochs x 2 minibatches on 8 envs x 8 steps, max_grad_norm above every norm (the two paths' norms may differ in the last place, and an
    active clip would scale by it): parameters, Adam state and ValueNorm1 bit-identical; the two gradient-norm columns within one unit in
    the last place of the MEAN of four norms each within one; every other info value identical."""
    cfg = copy.deepcopy(LC.CFG)
    cfg.update(ppo_epochs=2, num_minibatches=2, max_grad_norm=1e9)
    cpu = LC.make_state(3, 61)
    ro = LC.to_device(LC.make_rollout(cpu, 8, 8, 3, 62), "cuda")
    runs = []
    for group in (None, one_rank_group):
        state = LC.clone_state(cpu, "cuda")
        L = learner.DeviceLearner(state["actor"], state["critic"], cfg, tp_net=state["tp"], value_normalizer=state["vn"],
                                  generator=torch.Generator(device="cuda").manual_seed(9), group=group)
        info = L.train_rollout(**ro)
        torch.cuda.synchronize()
        runs.append((LC.state_tensors(state, LC.learner_opts(L)), info))
    LC.assert_same_state(runs[1][0], runs[0][0], "a one-rank group against group=None")
    plain, grouped = runs[0][1], runs[1][1]
    assert set(plain) == set(grouped)
    for k in plain:
        if k.endswith("_grad_norm"):
            assert DR.ulps(plain[k], grouped[k]) <= 1, (k, plain[k], grouped[k])
        else:
            assert plain[k] == grouped[k], (k, plain[k], grouped[k])


@gpu
@pytest.mark.timeout(700)
def test_two_ranks_on_one_gpu_over_gloo(tmp_path):
    """tests/dp_learner_job.py as a launcher starts it: two ranks share cuda:0 and the collectives run over gloo — a correctness run.  Each
    rank steps 4 envs for 8 steps (HIP env, collector, learner, predictor on) and all ranks train on the union: their parameters have one
    sha256.  The union of the ranks' rollouts, fed to ONE process with no group (one epoch of one minibatch: the union of the ranks' indices
    whatever the permutations), gives the same parameters under the update tests' bar against the fp64 train_op of
    tests/learner_f64_reference.py: e_two_ranks <= BAR max(e_one_process, 2^-24 max|p_64|) per tensor."""
    import learner_f64_reference as F64
    env = dict(os.environ, HNS_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", "29547", os.path.join(ROOT, "tests", "dp_learner_job.py"), "--out", str(tmp_path)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]           # nothing further is started after a failed job
    lines = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout                           # rank 0 only
    rep = lines[0]
    assert len(rep["digests"]) == 2 and rep["digests"][0] == rep["digests"][1]
    assert rep["infos"][0] == rep["infos"][1]
    saved = [torch.load(os.path.join(tmp_path, f"rank{r}.pt"), map_location="cpu") for r in range(2)]
    start, cfg = saved[0]["start"], saved[0]["cfg"]
    cat = lambda a, b: torch.cat([a, b]) if torch.is_tensor(a) else (tuple(cat(x, y) for x, y in zip(a, b)) if isinstance(a, tuple) else a)   # noqa: E731
    ro = {k: cat(saved[0]["rollout"][k], saved[1]["rollout"][k]) for k in saved[0]["rollout"]}
    final = saved[0]["final"]
    assert hashlib.sha256(b"".join(final[k].numpy().tobytes() for k in sorted(final))).hexdigest() == rep["digests"][0]

    A = ro["action"].shape[2]
    def fresh(device):
        critic = LC.PlainCritic(A)
        critic.load_state_dict(start["critic"])
        tp = LC.TPNet(start["tp_args"][0], start["tp_args"][1], start["tp_args"][2], start["tp_args"][3])
        tp.load_state_dict(start["tp"])
        return {"actor": {k: torch.nn.Parameter(v.clone().to(device)) for k, v in start["actor"].items()}, "critic": critic.to(device), "tp": tp.to(device),
                "vn": learner.ValueNorm1().to(device)}
    state = fresh("cuda")
    L = learner.DeviceLearner(state["actor"], state["critic"], cfg, tp_net=state["tp"], value_normalizer=state["vn"],
                              generator=torch.Generator(device="cuda").manual_seed(3))
    L.train_rollout(**LC.to_device(ro, "cuda"))
    torch.cuda.synchronize()
    one = {k: v.detach().cpu().double().numpy() for k, v in LC.state_tensors(state, {}).items()}
    N, T = ro["action"].shape[:2]
    future, keep = start["tp_args"][2], LC.FUTURE
    try:
        LC.FUTURE = future                                       # the env's predictor horizon, for the fp64 train_op's window selection
        x, _ = learner.tp_train.select_windows(*ro["tp"], future, start["tp_args"][3])
        ref = F64.train_op64(fresh("cpu"), dict(ro, agent_done=None), cfg, [list(range(x.shape[0] * x.shape[1]))], [list(range(N * T))])
    finally:
        LC.FUTURE = keep
    items = [(k, final[k].double().numpy(), ref[k], one[k]) for k in ref]
    assert len(items) == 23 + 22 + 6 + 3
    DR.assert_within_bar("two ranks against one process", items)
