"""The critic's update (hns_amd.critic_train), CPU part: the CPU path is the reference's torch statements (autograd, clip_grad_norm_,
torch.optim.Adam) — checked here against tests/critic_update_reference.py and against torch's own optimiser; the branch rule of the max of
the two mean losses, including the exact tie; ClippedAdam's state_dict through torch.optim.Adam both ways; the numpy restatement of clip +
Adam that hns_adam_clipped is held to on the device against torch (the checker checks itself); every refusal raised before any launch, and
the C entry points refusing bad arguments without a device.  The device part is tests/test_hip_critic_train.py."""
import copy
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

import critic_update_reference as U
from hns_amd import abi
from hns_amd import critic_train as CT
from hns_amd import policy as P


CASES = ["a3k5d35", "a3k8d20", "a1k5d20", "a6k16d24"]


def _digest(arrs):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a, dtype=np.float32).tobytes() for a in arrs)).hexdigest()


def _npz(name):
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))


@pytest.fixture
def one_thread():
    """The golden was written with one intra-op thread: CPU GEMMs split their sums by thread count."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("tag", CASES)
def test_cpu_update_matches_reference_golden_bit_for_bit(one_thread, tag):
    """g_critic_update.npz: the reference's own Critic + PartialAttentionEncoder through update_critic's statements, twice.  The CPU path
    gives the same bits: the three scalars of both updates, every clipped gradient (stored in full or through the sha256 over all of them),
    the parameters after the two updates."""
    critic, obs, bv, ret, index, loss, rec = U.golden_case(_npz("g_critic_update"), _npz("g_policy"), tag)
    p = {k: torch.nn.Parameter(torch.as_tensor(v)) for k, v in critic.items()}
    opt = CT.ClippedAdam(p.values(), lr=5e-4, max_grad_norm=10.0)
    t = torch.as_tensor
    cfg = {"clip_param": 0.1, "critic": {"use_huber_loss": loss == "huber", "huber_delta": 10}}
    for u in (1, 2):
        st = CT.update_critic(p, t(obs["state_self"]), t(obs["state_others"]) if "state_others" in obs else None, t(obs["cylinders"]), t(bv), t(ret),
                              opt, index=t(index), cfg=cfg, check_index=True)
        assert np.float32(st["value_loss"]) == rec[f"u{u}:value_loss"], (u, float(st["value_loss"]), rec[f"u{u}:value_loss"])
        assert np.float32(st["critic_grad_norm"]) == rec[f"u{u}:grad_norm"], u
        assert np.float32(st["explained_var"]) == rec[f"u{u}:explained_var"], u
        assert np.float32(st["value_loss"]) == max(rec[f"u{u}:l_orig"], rec[f"u{u}:l_clip"])
        grads = {k: v.grad.numpy() for k, v in p.items()}          # ClippedAdam leaves the clipped gradients, as torch does
        if u == 1:
            stored = [k for k in p if f"grad:{k}" in rec]
            assert len(stored) == (len(p) if tag == CASES[0] else len(p) - 4)
            for k in stored:
                assert np.array_equal(grads[k], rec[f"grad:{k}"]), k
        assert _digest(grads.values()) == str(rec[f"u{u}:grad_digest"]), u
    if tag == "a1k5d20":
        assert float(rec["u1:grad_norm"]) > 10.0                   # the case with the clip active
    for k, v in p.items():
        if f"final:{k}" in rec:
            assert np.array_equal(v.detach().numpy(), rec[f"final:{k}"]), k
    assert _digest([v.detach().numpy() for v in p.values()]) == str(rec["final_digest"])


@pytest.mark.parametrize("tag", CASES)
def test_fixture_cases_take_the_recorded_branch(tag):
    """The branch of the max the reference took (recorded from its two fp32 means) is the one the fp64 restatement takes, both branches occur
    across the cases, and the CPU path's value_loss is the recorded larger mean."""
    critic, obs, bv, ret, index, loss, rec = U.golden_case(_npz("g_critic_update"), _npz("g_policy"), tag)
    r = U.loss_and_grad(critic, obs, bv, ret, index, loss=loss)
    assert r["branch"] == int(rec["branch"]) == {"a3k5d35": 0, "a3k8d20": 1, "a1k5d20": 0, "a6k16d24": 1}[tag]
    assert abs(r["l_orig"] - float(rec["u1:l_orig"])) <= 1e-5 * r["value_loss"] and abs(r["l_clip"] - float(rec["u1:l_clip"])) <= 1e-5 * r["value_loss"]
    assert abs(r["l_orig"] - r["l_clip"]) >= 1e-3 * r["value_loss"]


def _case(S=24, A=3, K=5, D=20, seed=0, B=17):
    _, critic = P.random_parameters(D, A, seed)
    g = torch.Generator().manual_seed(seed + 1)
    critic = {k: (v + torch.randn(v.shape, generator=g) * 0.05) * (30.0 if k == "v_out.weight" else 1.0) for k, v in critic.items()}
    xs = torch.randn(S, A, 1, D, generator=g) * 0.7
    xo = torch.randn(S, A, A - 1, 3, generator=g) * 0.5 if A > 1 else None
    xc = torch.randn(S, A, K, 5, generator=g) * 0.5
    with torch.no_grad():
        v = P.torch_forward(None, {P.CRITIC_NAMES[k]: t for k, t in critic.items()}, xs, xo, xc, value_only=True).value
    bv = v + torch.randn(v.shape, generator=g) * 0.1
    ret = v + torch.randn(v.shape, generator=g)
    idx = torch.randperm(S, generator=g)[:B]
    return critic, xs, xo, xc, bv, ret, idx


def _obs_np(xs, xo, xc):
    o = {"state_self": xs.numpy(), "cylinders": xc.numpy()}
    if xo is not None:
        o["state_others"] = xo.numpy()
    return o


@pytest.mark.parametrize("loss", ["huber", "mse"])
@pytest.mark.parametrize("A", [3, 1])
def test_cpu_path_matches_the_fp64_restatement(loss, A):
    critic, xs, xo, xc, bv, ret, idx = _case(A=A, seed=3 + A)
    out = CT.value_loss_and_grad(critic, xs, xo, xc, bv, ret, idx, loss=loss)
    r = U.loss_and_grad({k: v.numpy() for k, v in critic.items()}, _obs_np(xs, xo, xc), bv.numpy(), ret.numpy(), idx.numpy(), loss=loss)
    assert out.value_loss.dim() == 0 and out.values.shape == (17, A, 1)
    for n in ("value_loss", "explained_var", "grad_norm"):
        assert abs(float(getattr(out, n)) - r[n]) <= 2e-5 * max(1.0, abs(r[n])), n
    for k, v in critic.items():
        assert v.grad.shape == v.shape
        assert np.abs(v.grad.numpy() - r["grads"][k]).max() <= 1e-4 * max(1e-3, np.abs(r["grads"][k]).max()), k
    # the rollout layout [N, T, A, ...] and the env's [.., A, 1, D] state_self read the same minibatch
    g1 = {k: v.grad.clone() for k, v in critic.items()}
    lay = lambda t: t.reshape(4, 6, *t.shape[1:]) if t is not None else None
    out2 = CT.value_loss_and_grad(critic, lay(xs), lay(xo), lay(xc), lay(bv), lay(ret), idx, loss=loss)
    assert torch.equal(out.value_loss, out2.value_loss) and all(torch.equal(g1[k], critic[k].grad) for k in critic)


def test_branch_rule_and_the_exact_tie():
    critic, xs, xo, xc, bv, ret, idx = _case(seed=11)
    with torch.no_grad():
        v = P.torch_forward(None, {P.CRITIC_NAMES[k]: t for k, t in critic.items()}, xs, xo, xc, value_only=True).value
    c_np, o_np = {k: t.numpy() for k, t in critic.items()}, _obs_np(xs, xo, xc)
    for shift, want in ((+0.3, 0), (-0.3, 1)):
        half = torch.arange(v.numel()).reshape(v.shape) % 2 == 0
        b2 = torch.where(half, v + shift * torch.sign(ret - v), v)
        r = U.loss_and_grad(c_np, o_np, b2.numpy(), ret.numpy(), idx.numpy())
        assert r["branch"] == want
        out = CT.value_loss_and_grad(critic, xs, xo, xc, b2, ret, idx)
        assert abs(float(out.value_loss) - max(r["l_orig"], r["l_clip"])) < 1e-5
        for k, t in critic.items():
            assert np.abs(t.grad.numpy() - r["grads"][k]).max() <= 1e-4 * max(1e-3, np.abs(r["grads"][k]).max()), (shift, k)
    # an exact tie: b_values = 0 and a clip wider than every |v| make clipped = 0 + (v - 0) = v bit for bit, so the two means are the same
    # number; torch.max's backward gives each branch half, and the halves add up to the unclipped loss's gradient (the branch-0 case above,
    # whose gradient does not depend on b_values)
    first = {k: t.grad.clone() for k, t in critic.items()}      # (the last loop iteration was branch 1: recompute branch 0)
    half = torch.arange(v.numel()).reshape(v.shape) % 2 == 0
    CT.value_loss_and_grad(critic, xs, xo, xc, torch.where(half, v + 0.3 * torch.sign(ret - v), v), ret, idx)
    first = {k: t.grad.clone() for k, t in critic.items()}
    zeros = torch.zeros_like(v)
    out = CT.value_loss_and_grad(critic, xs, xo, xc, zeros, ret, idx, clip_param=100.0)
    r = U.loss_and_grad(c_np, o_np, zeros.numpy(), ret.numpy(), idx.numpy(), clip_param=100.0, dtype=torch.float32)
    assert r["branch"] == 2 and r["l_orig"] == r["l_clip"]
    for k, t in critic.items():
        scale = max(1e-3, np.abs(r["grads"][k]).max())
        assert np.abs(t.grad.numpy() - r["grads"][k]).max() <= 1e-4 * scale, k
        assert np.abs(t.grad.numpy() - first[k].numpy()).max() <= 1e-4 * scale, k


def test_update_critic_is_clip_grad_norm_and_torch_adam():
    critic, xs, xo, xc, bv, ret, idx = _case(seed=21)
    ret = ret * 40.0                                            # the norm exceeds max_grad_norm: the clip is active
    a = {k: torch.nn.Parameter(v.clone()) for k, v in critic.items()}
    b = {k: torch.nn.Parameter(v.clone()) for k, v in critic.items()}
    oa = CT.make_optimizer(a)
    ob = torch.optim.Adam(b.values(), lr=5e-4)
    for it in range(3):
        st = CT.update_critic(a, xs, xo, xc, bv, ret, oa, index=idx)
        out = CT.value_loss_and_grad(b, xs, xo, xc, bv, ret, idx)
        norm = torch.nn.utils.clip_grad_norm_(list(b.values()), 10.0)
        ob.step()
        assert torch.equal(st["critic_grad_norm"], norm) and torch.equal(st["value_loss"], out.value_loss)
        assert it > 0 or float(norm) > 10.0                     # (after the first step every row has left the clip: zero gradients, Adam coasts)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    sa, sb = oa.state_dict(), ob.state_dict()
    assert sa["param_groups"] == sb["param_groups"]
    for i in sb["state"]:
        for n in sb["state"][i]:
            assert torch.equal(sa["state"][i][n], sb["state"][i][n]), (i, n)
    # both ways, then one more step each
    c = {k: torch.nn.Parameter(v.detach().clone()) for k, v in a.items()}
    d = {k: torch.nn.Parameter(v.detach().clone()) for k, v in a.items()}
    oc = CT.make_optimizer(c)
    oc.load_state_dict(copy.deepcopy(sb))
    od = torch.optim.Adam(d.values(), lr=5e-4)
    od.load_state_dict(copy.deepcopy(sa))
    CT.update_critic(c, xs, xo, xc, bv, ret, oc, index=idx)
    CT.value_loss_and_grad(d, xs, xo, xc, bv, ret, idx)
    torch.nn.utils.clip_grad_norm_(list(d.values()), 10.0)
    od.step()
    for k in c:
        assert torch.equal(c[k], d[k]), k


def _torch_sqrt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).sqrt().numpy()


@pytest.mark.parametrize("max_norm", [10.0, 1e9])
def test_numpy_clip_and_adam_restatement_matches_torch_on_cpu(max_norm):
    """(with torch's CPU sqrt passed in: it is not correctly rounded)"""
    gen = torch.Generator().manual_seed(5)
    shapes = [(128, 35), (128,), (384, 128), (1, 128), (1,)]
    ps = [torch.randn(s, generator=gen).requires_grad_(True) for s in shapes]
    opt = torch.optim.Adam(ps, lr=5e-4, foreach=False)
    pn = [p.detach().numpy().copy() for p in ps]
    ms, vs, step = [np.zeros(s, np.float32) for s in shapes], [np.zeros(s, np.float32) for s in shapes], np.float32(0)
    for it in range(6):
        gs = [torch.randn(s, generator=gen) * (10.0 ** (it % 3 - 1)) for s in shapes]
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        norm = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
        pn, cg, ms, vs, step = U.clip_adam_np(pn, [g.numpy() for g in gs], ms, vs, step, norm.numpy(), max_norm, sqrt=_torch_sqrt)
        for k, p in enumerate(ps):
            assert np.array_equal(cg[k], p.grad.numpy()), (it, k)
            assert np.array_equal(pn[k], p.detach().numpy()), (it, k)


@pytest.mark.parametrize("case", ["dtype_obs", "dtype_param", "noncontig_param", "shape_bv", "self_dim", "others_missing", "cyl_17", "index_range",
                                  "index_negative", "index_dtype", "index_empty", "index_strided", "plain_adam", "foreign_name", "rnn", "centralised", "weight_decay", "loss",
                                  "num_critics"])
def test_refusals_raise_before_any_launch(case):
    critic, xs, xo, xc, bv, ret, idx = _case(seed=31)
    err, cfg, opt = ValueError, None, None
    if case == "dtype_obs":
        xs, err = xs.double(), TypeError
    elif case == "dtype_param":
        critic["base.linear1.weight"] = critic["base.linear1.weight"].double()
        err = TypeError
    elif case == "noncontig_param":
        critic["base.linear1.weight"] = critic["base.linear1.weight"].t()
    elif case == "shape_bv":
        bv = bv[:-1]
    elif case == "self_dim":
        xs = xs[..., :-1]
    elif case == "others_missing":
        xo = None
    elif case == "cyl_17":
        xc = torch.zeros(24, 3, 17, 5)
    elif case == "index_range":
        idx, err = torch.tensor([0, 24]), IndexError
    elif case == "index_negative":
        idx, err = torch.tensor([-1, 3]), IndexError
    elif case == "index_dtype":
        idx, err = idx.int(), TypeError
    elif case == "index_empty":
        idx = idx[:0]
    elif case == "index_strided":
        idx = torch.stack([idx, idx], dim=1)[:, 0]              # a column of a [B, 2] tensor: 1-d, int64, in range, stride 2
        assert not idx.is_contiguous()
    elif case == "plain_adam":
        with pytest.raises(TypeError):
            CT.update_critic(critic, xs, xo, xc, bv, ret, torch.optim.Adam([torch.zeros(1, requires_grad=True)]), index=idx)
        return
    elif case == "foreign_name":
        critic["base.extra.weight"] = torch.zeros(3)
        err = P.PolicyConfigError
    elif case == "rnn":
        critic["rnn.weight_ih_l0"] = torch.zeros(3)
        err = P.PolicyConfigError
    elif case == "centralised":
        cfg, err = {"critic_input": "state"}, P.PolicyConfigError
    elif case == "weight_decay":
        cfg, err = {"critic": {"weight_decay": 0.01}}, NotImplementedError
    elif case == "num_critics":
        cfg, err = {"critic": {"num_critics": 2}}, P.PolicyConfigError
    elif case == "loss":
        with pytest.raises(ValueError):
            CT.value_loss_and_grad(critic, xs, xo, xc, bv, ret, idx, loss="l1")
        return
    with pytest.raises(err):
        if cfg is not None:
            CT.update_critic(critic, xs, xo, xc, bv, ret, CT.ClippedAdam([torch.zeros(1, requires_grad=True)]), index=idx, cfg=cfg)
        else:
            CT.value_loss_and_grad(critic, xs, xo, xc, bv, ret, idx)


def test_optimizer_refusals():
    with pytest.raises(NotImplementedError):
        CT.ClippedAdam([torch.zeros(1, requires_grad=True)], weight_decay=0.1)
    with pytest.raises(ValueError):
        CT.ClippedAdam([torch.zeros(1, requires_grad=True)], max_grad_norm=-1.0)


def test_c_entry_points_refuse_bad_arguments_without_a_device():
    lib = abi.load_library()
    assert lib.hns_critic_train_workspace_bytes(0, 35, 3, 5) == 0 and lib.hns_critic_train_workspace_bytes(96, 97, 3, 5) == 0
    assert lib.hns_critic_train_workspace_bytes(96, 35, 8, 5) == 0 and lib.hns_critic_train_workspace_bytes(96, 35, 3, 17) == 0
    assert lib.hns_critic_train_workspace_bytes(96, 35, 3, 5) > 12 * 96 * 512
    net, grd, b = abi.HnsPolicyNet(), abi.HnsPolicyNet(), abi.HnsCriticBatch()
    dummy = 4096
    assert lib.hns_critic_train_grad(None, C.byref(b), 35, 3, 5, 0.1, 0, 10.0, C.byref(grd), dummy, dummy, dummy, None, dummy, 1 << 30, None) == abi.HNS_ERR_INVALID_ARG
    for bad in ((0, 3, 5), (97, 3, 5), (35, 0, 5), (35, 8, 5), (35, 3, 0), (35, 3, 17)):
        assert lib.hns_critic_train_grad(C.byref(net), C.byref(b), *bad, 0.1, 0, 10.0, C.byref(grd), dummy, dummy, dummy, None, dummy, 1 << 30, None) == abi.HNS_ERR_INVALID_ARG
    assert lib.hns_critic_train_grad(C.byref(net), C.byref(b), 35, 3, 5, 0.1, 0, 10.0, C.byref(grd), dummy, dummy, dummy, None, dummy, 1 << 30, None) == abi.HNS_ERR_INVALID_ARG
    assert b"batch" in lib.hns_last_error()
    b.batch, b.num_envs, b.num_steps = 4, 2, 2
    assert lib.hns_critic_train_grad(C.byref(net), C.byref(b), 35, 3, 5, 0.1, 7, 10.0, C.byref(grd), dummy, dummy, dummy, None, dummy, 1 << 30, None) == abi.HNS_ERR_INVALID_ARG
    assert b"loss_kind" in lib.hns_last_error()
    assert lib.hns_critic_train_grad(C.byref(net), C.byref(b), 35, 3, 5, 0.1, 0, 10.0, C.byref(grd), dummy, dummy, dummy, None, dummy, 1 << 30, None) == abi.HNS_ERR_INVALID_ARG
    assert b"parameter" in lib.hns_last_error()
    t = (abi.HnsAdamTensor * 1)()
    assert lib.hns_adam_clipped(None, 1, dummy, None, 10.0, 5e-4, 0.9, 0.999, 1e-8, None) == abi.HNS_ERR_INVALID_ARG
    assert lib.hns_adam_clipped(t, 0, dummy, None, 10.0, 5e-4, 0.9, 0.999, 1e-8, None) == abi.HNS_ERR_INVALID_ARG
    assert lib.hns_adam_clipped(t, 1, dummy, None, 10.0, 5e-4, 0.9, 0.999, 1e-8, None) == abi.HNS_ERR_INVALID_ARG      # NULL arrays
    assert lib.hns_adam_clipped(t, 1, dummy, None, 10.0, 5e-4, 1.5, 0.999, 1e-8, None) == abi.HNS_ERR_INVALID_ARG
