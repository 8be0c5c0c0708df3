"""The actor's update (hns_amd.actor_train), CPU part: the CPU path is the reference's torch statements (autograd, clip_grad_norm_,
torch.optim.Adam) — checked here bit for bit against g_actor_update.npz (the reference's own update_actor, recorded), against
tests/actor_update_reference.py (fp32 to autograd's own error) and against torch's own optimiser; the per-row rule of the clipped surrogate's
backward pass against fp64 autograd; every refusal raised before any launch; the C entry points refusing bad arguments without a device; the
critic's workspace sizes unchanged by the actor's longer partial rows.  The device part is tests/test_hip_actor_train.py."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

import actor_update_reference as U
from hns_amd import abi
from hns_amd import actor_train as AT
from hns_amd import critic_train as CT
from hns_amd import policy as P

CASES = ["a3k5d35", "a3k8d20", "a1k5d20", "a6k16d24"]
BIG = 5                                                         # in_proj, out_proj, linear1, linear2, the state_self embedding: pinned by the digests


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
    """g_actor_update.npz: the reference's own Actor + DiagGaussian + PartialAttentionEncoder through update_actor's statements, twice.  The
    CPU path gives the same bits: the four scalars of both updates, every clipped gradient (stored in full or through the sha256 over all of
    them), the parameters after the two updates."""
    actor, obs, action, lpo, adv, index, ent_coef, rec = U.golden_case(_npz("g_actor_update"), _npz("g_policy"), tag)
    p = {k: torch.nn.Parameter(torch.as_tensor(v)) for k, v in actor.items()}
    cfg = {"clip_param": 0.1, "entropy_coef": ent_coef, "max_grad_norm": 10.0, "actor": {"lr": 5e-4}}
    opt = AT.make_optimizer(p, cfg)
    t = torch.as_tensor
    for u in (1, 2):
        st = AT.update_actor(p, t(obs["state_self"]), t(obs["state_others"]) if "state_others" in obs else None, t(obs["cylinders"]), t(action), t(lpo),
                             t(adv), opt, index=t(index), cfg=cfg, check_index=True)
        for mine, theirs in (("policy_loss", "policy_loss"), ("actor_grad_norm", "grad_norm"), ("entropy", "entropy"), ("ESS", "ESS")):
            assert np.float32(st[mine]) == rec[f"u{u}:{theirs}"], (u, mine, float(st[mine]), rec[f"u{u}:{theirs}"])
        grads = {k: v.grad.numpy() for k, v in p.items()}          # ClippedAdam leaves the clipped gradients, as torch does
        if u == 1:
            stored = [k for k in p if f"grad:{k}" in rec]
            assert len(stored) == len(p) - BIG
            for k in stored:
                assert np.array_equal(grads[k], rec[f"grad:{k}"]), k
        assert _digest(grads.values()) == str(rec[f"u{u}:grad_digest"]), u
    assert (float(rec["u1:grad_norm"]) > 10.0) == (tag == "a3k8d20")   # the case with the norm clip active
    assert (ent_coef == 0.0) == (tag == "a1k5d20")
    for k, v in p.items():
        if f"final:{k}" in rec:
            assert np.array_equal(v.detach().numpy(), rec[f"final:{k}"]), k
    assert _digest([v.detach().numpy() for v in p.values()]) == str(rec["final_digest"])


@pytest.mark.parametrize("tag", CASES)
def test_fixture_cases_stay_off_the_clip(tag):
    """In fp64: no ratio of a recorded case within 1e-3 of 1 +- clip_param (the smallest distance is >= 0.03 by construction), all three kinds of
    rows occur, and the fp64 restatement's scalars are the recorded fp32 ones to fp32's error."""
    actor, obs, action, lpo, adv, index, ent_coef, rec = U.golden_case(_npz("g_actor_update"), _npz("g_policy"), tag)
    r = U.loss_and_grad(actor, obs, action, lpo, adv, index, entropy_coef=ent_coef)
    assert U.assert_off_the_clip(r) > 0.03
    scale = max(1.0, np.abs(r["adv"]).max())
    assert abs(r["policy_loss"] - float(rec["u1:policy_loss"])) <= 1e-5 * scale
    assert abs(r["entropy"] - float(rec["u1:entropy"])) <= 1e-5 and abs(r["ess"] - float(rec["u1:ESS"])) <= 1e-5
    assert abs(r["grad_norm"] - float(rec["u1:grad_norm"])) <= 1e-4 * r["grad_norm"]


def _case(S=24, A=3, K=5, D=20, seed=0, B=17, adv_scale=1.0):
    actor, _ = P.random_parameters(D, A, seed)
    g = torch.Generator().manual_seed(seed + 1)
    actor = {k: v + torch.randn(v.shape, generator=g) * (0.2 if k.endswith("log_std") else 0.05) for k, v in actor.items()}
    xs = torch.randn(S, A, 1, D, generator=g) * 0.7
    xo = torch.randn(S, A, A - 1, 3, generator=g) * 0.5 if A > 1 else None
    xc = torch.randn(S, A, K, 5, generator=g) * 0.5
    a_np, o_np = {k: v.numpy() for k, v in actor.items()}, _obs_np(xs, xo, xc)
    action = U.sample_actions(a_np, o_np, seed + 2)
    lpo = U.make_old_log_probs(U.new_log_probs(a_np, o_np, action), seed + 3)
    adv = torch.randn(S, A, 1, generator=g) * adv_scale
    idx = torch.randperm(S, generator=g)[:B]
    return actor, xs, xo, xc, torch.as_tensor(action), torch.as_tensor(lpo), adv, idx


def _obs_np(xs, xo, xc):
    o = {"state_self": xs.numpy(), "cylinders": xc.numpy()}
    if xo is not None:
        o["state_others"] = xo.numpy()
    return o


@pytest.mark.parametrize("ent_coef", [0.001, 0.0])
@pytest.mark.parametrize("A", [3, 1])
def test_cpu_path_matches_the_restatement(ent_coef, A):
    """fp32 against fp32 to autograd's own error, fp32 against fp64 to fp32's; both layouts read the same minibatch."""
    actor, xs, xo, xc, action, lpo, adv, idx = _case(A=A, seed=3 + A)
    out = AT.policy_loss_and_grad(actor, xs, xo, xc, action, lpo, adv, idx, entropy_coef=ent_coef)
    args = ({k: v.numpy() for k, v in actor.items()}, _obs_np(xs, xo, xc), action.numpy(), lpo.numpy(), adv.numpy(), idx.numpy())
    r64 = U.loss_and_grad(*args, entropy_coef=ent_coef)
    r32 = U.loss_and_grad(*args, entropy_coef=ent_coef, dtype=torch.float32)
    U.assert_off_the_clip(r64)
    assert out.policy_loss.dim() == 0 and out.log_probs.shape == (17, A, 1) and len(actor) == (23 if A > 1 else 21)
    for n in ("policy_loss", "entropy", "ess", "grad_norm"):
        assert abs(float(getattr(out, n)) - r64[n]) <= 2e-5 * max(1.0, abs(r64[n])), n
        assert abs(float(getattr(out, n)) - r32[n]) <= 1e-5 * max(1.0, abs(r32[n])), n
    assert np.abs(out.log_probs.numpy() - r64["log_probs"]).max() <= 1e-4
    for k, v in actor.items():
        assert v.grad.shape == v.shape
        for r, tol in ((r64, 1e-4), (r32, 2e-5)):
            assert np.abs(v.grad.numpy() - r["grads"][k]).max() <= tol * max(1e-3, np.abs(r["grads"][k]).max()), k
    g1 = {k: v.grad.clone() for k, v in actor.items()}
    lay = lambda t: t.reshape(4, 6, *t.shape[1:]) if t is not None else None
    out2 = AT.policy_loss_and_grad(actor, lay(xs), lay(xo), lay(xc), lay(action), lay(lpo), lay(adv), idx, entropy_coef=ent_coef)
    assert torch.equal(out.policy_loss, out2.policy_loss) and all(torch.equal(g1[k], actor[k].grad) for k in actor)


@pytest.mark.parametrize("A", [3, 1])
def test_hand_derived_rule_matches_fp64_autograd(A):
    """d logp = -k adv r w / n with w from the clip, pushed through autograd of logp alone, plus -entropy_coef on log_std: the rule the kernel
    implements, against autograd of the loss as written, in fp64."""
    actor, xs, xo, xc, action, lpo, adv, idx = _case(A=A, seed=13 + A, adv_scale=3.0)
    args = ({k: v.numpy() for k, v in actor.items()}, _obs_np(xs, xo, xc), action.numpy(), lpo.numpy(), adv.numpy(), idx.numpy())
    ra, rh = U.loss_and_grad(*args), U.loss_and_grad(*args, hand=True)
    U.assert_off_the_clip(ra)
    for k in ra["grads"]:
        assert np.abs(ra["grads"][k] - rh["grads"][k]).max() <= 1e-13 * max(1.0, np.abs(ra["grads"][k]).max()), k
    # chunked (the large minibatches of the device tests) against one piece
    rc = U.loss_and_grad(*args, chunk=5)
    assert abs(rc["policy_loss"] - ra["policy_loss"]) <= 1e-13 and abs(rc["ess"] - ra["ess"]) <= 1e-13
    for k in ra["grads"]:
        assert np.abs(ra["grads"][k] - rc["grads"][k]).max() <= 1e-13 * max(1.0, np.abs(ra["grads"][k]).max()), k


def test_update_actor_is_clip_grad_norm_and_torch_adam():
    actor, xs, xo, xc, action, lpo, adv, idx = _case(seed=21, adv_scale=40.0)       # the norm exceeds max_grad_norm: the clip is active
    a = {k: torch.nn.Parameter(v.clone()) for k, v in actor.items()}
    b = {k: torch.nn.Parameter(v.clone()) for k, v in actor.items()}
    oa = AT.make_optimizer(a)
    ob = torch.optim.Adam(b.values(), lr=5e-4)
    for it in range(3):
        st = AT.update_actor(a, xs, xo, xc, action, lpo, adv, oa, index=idx)
        out = AT.policy_loss_and_grad(b, xs, xo, xc, action, lpo, adv, idx)
        norm = torch.nn.utils.clip_grad_norm_(list(b.values()), 10.0)
        ob.step()
        assert torch.equal(st["actor_grad_norm"], norm) and torch.equal(st["policy_loss"], out.policy_loss) and torch.equal(st["ESS"], out.ess)
        assert torch.equal(st["entropy"], out.entropy) and set(st) == {"policy_loss", "actor_grad_norm", "entropy", "ESS"}
        assert it > 0 or float(norm) > 10.0
    for k in a:
        assert torch.equal(a[k], b[k]), k
    sa, sb = oa.state_dict(), ob.state_dict()
    assert sa["param_groups"] == sb["param_groups"]
    for i in sb["state"]:
        for n in sb["state"][i]:
            assert torch.equal(sa["state"][i][n], sb["state"][i][n]), (i, n)
    assert all(v._version > 0 for v in a.values())              # the step bumps the version counters: DevicePolicy re-packs


@pytest.mark.parametrize("case", ["dtype_obs", "dtype_param", "dtype_action", "noncontig_param", "shape_adv", "shape_logp", "shape_action", "self_dim",
                                  "others_missing", "cyl_17", "index_range", "index_negative", "index_dtype", "index_empty", "index_strided", "plain_adam",
                                  "foreign_name", "rnn", "per_agent_actor", "share_actor", "tanh", "actor_rnn", "lr_scheduler", "weight_decay",
                                  "group_weight_decay", "clip_param", "critic_params"])
def test_refusals_raise_before_any_launch(case):
    actor, xs, xo, xc, action, lpo, adv, idx = _case(seed=31)
    err, cfg = ValueError, None
    if case == "dtype_obs":
        xs, err = xs.double(), TypeError
    elif case == "dtype_param":
        actor["encoder.linear1.weight"] = actor["encoder.linear1.weight"].double()
        err = TypeError
    elif case == "dtype_action":
        action, err = action.double(), TypeError
    elif case == "noncontig_param":
        actor["encoder.linear1.weight"] = actor["encoder.linear1.weight"].t()
    elif case == "shape_adv":
        adv = adv[:-1]
    elif case == "shape_logp":
        lpo = lpo[:-1]
    elif case == "shape_action":
        action = action[..., :3]
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
        idx = torch.stack([idx, idx], dim=1)[:, 0]
        assert not idx.is_contiguous()
    elif case == "plain_adam":
        with pytest.raises(TypeError):
            AT.update_actor(actor, xs, xo, xc, action, lpo, adv, torch.optim.Adam([torch.zeros(1, requires_grad=True)]), index=idx)
        return
    elif case == "foreign_name":
        actor["encoder.extra.weight"] = torch.zeros(3)
        err = P.PolicyConfigError
    elif case == "rnn":
        actor["rnn.weight_ih_l0"] = torch.zeros(3)
        err = P.PolicyConfigError
    elif case == "per_agent_actor":                              # share_actor: False stacks every parameter over the agents
        actor = {k: torch.stack([v, v, v]) for k, v in actor.items()}
        err = P.PolicyConfigError
    elif case == "critic_params":                                # the critic's network is not an actor
        _, critic = P.random_parameters(20, 3, 0)
        actor, err = critic, P.PolicyConfigError
    elif case == "share_actor":
        cfg, err = {"share_actor": False}, P.PolicyConfigError
    elif case == "tanh":
        cfg, err = {"actor": {"tanh": True}}, P.PolicyConfigError
    elif case == "actor_rnn":
        cfg, err = {"actor": {"rnn": {"cls": "gru"}}}, P.PolicyConfigError
    elif case == "lr_scheduler":
        cfg, err = {"actor": {"lr_scheduler": "LinearLR"}}, P.PolicyConfigError
    elif case == "weight_decay":
        cfg, err = {"actor": {"weight_decay": 0.01}}, NotImplementedError
    elif case == "group_weight_decay":
        opt = CT.ClippedAdam([torch.zeros(1, requires_grad=True)])
        opt.param_groups[0]["weight_decay"] = 0.1
        with pytest.raises(NotImplementedError):
            AT.update_actor(actor, xs, xo, xc, action, lpo, adv, opt, index=idx)
        return
    elif case == "clip_param":
        with pytest.raises(ValueError):
            AT.policy_loss_and_grad(actor, xs, xo, xc, action, lpo, adv, idx, clip_param=-0.1)
        return
    with pytest.raises(err):
        if cfg is not None:
            if case in ("lr_scheduler", "weight_decay"):
                AT.make_optimizer(actor, cfg)
            AT.update_actor(actor, xs, xo, xc, action, lpo, adv, CT.ClippedAdam([torch.zeros(1, requires_grad=True)]), index=idx, cfg=cfg)
        else:
            AT.policy_loss_and_grad(actor, xs, xo, xc, action, lpo, adv, idx)
    assert all(getattr(v, "grad", None) is None for v in actor.values())


def test_make_optimizer_follows_the_cfg_and_the_parameter_order():
    actor, *_ = _case(seed=41)
    p = {k: torch.nn.Parameter(v) for k, v in actor.items()}
    opt = AT.make_optimizer(p, {"actor": {"lr": 3e-4}, "max_grad_norm": 5.0})
    assert isinstance(opt, CT.ClippedAdam) and opt.param_groups[0]["lr"] == 3e-4 and opt.max_grad_norm == 5.0
    assert [id(t) for t in opt.param_groups[0]["params"]] == [id(t) for t in p.values()] and len(p) == 23
    assert AT.make_optimizer(p).param_groups[0]["lr"] == 5e-4


def test_c_entry_points_refuse_bad_arguments_without_a_device():
    lib = abi.load_library()
    f = lib.hns_actor_train_workspace_bytes
    assert f(0, 35, 3, 5) == 0 and f(96, 97, 3, 5) == 0 and f(96, 35, 8, 5) == 0 and f(96, 35, 3, 17) == 0
    assert f(96, 35, 3, 5) > 12 * 96 * 512
    net, grd, b = abi.HnsPolicyNet(), abi.HnsPolicyNet(), abi.HnsActorBatch()
    dummy = 4096
    call = lambda n, D, A, K, clip=0.1, ws=1 << 30: lib.hns_actor_train_grad(n, C.byref(b), D, A, K, clip, 0.001, C.byref(grd), dummy, dummy, dummy, dummy, None,
                                                                             dummy, ws, None)
    assert call(None, 35, 3, 5) == abi.HNS_ERR_INVALID_ARG
    for bad in ((0, 3, 5), (97, 3, 5), (35, 0, 5), (35, 8, 5), (35, 3, 0), (35, 3, 17)):
        assert call(C.byref(net), *bad) == abi.HNS_ERR_INVALID_ARG
    assert call(C.byref(net), 35, 3, 5) == abi.HNS_ERR_INVALID_ARG
    assert b"batch" in lib.hns_last_error()
    b.batch, b.num_envs, b.num_steps = 4, 2, 2
    assert call(C.byref(net), 35, 3, 5, clip=-1.0) == abi.HNS_ERR_INVALID_ARG
    assert b"clip_param" in lib.hns_last_error()
    assert call(C.byref(net), 35, 3, 5) == abi.HNS_ERR_INVALID_ARG
    assert b"parameter" in lib.hns_last_error()
    for fld in abi.POLICY_NET_FIELDS:
        setattr(net, fld, 4096)
        setattr(grd, fld, 4096)
    assert call(C.byref(net), 35, 3, 5) == abi.HNS_ERR_INVALID_ARG
    assert b"observation" in lib.hns_last_error()
    b.obs_self = b.obs_others = b.obs_cylinders = 4096
    assert call(C.byref(net), 35, 3, 5) == abi.HNS_ERR_INVALID_ARG
    assert b"action" in lib.hns_last_error()
    b.action = b.log_probs_old = b.advantages = 4096
    assert call(C.byref(net), 35, 3, 5, ws=1024) == abi.HNS_ERR_INVALID_ARG
    assert b"workspace too small" in lib.hns_last_error()
    net.log_std = 4100                                          # 4-byte aligned only
    assert call(C.byref(net), 35, 3, 5) == abi.HNS_ERR_INVALID_ARG
    assert b"aligned" in lib.hns_last_error()


# hns_critic_train_workspace_bytes(rows, self_dim, num_agents, num_cylinders) as the library returned them before the actor's head joined the
# partial-row layout
CRITIC_WORKSPACE = {(1, 1, 1, 1): 1436928, (33, 20, 3, 5): 2097920, (24576, 35, 3, 5): 212594432, (786432, 35, 3, 5): 6187259648,
                    (51, 20, 1, 5): 2097920, (102, 24, 6, 16): 3379968, (7, 96, 7, 16): 1582848, (196608, 35, 3, 5): 1561712384,
                    (0, 35, 3, 5): 0, (32, 97, 3, 5): 0}


def test_critic_workspace_bytes_are_unchanged():
    lib = abi.load_library()
    for shape, want in CRITIC_WORKSPACE.items():
        assert lib.hns_critic_train_workspace_bytes(*shape) == want, shape
        if want:
            more = lib.hns_actor_train_workspace_bytes(*shape) - want
            tiles = (shape[0] + 31) // 32
            assert 0 < more <= tiles * (2 * 388 * 4 + 17 * 8) + 4 * 256, shape       # three head rows + log_std per partial row, 17 more fp64 partials per tile
