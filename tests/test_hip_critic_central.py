"""The centralised critic's update on the device (hns_critic_train_grad_central, hns_adam_clipped through
hns_amd.critic_train.update_critic_central) on an MI355X.  DESIGN.md §7.20.

Shapes (A, K, D, env-steps): (3, 5, 35, 33) — two tiles, the second with one live row —, the limits (7, 16, 96, 9), one env-step of two agents,
(3, 5, 35, 65) read through a permuted index with one out-of-range entry, and one agent.  Variants as tests/test_hip_critic_train.py names
them: huber, mse, far_returns (the clipped branch wins) and an exact tie.  All 20 gradients, value_loss, explained_var, grad_norm and values
are held to the project's fp64 gate (tests/central_reference.py, BAR 8); one agent to hns_critic_train_grad's bits."""
import numpy as np
import pytest
import torch

import central_reference as CR
import critic_update_reference as U
from hns_amd import critic_train as CT
from hns_amd import policy as P

pytestmark = pytest.mark.gpu

SHAPES = [(3, 5, 35, 33), (7, 16, 96, 9), (2, 1, 20, 1), (3, 5, 35, 65), (1, 5, 20, 40)]
VARIANTS = {"huber": {}, "mse": {"loss": "mse"}, "far_returns": {}, "tie": {"clip_param": 100.0}}
RATIOS = {}


def _case(shape, variant):
    """(critic, state_drones, cylinders, b_values, b_returns, index, kwargs, live index) as numpy; the (.., 65) shape reads 50 of its
    env-steps through a permuted index whose entry 7 lies outside the rollout (it contributes nothing: `live` is the index without it)."""
    A, K, D, S = shape
    critic = CR.random_critic(D, A, 100 + A + K)
    sd, cyl = CR.random_state(S, A, K, D, 101)
    far = variant == "far_returns"
    bv, ret = CR.targets(critic, sd, cyl, 102, ret_scale=40.0 if far else 1.0, shift=-0.5 if far else None)
    if variant == "tie":
        bv = np.zeros_like(bv)
    index = live = None
    if S == 65:
        index = np.random.default_rng(5).permutation(S)[:50].astype(np.int64)
        live = np.delete(index, 7)
        index[7] = S + 3
    return critic, sd, cyl, bv, ret, index, VARIANTS[variant], live


def _dev(critic, sd, cyl, bv, ret, index, **kw):
    d = lambda x: torch.as_tensor(x).cuda()
    c = {k: d(v) for k, v in critic.items()}
    out = CT.value_loss_and_grad_central(c, d(sd), d(cyl), d(bv), d(ret), d(index) if index is not None else None, check_index=False, **kw)
    torch.cuda.synchronize()
    return c, out


def _got(c, out, rows=None):
    v = out.values.cpu().numpy()
    return {"value_loss": float(out.value_loss), "explained_var": float(out.explained_var), "grad_norm": float(out.grad_norm),
            "values": v if rows is None else v[rows], "grads": {k: t.grad.cpu().double().numpy() for k, t in c.items()}}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("shape", SHAPES, ids=["a%dk%dd%ds%d" % s for s in SHAPES])
def test_update_passes_the_fp64_gate(shape, variant):
    A, K, D, S = shape
    critic, sd, cyl, bv, ret, index, kw, live = _case(shape, variant)
    # the out-of-range entry contributes nothing: the yardstick sees the minibatch without it — but the means divide by the full batch
    ref_index = live if live is not None else index
    r64 = CR.loss_and_grad(critic, sd, cyl, bv, ret, ref_index, dtype=torch.float64, **kw)
    r32 = CR.loss_and_grad(critic, sd, cyl, bv, ret, ref_index, dtype=torch.float32, **kw)
    if variant == "tie":
        assert r64["branch"] == 2 and r32["branch"] == 2
    elif S * A > 1:
        sep = abs(r64["l_orig"] - r64["l_clip"])
        assert sep >= 1e-3 * r64["value_loss"], f"the two mean losses are {sep:.3e} apart: the case sits on the tie"
        if variant == "far_returns":
            assert r64["branch"] == 1
    c, out = _dev(critic, sd, cyl, bv, ret, index, **kw)
    rows = None
    if live is not None:
        # 49 live env-steps of a batch of 50: the kernel's means are over 50 A values (include/hns.h: "contributes nothing"), the
        # yardstick's over 49 A; value_loss and every gradient scale by 49 / 50 exactly in real arithmetic, explained_var uses n = 50
        rows = [i for i in range(50) if i != 7]
        f = 49.0 / 50.0
        for r in (r64, r32):
            r["value_loss"] *= f
            r["grad_norm"] *= f
            r["grads"] = {k: g * f for k, g in r["grads"].items()}
            v, t = r["values"].ravel(), (ret[live].astype(np.float64)).ravel()
            n = 50.0 * A
            r["explained_var"] = 1.0 - (((v - t) ** 2).sum() / n) / ((np.sum(t * t) - t.sum() ** 2 / n) / (n - 1.0))
    got = _got(c, out, rows)
    if S * A == 1:                                             # the variance of one return: NaN on every side
        assert np.isnan(got["explained_var"]) and np.isnan(r64["explained_var"])
        got["explained_var"] = r64["explained_var"] = r32["explained_var"] = 0.0
    RATIOS[(shape, variant)] = CR.gate_update("a%dk%dd%ds%d-%s" % (*shape, variant), got, r64, r32)
    kb = c["base.attn.in_proj_bias"].grad[128:256]
    assert bool((kb == 0).all())                                # in_proj_b's k third: the softmax cancels it
    assert out.values.shape == ((50 if live is not None else S), A, 1)


def test_one_agent_is_the_obs_critics_update_bit_for_bit():
    """A = 1 (1, 5, 20, 40): hns_critic_train_grad on the same tensors — state_drones as obs_self, the cylinders as its [S, 1, K, 5]."""
    critic, sd, cyl, bv, ret, _, kw, _ = _case((1, 5, 20, 40), "huber")
    index = np.random.default_rng(1).permutation(40)[:33].astype(np.int64)
    c, out = _dev(critic, sd, cyl, bv, ret, index)
    d = lambda x: torch.as_tensor(x).cuda()
    o = {k.replace("state_drones", "state_self"): d(v) for k, v in critic.items()}
    ref = CT.value_loss_and_grad(o, d(sd), None, d(cyl[:, None]), d(bv), d(ret), d(index))
    for n in ("value_loss", "explained_var", "grad_norm", "values"):
        assert torch.equal(getattr(out, n), getattr(ref, n)), n
    for k, v in c.items():
        assert torch.equal(v.grad, o[k.replace("state_drones", "state_self")].grad), k


def test_same_bits_across_calls_identity_index_and_layouts():
    shape = (3, 5, 35, 65)
    critic, sd, cyl, bv, ret, _, kw, _ = _case(shape, "huber")
    c1, o1 = _dev(critic, sd, cyl, bv, ret, None)
    c2, o2 = _dev(critic, sd, cyl, bv, ret, None)
    c3, o3 = _dev(critic, sd, cyl, bv, ret, np.arange(65, dtype=np.int64))
    d = lambda x: torch.as_tensor(x).cuda()
    # the rollout's [N, T, A, K, 5] observation tensor (agent 0's rows in place) and an [N, T, ...] layout
    wide = np.repeat(cyl[:, None], 3, axis=1)
    wide[:, 1:] += 1.0
    lay = lambda x: d(x).reshape(5, 13, *x.shape[1:])
    c4 = {k: d(v) for k, v in critic.items()}
    o4 = CT.value_loss_and_grad_central(c4, lay(sd), lay(wide), lay(bv), lay(ret))
    for c, o in ((c2, o2), (c3, o3), (c4, o4)):
        for n in ("value_loss", "explained_var", "grad_norm", "values"):
            assert torch.equal(getattr(o1, n), getattr(o, n)), n
        for k in c1:
            assert torch.equal(c1[k].grad, c[k].grad), k


def test_update_critic_central_end_to_end_and_the_policy_follows():
    """One step: the parameters equal clip_adam_np applied to the device gradients bit for bit (the clip active: max_grad_norm 0.05), and
    the policy's next value follows the step without an explicit refresh."""
    shape = A, K, D, S = (3, 5, 35, 33)
    critic, sd, cyl, bv, ret, _, kw, _ = _case(shape, "huber")
    d = lambda x: torch.as_tensor(x).cuda()
    _, out = _dev(critic, sd, cyl, bv, ret, None)
    c0, o0 = _dev(critic, sd, cyl, bv, ret, None)
    grads = [c0[k].grad.cpu().numpy() for k in critic]
    norm = np.float32(float(o0.grad_norm))
    dev = {k: torch.nn.Parameter(d(v)) for k, v in critic.items()}
    cfg = {"critic_input": "state", "max_grad_norm": 0.05}
    opt = CT.make_optimizer(dev, cfg=cfg)
    actor, _ = P.random_parameters(D, A, 5)
    pol = P.CentralCriticDevicePolicy({k: v.cuda() for k, v in actor.items()}, dev, cfg=cfg)
    obs = (torch.zeros(S, A, D, device="cuda"), torch.zeros(S, A, A - 1, 3, device="cuda"), d(np.repeat(cyl[:, None], A, axis=1)))
    before = pol.forward(*obs, d(sd), value_only=True).value.clone()
    info = CT.update_critic_central(dev, d(sd), d(cyl), d(bv), d(ret), opt, cfg=cfg)
    assert set(info) == {"value_loss", "critic_grad_norm", "explained_var"} and all(v.dim() == 0 and v.is_cuda for v in info.values())
    assert float(info["critic_grad_norm"]) == float(norm) > 0.05 and torch.equal(info["value_loss"], o0.value_loss)
    ps, _, _, _, _ = U.clip_adam_np([critic[k] for k in critic], grads, [np.zeros_like(critic[k]) for k in critic],
                                    [np.zeros_like(critic[k]) for k in critic], np.float32(0), norm, 0.05)
    for k, want in zip(critic, ps):
        assert np.array_equal(dev[k].detach().cpu().numpy(), want), k
    after = pol.forward(*obs, d(sd), value_only=True).value
    assert not torch.equal(before, after)
    new = {k: v.detach().cpu().numpy() for k, v in dev.items()}
    x = CR.ratio(after.cpu().numpy(), CR.value_np(new, sd, cyl, torch.float64), CR.value_np(new, sd, cyl, torch.float32))
    assert x <= CR.BAR, f"value after the step: ratio {x:.2f}"


def test_device_refusals_raise_before_any_launch():
    critic, sd, cyl, bv, ret, _, kw, _ = _case((3, 5, 35, 33), "huber")
    d = lambda x: torch.as_tensor(x).cuda()
    c = {k: d(v) for k, v in critic.items()}
    with pytest.raises(ValueError, match="share one device"):
        CT.value_loss_and_grad_central(c, d(sd), d(cyl), d(bv), torch.as_tensor(ret))
    odd = torch.zeros(129, device="cuda")[1:]
    with pytest.raises(ValueError, match="16-byte aligned"):
        CT.value_loss_and_grad_central({**c, "base.norm1.bias": odd.copy_(c["base.norm1.bias"])}, d(sd), d(cyl), d(bv), d(ret))
    with pytest.raises(ValueError, match="workspace"):
        CT.value_loss_and_grad_central(c, d(sd), d(cyl), d(bv), d(ret), workspace=torch.empty(256, dtype=torch.uint8, device="cuda"))
    assert all(v.grad is None for v in c.values())


def test_report_ratios():
    print("central critic gate ratios:", {"a%dk%dd%ds%d-%s" % (*k[0], k[1]): round(v, 2) for k, v in RATIOS.items()})
