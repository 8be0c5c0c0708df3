"""The MAPPO policy's forward pass on the device (hns_policy_forward through hns_amd.policy.DevicePolicy) on an MI355X.

Accuracy gate (the rule of test_tp_train.py): per output, e_hip <= 8 max(e_32, 2^-24 max|ref_64|), errors as max-abs against the fp64
restatement (tests/policy_reference.py), e_32 the error of the same statements in CPU torch fp32.  Outputs: loc, log_prob (eps supplied) and
value, on every golden case, random batches at 2 048 and 65 536 envs and three numerical edges (near-constant tokens, a saturated softmax,
observations of large magnitude), and a log_std that differs per component.  Worst measured ratio per case: see RATIOS below.
tests/test_policy_net.py proves on the CPU that this gate fails on these cases for eight seeded defects of an fp32 emulation of the kernel;
tests/test_hip_policy_edges.py holds the shape limits, a seeded shape sweep, strided views, guarded outputs and the noise contract."""
import math

import numpy as np
import pytest
import torch

import policy_reference as R
from hns_amd import policy as P

pytestmark = pytest.mark.gpu

CASES = ["a3k5d35", "a3k8d20", "a1k5d20", "a6k16d24"]
BAR = R.BAR
# worst e_hip / max(e_32, 2^-24 max|ref_64|) over loc, log_prob and value, measured on an MI355X:
#   a3k5d35 1.06, a3k8d20 1.05, a1k5d20 1.00, a6k16d24 1.10, random 2 048 envs 1.01, 65 536 envs 1.02,
#   flat_tokens 3.86 (loc), saturated_softmax 1.65 (loc), large_obs 1.03, 64-step rollout (log_prob, value) 1.15
RATIOS = {}


@pytest.fixture(scope="module")
def gp():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g_policy.npz"))


def _dev(d):
    return {k: torch.as_tensor(np.asarray(v)).cuda() for k, v in d.items()}


def _obs_dev(obs):
    return (torch.as_tensor(obs["state_self"]).cuda(), torch.as_tensor(obs["state_others"]).cuda() if "state_others" in obs else None,
            torch.as_tensor(obs["cylinders"]).cuda())


def _ref(actor, critic, obs, eps, dtype, chunk=8192):
    """The restatement in chunks of envs (the fp64 attention over all tokens is memory-hungry at 65 536 envs)."""
    E = obs["state_self"].shape[0]
    outs = []
    for s in range(0, E, chunk):
        o = {k: v[s:s + chunk] for k, v in obs.items()}
        loc, _, _, logp, value = R.forward(actor, critic, o, eps[s:s + chunk], dtype=dtype)
        outs.append((loc.double().numpy(), logp.double().numpy(), value.double().numpy()))
    return [np.concatenate([o[i] for o in outs]) for i in range(3)]


def gate(actor, critic, obs, eps):
    """Worst ratio over loc, log_prob and value; asserts the bar."""
    pol = P.DevicePolicy(_dev(actor), _dev(critic))
    out = pol.forward(*_obs_dev(obs), eps=torch.as_tensor(eps).cuda())
    hip = [out.loc.cpu().double().numpy(), out.log_prob.cpu().double().numpy(), out.value.cpu().double().numpy()]
    r64 = _ref(actor, critic, obs, eps, torch.float64)
    r32 = _ref(actor, critic, obs, eps, torch.float32)
    worst = 0.0
    for name, h, a, b in zip(("loc", "log_prob", "value"), hip, r64, r32):
        assert np.isfinite(h).all(), name
        e_hip, e_32 = float(np.abs(h - a).max()), float(np.abs(b - a).max())
        bound = max(e_32, 2.0 ** -24 * float(np.abs(a).max()))
        ratio = e_hip / bound
        print(f"  {name}: e_hip {e_hip:.3e} e_32 {e_32:.3e} ratio {ratio:.2f}")
        assert ratio <= BAR, f"{name}: e_hip {e_hip:.3e} > {BAR} x {bound:.3e}"
        worst = max(worst, ratio)
    return worst


_random_net, _random_obs = R.random_net, R.random_obs      # shared with the CPU defect table of test_policy_net.py


@pytest.mark.parametrize("tag", CASES)
def test_golden_cases_pass_the_fp64_gate(gp, tag):
    actor, critic, obs, eps, _ = R.golden_case(gp, tag)
    RATIOS[tag] = gate(actor, critic, obs, eps)


@pytest.mark.parametrize("E", [2048, 65536])
def test_random_batches_pass_the_fp64_gate(E):
    actor, critic = _random_net(35, 3, 11)
    obs, eps = _random_obs(E, 3, 5, 35, 12)
    RATIOS[f"random{E}"] = gate(actor, critic, obs, eps)


@pytest.mark.parametrize("mode", ["flat_tokens", "saturated_softmax", "large_obs"])
def test_numerical_edges_pass_the_fp64_gate(mode):
    actor, critic, obs, eps = R.edge_case(mode)                 # the cases test_policy_net.py's seeded defects are held to on the CPU
    RATIOS[mode] = gate(actor, critic, obs, eps)


def test_a_log_std_per_component_passes_the_fp64_gate():
    """log_std [-0.5, 0.2, 0.6, -0.1] (test_hip_actor_train.py's): the case on which a log-probability formed with one component's log_std
    for all four fails the gate by 2.9e7 (test_policy_net.py)."""
    actor, critic, obs, eps = R.log_std_case()
    assert len(set(np.asarray(actor["act_dist.log_std"]).tolist())) == 4
    RATIOS["log_std"] = gate(actor, critic, obs, eps)


def _golden_policy(gp, tag="a3k5d35", seed=5):
    actor, critic, obs, eps, _ = R.golden_case(gp, tag)
    return P.DevicePolicy(_dev(actor), _dev(critic), seed=seed), obs, eps


def test_action_log_prob_and_mode_are_consistent(gp):
    pol, obs, eps = _golden_policy(gp)
    x = _obs_dev(obs)
    out = pol.forward(*x, eps=torch.as_tensor(eps).cuda())
    loc, act, scale = out.loc.cpu().numpy(), out.action.cpu().numpy(), pol.scale.cpu().numpy()
    assert np.array_equal(act, (loc + scale * eps).astype(np.float32))        # bit for bit: two fp32 roundings
    var = (scale * scale).astype(np.float32)
    lp = (-((act - loc) ** 2) / (np.float32(2) * var) - np.log(scale) - np.float32(math.log(math.sqrt(2 * math.pi)))).astype(np.float32).sum(-1)
    got = out.log_prob.cpu().numpy()[..., 0]
    assert np.all(np.abs(got - lp) <= 1e-6 * (1 + np.abs(lp)))
    det = pol.forward(*x, deterministic=True)
    assert torch.equal(det.action, det.loc) and torch.equal(det.loc, out.loc) and torch.equal(det.value, out.value)
    assert torch.equal(pol.forward(*x, value_only=True).value, out.value)


def test_philox_noise_is_reproducible_fresh_and_normal(gp):
    pol, obs, _ = _golden_policy(gp, seed=123)
    x = _obs_dev(obs)
    c0 = pol.counter.clone()
    a1 = pol.forward(*x).action
    assert int(pol.counter) == int(c0) + 1
    a2 = pol.forward(*x).action
    assert not torch.equal(a1, a2)
    pol.counter.copy_(c0)
    assert torch.equal(pol.forward(*x).action, a1)          # same seed and counter: same noise
    # KS test of (action - loc) / scale over 65 536 x 3 x 4 draws
    actor, critic = _random_net(20, 3, 31)
    big = P.DevicePolicy(_dev(actor), _dev(critic), seed=2024)
    o, _ = _random_obs(65536, 3, 5, 20, 32)
    out = big.forward(*_obs_dev(o))
    z = ((out.action - out.loc) / big.scale).double().cpu().numpy().ravel()
    z.sort()
    n = z.size
    cdf = 0.5 * (1.0 + _erf(z / math.sqrt(2.0)))
    d = max(float(np.max(np.arange(1, n + 1) / n - cdf)), float(np.max(cdf - np.arange(0, n) / n)))
    assert d < 1.63 / math.sqrt(n), f"KS D = {d:.2e} (1% critical value {1.63 / math.sqrt(n):.2e})"
    assert abs(float(z.mean())) < 5e-3 and abs(float(z.std()) - 1.0) < 5e-3


def _erf(x):
    return torch.erf(torch.from_numpy(x)).numpy()


def test_two_calls_give_identical_bits_and_a_graph_replays_them(gp):
    pol, obs, eps = _golden_policy(gp)
    x = _obs_dev(obs)
    e = torch.as_tensor(eps).cuda()
    a, b = pol.forward(*x, eps=e), pol.forward(*x, eps=e)
    for n in ("action", "log_prob", "value", "loc"):
        assert torch.equal(getattr(a, n), getattr(b, n))
    pol.refresh()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pol.forward(*x)                                     # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eo = pol.forward(*x, eps=e)
        so = pol.forward(*x)
    c = int(pol.counter)
    g.replay()
    torch.cuda.synchronize()
    for n in ("action", "log_prob", "value", "loc"):
        assert torch.equal(getattr(eo, n), getattr(a, n))
    first = so.action.clone()
    assert int(pol.counter) == c + 1
    g.replay()
    torch.cuda.synchronize()
    assert int(pol.counter) == c + 2
    assert not torch.equal(first, so.action)               # fresh noise on every replay
    pol.counter.fill_(c)
    assert torch.equal(pol.forward(*x).action, first)       # ... the eager call with the same counter draws the same


def test_the_next_call_follows_an_in_place_adam_step(gp):
    actor, critic, obs, eps, _ = R.golden_case(gp, "a3k8d20")
    a_dev = {k: torch.nn.Parameter(v) for k, v in _dev(actor).items()}
    pol = P.DevicePolicy(a_dev, _dev(critic))
    x = _obs_dev(obs)
    e = torch.as_tensor(eps).cuda()
    before = pol.forward(*x, eps=e).loc.clone()
    opt = torch.optim.Adam(a_dev.values(), lr=1e-2)
    for p in a_dev.values():
        p.grad = torch.randn_like(p)
    opt.step()
    after = pol.forward(*x, eps=e)
    assert not torch.equal(before, after.loc)
    new = {k: v.detach().cpu().numpy() for k, v in a_dev.items()}
    r64 = R.forward(new, critic, obs, eps, dtype=torch.float64)
    assert np.abs(after.loc.cpu().double().numpy() - r64[0].numpy()).max() < 1e-4


def test_end_to_end_rollout_log_probs_match_the_restatement():
    from hns_amd import config
    from hns_amd.env import HideAndSeek
    E = 2048
    cfg = config.make_cfg({"num_agents": 3, "cylinder": {"max_num": 5, "min_num": 5}, "env": {"num_envs": E}}, algo={"use_TP_net": 1})
    env = HideAndSeek(cfg, headless=True)
    env.set_seed(0)
    td = env.reset()
    D = td[("agents", "observation", "state_self")].shape[-1]
    actor, critic = (dict((k, v.cuda()) for k, v in p.items()) for p in P.random_parameters(D, 3, seed=3))
    pol = P.DevicePolicy(actor, critic, seed=9)
    rec = []
    cur = td
    for t in range(64):
        cur = pol(cur)
        o = cur[("agents", "observation")]
        if t % 16 == 0:
            rec.append(({k: o[k].cpu().numpy().copy() for k in ("state_self", "state_others", "cylinders")},
                        cur[("agents", "action")].cpu().numpy().copy(), cur["drone.action_logp"].cpu().numpy().copy(),
                        cur["state_value"].cpu().numpy().copy()))
        assert cur[("agents", "action")].shape == (E, 3, 4) and cur["drone.action_logp"].shape == (E, 3, 1) and cur["state_value"].shape == (E, 3, 1)
        nxt = env.step(env.rand_step_input(cur[("agents", "action")]))["next"]
        done = nxt["done"].squeeze(-1)
        if bool(done.any()):
            rtd = env.rand_step_input()
            rtd.set("_reset", done)
            cur = env.reset(rtd)
        else:
            cur = nxt
    a_np = {k: v.cpu().numpy() for k, v in actor.items()}
    c_np = {k: v.cpu().numpy() for k, v in critic.items()}
    worst = 0.0
    for obs, act, logp, value in rec:
        _, _, _, l64, v64 = R.forward(a_np, c_np, obs, action=act, dtype=torch.float64)
        _, _, _, l32, v32 = R.forward(a_np, c_np, obs, action=act, dtype=torch.float32)
        for h, a, b in ((logp, l64.numpy(), l32.double().numpy()), (value, v64.numpy(), v32.double().numpy())):
            e_hip, e_32 = float(np.abs(h - a).max()), float(np.abs(b - a).max())
            ratio = e_hip / max(e_32, 2.0 ** -24 * float(np.abs(a).max()))
            worst = max(worst, ratio)
            assert ratio <= BAR, (e_hip, e_32)
    RATIOS["rollout"] = worst


def test_report_ratios():
    print("policy gate ratios:", {k: round(v, 2) for k, v in RATIOS.items()})
