"""The recurrent update on the CPU (hns_amd.rnn_train, learner.RecurrentDeviceLearner).  The device kernels:
tests/test_hip_rnn_train.py, tests/test_hip_rnn_learner.py.

  * the head restatements (`actor_head`, `critic_head`: the kernels' statements with their hand-derived dy) in fp64 against fp64 autograd of the
    reference's statements (tests/rnn_update_reference.py), to 1e-10 of the largest entry, every row compared;
  * `update_*_rnn`'s gradient-only forms in fp32 against the helper's independent flow (nn.GRUCell loop, LayerNorm(h + x), torch head,
    .backward()): e <= 8 max(e_32, 2^-24 max|ref_64|) per gradient tensor and scalar;
  * `RecurrentDeviceLearner` over a collected rollout: one train_rollout equals the same blocks driven by hand bit for bit; the segment
    permutation; the refusals; the checkpoint round trip;
  * the ABI's new entries."""
import copy
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import rnn_update_reference as U
from hns_amd import abi, collector, gae, learner, rnn_train, tp_train
from hns_amd import policy as P
from hns_amd import rnn as RN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hns_rnn_actor_head_workspace_bytes", "hns_rnn_critic_head_workspace_bytes", "hns_rnn_actor_head_grad", "hns_rnn_critic_head_grad")
SHAPES = [(1, 1, 1), (2, 16, 3), (3, 5, 2), (1, 64, 7)]
TOL = 1e-10


def _example():
    spec = importlib.util.spec_from_file_location("recurrent_policy_example", os.path.join(ROOT, "examples", "recurrent_policy.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _close(tag, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), tag     # (one row: the unbiased variance of one return is NaN on both sides)
    if np.isnan(want).all():
        return
    top = np.abs(want).max()
    assert np.abs(got - want).max() <= TOL * max(top, 1e-300), f"{tag}: {np.abs(got - want).max():.3e} of {top:.3e}"


def _head_restatements(c, **kw):
    t = lambda k: torch.as_tensor(c[k]).double()                # noqa: E731
    a = rnn_train.actor_head(t("head_w"), t("head_b"), t("log_std"), t("y"), t("action"), t("log_probs_old"), t("advantages"), 0.1, 1e-3)
    v = rnn_train.critic_head(t("v_w"), t("v_b"), t("y"), t("b_values"), t("b_returns"), 0.1, kw.get("loss", "huber"), kw.get("huber_delta", 10.0))
    return a, v


def _check_heads(tag, c, tie=False, need=None, **kw):
    a64, c64 = U.actor_head_autograd(c, torch.float64), U.critic_head_autograd(c, torch.float64, **kw)
    U.assert_off_the_edges(a64, c64, tie=tie)
    if need is not None:
        inside = (a64["ratio"] >= 0.9) & (a64["ratio"] <= 1.1)
        assert inside.all() if need == "inside" else (~inside).all()
    a, v = _head_restatements(c, **kw)
    for k in ("dy", "d_head_w", "d_head_b", "d_log_std", "policy_loss", "entropy", "ess", "log_probs"):
        _close(f"{tag} actor {k}", a[k], a64[k])
    for k in ("dy", "d_head_w", "d_head_b", "value_loss", "explained_var", "values"):
        _close(f"{tag} critic {k}", v[k], c64[k])
    return a64, c64


@pytest.mark.parametrize("B,L,A", SHAPES)
def test_head_restatements_equal_fp64_autograd_of_the_references_statements(B, L, A):
    _check_heads(f"{B}x{L}x{A}", U.head_case(B, L, A, 10 * B + L + A))


@pytest.mark.parametrize("variant", ["inside", "outside", "orig", "clip", "tie", "mse"])
def test_head_restatements_at_the_clip_the_branches_and_the_tie(variant):
    bands = {"inside": ((0.0, 0.05),), "outside": ((0.15, 0.40),)}.get(variant, ((0.0, 0.05), (0.15, 0.40)))
    c = U.head_case(3, 5, 2, 77, bands=bands, branch=variant if variant in ("orig", "clip", "tie") else "orig")
    kw = {"loss": "mse"} if variant == "mse" else {}
    a64, c64 = _check_heads(variant, c, tie=variant == "tie", need=variant if variant in ("inside", "outside") else None, **kw)
    if variant == "orig":
        assert c64["l_orig"] > c64["l_clip"]
    if variant == "clip":
        assert c64["l_clip"] > c64["l_orig"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the update functions in fp32 against the independent flow
def _fields(net, actor):
    """{reference name: (group, field)} of rnn_train.network_parameters' three mappings."""
    names = dict(P.ACTOR_NAMES if actor else P.CRITIC_NAMES)
    out = {k: ("encoder" if f not in ("head_w", "head_b", "log_std") else "head", f) for k, f in names.items()}
    out.update({"rnn." + k: ("gru", f) for k, f in RN.NAMES.items()})
    return {k: v for k, v in out.items() if k in net}


@pytest.mark.parametrize("A,K,D", [(3, 5, 35), (1, 5, 20)])
@pytest.mark.parametrize("actor", [True, False])
def test_update_gradients_in_fp32_against_the_independent_flow(A, K, D, actor):
    N, T, L = 3, 8, 4
    a_net, c_net, obs, states, is_init = U.rollout_case(N, T, A, K, D, L, 900 + A)
    net = a_net if actor else c_net
    state = states["actor" if actor else "critic"]
    assert is_init[0, 0, 0] and is_init[N - 1, L // 2, 0] and np.abs(state).min() > 0
    rows = U.per_row_case(actor, N, T, A, 31, net, obs, state, is_init, L)
    seg = np.array([4, 0, 5, 2, 1], np.int64)                   # a permutation's part: the flagged segments 0 and 5 among them
    g64, s64 = U.flow(net, actor, obs, state, is_init, rows, seg, L, torch.float64)
    g32, s32 = U.flow(net, actor, obs, state, is_init, rows, seg, L, torch.float32)
    if actor:
        d = np.minimum(np.abs(s64["ratio"] - 0.9), np.abs(s64["ratio"] - 1.1))
        assert d.min() >= U.MARGIN and np.array_equal(s64["w"], s32["w"])
    else:
        assert float(s64["dist"]) >= U.MARGIN and abs(float(s64["l_orig"] - s64["l_clip"])) >= 1e-3 * float(s64["value_loss"])
    live = {k: torch.as_tensor(v).clone() for k, v in net.items()}
    t = lambda v: torch.as_tensor(v)                            # noqa: E731
    fn = rnn_train.policy_loss_and_grad_rnn if actor else rnn_train.value_loss_and_grad_rnn
    res = fn(live, t(obs["state_self"]), t(obs["state_others"]) if A > 1 else None, t(obs["cylinders"]), t(state), t(is_init), *(t(r) for r in rows),
             segment=t(seg), seq_len=L, **({"entropy_coef": 1e-3} if actor else {}))
    names = _fields(net, actor)
    assert set(names) == set(net)
    items = [(k, live[k].grad.numpy(), g64[k], g32[k]) for k in net]
    scal = (("policy_loss", res.policy_loss), ("entropy", res.entropy), ("ess", res.ess), ("log_probs", res.log_probs.squeeze(-1))) if actor else \
        (("value_loss", res.value_loss), ("explained_var", res.explained_var), ("values", res.values.squeeze(-1)))
    items += [(k, v.detach().numpy(), s64[k], s32[k]) for k, v in scal]
    items.append(("grad_norm", res.grad_norm.numpy(), s64["grad_norm"], s32["grad_norm"]))
    worst, bad = U.gate(f"{'actor' if actor else 'critic'}-a{A}k{K}d{D}", items)
    assert not bad, "; ".join(bad)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the learner over a collected rollout
CFG = {"ppo_epochs": 2, "num_minibatches": 2, "TP_epochs": 2, "use_TP_net": 1, "actor": {"rnn": {"train_seq_len": 4}}, "critic": {"rnn": {"train_seq_len": 4}}}


def _setup(seed=0, N=5, T=8, L=4):
    ex = _example()
    ex.SEQ = L
    torch.manual_seed(seed)
    env = ex.StandInEnv(N)
    actor, critic = ex.Network(env.D, env.A, True, 0), ex.Network(env.D, env.A, False, 1)
    pol = P.RecurrentDevicePolicy(actor.names(), critic.names(), seed=0)
    col = collector.DeviceCollector(env, pol, T, rnn_seq_len=L)
    return actor, critic, pol, col


def _with_tp(kw, N=5, T=8):
    """learner_kwargs() of the stand-in env's storage with the predictor's entries beside them."""
    return {**kw, "tp": U.predictor_rollout(N, T, 3, 17)}


def _snapshot(lrn):
    """Parameters of the three networks, the three Adam states, ValueNorm1."""
    out = [v.detach().clone() for v in (*lrn.actor.values(), *lrn.critic.values(), *tp_train.parameters(lrn.tp_net))]
    assert lrn.tp_opt.state_dict()["state"]
    for opt in (lrn.actor_opt, lrn.critic_opt, lrn.tp_opt):
        for st in opt.state_dict()["state"].values():
            out += [st["step"].clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
    vn = lrn.value_normalizer
    return out + [vn.running_mean.clone(), vn.running_mean_sq.clone(), vn.debiasing_term.clone()]


def _by_hand(lrn, kw, rk, gen):
    """train_rollout's blocks through the public calls."""
    L = rk["rnn_seq_len"]
    xs, xo, xc = kw["obs_self"], kw["obs_others"], kw["obs_cylinders"]
    N, T = kw["reward"].shape[:2]
    nv = lrn.policy.forward(*kw["next_obs_last"], critic_state=rk["last_critic_rnn_state"], is_init=rk["last_is_init"], value_only=True).value
    adv, ret, _, (am, asd) = gae.rollout_targets(kw["reward"], kw["done"].unsqueeze(-1), kw["state_value"], nv, lrn.gamma, lrn.gae_lambda,
                                                 value_normalizer=lrn.value_normalizer, normalize_advantages=True, return_moments=True)
    tp_loss = tp_train.update_tp(lrn.tp_net, *kw["tp"], U.FUTURE, 1, lrn.num_minibatches, lrn.tp_epochs, lrn.tp_opt, generator=gen)
    rows, perms = [], []
    for _ in range(lrn.ppo_epochs):
        perm = torch.randperm((N * (T // L) // lrn.num_minibatches) * lrn.num_minibatches, generator=gen).reshape(lrn.num_minibatches, -1)
        perms.append(perm)
        for idx in perm:
            sa = rnn_train.update_actor_rnn(lrn.actor, xs, xo, xc, rk["actor_rnn_state"], rk["is_init"], kw["action"], kw["log_probs"], adv, lrn.actor_opt,
                                            segment=idx, cfg=lrn.cfg)
            sc = rnn_train.update_critic_rnn(lrn.critic, xs, xo, xc, rk["critic_rnn_state"], rk["is_init"], kw["state_value"], ret, lrn.critic_opt,
                                             segment=idx, cfg=lrn.cfg)
            rows.append(torch.stack([(sa | sc)[k].reshape(()).float() for k in learner.COLUMNS]))
    table = torch.stack(rows)
    a = kw["action"].reshape(-1, 4).double()
    info = dict(zip(learner.COLUMNS, learner._mean_row(table)))
    info["action_norm"] = float(np.float32(a.square().sum(-1).sqrt().sum().item() / a.shape[0]))
    info["TP_loss"] = float(tp_loss)
    info["advantages_mean"], info["advantages_std"] = float(am), float(asd)
    info["value_running_mean"] = float(lrn.value_normalizer.running_mean.mean())
    return info, perms


def test_train_rollout_equals_the_hand_driven_blocks_bit_for_bit():
    runs = []
    for by_hand in (False, True):
        actor, critic, pol, col = _setup()
        gen = torch.Generator().manual_seed(5)
        lrn = learner.RecurrentDeviceLearner(actor.names(), critic.names(), CFG, tp_net=U.predictor(3, 41), value_normalizer=learner.ValueNorm1(), generator=gen, device_policy=pol)
        assert lrn.train_seq_len == 4 and lrn.actor_opt is not lrn.critic_opt
        st = col.collect()
        kw, rk = _with_tp(st.learner_kwargs()), st.recurrent_kwargs()
        before = pol.forward(*kw["next_obs_last"], critic_state=rk["last_critic_rnn_state"], is_init=rk["last_is_init"], value_only=True).value.clone()
        if by_hand:
            info, perms = _by_hand(lrn, kw, rk, gen)
            info = {f"drone/{k}": v for k, v in info.items()}
            # the permutation: randperm((N S // M) M).reshape(M, -1) from an equally seeded generator; 10 segments, 2 minibatches of 5 —
            # drawn BEHIND the predictor's epochs (one stream serves the call): 5 envs x (8 - 5) selected windows, 2 minibatches of 7
            want = torch.Generator().manual_seed(5)
            for _ in range(lrn.tp_epochs):
                tp_train.minibatches(5 * (8 - U.FUTURE), 2, torch.device("cpu"), want)
            for p in perms:
                assert torch.equal(p, torch.randperm(10, generator=want).reshape(2, -1))
        else:
            info = lrn.train_rollout(**kw, **rk)
            assert tuple(k.split("/")[1] for k in info) == learner.INFO_KEYS
            after = pol.forward(*kw["next_obs_last"], critic_state=rk["last_critic_rnn_state"], is_init=rk["last_is_init"], value_only=True).value
            assert not torch.equal(before, after)               # the policy's next forward reflects the stepped parameters
        runs.append((info, _snapshot(lrn)))
    (i0, s0), (i1, s1) = runs
    assert set(i0) == set(i1)
    for k in i0:
        assert np.float32(i0[k]) == np.float32(i1[k]), (k, i0[k], i1[k])
    assert len(s0) == len(s1) and all(torch.equal(a, b) for a, b in zip(s0, s1))


def test_refusals():
    actor, critic, pol, col = _setup()
    a, c = actor.names(), critic.names()
    with pytest.raises(NotImplementedError, match="group"):
        learner.RecurrentDeviceLearner(a, c, CFG, group="world")
    with pytest.raises(P.PolicyConfigError):                    # DeviceLearner still refuses a recurrent policy
        learner.DeviceLearner(a, c, None, device_policy=pol)
    with pytest.raises(P.PolicyConfigError):
        learner.RecurrentDeviceLearner(a, c, {**CFG, "share_actor": False})
    with pytest.raises(P.PolicyConfigError):
        learner.RecurrentDeviceLearner(a, c, {**CFG, "actor": {"tanh": True, "rnn": {"train_seq_len": 4}}})
    plain = {k: v for k, v in a.items() if not k.startswith("rnn.")}
    with pytest.raises(P.PolicyConfigError, match="GRU"):
        learner.RecurrentDeviceLearner(plain, c, CFG)
    lrn = learner.RecurrentDeviceLearner(a, c, {**CFG, "actor": {"rnn": {"train_seq_len": 3}}}, device_policy=pol)
    st = col.collect()
    kw, rk = _with_tp(st.learner_kwargs()), st.recurrent_kwargs()
    with pytest.raises(ValueError, match="train_seq_len"):       # stored in segments of 4
        lrn.train_rollout(**kw, **rk)
    with pytest.raises(ValueError, match="divide"):
        lrn.train_rollout(**kw, **{**rk, "rnn_seq_len": None})   # 3 does not divide 8
    with pytest.raises(ValueError, match="recurrent_kwargs"):
        learner.RecurrentDeviceLearner(a, c, CFG, device_policy=pol).train_rollout(**kw)
    with pytest.raises(TypeError, match="ClippedAdam"):
        rnn_train.update_actor_rnn(a, kw["obs_self"], kw["obs_others"], kw["obs_cylinders"], rk["actor_rnn_state"], rk["is_init"], kw["action"],
                                   kw["log_probs"], kw["state_value"], torch.optim.Adam(list(a.values())))
    with pytest.raises(IndexError):
        rnn_train.policy_loss_and_grad_rnn(a, kw["obs_self"], kw["obs_others"], kw["obs_cylinders"], rk["actor_rnn_state"], rk["is_init"], kw["action"],
                                           kw["log_probs"], kw["state_value"], segment=torch.tensor([0, 10]), seq_len=4)


def test_state_dict_round_trips_into_a_fresh_learner_that_takes_an_identical_step():
    actor, critic, pol, col = _setup()
    lrn = learner.RecurrentDeviceLearner(actor.names(), critic.names(), CFG, tp_net=U.predictor(3, 41), value_normalizer=learner.ValueNorm1(),
                                         generator=torch.Generator().manual_seed(1), device_policy=pol)
    st = col.collect()
    kw, rk = _with_tp(st.learner_kwargs()), st.recurrent_kwargs()
    lrn.train_rollout(**kw, **rk)
    sd = lrn.state_dict()
    assert any(k.startswith("rnn.") for k in sd["actor_params"]) and any(k.startswith("rnn.") for k in sd["critic"])
    assert set(sd) == {"TP", "critic", "actor_params", "value_normalizer", "actor_opt", "critic_opt", "TP_opt"} and sd["TP_opt"]["state"]
    sd = copy.deepcopy(sd)                                      # (state_dict() hands out the live tensors, the optimisers' included)
    actor2, critic2, pol2, _ = _setup(seed=9)
    fresh = learner.RecurrentDeviceLearner(actor2.names(), critic2.names(), CFG, tp_net=U.predictor(3, 99), value_normalizer=learner.ValueNorm1(),
                                           device_policy=pol2)
    assert not torch.equal(fresh.tp_net.fc.weight, lrn.tp_net.fc.weight)
    fresh.load_state_dict(sd)
    lrn.generator, fresh.generator = torch.Generator().manual_seed(2), torch.Generator().manual_seed(2)
    i0, i1 = lrn.train_rollout(**kw, **rk), fresh.train_rollout(**kw, **rk)
    assert i0 == i1
    assert all(torch.equal(a, b) for a, b in zip(_snapshot(lrn), _snapshot(fresh)))


def test_train_op_reads_the_references_keys():
    from hns_amd.tensordict_shim import TensorDict
    actor, critic, pol, col = _setup()
    mk = lambda: learner.RecurrentDeviceLearner(actor.names(), critic.names(), CFG, tp_net=U.predictor(3, 41), value_normalizer=learner.ValueNorm1(),   # noqa: E731
                                                generator=torch.Generator().manual_seed(3), device_policy=pol)
    st = col.collect()
    kw, rk = _with_tp(st.learner_kwargs()), st.recurrent_kwargs()
    N, T, L = 5, 8, 4
    obs = {"state_self": kw["obs_self"], "state_others": kw["obs_others"], "cylinders": kw["obs_cylinders"]}
    pad = lambda s: s.repeat_interleave(L, dim=1)               # noqa: E731  (the state going into a segment, at every step of it)
    nxt_obs = {k: torch.cat([v[:, 1:], last.unsqueeze(1)], 1) for (k, v), last in zip(obs.items(), kw["next_obs_last"])}
    tp = dict(zip(("TP_input", "TP_groundtruth", "TP_done"), kw["tp"]))
    nxt = TensorDict({"agents": {"observation": nxt_obs, "reward": kw["reward"], "TP": tp}, "done": kw["done"],
                      "drone.critic_rnn_state": rk["last_critic_rnn_state"].unsqueeze(1).expand(N, T, 3, 128),
                      "is_init": rk["last_is_init"].unsqueeze(1).expand(N, T, 1)}, [N, T])
    td = TensorDict({"agents": {"observation": obs, "action": kw["action"]}, "drone.action_logp": kw["log_probs"], "state_value": kw["state_value"],
                     "is_init": rk["is_init"], "drone.actor_rnn_state": pad(rk["actor_rnn_state"]), "drone.critic_rnn_state": pad(rk["critic_rnn_state"]),
                     "next": nxt}, [N, T])
    sd = {k: v.detach().clone() for k, v in {**actor.names(), **{"c." + k: v for k, v in critic.names().items()}}.items()}
    i0 = mk().train_op(td)
    with torch.no_grad():
        for k, v in {**actor.names(), **{"c." + k: v for k, v in critic.names().items()}}.items():
            v.copy_(sd[k])
    i1 = mk().train_rollout(**kw, **rk)
    assert i0 == i1


# ---------------------------------------------------------------------------------------------------------------------------------------
# the ABI
def test_library_exports_and_declares_the_new_entries():
    lib = ctypes.CDLL(abi.library_path())
    for sym in NEW:
        getattr(lib, sym)
        assert sym in abi.EXPORTED_SYMBOLS
    lib = abi.load_library()
    assert lib.hns_abi_version() == 8                           # purely additive
    assert len(lib.hns_rnn_actor_head_grad.argtypes) == 20 and len(lib.hns_rnn_critic_head_grad.argtypes) == 17
    assert ctypes.sizeof(abi.HnsRnnRows) == 72 and abi.HnsRnnRows.segment.offset == 56 and abi.HnsRnnRows.steps.offset == 48
    header = open(os.path.join(ROOT, "include", "hns.h")).read()
    body = header[header.index("typedef struct hns_rnn_rows {"):header.index("} hns_rnn_rows;")]
    assert [ln.split(";")[0].split()[-1].lstrip("*").split("[")[0] for ln in body.splitlines()[1:] if ";" in ln] == \
        ["y", "y_stride", "inner", "steps", "segment", "num_segments"]                       # (outer, inner share a line)
    for fn in (lib.hns_rnn_actor_head_workspace_bytes, lib.hns_rnn_critic_head_workspace_bytes):
        assert fn.restype is ctypes.c_size_t
        n = fn(512, 3, 16)
        assert n % 256 == 0 and n >= 512 * 3 * 16 * 4 and fn(1024, 3, 16) > n
        for shape in ((0, 3, 16), (1, 0, 16), (1, 8, 16), (1, 3, 0), (1, 3, 65), (2 ** 40, 3, 16)):
            assert fn(*shape) == 0, shape
