"""The MAPPO policy's forward pass (hns_amd.policy), CPU side: the restatements against the reference's own networks (g_policy.npz, written by
tests/golden/make_golden_policy.py), parameter parsing from live objects and checkpoints, refusals (every refusal branch of hns_policy_forward
and hns_policy_pack, and DevicePolicy.forward's own checks), the library's new symbols, and the proof that the fp64 gate of test_hip_policy.py
has teeth: an fp32 emulation of the kernel's algorithm (policy_reference.emulate_kernel) passes it on every committed case, and each of eight
seeded defects fails it on a named one."""
import ctypes
import os

import numpy as np
import pytest
import torch

import policy_reference as R
from hns_amd import abi
from hns_amd import policy as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["a3k5d35", "a3k8d20", "a1k5d20", "a6k16d24"]


@pytest.fixture(scope="module")
def gp():
    return np.load(os.path.join(ROOT, "tests", "golden", "g_policy.npz"))


def _obs_t(obs):
    return (torch.from_numpy(obs["state_self"]), torch.from_numpy(obs["state_others"]) if "state_others" in obs else None,
            torch.from_numpy(obs["cylinders"]))


@pytest.mark.parametrize("tag", CASES)
def test_restatements_match_the_reference_networks(gp, tag):
    actor, critic, obs, eps, exp = R.golden_case(gp, tag)
    for dtype in (torch.float32, torch.float64):
        loc, _, action, logp, value = R.forward(actor, critic, obs, eps, dtype=dtype)
        for name, got in (("loc", loc), ("action", action), ("log_prob", logp), ("value", value)):
            np.testing.assert_allclose(got.double().numpy(), exp[name], atol=1e-5, rtol=1e-5, err_msg=f"{tag} {name} {dtype}")
    # the product's CPU path (torch statements, F.multi_head_attention_forward)
    pol = P.DevicePolicy({k: torch.from_numpy(v) for k, v in actor.items()}, {k: torch.from_numpy(v) for k, v in critic.items()})
    out = pol.forward(*_obs_t(obs), eps=torch.from_numpy(eps))
    for name in ("loc", "action", "log_prob", "value"):
        np.testing.assert_allclose(getattr(out, name).numpy(), exp[name], atol=1e-5, rtol=1e-5, err_msg=f"{tag} {name} (policy.py)")
    det = pol.forward(*_obs_t(obs), deterministic=True)
    np.testing.assert_allclose(det.action.numpy(), exp["mode"], atol=1e-5, rtol=1e-5)
    assert torch.equal(det.action, det.loc)
    np.testing.assert_allclose(pol.forward(*_obs_t(obs), value_only=True).value.numpy(), exp["value"], atol=1e-5, rtol=1e-5)


class FakeTD:
    """TensorDictParams-like: nested keys, flatten_keys(sep) and items()."""

    def __init__(self, flat):
        self.flat = flat

    def flatten_keys(self, sep="."):
        return dict(self.flat)

    def items(self):
        return self.flat.items()


def _golden_params(gp, tag):
    actor, critic, _, _, _ = R.golden_case(gp, tag)
    return {k: torch.from_numpy(v.copy()) for k, v in actor.items()}, {k: torch.from_numpy(v.copy()) for k, v in critic.items()}


def test_names_with_and_without_the_module_prefix(gp):
    actor, critic = _golden_params(gp, "a3k5d35")
    plain = P.DevicePolicy(actor, critic)
    pref = P.DevicePolicy(FakeTD({"module." + k: v for k, v in actor.items()}), {"module." + k: v for k, v in critic.items()})
    assert pref.self_dim == plain.self_dim == 35
    for f in plain.actor_p:
        assert pref.actor_p[f] is plain.actor_p[f]
    # a nested mapping (TensorDict keys as tuples / sub-dicts)
    nested = {"module": {}}
    for k, v in actor.items():
        d = nested["module"]
        parts = k.split(".")
        for p in parts[:-1]:
            d = d.setdefault(p, {})
        d[parts[-1]] = v
    assert set(P.DevicePolicy(nested, critic).actor_p) == set(plain.actor_p)


def test_live_modules_and_checkpoints(gp, tmp_path):
    actor, critic = _golden_params(gp, "a3k8d20")

    class Holder(torch.nn.Module):                     # an nn.Module whose named_parameters carry the reference's names under module.
        def __init__(self, params):
            super().__init__()
            self.module = torch.nn.Module()
            for k, v in params.items():
                mod = self.module
                parts = k.split(".")
                for p in parts[:-1]:
                    if not hasattr(mod, p):
                        mod.add_module(p, torch.nn.Module())
                    mod = getattr(mod, p)
                mod.register_parameter(parts[-1], torch.nn.Parameter(v.clone()))

    crit = Holder(critic)
    pol = P.DevicePolicy(FakeTD(actor), crit)
    assert pol.critic_p["head_w"] is crit.module.v_out.weight
    ckpt = {"actor_params": {"module." + k: v for k, v in actor.items()}, "critic": crit.state_dict(), "TP": {}, "value_normalizer": {}}
    path = tmp_path / "checkpoint_final.pt"
    torch.save(ckpt, path)
    for src in (ckpt, str(path)):
        p2 = P.DevicePolicy.from_checkpoint(src)
        assert torch.equal(p2.critic_p["head_w"], crit.module.v_out.weight.detach())
    with pytest.raises(KeyError):
        P.DevicePolicy.from_checkpoint({"TP": {}})


def test_unsupported_configurations_are_refused(gp):
    actor, critic = _golden_params(gp, "a3k5d35")
    for cfg, what in (({"share_actor": False}, "share_actor"), ({"critic_input": "state"}, "critic_input"),
                      ({"actor": {"rnn": {"cls": "gru"}}}, "rnn"), ({"critic": {"rnn": {"cls": "gru"}}}, "rnn"), ({"actor": {"tanh": True}}, "tanh")):
        with pytest.raises(P.PolicyConfigError, match=what):
            P.DevicePolicy(actor, critic, cfg=cfg)
    P.DevicePolicy(actor, critic, cfg={"share_actor": True, "critic_input": "obs", "actor": {"tanh": False}, "critic": {}})
    # the same things seen in the parameters themselves
    stacked = {k: v.expand(3, *v.shape) for k, v in actor.items()}
    with pytest.raises(P.PolicyConfigError, match="share_actor"):
        P.DevicePolicy(stacked, critic)
    with pytest.raises(P.PolicyConfigError, match="rnn"):
        P.DevicePolicy({**actor, "rnn.gru.weight_ih": torch.zeros(3, 128)}, critic)
    central = {k.replace("state_self", "state_drones"): v for k, v in critic.items()}
    with pytest.raises(P.PolicyConfigError):
        P.DevicePolicy(actor, central)
    tanh_actor = {k.replace("act_dist.fc_mean", "act_dist.operator"): v for k, v in actor.items()}
    with pytest.raises(P.PolicyConfigError):
        P.DevicePolicy(tanh_actor, critic)
    wide = dict(actor)
    wide["encoder.linear1.weight"] = torch.zeros(256, 128)
    with pytest.raises(P.PolicyConfigError, match="128"):
        P.DevicePolicy(wide, critic)
    big_head = dict(critic)
    big_head["v_out.weight"] = torch.zeros(2, 128)
    with pytest.raises(P.PolicyConfigError, match="head"):
        P.DevicePolicy(actor, big_head)
    with pytest.raises(P.PolicyConfigError, match="missing"):
        P.DevicePolicy({k: v for k, v in actor.items() if "log_std" not in k}, critic)


def test_observation_shapes_are_checked(gp):
    actor, critic, obs, _, _ = R.golden_case(gp, "a3k5d35")
    pol = P.DevicePolicy({k: torch.from_numpy(v) for k, v in actor.items()}, {k: torch.from_numpy(v) for k, v in critic.items()})
    xs, xo, xc = _obs_t(obs)
    with pytest.raises(ValueError):
        pol.forward(xs[..., :20], xo, xc)
    with pytest.raises(ValueError):
        pol.forward(xs, None, xc)
    with pytest.raises(ValueError):
        pol.forward(xs, xo, xc[..., :4])


def test_new_symbols_are_exported_and_refuse_bad_arguments():
    import __graft_entry__ as g
    lib = ctypes.CDLL(g.build())
    for sym in ("hns_policy_packed_bytes", "hns_policy_pack", "hns_policy_forward"):
        assert sym in abi.EXPORTED_SYMBOLS
        assert hasattr(lib, sym)
    L = abi.load_library()
    per_net = lambda D: 6 * 128 * 128 + 18 * 128 + 12 + (D + 8) * 128
    assert L.hns_policy_packed_bytes(35) == 2 * per_net(35) * 4
    assert L.hns_policy_packed_bytes(0) == 0 and L.hns_policy_packed_bytes(97) == 0
    io = abi.HnsPolicyIo()
    fake = ctypes.c_void_p(1 << 20)
    assert L.hns_policy_forward(fake, 35, 4, 8, 5, ctypes.byref(io), 0, 0, None, None) == abi.HNS_ERR_INVALID_ARG
    assert b"num_agents" in L.hns_last_error()
    assert L.hns_policy_forward(fake, 35, 4, 3, 17, ctypes.byref(io), 0, 0, None, None) == abi.HNS_ERR_INVALID_ARG
    assert b"num_cylinders" in L.hns_last_error()
    assert L.hns_policy_forward(fake, 120, 4, 3, 5, ctypes.byref(io), 0, 0, None, None) == abi.HNS_ERR_INVALID_ARG
    assert b"self_dim" in L.hns_last_error()
    net = abi.HnsPolicyNet()
    assert L.hns_policy_pack(ctypes.byref(net), ctypes.byref(net), 35, 3, fake, None) == abi.HNS_ERR_INVALID_ARG
    assert b"non-NULL" in L.hns_last_error()


def test_the_entry_table_of_the_four_classes_names_the_eight_exported_entries():
    """For every (per_agent, recurrent, act) the class's entry is a symbol of the loaded library, and the four classes together name exactly
    the eight forward / act entries that include/hns.h declares."""
    import re
    with open(os.path.join(ROOT, "include", "hns.h")) as f:
        declared = set(re.findall(r"^int (hns_policy_(?:forward|act)\w*)\(", f.read(), re.M))
    assert len(declared) == 8
    lib = abi.load_library()
    classes = [P.DevicePolicy, P.PerAgentDevicePolicy, P.RecurrentDevicePolicy, P.PerAgentRecurrentDevicePolicy]
    assert sorted((c.per_agent, c.recurrent) for c in classes) == [(False, False), (False, True), (True, False), (True, True)]
    named = set()
    for c in classes:
        for act in (False, True):
            sym = P.ENTRIES[c.per_agent, c.recurrent, act]
            assert sym in abi.EXPORTED_SYMBOLS and getattr(lib, sym).argtypes, sym       # exported, and its arguments declared in abi.py
            assert ("_agents" in sym, "_rnn" in sym, "_act" in sym) == (c.per_agent, c.recurrent, act), sym
            named.add(sym)
    assert named == declared == set(P.ENTRIES.values())


FAKE = 1 << 20                                   # a made-up, 16-byte aligned address: every call below is refused by argument checking alone
DET, VAL = abi.HNS_POLICY_DETERMINISTIC, abi.HNS_POLICY_VALUE_ONLY


def _io(**kw):
    """An hns_policy_io that passes every check (made-up aligned pointers, contiguous strides of A = 3, K = 5, D = 35), then `kw` on top."""
    io = abi.HnsPolicyIo()
    io.obs_self, io.obs_others, io.obs_cylinders = FAKE, FAKE + 4096, FAKE + 8192
    io.self_stride[:], io.others_stride[:], io.cyl_stride[:] = [105, 35], [18, 6, 3], [75, 25, 5]
    io.eps, io.action, io.loc, io.log_prob, io.value = FAKE + 12288, FAKE + 16384, FAKE + 20480, FAKE + 24576, FAKE + 28672
    for k, v in kw.items():
        if isinstance(v, tuple):                 # (index, value): one entry of a stride array
            getattr(io, k)[v[0]] = v[1]
        else:
            setattr(io, k, v)
    return io


# (what, message fragment, keyword arguments of the call, fields of the io set on top of a valid one): ONE thing wrong per row
FORWARD_REFUSALS = [
    ("null image", b"null or misaligned packed image", dict(packed=None), {}),
    ("image 8 bytes off 16-byte alignment", b"null or misaligned packed image", dict(packed=FAKE + 8), {}),
    ("null io", b"null or misaligned packed image", dict(io=None), {}),
    ("self_dim 0", b"self_dim must be in [1, 96]", dict(D=0), {}),
    ("self_dim 97", b"self_dim must be in [1, 96]", dict(D=97), {}),
    ("num_agents 0", b"num_agents must be in [1, 7]", dict(A=0), {}),
    ("num_agents 8", b"num_agents must be in [1, 7]", dict(A=8), {}),
    ("num_cylinders 0", b"num_cylinders must be in [1, 16]", dict(K=0), {}),
    ("num_cylinders 17", b"num_cylinders must be in [1, 16]", dict(K=17), {}),
    ("num_envs 0", b"num_envs must be in [1, 2^31 / 7]", dict(E=0), {}),
    ("num_envs negative", b"num_envs must be in [1, 2^31 / 7]", dict(E=-1), {}),
    ("num_envs 2^31 / 7 + 1", b"num_envs must be in [1, 2^31 / 7]", dict(E=(1 << 31) // 7 + 1), {}),
    ("unknown flag bit", b"unknown flag", dict(flags=4), {}),
    ("unknown flag bit beside known ones", b"unknown flag", dict(flags=DET | VAL | 8), {}),
    ("obs_self missing", b"observation pointer missing", {}, dict(obs_self=None)),
    ("obs_cylinders missing", b"observation pointer missing", {}, dict(obs_cylinders=None)),
    ("obs_others missing with A = 3", b"observation pointer missing", {}, dict(obs_others=None)),
    ("obs_others missing with A = 2", b"observation pointer missing", dict(A=2), dict(obs_others=None)),
    ("obs_self 2 bytes off", b"misaligned observation", {}, dict(obs_self=FAKE + 2)),
    ("obs_others 2 bytes off", b"misaligned observation", {}, dict(obs_others=FAKE + 4098)),
    ("obs_others 2 bytes off with A = 1", b"misaligned observation", dict(A=1), dict(obs_others=FAKE + 4098)),
    ("obs_cylinders 2 bytes off", b"misaligned observation", {}, dict(obs_cylinders=FAKE + 8194)),
    ("self_stride[0] < 0", b"negative stride", {}, dict(self_stride=(0, -105))),
    ("self_stride[1] < 0", b"negative stride", {}, dict(self_stride=(1, -1))),
    ("others_stride[0] < 0", b"negative stride", {}, dict(others_stride=(0, -18))),
    ("others_stride[1] < 0", b"negative stride", {}, dict(others_stride=(1, -6))),
    ("others_stride[2] < 0", b"negative stride", {}, dict(others_stride=(2, -3))),
    ("cyl_stride[0] < 0", b"negative stride", {}, dict(cyl_stride=(0, -75))),
    ("cyl_stride[1] < 0", b"negative stride", {}, dict(cyl_stride=(1, -25))),
    ("cyl_stride[2] < 0", b"negative stride", {}, dict(cyl_stride=(2, -5))),
    ("value missing", b"value output missing or misaligned", {}, dict(value=None)),
    ("value missing, value only", b"value output missing or misaligned", dict(flags=VAL), dict(value=None)),
    ("value 2 bytes off", b"value output missing or misaligned", {}, dict(value=FAKE + 28674)),
    ("action missing", b"action / log_prob outputs missing or misaligned", {}, dict(action=None)),
    ("log_prob missing", b"action / log_prob outputs missing or misaligned", {}, dict(log_prob=None)),
    ("action missing, deterministic", b"action / log_prob outputs missing or misaligned", dict(flags=DET), dict(action=None)),
    ("action 2 bytes off", b"action / log_prob outputs missing or misaligned", {}, dict(action=FAKE + 16386)),
    ("log_prob 2 bytes off", b"action / log_prob outputs missing or misaligned", {}, dict(log_prob=FAKE + 24578)),
    ("loc 2 bytes off", b"action / log_prob outputs missing or misaligned", {}, dict(loc=FAKE + 20482)),
    ("sampling without eps and without a counter", b"sampling without eps needs the device call counter", dict(counter=None), dict(eps=None)),
    ("sampling without eps, counter 4 bytes off 8-byte alignment", b"sampling without eps needs the device call counter",
     dict(counter=FAKE + 32772), dict(eps=None)),
    ("eps 2 bytes off", b"misaligned eps", {}, dict(eps=FAKE + 12290)),
    ("eps 2 bytes off, no counter", b"misaligned eps", dict(counter=None), dict(eps=FAKE + 12290)),
]


@pytest.mark.parametrize("row", FORWARD_REFUSALS, ids=[r[0].replace(" ", "_") for r in FORWARD_REFUSALS])
def test_every_refusal_branch_of_hns_policy_forward(row):
    """Each refusal of hns_policy_forward, one wrong argument at a time on an otherwise valid call.  The refusals return before any launch and
    do not depend on the machine: every pointer here is made up, so a row that were NOT refused must never be committed."""
    _, fragment, call, fields = row
    L = abi.load_library()
    a = dict(packed=FAKE + 65536, D=35, E=4, A=3, K=5, io=_io(**fields), flags=0, seed=7, counter=FAKE + 32768)
    a.update(call)
    io = ctypes.byref(a["io"]) if a["io"] is not None else None
    rc = L.hns_policy_forward(a["packed"], a["D"], a["E"], a["A"], a["K"], io, a["flags"], a["seed"], a["counter"], None)
    assert rc == abi.HNS_ERR_INVALID_ARG
    err = L.hns_last_error()
    assert err.startswith(b"hns_policy_forward: ") and fragment in err, err


def _net(**kw):
    n = abi.HnsPolicyNet()
    for i, f in enumerate(abi.POLICY_NET_FIELDS):
        setattr(n, f, FAKE + 4096 * i)
    for k, v in kw.items():
        setattr(n, k, v)
    return n


# (what, message fragment, keyword arguments of the call, fields of the ACTOR set on top of a valid one, likewise the CRITIC)
PACK_REFUSALS = [
    ("self_dim 0", b"self_dim must be in [1, 96]", dict(D=0), {}, {}),
    ("self_dim 97", b"self_dim must be in [1, 96]", dict(D=97), {}, {}),
    ("num_agents 0", b"num_agents must be in [1, 7]", dict(A=0), {}, {}),
    ("num_agents 8", b"num_agents must be in [1, 7]", dict(A=8), {}, {}),
    ("null image", b"packed image must be a 16-byte aligned device array", dict(packed=None), {}, {}),
    ("image 8 bytes off", b"packed image must be a 16-byte aligned device array", dict(packed=FAKE + 8), {}, {}),
    ("null actor", b"null network", dict(actor=None), {}, {}),
    ("null critic", b"null network", dict(critic=None), {}, {}),
    ("actor parameter missing", b"every parameter pointer must be a non-NULL fp32 array", {}, dict(norm2_b=None), {}),
    ("actor parameter 2 bytes off", b"every parameter pointer must be a non-NULL fp32 array", {}, dict(in_proj_w=FAKE + 2), {}),
    ("critic head missing", b"every parameter pointer must be a non-NULL fp32 array", {}, {}, dict(head_w=None)),
    ("actor others weight missing with A = 2", b"state_others embedding missing", dict(A=2), dict(embed_others_w=None), {}),
    ("actor others bias missing with A = 7", b"state_others embedding missing", dict(A=7), dict(embed_others_b=None), {}),
    ("critic others weight missing with A = 3", b"state_others embedding missing", {}, {}, dict(embed_others_w=None)),
    ("actor without log_std", b"the actor needs log_std", {}, dict(log_std=None), {}),
    ("actor without log_std, A = 1", b"the actor needs log_std", dict(A=1), dict(log_std=None, embed_others_w=None, embed_others_b=None), {}),
]


@pytest.mark.parametrize("row", PACK_REFUSALS, ids=[r[0].replace(" ", "_") for r in PACK_REFUSALS])
def test_every_refusal_branch_of_hns_policy_pack(row):
    """Each refusal of hns_policy_pack and of its per-network check, on made-up pointers (refused before the launch)."""
    _, fragment, call, actor, critic = row
    L = abi.load_library()
    a = dict(actor=_net(**actor), critic=_net(**critic), D=35, A=3, packed=FAKE + (1 << 19))
    a.update(call)
    ref = lambda n: ctypes.byref(n) if n is not None else None
    rc = L.hns_policy_pack(ref(a["actor"]), ref(a["critic"]), a["D"], a["A"], a["packed"], None)
    assert rc == abi.HNS_ERR_INVALID_ARG
    err = L.hns_last_error()
    assert err.startswith(b"hns_policy_pack: ") and fragment in err, err


def test_device_policy_forward_refuses_bad_shapes_on_the_cpu_path(gp):
    """DevicePolicy.forward's own checks run before the device is looked at: wrong eps, a state_self with two tokens, 17 cylinders,
    state_others with one agent."""
    actor, critic, obs, eps, _ = R.golden_case(gp, "a3k5d35")
    t = lambda p: {k: torch.from_numpy(v) for k, v in p.items()}
    pol = P.DevicePolicy(t(actor), t(critic))
    xs, xo, xc = _obs_t(obs)
    E, A = xs.shape[:2]
    e = torch.from_numpy(eps)
    pol.forward(xs, xo, xc, eps=e)
    pol.forward(xs.squeeze(2), xo, xc, eps=e)                   # [E, A, D] is the other accepted form
    for bad in (e[:, :, :3], e[:-1], e.reshape(E * A, 4), e.unsqueeze(-1), e.double(), e.to(torch.float16)):
        with pytest.raises(ValueError, match="eps must be float32"):
            pol.forward(xs, xo, xc, eps=bad)
    with pytest.raises(ValueError, match=r"state_self must be \[E, A, D\] or \[E, A, 1, D\]"):
        pol.forward(xs.expand(E, A, 2, xs.shape[-1]), xo, xc)
    with pytest.raises(ValueError, match="cylinders must be"):
        pol.forward(xs, xo, torch.zeros(E, A, 17, 5))
    with pytest.raises(ValueError, match="cylinders must be"):
        pol.forward(xs, xo, torch.zeros(E, A, 0, 5))
    with pytest.raises(ValueError, match="state_others is absent"):          # this network has the state_others key: one agent cannot feed it
        pol.forward(xs[:, :1], torch.zeros(E, 1, 0, 3), xc[:, :1])
    with pytest.raises(ValueError, match="state_others must be"):
        pol.forward(xs, xo[:, :, :1], xc)
    with pytest.raises(TypeError, match="float32"):
        pol.forward(xs.double(), xo, xc)
    actor1, critic1, obs1, _, _ = R.golden_case(gp, "a1k5d20")
    pol1 = P.DevicePolicy(t(actor1), t(critic1))
    xs1, _, xc1 = _obs_t(obs1)
    pol1.forward(xs1, None, xc1)
    with pytest.raises(ValueError, match="state_others is absent"):          # ... and a one-agent network takes none
        pol1.forward(xs1, torch.zeros(xs1.shape[0], 1, 0, 3), xc1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Does the fp64 gate have teeth?  emulate_kernel is an fp32 restatement of the kernel's algorithm; the cases are the ones the GPU gate runs.
GATE_CASES = CASES + list(R.EDGES) + [R.limit_tag(s) for s in R.LIMIT_SHAPES] + ["log_std"]


@pytest.fixture(scope="module")
def gate_cases(gp):
    """tag -> (case, fp64 outputs, fp32 outputs) of every committed case of the GPU gate."""
    cases = {tag: R.golden_case(gp, tag)[:4] for tag in CASES}
    cases.update({m: R.edge_case(m) for m in R.EDGES})
    cases.update({R.limit_tag(s): R.limit_case(s) for s in R.LIMIT_SHAPES})
    cases["log_std"] = R.log_std_case()
    assert list(cases) == GATE_CASES
    return {k: (v, R.reference_outputs(*v, torch.float64), R.reference_outputs(*v, torch.float32)) for k, v in cases.items()}


def test_the_kernels_algorithm_in_fp32_passes_the_gate_on_every_committed_case(gate_cases):
    """No defect: the emulation stays under the bar on the golden cases, the three edges, every shape limit and the per-component log_std
    case, sampling (eps supplied) and at the mode (eps None: the log-probability at the mode).  Measured worst ratio 1.38."""
    worst = 0.0
    for tag, (case, r64, r32) in gate_cases.items():
        ratios = R.gate_ratios(R.emulate_kernel(*case), r64, r32)
        a, c, obs, _ = case
        det = R.gate_ratios(R.emulate_kernel(a, c, obs, None), R.reference_outputs(a, c, obs, None, torch.float64),
                            R.reference_outputs(a, c, obs, None, torch.float32))
        for name in R.OUTPUTS:
            assert ratios[name] <= R.BAR and det[name] <= R.BAR, (tag, name, ratios, det)
        worst = max(worst, *ratios.values(), *det.values())
    print(f"  emulate_kernel, no defect: worst ratio {worst:.2f} of {R.BAR}")


# defect -> the committed case that must fail the gate with it, and the output it fails on.  Measured ratios (bar 8), named case / weakest
# failing case / cases that still pass:
#   softmax_rescale_omitted    a3k8d20 2.8e5 / flat_tokens 69 / none
#   layernorm_eps_0            flat_tokens 2.4e4 / large_obs 16 / none
#   score_scale_bf16           limit-a3k16d20e33 76 / a1k5d20 17 / flat_tokens, saturated_softmax (one-hot or uniform weights either way)
#   gelu_tanh                  a3k5d35 139 / limit-a3k5d1e33 83 / flat_tokens, saturated_softmax
#   value_bias_dropped         a6k16d24 7.0e4 / saturated_softmax 9.3 / none
#   last_cylinder_skipped      limit-a3k1d20e33 1.1e6 / flat_tokens 172 / none
#   others_with_cylinder_bias  limit-a2k5d20e40 1.2e6 / saturated_softmax 5.7e3 / the A = 1 cases (no such token), flat_tokens (equal biases)
#   log_std_of_component_0     log_std 2.9e7 / limit-a1k5d35e1 2.3e5 / none
DEFECT_TABLE = {
    "softmax_rescale_omitted": ("a3k8d20", "loc"),
    "layernorm_eps_0": ("flat_tokens", "loc"),
    "score_scale_bf16": ("limit-a3k16d20e33", "loc"),
    "gelu_tanh": ("a3k5d35", "loc"),
    "value_bias_dropped": ("a6k16d24", "value"),
    "last_cylinder_skipped": ("limit-a3k1d20e33", "value"),
    "others_with_cylinder_bias": ("limit-a2k5d20e40", "loc"),
    "log_std_of_component_0": ("log_std", "log_prob"),
}


def test_the_defect_table_names_every_defect():
    assert set(DEFECT_TABLE) == set(R.DEFECTS) and all(tag in GATE_CASES for tag, _ in DEFECT_TABLE.values())


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_each_seeded_defect_fails_the_gate_on_its_named_case(gate_cases, defect):
    """A subtly wrong kernel does not pass: the same emulation with ONE defect exceeds the bar on the named case and output; the other cases it
    fails on are printed."""
    tag, name = DEFECT_TABLE[defect]
    case, r64, r32 = gate_cases[tag]
    assert max(R.gate_ratios(R.emulate_kernel(*case), r64, r32).values()) <= R.BAR
    ratios = R.gate_ratios(R.emulate_kernel(*case, defect=defect), r64, r32)
    assert ratios[name] > R.BAR, (defect, tag, ratios)
    failing = [t for t, (cs, a, b) in gate_cases.items() if max(R.gate_ratios(R.emulate_kernel(*cs, defect=defect), a, b).values()) > R.BAR]
    print(f"  {defect}: {tag} {name} {ratios[name]:.3g}; fails on {len(failing)} of {len(gate_cases)} cases")
