"""Accuracy of the trajectory predictor (hns_tp_observe) against an fp64 LSTM (tp_f64_reference.py), at its numerical edges.

The other tests of the predictor allow 1e-5 against the fp32 oracle, which a kernel that lost one term of its fp16 splits still passes.
Here the gate is relative to plain fp32: for `pred` and for the rpos_pred columns of `obs_self` / `state_drones`,

    e_hip <= C_GATE * max(e_32, u)

with e_hip / e_32 the largest absolute error against fp64 of the kernel / of the oracle (fp32 + libm) on the same window and weights, and
u = 2^-24 * max |fp64 output|.  The columns that are not predictions must be bit-exact with the oracle.

CPU part: the fp64 reference against the reference's goldens, the oracle against the fp64 reference on the stress cases (the checker
checks itself), and a numpy emulation of the shipped split arithmetic (csrc/hns_tp.hip) that passes the gate
while the same emulation with one low split term dropped fails it.  GPU part: the kernel on the same stress cases."""
import json
import zlib

import numpy as np
import pytest
import torch

import hns_oracle as O
import tp_f64_reference as R64
from hns_amd import abi, config

C_GATE = 5.0        # MI355X: worst e_hip / max(e_32, u) 2.37 over every case, output and call ("wide_early"); 2.1x headroom.
                    # One low split term dropped from the kernel (recurrent h, W_hh, last frame chunk, output layer, W_ih chunk 0): 6.9 .. 4 600
ARENA, MAX_H = 0.9, 1.2


def gate_errors(got, ref):
    """(largest absolute error, u = 2^-24 * largest |reference|)."""
    return float(np.abs(np.asarray(got, np.float64) - ref).max()), float(2.0 ** -24 * np.abs(ref).max())


def ratio(e_k, e_32, u):
    return e_k / max(e_32, u)


# ---- stress cases --------------------------------------------------------------------------------------------------------------------
# weights: ref (the golden weights where the shape is the golden's, else torch's default init U(-1/8, 1/8)), x3, wide (row scales
# log-uniform over [2^-16, 4], entries exactly representable in fp16 after the kernel's gate scaling, entries whose fp16 high part is
# subnormal), gates (some gates near z = 0, others saturated), fcsat (output layer near tanh saturation).
# prog: progress range of the frames (the frame's first value; above 2048 its fp16 high part is no longer exact).
def _case(name, E=256, A=3, NT=1, obst=0, Cn=5, T=10, F=5, max_len=800, prog=(0, 40), weights="ref", det="mixed", cpu=True):
    return dict(name=name, E=E, A=A, NT=NT, obst=obst, Cn=Cn, T=T, F=F, max_len=max_len, prog=prog, weights=weights, det=det, cpu=cpu)


CASES = [
    _case("ref_3v1_2048", E=2048, weights="ref"),
    _case("x3_late", weights="x3", prog=(790, 799)),
    _case("x3_long_episode", weights="x3", max_len=5000, prog=(4985, 4999)),
    _case("wide_early", weights="wide"),
    _case("wide_long_episode", weights="wide", max_len=5000, prog=(4985, 4999)),
    _case("gates_late", weights="gates", prog=(790, 799)),
    _case("fcsat", weights="fcsat", prog=(790, 799)),
    _case("all_detected", weights="x3", det="all"),
    _case("cyl_2chunks", A=3, obst=1, Cn=5, weights="x3", prog=(790, 799)),           # 31 values
    _case("cyl_3chunks", A=4, obst=1, Cn=8, weights="wide"),                           # 43 values
    _case("cyl_4chunks", A=6, obst=1, Cn=12, weights="x3", prog=(790, 799)),          # 61 values
    _case("cyl_5chunks", A=7, obst=1, Cn=16, weights="gates"),                         # 76 values
    _case("T1", T=1, weights="x3", prog=(790, 799)),
    _case("T16", T=16, weights="wide", max_len=5000, prog=(4980, 4999)),
    _case("F1", F=1, weights="fcsat"),
    _case("F10", F=10, weights="x3", prog=(790, 799)),
    _case("3v2", NT=2, weights="x3", prog=(790, 799)),
    _case("3v2_wide", NT=2, weights="wide", E=100),
    _case("ragged_97", E=97, A=2, weights="gates", prog=(790, 799)),
    _case("ragged_1", E=1, A=5, weights="x3"),
    _case("e65536", E=65536, weights="x3", prog=(790, 799), cpu=False),
]
CASE_IDS = [c["name"] for c in CASES]
N_CALLS = 3


def frame_dim(cs):
    return 7 + 3 * cs["A"] + (3 * cs["Cn"] if cs["obst"] else 0)


def make_cfg(cs):
    task = {"num_agents": cs["A"], "num_targets": cs["NT"], "use_obstacles": cs["obst"], "history_step": cs["T"], "future_predcition_step": cs["F"],
            "cylinder": {"max_num": cs["Cn"], "min_num": min(3, cs["Cn"]), "obs_max_cylinder": min(3, cs["Cn"])},
            "env": {"num_envs": cs["E"], "max_episode_length": cs["max_len"]}}
    return config.make_cfg(task, algo={"use_TP_net": 1, "critic_input": "state"})


def _fp16_exact_after(w, s):
    """Values near w whose product with the kernel's gate scale s (fp32) is an fp16 number: their low split term is 0."""
    h = (w.astype(np.float32) * np.float32(s)).astype(np.float16).astype(np.float32)
    cand = (h / np.float32(s)).astype(np.float32)
    ok = (cand * np.float32(s)).astype(np.float32) == h
    return np.where(ok, cand, w).astype(np.float32)


def make_weights(cs, golden=None):
    """fp32 parameters of the case (the fields of abi.TP_STATE_DICT_KEYS)."""
    I, F, H = frame_dim(cs), cs["F"], abi.HNS_TP_HIDDEN
    r = np.random.RandomState(zlib.crc32(cs["name"].encode()))
    shapes = {"w_ih": (4 * H, I), "w_hh": (4 * H, H), "b_ih": (4 * H,), "b_hh": (4 * H,), "w_fc": (3 * F, H), "b_fc": (3 * F,)}
    if golden is not None and I == 16 and F == 5:
        w = {f: golden["w_" + k.replace(".", "_")].astype(np.float32) for f, k in abi.TP_STATE_DICT_KEYS.items()}
    else:
        w = {f: r.uniform(-0.125, 0.125, s).astype(np.float32) for f, s in shapes.items()}
    kind = cs["weights"]
    if kind in ("x3", "gates", "fcsat"):
        w = {f: (v * np.float32(3.0)).astype(np.float32) for f, v in w.items()}
    if kind == "wide":
        gscale = np.where((np.arange(4 * H) // H) == 2, np.float32(2 * -1.4426950408889634), np.float32(-1.4426950408889634)).astype(np.float32)
        for f in ("w_ih", "w_hh", "w_fc"):
            v = r.uniform(-1, 1, shapes[f]) * np.exp2(r.uniform(-16, 2, (shapes[f][0], 1)))
            v = v.astype(np.float32)
            sel = r.rand(*shapes[f])
            s = (np.float32(2 * -1.4426950408889634) * np.ones((shapes[f][0], 1), np.float32)) if f == "w_fc" else gscale[:, None]
            v = np.where(sel < 0.15, _fp16_exact_after(v, s), v)                              # low term 0
            v = np.where(sel > 0.85, (r.uniform(-1, 1, shapes[f]) * np.exp2(r.uniform(-24, -15, shapes[f]))).astype(np.float32), v)   # subnormal high part
            w[f] = v.astype(np.float32)
        for f in ("b_ih", "b_hh", "b_fc"):
            w[f] = (r.uniform(-1, 1, shapes[f]) * np.exp2(r.uniform(-16, 1, shapes[f]))).astype(np.float32)
    if kind == "gates":                              # per hidden unit: all four gates near z = 0, or saturated by the bias
        unit = np.arange(4 * H) % H
        near0 = (unit % 3) == 0
        sat = (unit % 3) == 1
        w["w_ih"] = np.where(near0[:, None], w["w_ih"] * np.float32(1e-3), w["w_ih"]).astype(np.float32)
        w["w_hh"] = np.where(near0[:, None], w["w_hh"] * np.float32(1e-3), w["w_hh"]).astype(np.float32)
        b = np.where(sat, r.choice([-1.0, 1.0], 4 * H) * r.uniform(8, 30, 4 * H), np.where(near0, r.uniform(-1e-3, 1e-3, 4 * H), w["b_ih"]))
        w["b_ih"] = b.astype(np.float32)
        w["b_hh"] = np.where(near0 | sat, np.float32(0), w["b_hh"]).astype(np.float32)
    if kind == "fcsat":                              # |W_fc h + b| around 2-6: tanh within 1e-2 .. 1e-5 of +-1
        w["w_fc"] = (w["w_fc"] * np.float32(4.0)).astype(np.float32)
        w["b_fc"] = (r.choice([-1.0, 1.0], 3 * F) * r.uniform(2.0, 4.0, 3 * F)).astype(np.float32)
    return w


def make_state(cs, c, call, seed):
    """Host arrays of one call: positions in the arena, progress in the case's range (one more per call), mixed detection."""
    r = np.random.RandomState(seed)
    arrs = O.alloc_buffers(c)
    E, A, NT = cs["E"], cs["A"], cs["NT"]
    ds = arrs["drone_state"]
    ds[..., 0:2] = r.uniform(-0.45, 0.45, (E, A, 2))
    ds[..., 2] = r.uniform(0.0, 1.2, (E, A))
    ds[..., 3] = 1.0
    ds[..., 7:13] = r.uniform(-1, 1, (E, A, 6))
    tp, tv = arrs["target_pos"], arrs["target_vel"]
    tp[...] = np.concatenate([r.uniform(-0.45, 0.45, tp.shape[:-1] + (2,)), r.uniform(0.0, 1.2, tp.shape[:-1] + (1,))], -1)
    tv[...] = r.uniform(-1.5, 1.5, tv.shape)
    lo, hi = cs["prog"]
    base = np.random.RandomState(seed - call).randint(lo, max(lo + 1, hi - N_CALLS + 2), E)    # the same envs move on by one per call
    arrs["progress"][:] = np.minimum(base + call, hi).astype(np.float32)
    if cs["det"] == "all":
        arrs["detect"][:] = 3 if NT == 2 else 1
    else:
        arrs["detect"][:] = r.randint(0, 4 if NT == 2 else 2, E)
    cyl = arrs["cylinders"]
    cyl[..., 0:2] = r.uniform(-0.45, 0.45, cyl.shape[:-1] + (2,))
    cyl[..., 2] = r.uniform(0.0, 1.2, cyl.shape[:-1])
    arrs["obs_self"][...] = r.standard_normal(arrs["obs_self"].shape).astype(np.float32)
    return arrs


def oracle_tp_arrays(cs, c, w):
    tpa = O.alloc_tp_buffers(c, cs["T"], cs["F"]) if cs["NT"] == 1 else {
        k: np.zeros(shape if k != "packed" else (16,), dtype=dt)
        for k, (shape, dt) in abi.tp_buffer_shapes(c.num_envs, c.num_agents, cs["T"], cs["F"], frame_dim(cs), 2).items()}
    for f in R64.WEIGHT_FIELDS:
        tpa[f][...] = w[f]
    return tpa


def measure(cs, outs, history, arrs, w):
    """{output: (e, u)} of one implementation's outputs against the fp64 reference on `history`."""
    ref = R64.predict(history, w, ARENA, MAX_H, arrs["drone_state"][..., 0:3], cs["NT"])
    res = {"pred": gate_errors(outs["pred"], ref["pred"])}
    for k in ("obs_self", "state_drones"):
        res[k] = gate_errors(R64.row_rpos(outs[k], cs["F"], cs["NT"]), ref["rpos"])
    return res


# ---- CPU: the fp64 reference against the goldens -----------------------------------------------------------------------------------
GOLDENS = ["g_tp_obs", "g_tp_obs_a6", "g_tp_obs_obst", "g_tp_obs_obst_c8"]


@pytest.mark.parametrize("name", GOLDENS)
def test_f64_reference_matches_reference_goldens(golden, name):
    """tanh(FC(LSTM)) in fp64 on the golden windows, rescaled and subtracted from the pursuers: the reference's own rows within 1e-5."""
    g = golden(name)
    E, A, Cn, T, _ = (int(x) for x in g["meta"])
    w = {f: g["w_" + k.replace(".", "_")] for f, k in abi.TP_STATE_DICT_KEYS.items()}
    worst = 0.0
    for t in range(T):
        ref = R64.predict(g["TP_input"][t], w, ARENA, MAX_H, g["pos"][t])
        for key in ("state_self", "state_drones"):
            rows = g[key][t][:, :, 0] if key == "state_self" else g[key][t]
            got = R64.row_rpos(rows, 5)
            np.testing.assert_allclose(got, ref["rpos"], rtol=0, atol=1e-5)
            worst = max(worst, float(np.abs(got - ref["rpos"]).max()))
    assert worst > 0                                 # the goldens are fp32: some difference must show


@pytest.mark.parametrize("cs", [c for c in CASES if c["cpu"]], ids=[c["name"] for c in CASES if c["cpu"]])
def test_oracle_is_as_accurate_as_fp32(golden, cs):
    """The oracle (fp32 + libm) against fp64 on the stress cases, next to a numpy fp32 LSTM on the same window: within the gate of it,
    and within 1e-5 absolute.  What the GPU tests compare the kernel with is sound."""
    c = config.resolve_hns_cfg(make_cfg(cs))
    w = make_weights(cs, golden("g_tp_obs"))
    tpa = oracle_tp_arrays(cs, c, w)
    for call in range(N_CALLS):
        arrs = make_state(cs, c, call, 1000 + call)
        O.tp_observe(c, arrs, tpa, fill=(call == 0))
        res = measure(cs, tpa, tpa["history"], arrs, w)
        ref = R64.rescale(R64.lstm_fc_tanh(tpa["history"], w), ARENA, MAX_H)
        e_np, _ = gate_errors(emulate(tpa["history"], w, "f32", ARENA, MAX_H), ref)
        e_or, u = res["pred"]
        assert e_or <= 1e-5, (cs["name"], call, e_or)
        assert ratio(e_or, e_np, u) <= C_GATE, (cs["name"], call, e_or, e_np, u)
        for k in ("obs_self", "state_drones"):
            assert res[k][0] <= 1e-5, (cs["name"], k, res[k])


# ---- CPU: emulation of the shipped split -------------------------------------------------------------------------------------------
NEG_LOG2E = np.float32(-1.4426950408889634)
DROPS = ("h_lo", "whh_lo", "x_lo_last", "fc_lo", "wih_lo_c0")       # M1..M5 of the mutation check


def _split(v):
    """Unscaled two-term fp16 split of the weight-stationary kernel: hi = fp16(v), lo = fp16(v - hi) (fp16 subnormals kept)."""
    v = np.asarray(v, np.float32)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def _mfma(acc, a, b):
    """acc[N,M] += b[N,16] . a[M,16]^T: exact fp16 products, one fp32 rounding per 16-wide op."""
    return (acc.astype(np.float64) + b @ a.T).astype(np.float32)


@np.errstate(over="ignore")                          # exp / exp2 of saturated gates: inf, as on the device
def emulate(history, w, mode, arena_size, max_height, drop=None):
    """pred [U,F,3] of the weight-stationary kernel's arithmetic (mode "split"; `drop` zeroes one low term) or of a plain fp32 LSTM (mode "f32")."""
    X = np.asarray(history, np.float32)
    U, T, I = X.shape
    H = abi.HNS_TP_HIDDEN
    Wih, Whh, Wfc = (np.asarray(w[k], np.float32) for k in ("w_ih", "w_hh", "w_fc"))
    b = (np.asarray(w["b_ih"], np.float32) + np.asarray(w["b_hh"], np.float32)).astype(np.float32)
    bfc = np.asarray(w["b_fc"], np.float32)
    if mode == "f32":
        h = np.zeros((U, H), np.float32)
        c = np.zeros((U, H), np.float32)
        sig = lambda z: (1.0 / (1.0 + np.exp(-z.astype(np.float64)))).astype(np.float32)
        for t in range(T):
            z = (X[:, t] @ Wih.T + h @ Whh.T + b).astype(np.float32)
            i, f, g, o = sig(z[:, :H]), sig(z[:, H:2 * H]), np.tanh(z[:, 2 * H:3 * H]), sig(z[:, 3 * H:])
            c = (f * c + i * g).astype(np.float32)
            h = (o * np.tanh(c)).astype(np.float32)
        v = np.tanh((h @ Wfc.T + bfc).astype(np.float32))
        return R64.rescale(v, arena_size, max_height).astype(np.float32)
    gs = np.where((np.arange(4 * H) // H) == 2, np.float32(2) * NEG_LOG2E, NEG_LOG2E).astype(np.float32)
    nxc = (I + 15) // 16
    Wx = np.zeros((4 * H, 16 * nxc), np.float32)
    Wx[:, :I] = Wih * gs[:, None]
    Wx[:, 0] = Wx[:, 0] * np.float32(1024.0)                          # progress enters as progress / 1024 against its column x 1024
    wx1, wx2 = _split(Wx)
    wh1, wh2 = _split(Whh * gs[:, None])
    wf1, wf2 = _split(Wfc * (np.float32(2) * NEG_LOG2E))
    bias = (b * gs).astype(np.float32)
    bf = (bfc * (np.float32(2) * NEG_LOG2E)).astype(np.float32)
    if drop == "whh_lo":
        wh2[:] = 0
    if drop == "fc_lo":
        wf2[:] = 0
    if drop == "wih_lo_c0":
        wx2[:, :16] = 0
    if drop == "x_lo_last":
        wx2[:, 16 * (nxc - 1):] = 0
    e2 = lambda a: np.exp2(a.astype(np.float64))
    h1 = h2 = None
    c = np.zeros((U, H), np.float32)
    for t in range(T):
        x = np.zeros((U, 16 * nxc), np.float32)
        x[:, :I] = X[:, t]
        x[:, 0] = x[:, 0] * np.float32(1.0 / 1024.0)
        x1, x2 = _split(x)
        if drop == "x_lo_last":
            x2[:, 16 * (nxc - 1):] = 0
        acc = np.broadcast_to(bias, (U, 4 * H)).astype(np.float32)
        chunks = [(wx1[:, s], wx2[:, s], x1[:, s], x2[:, s]) for s in (slice(16 * k, 16 * k + 16) for k in range(nxc))]
        if t > 0:
            chunks += [(wh1[:, s], wh2[:, s], h1[:, s], h2[:, s]) for s in (slice(16 * k, 16 * k + 16) for k in range(4))]
        for a1, a2, v1, v2 in chunks:                                 # per chunk: w_lo v_hi, w_hi v_hi, w_hi v_lo
            acc = _mfma(acc, a2, v1)
            acc = _mfma(acc, a1, v1)
            acc = _mfma(acc, a1, v2)
        ei, ef, eo = e2(acc[:, :H]), e2(acc[:, H:2 * H]), e2(acc[:, 3 * H:])
        eg = e2(np.minimum(acc[:, 2 * H:3 * H], 64.0))
        ig = ((1 - eg) / (ei * (1 + eg) + (1 + eg))).astype(np.float32)
        c = (1 / (1 + ef) * c + ig).astype(np.float32)
        ec = e2(c * (np.float32(2) * NEG_LOG2E))
        h = ((1 - ec) / (eo * (1 + ec) + (1 + ec))).astype(np.float32)
        h1, h2 = _split(h)
        if drop == "h_lo" and t + 1 < T:
            h2 = np.zeros_like(h2)
    o = np.broadcast_to(bf, (U, bf.shape[0])).astype(np.float32)
    for k in range(4):
        s = slice(16 * k, 16 * k + 16)
        o = _mfma(o, wf2[:, s], h1[:, s])
        o = _mfma(o, wf1[:, s], h2[:, s])
    for k in range(4):
        s = slice(16 * k, 16 * k + 16)
        o = _mfma(o, wf1[:, s], h1[:, s])
    v = (2.0 / (1.0 + e2(o)) - 1.0).astype(np.float32)
    return R64.rescale(v, arena_size, max_height).astype(np.float32)


EMU_CASES = ["golden", "x3_late", "x3_long_episode", "wide_early", "cyl_2chunks"]


def _emu_inputs(golden, which):
    g = golden("g_tp_obs")
    if which == "golden":
        X = g["TP_input"][-1].astype(np.float32)
        w = {f: g["w_" + k.replace(".", "_")] for f, k in abi.TP_STATE_DICT_KEYS.items()}
        return X, w
    cs = dict(next(c for c in CASES if c["name"] == which), E=64)
    c = config.resolve_hns_cfg(make_cfg(cs))
    w = make_weights(cs, g)
    tpa = oracle_tp_arrays(cs, c, w)
    for call in range(N_CALLS):
        O.tp_observe(c, make_state(cs, c, call, 1000 + call), tpa, fill=(call == 0))
    return tpa["history"].copy(), w


@pytest.fixture(scope="module")
def emu_inputs(golden):
    return {k: _emu_inputs(golden, k) for k in EMU_CASES}


@pytest.mark.parametrize("which", EMU_CASES)
def test_emulated_split_passes_the_gate(emu_inputs, which):
    X, w = emu_inputs[which]
    ref = R64.rescale(R64.lstm_fc_tanh(X, w), ARENA, MAX_H)
    e32, u = gate_errors(emulate(X, w, "f32", ARENA, MAX_H), ref)
    es, _ = gate_errors(emulate(X, w, "split", ARENA, MAX_H), ref)
    print(f"{which}: e_split {es:.2e} e_32 {e32:.2e} u {u:.2e} ratio {ratio(es, e32, u):.2f}")
    assert ratio(es, e32, u) <= C_GATE / 2, (es, e32, u)             # with the headroom the hardware's exp / rcp need


@pytest.mark.parametrize("drop", DROPS)
def test_emulated_split_without_a_low_term_fails_the_gate(emu_inputs, drop):
    """The gate's power: one low split term dropped is caught on at least one input (the reference init's golden window for most)."""
    worst = {}
    for which, (X, w) in emu_inputs.items():
        ref = R64.rescale(R64.lstm_fc_tanh(X, w), ARENA, MAX_H)
        e32, u = gate_errors(emulate(X, w, "f32", ARENA, MAX_H), ref)
        ed, _ = gate_errors(emulate(X, w, "split", ARENA, MAX_H, drop=drop), ref)
        worst[which] = ratio(ed, e32, u)
    print(drop, {k: round(v, 1) for k, v in worst.items()})
    assert max(worst.values()) > 2 * C_GATE, worst


# ---- GPU: the kernel against fp64, next to the oracle ------------------------------------------------------------------------------
def run_gpu_case(cs, g):
    """N_CALLS calls of hns_tp_observe on crafted states: per call and output, (e_hip, e_32, u).  Asserts on the way that the window
    is the oracle's and that every column of the rows that is not a prediction is the oracle's, bit for bit."""
    from hns_amd.env import HideAndSeek
    env = HideAndSeek(make_cfg(cs))
    c = env.hcfg
    w = make_weights(cs, g)
    with torch.no_grad():                            # in place, as an optimiser step: the version counters move, the image is re-packed
        for f, key in abi.TP_STATE_DICT_KEYS.items():
            env.TP.get_parameter(key).copy_(torch.from_numpy(w[f]))
    tpa = oracle_tp_arrays(cs, c, w)
    O.set_threads(16 if cs["E"] > 4096 else 1)
    D = tpa["obs_self"].shape[-1]
    keep = R64.other_columns(D, cs["F"], cs["NT"])
    out = []
    for call in range(N_CALLS):
        arrs = make_state(cs, c, call, 1000 + call)
        env.import_state(arrs)
        env._tp_observe()
        O.tp_observe(c, arrs, tpa, fill=(call == 0))
        dev = {k: v.cpu().numpy() for k, v in env._tp_bufs.items() if k != "packed"}
        what = f"{cs['name']} call {call}"
        assert np.array_equal(dev["history"], tpa["history"]), what
        for k in ("obs_self", "state_drones"):
            assert np.array_equal(dev[k][..., keep], tpa[k][..., keep]), f"{what}: non-predicted columns of {k}"
        hip, o32 = measure(cs, dev, dev["history"], arrs, w), measure(cs, tpa, tpa["history"], arrs, w)
        out.append({k: (hip[k][0], o32[k][0], hip[k][1]) for k in hip})
    assert np.abs(tpa["pred"]).max() > 0.05
    return out


def check_gate(name, calls):
    worst = 0.0
    for call, res in enumerate(calls):
        for k, (e_hip, e_32, u) in res.items():
            q = ratio(e_hip, e_32, u)
            worst = max(worst, q)
            assert q <= C_GATE, f"{name} call {call} {k}: e_hip {e_hip:.3e} > {C_GATE} x max(e_32 {e_32:.3e}, u {u:.3e})"
    return worst


def _report(name, calls):
    """One line per case (pytest -s): the largest e_hip, e_32 and ratio over the calls and outputs."""
    rows = [(e_hip, e_32, u, ratio(e_hip, e_32, u)) for res in calls for (e_hip, e_32, u) in res.values()]
    k = max(range(len(rows)), key=lambda i: rows[i][3])
    print("TPACC " + json.dumps({"case": name, "e_hip": max(r[0] for r in rows), "e_32": max(r[1] for r in rows),
                                 "u": max(r[2] for r in rows), "worst_ratio": rows[k][3]}))


@pytest.mark.gpu
@pytest.mark.parametrize("cs", CASES, ids=CASE_IDS)
def test_kernel_is_as_accurate_as_fp32(golden, cs):
    """hns_tp_observe as shipped (one kernel serves every frame width and batch size) within the gate."""
    calls = run_gpu_case(cs, golden("g_tp_obs"))
    _report(cs["name"], calls)
    check_gate(cs["name"], calls)
