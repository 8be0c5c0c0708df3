"""The predictor's training step (hns_amd.tp_train: hns_tp_train_grad, hns_tp_adam, update_tp) against the reference and against fp64.

CPU part: the CPU path of update_tp / loss_and_grad / TPAdam reproduces g_tp_train.npz (the reference's TP_net, update_TP and train_op block
executed by tests/golden/make_golden_tp_train.py) bit for bit; TPAdam's state_dict loads into torch.optim.Adam and back; the numpy fp32
restatement of Adam that the kernel is held to matches torch.optim.Adam(foreach=False) bit for bit (the checker checks itself); every refusal
raises before anything is launched, and the C entry points refuse bad arguments without touching a device.

GPU part: the accuracy gate e_hip <= C * max(e_32, 2^-24 * max|g64|) for the loss and each gradient, with e_hip / e_32 the kernel's and CPU
torch fp32 autograd's largest errors against fp64 autograd of the same network (C = 8; the worst measured ratio is recorded below), over stress
cases; bit identity across calls, index vs gather, strided vs contiguous x, graph replay vs eager; the Adam step (TPAdam, and raw hns_tp_adam /
hns_adam_clipped calls from the same state) bit for bit against the numpy restatement of tests/adam_reference.py and, step by step from the same state, within 4 ulp (of max(|p|, lr)) of torch's Adam on the device; update_tp end to end on the golden rollout; the env picking up TPAdam's steps.

Worst measured gate ratio on an MI355X: WORST_RATIO below (C = 8 leaves 1.75x headroom).
"""
import copy
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

from adam_reference import _fma32, adam_np, bump
from hns_amd import abi
from hns_amd import tp_train as TT
from hns_amd.tp_net import TPNet

GATE = 8.0
WORST_RATIO = 4.57        # measured on an MI355X: 4.57 over the golden rollout's 16 minibatches; 0.75-2.18 over the stress cases (0.75 at 65 536 envs)
KEYS = ["lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0", "fc.weight", "fc.bias"]


def _net(I, F, state=None, seed=0):
    torch.manual_seed(seed)
    net = TPNet(I, 3 * F, F, 1)
    if state is not None:
        net.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in state.items()})
    return net


def _tp_golden(golden):
    """g_tp_train.npz with its derived entries: TP_input cut from the stored frame sequence (step s sees frames s + 1 .. s + T, as
    make_golden_tp_train.py builds it) and the initial weights (g_tp_obs.npz's, which the generator started from)."""
    g = dict(golden("g_tp_train"))
    if "tp_input" not in g:
        T = int(g["meta"][3])
        fr = g["frames"]
        g["tp_input"] = np.ascontiguousarray(np.stack([fr[:, s + 1:s + 1 + T] for s in range(fr.shape[1] - T)], axis=1))
        w0 = golden("g_tp_obs")
        for k in KEYS:
            g["init_" + k] = w0["w_" + k.replace(".", "_")]
    return g


def _grad_digest(grads):
    return hashlib.sha256(b"".join(np.ascontiguousarray(g, dtype=np.float32).tobytes() for g in grads)).hexdigest()


def _golden_net(g):
    return _net(16, 5, {k: g["init_" + k] for k in KEYS})


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def one_thread():
    """The golden was written with one intra-op thread: CPU GEMMs split their sums by thread count."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def test_cpu_update_matches_reference_golden_bit_for_bit(golden, one_thread):
    g = _tp_golden(golden)
    E, STEPS, A, T, F, NMB, EPOCHS, WS = (int(v) for v in g["meta"])
    net = _golden_net(g)
    opt = TT.TPAdam(net.parameters(), lr=1e-4)
    x, y = TT.select_windows(torch.from_numpy(g["tp_input"]), torch.from_numpy(g["tp_groundtruth"]), torch.from_numpy(g["tp_done"]), F, WS)
    assert x.shape[1] == int(g["n_sel"]) and not x.is_contiguous()
    torch.manual_seed(int(g["seed"]))
    perm = TT.minibatches(x.shape[0] * x.shape[1], NMB, x.device)
    assert torch.equal(perm, torch.from_numpy(g["perm"]))              # make_dataset_naive's permutation, same generator calls
    for b, idx in enumerate(perm):
        loss = TT.loss_and_grad(net, x, y, idx)
        assert loss.dim() == 0 and np.float32(loss) == g["loss"][b], b
        grads = [p.grad.numpy() for p in TT.parameters(net)]
        assert _grad_digest(grads) == g["grad_digest"][b], b           # every gradient of every minibatch, bit for bit
        if b == 0:
            for k, gr in zip(KEYS, grads):
                assert np.array_equal(gr, g["grad0_" + k]), k
        opt.step()
    for k, p in zip(KEYS, TT.parameters(net)):
        assert np.array_equal(p.detach().numpy(), g["final_" + k]), k
        st = opt.state[p]
        assert np.array_equal(st["exp_avg"].numpy(), g["exp_avg_" + k]) and np.array_equal(st["exp_avg_sq"].numpy(), g["exp_avg_sq_" + k]), k
        assert float(st["step"]) == float(g["step"])
    # update_tp as one call: the same statements, the same minibatches, the same result
    net2 = _golden_net(g)
    opt2 = TT.TPAdam(net2.parameters(), lr=1e-4)
    torch.manual_seed(int(g["seed"]))
    mean = TT.update_tp(net2, torch.from_numpy(g["tp_input"]), torch.from_numpy(g["tp_groundtruth"]), torch.from_numpy(g["tp_done"]), F, WS, NMB,
                        EPOCHS, opt2)
    assert float(mean) == float(torch.tensor(g["loss"]).mean())
    for k, p in zip(KEYS, TT.parameters(net2)):
        assert np.array_equal(p.detach().numpy(), g["final_" + k]), k


def test_state_dict_round_trips_through_torch_adam(golden):
    g = _tp_golden(golden)
    x = torch.from_numpy(g["tp_input"]).reshape(-1, 10, 16)[:64]
    y = torch.from_numpy(g["tp_groundtruth"]).reshape(-1, 3)[:64].repeat(1, 5)
    net_a, net_b = _golden_net(g), _golden_net(g)
    ta = TT.TPAdam(net_a.parameters(), lr=3e-4)
    ref = torch.optim.Adam(net_b.parameters(), lr=3e-4)           # the reference's construction (single-tensor on the CPU)
    for _ in range(3):
        TT.loss_and_grad(net_a, x, y)
        ta.step()
        TT.loss_and_grad(net_b, x, y)
        ref.step()
    sa, sr = ta.state_dict(), ref.state_dict()
    assert sa["param_groups"] == sr["param_groups"]
    for i in sr["state"]:
        assert set(sa["state"][i]) == set(sr["state"][i])
        for n in sr["state"][i]:
            assert sa["state"][i][n].device == sr["state"][i][n].device and torch.equal(sa["state"][i][n], sr["state"][i][n]), (i, n)
    # both ways: Adam's state into TPAdam, TPAdam's into Adam; one more step each lands on the same bits
    net_c, net_d = _golden_net(g), _golden_net(g)
    net_c.load_state_dict(net_b.state_dict())
    net_d.load_state_dict(net_a.state_dict())
    tc = TT.TPAdam(net_c.parameters())
    tc.load_state_dict(copy.deepcopy(sr))                     # (state_dict() hands out the live moment tensors, as Adam's does)
    rd = torch.optim.Adam(net_d.parameters())
    rd.load_state_dict(copy.deepcopy(sa))
    for net, opt in ((net_a, ta), (net_b, ref), (net_c, tc), (net_d, rd)):
        TT.loss_and_grad(net, x, y)
        opt.step()
    for pa, pb, pc, pd in zip(*(TT.parameters(n) for n in (net_a, net_b, net_c, net_d))):
        assert torch.equal(pa, pb) and torch.equal(pa, pc) and torch.equal(pa, pd)


def torch_sqrt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).sqrt().numpy()


def test_numpy_adam_restatement_matches_torch_adam_on_cpu():
    gen = torch.Generator().manual_seed(5)
    for n in (1, 15, 4096 + 13, 20480):
        p = torch.randn(n, generator=gen)
        q = p.clone().requires_grad_(True)
        opt = torch.optim.Adam([q], lr=1e-4, foreach=False)
        pn, m, v, step = p.numpy().copy(), np.zeros(n, np.float32), np.zeros(n, np.float32), np.float32(0)
        for it in range(20):
            grad = torch.randn(n, generator=gen) * (10.0 ** (it % 5 - 3))
            q.grad = grad.clone()
            opt.step()
            step = bump(step)
            pn, m, v = adam_np(pn, grad.numpy(), m, v, step, 1e-4, sqrt=torch_sqrt)
            assert np.array_equal(pn, q.detach().numpy()), (n, it)
            assert np.array_equal(m, opt.state[q]["exp_avg"].numpy()) and np.array_equal(v, opt.state[q]["exp_avg_sq"].numpy())
    # the checker's power: the unfused lerp or an unfused addcmul is caught
    g = np.random.default_rng(0).standard_normal(100000).astype(np.float32)
    m0 = np.random.default_rng(1).standard_normal(100000).astype(np.float32)
    assert not np.array_equal(_fma32(np.float32(0.1), g - m0, m0), m0 + np.float32(0.1) * (g - m0))


def test_tpadam_steps_nine_parameters_on_the_cpu_as_torch_adam():
    """More tensors than hns_tp_adam's cap of 8: TPAdam has no cap of its own (on the device it goes through hns_adam_clipped)."""
    gen = torch.Generator().manual_seed(9)
    ps = [torch.randn(n, generator=gen).requires_grad_(True) for n in range(1, 10)]
    qs = [p.detach().clone().requires_grad_(True) for p in ps]
    opt, ref = TT.TPAdam(ps), torch.optim.Adam(qs, lr=1e-4, foreach=False)
    for it in range(3):
        for p, q in zip(ps, qs):
            p.grad = torch.randn(p.shape, generator=gen)
            q.grad = p.grad.clone()
        opt.step()
        ref.step()
    for p, q in zip(ps, qs):
        assert torch.equal(p, q) and torch.equal(opt.state[p]["exp_avg_sq"], ref.state[q]["exp_avg_sq"]) and float(opt.state[p]["step"]) == 3.0
    with pytest.raises(TypeError):
        opt.step(grad_norm=torch.tensor(1.0))                    # the predictor's step does not clip and takes no norm


def _refusal_inputs():
    net = _net(16, 5)
    x = torch.randn(4, 6, 10, 16)
    y = torch.randn(24, 15)
    return net, x, y


@pytest.mark.parametrize("case", ["dtype_x", "dtype_y", "dtype_w", "shape_y", "I_mismatch", "I_81", "T_17", "F_11", "blocks", "index_range",
                                  "index_negative", "index_dtype", "index_empty"])
def test_refusals_raise_before_any_launch(case):
    net, x, y = _refusal_inputs()
    idx = None
    err = ValueError
    if case == "dtype_x":
        x, err = x.double(), TypeError
    elif case == "dtype_y":
        y, err = y.half(), TypeError
    elif case == "dtype_w":
        net = net.double()
        err = TypeError
    elif case == "shape_y":
        y = y[:23]
    elif case == "I_mismatch":
        x = torch.randn(4, 6, 10, 17)
    elif case == "I_81":
        net, x = _net(81, 5), torch.randn(4, 6, 10, 81)
    elif case == "T_17":
        x = torch.randn(4, 6, 17, 16)
    elif case == "F_11":
        net, y = _net(16, 11), torch.randn(24, 33)
    elif case == "blocks":
        x = torch.randn(4, 6, 16, 10).transpose(2, 3)
    elif case == "index_range":
        idx, err = torch.tensor([0, 24]), IndexError
    elif case == "index_negative":
        idx, err = torch.tensor([-1, 3]), IndexError
    elif case == "index_dtype":
        idx, err = torch.tensor([0, 1], dtype=torch.int32), TypeError
    elif case == "index_empty":
        idx = torch.zeros(0, dtype=torch.int64)
    before = [p.detach().clone() for p in TT.parameters(net)]
    with pytest.raises(err):
        TT.loss_and_grad(net, x, y, idx)
    assert all(p.grad is None for p in TT.parameters(net))
    assert all(torch.equal(a, b) for a, b in zip(before, TT.parameters(net)))


def test_c_entry_points_refuse_bad_arguments_without_a_device():
    lib = abi.load_library()
    fake = 1 << 20                                              # never dereferenced: the checks come first
    pw = abi.HnsTpParams(*([fake] * 6))
    ws = lib.hns_tp_train_workspace_bytes(7552, 16, 5)
    assert ws > 0 and ws == lib.hns_tp_train_workspace_bytes(10 ** 7, 16, 5)          # grows with the workgroups, not with B beyond them
    assert lib.hns_tp_train_workspace_bytes(1, 16, 5) < ws and lib.hns_tp_train_workspace_bytes(0, 16, 5) == 0
    assert lib.hns_tp_train_workspace_bytes(7552, 81, 5) == 0 and lib.hns_tp_train_workspace_bytes(7552, 16, 11) == 0

    def call(E=4, S=6, sE=960, sS=160, T=10, I=16, B=24, F=5, index=None, wsb=ws, x=fake, wsp=fake):
        return lib.hns_tp_train_grad(C.byref(pw), x, E, S, sE, sS, T, I, fake, index, B, F, C.byref(pw), fake, wsp, wsb, None)
    for kw in ({"T": 17}, {"T": 0}, {"I": 81}, {"I": 0}, {"F": 11}, {"F": 0}, {"B": 0}, {"B": 25}, {"sS": 159}, {"sE": 959}, {"wsb": 16},
               {"x": fake + 2}, {"wsp": fake + 4}, {"index": fake + 4}):
        assert lib.hns_tp_train_grad is not None
        assert call(**kw) == abi.HNS_ERR_INVALID_ARG, kw
    t = abi.HnsTpAdamTensor(fake, fake, fake, fake, 10)
    arr = (abi.HnsTpAdamTensor * 1)(t)
    assert lib.hns_tp_adam(arr, 0, fake, 1e-4, 0.9, 0.999, 1e-8, None) == abi.HNS_ERR_INVALID_ARG
    assert lib.hns_tp_adam(arr, 9, fake, 1e-4, 0.9, 0.999, 1e-8, None) == abi.HNS_ERR_INVALID_ARG
    assert lib.hns_tp_adam(arr, 1, fake, 1e-4, 1.0, 0.999, 1e-8, None) == abi.HNS_ERR_INVALID_ARG
    assert lib.hns_tp_adam(arr, 1, None, 1e-4, 0.9, 0.999, 1e-8, None) == abi.HNS_ERR_INVALID_ARG


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------------

def _grads(net):
    return [p.grad.detach().double().cpu() for p in TT.parameters(net)]


def _reference64(net, xg, yg):
    """(loss, grads) of fp64 autograd and of CPU fp32 autograd on the same fp32 minibatch xg [B, T, I], yg [B, 3F]."""
    out = []
    for dt in (torch.float64, torch.float32):
        n = _net(net.lstm.input_size, net.fc.out_features // 3, {k: v.detach().cpu() for k, v in net.state_dict().items()})
        n = n.to(dt)
        loss = TT._torch_loss_and_grad(n, TT._as_blocks(xg.detach().cpu().to(dt)), yg.detach().cpu().to(dt).reshape(xg.shape[0], -1), None)
        out.append((loss.double(), _grads(n)))
    return out


def _gather(x, y, index):
    x4 = TT._as_blocks(x)
    xg = x4.reshape(-1, x4.shape[2], x4.shape[3])
    yg = y.reshape(xg.shape[0], -1)
    return (xg, yg) if index is None else (xg[index], yg[index])


def gate_ratio(net_dev, x, y, index=None):
    """Largest e_hip / max(e_32, 2^-24 max|g64|) over the loss and the six gradients."""
    loss = TT.loss_and_grad(net_dev, x, y, index)
    torch.cuda.synchronize()
    (l64, g64), (l32, g32) = _reference64(net_dev, *_gather(x, y, index))
    worst = 0.0
    for hip, r32, r64 in zip([loss.double().cpu()] + _grads(net_dev), [l32] + g32, [l64] + g64):
        e_hip = float((hip - r64).abs().max())
        e_32 = float((r32 - r64).abs().max())
        floor = 2.0 ** -24 * float(r64.abs().max())
        worst = max(worst, e_hip / max(e_32, floor, 1e-30))
    return worst


def _stress_case(I, T, F, B, mode, seed, golden=None):
    gen = torch.Generator().manual_seed(seed)
    net = _net(I, F, seed=seed)
    if mode in ("golden", "late") and golden is not None and I == 16 and F == 5:
        net.load_state_dict({k: torch.from_numpy(golden["init_" + k]) for k in KEYS})
    with torch.no_grad():
        if mode == "x3":
            for p in net.parameters():
                p.mul_(3.0)
        elif mode == "saturated":
            net.lstm.bias_ih_l0.add_(torch.randn(4 * 64, generator=gen) * 6.0)
            net.lstm.weight_ih_l0.mul_(4.0)
        elif mode == "out_saturated":
            net.fc.bias.add_(torch.sign(torch.randn(3 * F, generator=gen)) * 3.0)
    x = torch.randn(B, T, I, generator=gen) * 0.5
    if mode == "late":
        x[..., 0] = torch.randint(700, 800, (B, 1), generator=gen).float() - torch.arange(T - 1, -1, -1).float()
    y = (torch.rand(B, 3 * F, generator=gen) * 2 - 1) * 0.95
    return net, x, y


STRESS = ["golden", "x3", "saturated", "out_saturated", "late", "I10", "I31", "I76", "T1", "T16", "F1", "F10", "B1", "B31", "B33", "B7552"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", STRESS)
def test_gradients_pass_the_fp64_gate(golden, name):
    g = _tp_golden(golden)
    I, T, F = {"I10": (10, 10, 5), "I31": (31, 10, 5), "I76": (76, 10, 5), "T1": (16, 1, 5), "T16": (16, 16, 5), "F1": (16, 10, 1),
               "F10": (16, 10, 10)}.get(name, (16, 10, 5))
    B = {"saturated": 512, "out_saturated": 512, "B1": 1, "B31": 31, "B33": 33, "B7552": 7552}.get(name, 1024 if name in ("golden", "x3", "late") else 256)
    mode = name if name in ("x3", "saturated", "out_saturated", "late") else ("golden" if name in ("golden", "B7552") else "default")
    net, x, y = _stress_case(I, T, F, B, mode, seed=sum(map(ord, name)), golden=g)
    r = gate_ratio(net.cuda(), x.cuda(), y.cuda())
    print(f"gate {name}: {r:.3f}")
    assert r <= GATE, r


@pytest.mark.gpu
def test_full_65536_env_minibatch_passes_the_gate(golden):
    """One minibatch of a 65 536-env rollout (65 536 x 59 / 16 = 241 664 sequences), read through an index from the [E, n_sel] layout."""
    g = _tp_golden(golden)
    E, S, B = 65536, 59, 241664
    gen = torch.Generator().manual_seed(11)
    net = _net(16, 5, {k: g["init_" + k] for k in KEYS}).cuda()
    x = (torch.randn(E, S + 1, 10, 16, generator=gen) * 0.5)[:, :S]
    y = (torch.rand(E * S, 15, generator=gen) * 2 - 1) * 0.9
    idx = torch.randperm(E * S, generator=gen)[:B]
    xd = torch.empty((E, S + 1, 10, 16), device="cuda")[:, :S]
    xd.copy_(x)
    del x
    r = gate_ratio(net, xd, y.cuda(), idx.cuda())
    print(f"gate full65536: {r:.3f}")
    assert r <= GATE, r


@pytest.mark.gpu
def test_bit_identity_calls_index_strides_and_graph_replay(golden):
    g = _tp_golden(golden)
    dev = torch.device("cuda")
    net = _golden_net(g).to(dev)
    x, y = TT.select_windows(torch.from_numpy(g["tp_input"]).to(dev), torch.from_numpy(g["tp_groundtruth"]).to(dev),
                             torch.from_numpy(g["tp_done"]).to(dev), 5, 1)
    assert not x.is_contiguous()
    idx = torch.from_numpy(g["perm"][0]).to(dev)

    def run(xx, yy, ii):
        loss = TT.loss_and_grad(net, xx, yy, ii)
        return [loss.clone()] + [p.grad.clone() for p in TT.parameters(net)]
    a, b = run(x, y, idx), run(x, y, idx)
    assert all(torch.equal(u, v) for u, v in zip(a, b)), "two calls differ"
    gathered = run(x.reshape(-1, 10, 16)[idx].contiguous(), y[idx].contiguous(), None)
    assert all(torch.equal(u, v) for u, v in zip(a, gathered)), "index differs from the gathered copy"
    contig = run(x.contiguous(), y, idx)
    assert all(torch.equal(u, v) for u, v in zip(a, contig)), "strided x differs from .contiguous()"

    # one loss_and_grad + TPAdam.step captured and replayed, against the same two calls eagerly from the same state
    opt = TT.TPAdam(net.parameters())
    TT.loss_and_grad(net, x, y, idx, check_index=False)
    opt.step()                                                  # state exists before the capture
    torch.cuda.synchronize()
    snap_p = [p.detach().clone() for p in TT.parameters(net)]
    snap_s = {id(p): {k: v.clone() for k, v in opt.state[p].items()} for p in TT.parameters(net)}
    eager_loss = TT.loss_and_grad(net, x, y, idx, check_index=False).clone()
    opt.step()
    eager = [p.detach().clone() for p in TT.parameters(net)] + [opt.state[p]["exp_avg_sq"].clone() for p in TT.parameters(net)]
    with torch.no_grad():
        for p, s in zip(TT.parameters(net), snap_p):
            p.copy_(s)
        for p in TT.parameters(net):
            for k, v in snap_s[id(p)].items():
                opt.state[p][k].copy_(v)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            gl = TT.loss_and_grad(net, x, y, idx, check_index=False)
            opt.step()
    torch.cuda.current_stream().wait_stream(side)
    with torch.no_grad():                                       # capture does not run the kernels; restore anyway (defensive)
        for p, s in zip(TT.parameters(net), snap_p):
            p.copy_(s)
        for p in TT.parameters(net):
            for k, v in snap_s[id(p)].items():
                opt.state[p][k].copy_(v)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [p.detach().clone() for p in TT.parameters(net)] + [opt.state[p]["exp_avg_sq"].clone() for p in TT.parameters(net)]
    assert torch.equal(gl, eager_loss)
    assert all(torch.equal(u, v) for u, v in zip(eager, replayed)), "graph replay differs from eager"


@pytest.mark.gpu
def test_adam_kernel_matches_numpy_restatement_and_torch_adam(golden):
    g = _tp_golden(golden)
    dev = torch.device("cuda")
    net = _golden_net(g).to(dev)
    ref = _golden_net(g).to(dev)
    opt = TT.TPAdam(net.parameters(), lr=1e-4)
    topt = torch.optim.Adam(ref.parameters(), lr=1e-4, foreach=False)
    host = {k: (p.detach().cpu().numpy().copy(), np.zeros(p.shape, np.float32), np.zeros(p.shape, np.float32)) for k, p in zip(KEYS, TT.parameters(net))}
    step = np.float32(0)
    gen = torch.Generator().manual_seed(3)
    worst = 0.0
    for it in range(20):
        grads = [torch.randn(p.shape, generator=gen) * (10.0 ** (it % 4 - 3)) for p in TT.parameters(net)]
        if it > 0:                                              # torch's Adam steps from the kernel's state: the difference of one step
            with torch.no_grad():
                for p, q in zip(TT.parameters(net), TT.parameters(ref)):
                    q.copy_(p)
                    topt.state[q]["exp_avg"].copy_(opt.state[p]["exp_avg"])
                    topt.state[q]["exp_avg_sq"].copy_(opt.state[p]["exp_avg_sq"])
        for p, q, gr in zip(TT.parameters(net), TT.parameters(ref), grads):
            p.grad, q.grad = gr.to(dev), gr.to(dev)
        opt.step()
        topt.step()
        step = bump(step)
        for k, gr in zip(KEYS, grads):
            host[k] = adam_np(host[k][0], gr.numpy(), *host[k][1:], step, 1e-4)
        for k, p in zip(KEYS, TT.parameters(net)):
            assert np.array_equal(p.detach().cpu().numpy(), host[k][0]), (it, k)
            assert np.array_equal(opt.state[p]["exp_avg"].cpu().numpy(), host[k][1]), (it, k)
            assert np.array_equal(opt.state[p]["exp_avg_sq"].cpu().numpy(), host[k][2]), (it, k)
        for p, q in zip(TT.parameters(net), TT.parameters(ref)):
            # 4 ulp of the parameter, or of the step size where the parameter is smaller than one step (its own ulp is then finer than the
            # rounding of the update both compute)
            a, b = p.detach().cpu().numpy(), q.detach().cpu().numpy()
            u = np.abs(a - b) / np.spacing(np.maximum(np.abs(b), np.float32(1e-4)))
            worst = max(worst, float(u.max()))
    print(f"adam: worst {worst:.1f} ulp against torch.optim.Adam(foreach=False) on the device")
    assert worst <= 4, worst
    assert float(opt.state[TT.parameters(net)[0]]["step"]) == 20.0


DOOR_SIZES = (0, 1, 255, 256, 257, 65537)    # nothing, one thread, around one workgroup, and one value past 256 workgroups x 256 threads (a second grid-stride trip)


def _descriptors(tensors, spare):
    """hns_adam_tensor descriptors of (param, grad, exp_avg, exp_avg_sq) tuples.  An empty tensor has no address; the entry points want a
    non-NULL one and read nothing through it: `spare`."""
    arr = (abi.HnsAdamTensor * len(tensors))()
    for j, ts in enumerate(tensors):
        arr[j] = abi.HnsAdamTensor(*(t.data_ptr() or spare for t in ts), ts[0].numel())
    return arr


def _adam_np_steps(p0, grads, lr):
    """p0 after one adam_np step per entry of grads, from zero moments: ([p...], [m...], [v...], step)."""
    host, step = [(p.numpy().copy(), np.zeros(p.shape, np.float32), np.zeros(p.shape, np.float32)) for p in p0], np.float32(0)
    for gs in grads:
        step = bump(step)
        host = [adam_np(*h, step, lr) for h in ((h[0], g.numpy(), h[1], h[2]) for h, g in zip(host, gs))]
    return [h[0] for h in host], [h[1] for h in host], [h[2] for h in host], step


def _tpadam_steps(p0, grads, lr):
    ps = [torch.nn.Parameter(p.cuda()) for p in p0]
    opt = TT.TPAdam(ps, lr=lr)
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.cuda()
        opt.step()
    torch.cuda.synchronize()
    st = [opt.state[p] for p in ps]
    assert all(s["step"] is st[0]["step"] for s in st)
    return ([p.detach().cpu().numpy() for p in ps], [s["exp_avg"].cpu().numpy() for s in st], [s["exp_avg_sq"].cpu().numpy() for s in st],
            np.float32(st[0]["step"].item()))


@pytest.mark.gpu
def test_one_adam_step_behind_hns_tp_adam_hns_adam_clipped_and_tpadam():
    """The same parameters, moments, counter and gradients through a raw hns_tp_adam call, a raw hns_adam_clipped call without a norm and
    TPAdam.step(): three steps with gradients at 1e-3, 1 and 1e3, every array and the counter identical and equal to adam_np's."""
    lib = abi.load_library()
    gen = torch.Generator().manual_seed(9)
    p0 = [torch.randn(n, generator=gen) for n in DOOR_SIZES]
    grads = [[torch.randn(n, generator=gen) * s for n in DOOR_SIZES] for s in (1e-3, 1.0, 1e3)]
    got = {"TPAdam": _tpadam_steps(p0, grads, 1e-4)}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for door in ("hns_tp_adam", "hns_adam_clipped"):
        ps, ms, vs = [p.cuda() for p in p0], [torch.zeros_like(p).cuda() for p in p0], [torch.zeros_like(p).cuda() for p in p0]
        step = torch.zeros((), device="cuda")
        for gs in grads:
            gd = [g.cuda() for g in gs]
            arr = _descriptors(list(zip(ps, gd, ms, vs)), step.data_ptr())
            if door == "hns_tp_adam":
                rc = lib.hns_tp_adam(arr, len(ps), step.data_ptr(), 1e-4, 0.9, 0.999, 1e-8, stream)
            else:
                rc = lib.hns_adam_clipped(arr, len(ps), step.data_ptr(), None, 10.0, 1e-4, 0.9, 0.999, 1e-8, stream)
            assert rc == abi.HNS_OK, lib.hns_last_error()
            torch.cuda.synchronize()
        got[door] = ([p.cpu().numpy() for p in ps], [m.cpu().numpy() for m in ms], [v.cpu().numpy() for v in vs], np.float32(step.item()))
    want = _adam_np_steps(p0, grads, 1e-4)
    assert float(want[3]) == 3.0
    for door, (ps, ms, vs, step) in got.items():
        assert step == want[3], door
        for k, n in enumerate(DOOR_SIZES):
            assert ps[k].shape == (n,) and np.array_equal(ps[k], want[0][k]), (door, n)
            assert np.array_equal(ms[k], want[1][k]) and np.array_equal(vs[k], want[2][k]), (door, n)


@pytest.mark.gpu
def test_tpadam_steps_nine_tensors_on_the_device():
    """One more than hns_tp_adam takes: TPAdam steps them in one call of hns_adam_clipped, bit for bit with adam_np."""
    gen = torch.Generator().manual_seed(10)
    p0 = [torch.randn(n, generator=gen) for n in (5, 64, 1, 300, 17, 2, 129, 33, 8)]
    grads = [[torch.randn(p.shape, generator=gen) * s for p in p0] for s in (1.0, 1e-2)]
    got, want = _tpadam_steps(p0, grads, 1e-4), _adam_np_steps(p0, grads, 1e-4)
    assert got[3] == want[3] == 2.0
    for k in range(9):
        assert all(np.array_equal(got[j][k], want[j][k]) for j in range(3)), k


@pytest.mark.gpu
def test_update_tp_end_to_end_on_the_golden_rollout(golden):
    g = _tp_golden(golden)
    dev = torch.device("cuda")
    net = _golden_net(g).to(dev)
    opt = TT.TPAdam(net.parameters(), lr=1e-4)
    x, y = TT.select_windows(torch.from_numpy(g["tp_input"]).to(dev), torch.from_numpy(g["tp_groundtruth"]).to(dev),
                             torch.from_numpy(g["tp_done"]).to(dev), 5, 1)
    cpu = _golden_net(g)
    worst = 0.0
    for b, idx in enumerate(torch.from_numpy(g["perm"])):
        loss = TT.loss_and_grad(net, x, y, idx.to(dev))
        # the gate on every minibatch: fp64 and CPU fp32 autograd from the kernel's current weights
        cpu.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
        (l64, g64), (l32, g32) = _reference64(cpu, *_gather(x, y, idx.to(dev)))
        hips = [loss.double().cpu()] + _grads(net)
        for hip, r32, r64 in zip(hips, [l32] + g32, [l64] + g64):
            e_hip, e_32 = float((hip - r64).abs().max()), float((r32 - r64).abs().max())
            worst = max(worst, e_hip / max(e_32, 2.0 ** -24 * float(r64.abs().max()), 1e-30))
        # against the reference's own run: the loss of every minibatch (the weights drift apart by rounding only), all gradients of the first
        assert abs(float(loss) - float(g["loss"][b])) <= 1e-4 * float(g["loss"][b]), b
        if b == 0:
            for hip, k, r64 in zip(hips[1:], KEYS, g64):
                gold = torch.from_numpy(g["grad0_" + k]).double()
                e_gold = float((gold - r64).abs().max())
                worst = max(worst, float((hip - r64).abs().max()) / max(e_gold, 2.0 ** -24 * float(r64.abs().max()), 1e-30))
        opt.step()
    print(f"gate end_to_end: {worst:.3f}")
    assert worst <= GATE, worst
    for k, p in zip(KEYS, TT.parameters(net)):
        d = (p.detach().cpu() - torch.from_numpy(g["final_" + k])).abs()
        assert float(d.max()) <= 16 * 2e-4 and float(d.median()) <= 1e-6, k
    # update_tp as one call on the device: 64 updates lower the loss
    net2 = _golden_net(g).to(dev)
    opt2 = TT.TPAdam(net2.parameters(), lr=1e-3)
    args = [torch.from_numpy(g[k]).to(dev) for k in ("tp_input", "tp_groundtruth", "tp_done")]
    torch.manual_seed(0)
    means = [float(TT.update_tp(net2, *args, 5, 1, 16, 1, opt2)) for _ in range(4)]
    assert means[-1] < means[0], means


@pytest.mark.gpu
def test_env_sees_tpadam_steps_without_a_refresh():
    from hns_amd import config
    from hns_amd.env import HideAndSeek

    def env():
        cfg = config.make_cfg({"num_agents": 3, "cylinder": {"max_num": 5, "min_num": 3}, "env": {"num_envs": 128, "max_episode_length": 40}},
                              algo={"use_TP_net": 1})
        e = HideAndSeek(cfg)
        e.set_seed(3)
        e.reset()
        return e
    a, b = env(), env()
    b.TP.load_state_dict(a.TP.state_dict())
    gen = torch.Generator().manual_seed(1)
    act = [torch.randn(128, 3, 4, generator=gen).cuda() for _ in range(2)]
    for e in (a, b):
        e.step(e.rand_step_input(act[0]))
    assert torch.equal(a._tp_bufs["pred"], b._tp_bufs["pred"])
    x = torch.randn(64, 10, a.TP.lstm.input_size, generator=gen).cuda()
    y = torch.rand(64, a.TP.fc.out_features, generator=gen).cuda()
    opt = TT.TPAdam(a.TP.parameters(), lr=1e-2)
    TT.loss_and_grad(a.TP, x, y)
    opt.step()
    b.TP.load_state_dict(a.TP.state_dict())
    before = a._tp_bufs["pred"].clone()
    for e in (a, b):
        e.step(e.rand_step_input(act[1]))
    assert torch.equal(a._tp_bufs["pred"], b._tp_bufs["pred"]) and torch.equal(a._tp_bufs["obs_self"], b._tp_bufs["obs_self"])
    assert not torch.equal(before, a._tp_bufs["pred"])
