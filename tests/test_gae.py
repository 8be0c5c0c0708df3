"""The rollout boundary (hns_amd.gae; csrc/hns_gae.hip): GAE, the moment row and the normalisation of advantages and returns against the reference's
compute_gae / compute_gae_ and MAPPOPolicy.train_op block executed as written (tests/golden/g_gae.npz, tests/golden/make_golden_gae.py).

CPU tests: the torch restatement against the fixture bit for bit, rollout_targets against train_op, the C ABI's refusals (before any launch), the
kernels' resources.  GPU tests (-m gpu): hns_gae bit for bit against the fixture and against the torch loop on the same device, the moment row,
hns_rollout_normalise against sharding's expression, a split rollout, a captured graph."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits_equal(a, b):
    """Same shape and the same bits (so -0.0 != +0.0)."""
    a, b = torch.as_tensor(a).detach().cpu().contiguous(), torch.as_tensor(b).detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


class _ValueNorm1:
    """The state and read-outs of the reference's ValueNorm1 (learning/utils/valuenorm.py:45-106) that rollout_targets works on."""

    def __init__(self, beta, epsilon=1e-5, device="cpu"):
        self.beta, self.epsilon = beta, epsilon
        self.running_mean, self.running_mean_sq = torch.zeros(1, device=device), torch.zeros(1, device=device)
        self.debiasing_term = torch.tensor(0.0, device=device)

    def running_mean_var(self):
        d = self.debiasing_term.clamp(min=self.epsilon)
        mean, mean_sq = self.running_mean / d, self.running_mean_sq / d
        return mean, (mean_sq - mean ** 2).clamp(min=1e-2)


def _cases(g):
    for T, K, E, Kd in (tuple(int(x) for x in c) for c in g["cases"]):
        cid = f"t{T}k{K}"
        yield cid, T, K, E, Kd, (torch.from_numpy(g[f"{cid}_{n}"]) for n in ("reward", "done", "value", "next_value"))


def _tm(x):
    return x.transpose(0, 1).contiguous()


# ---- CPU -------------------------------------------------------------------------------------------------------------------------------------
def test_golden_covers_the_cases_the_issue_names(golden):
    g = golden("g_gae")
    cases = [tuple(int(x) for x in c) for c in g["cases"]]
    assert {c[0] for c in cases} == {1, 8, 64} and {c[1] for c in cases} == {1, 3, 7} and max(c[2] for c in cases) <= 64
    assert {c[3] == c[1] for c in cases if c[1] > 1} == {True, False}            # Kd = K and Kd = 1 (broadcast)
    assert [tuple(p) for p in g["pairs"]] == [(0.99, 0.95), (0.995, 0.95)]
    for cid, T, K, E, Kd, (reward, done, value, nv) in _cases(g):
        assert done[0, 0].all() and done[1, T // 2].all() and done[2, T - 1].all() and done[3].all()
        adv = torch.from_numpy(g[f"{cid}_g0_adv"])
        assert reward[4, T - 1, 0] == 0 and torch.signbit(reward[4, T - 1, 0]) and not torch.signbit(adv[4, T - 1, 0])


def test_cpu_compute_gae_is_the_reference_bit_for_bit(golden):
    from hns_amd import gae
    g = golden("g_gae")
    for cid, T, K, E, Kd, (reward, done, value, nv) in _cases(g):
        for gi, (gamma, lmbda) in enumerate(g["pairs"]):
            adv, ret = gae.compute_gae(reward, done, value, nv, gamma=float(gamma), lmbda=float(lmbda))
            assert _bits_equal(adv, g[f"{cid}_g{gi}_adv"]) and _bits_equal(ret, g[f"{cid}_g{gi}_ret"]), (cid, gi)
            adv, ret = gae.compute_gae_(_tm(reward), _tm(done), _tm(value), nv, gamma=float(gamma), lmbda=float(lmbda))
            assert _bits_equal(adv, g[f"{cid}_g{gi}_adv_tm"]) and _bits_equal(ret, g[f"{cid}_g{gi}_ret_tm"]), (cid, gi)
        scale, shift = torch.from_numpy(g["dn_scale"]), torch.from_numpy(g["dn_shift"])
        gamma, lmbda = (float(x) for x in g["pairs"][1])
        adv, ret = gae.compute_gae(reward, done, value * scale + shift, nv * scale + shift, gamma=gamma, lmbda=lmbda)
        assert _bits_equal(adv, g[f"{cid}_dn_adv"]) and _bits_equal(ret, g[f"{cid}_dn_ret"]), cid


def _check_train_op(g, r, adv, ret, vn, what):
    p = f"r{r}_"
    np.testing.assert_allclose(adv, g[p + "adv_normalised"], rtol=2e-5, atol=2e-5, err_msg=what)
    np.testing.assert_allclose(ret, g[p + "ret_normalised"], rtol=2e-5, atol=2e-5, err_msg=what)
    np.testing.assert_allclose(vn.running_mean.cpu().numpy(), g[p + "running_mean"], rtol=2e-5, atol=1e-7, err_msg=what)
    np.testing.assert_allclose(vn.running_mean_sq.cpu().numpy(), g[p + "running_mean_sq"], rtol=2e-5, atol=1e-7, err_msg=what)
    np.testing.assert_allclose(float(vn.debiasing_term), float(g[p + "debiasing_term"]), rtol=1e-6, err_msg=what)


def _train_op_rollouts(g, device, done_key="dones"):
    E, T, A, R = (int(x) for x in g["train_meta"])
    for r in range(R):
        p = f"r{r}_"
        yield r, tuple(torch.from_numpy(g[p + n]).to(device) for n in ("reward", done_key, "value", "next_value"))


def test_cpu_rollout_targets_is_the_train_op_block(golden):
    from hns_amd import gae
    g = golden("g_gae")
    gamma, lmbda = (float(x) for x in g["train_gamma_lambda"])
    vn = _ValueNorm1(float(g["beta"]))
    for r, (reward, done, value, nv) in _train_op_rollouts(g, "cpu"):
        success = (torch.arange(reward.shape[0]) % 3 == 0).float()
        adv, ret, rate = gae.rollout_targets(reward, done, value, nv, gamma, lmbda, value_normalizer=vn, success=success)
        _check_train_op(g, r, adv.numpy(), ret.numpy(), vn, f"rollout {r}")
        assert abs(float(rate) - float(success.mean())) < 1e-12


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from hns_amd import abi
    ge.build()
    lib = abi.load_library()
    lib.hns_last_error.restype = ctypes.c_char_p
    return lib


def test_abi_refuses_bad_arguments_before_any_launch(lib):
    """Every refusal happens on the host (no device needed): HNS_ERR_INVALID_ARG and a message naming the argument."""
    from hns_amd import abi
    P = 4096                                  # a non-NULL address; nothing is launched for a refused call
    ok = dict(reward=P, value=P, done=P, nv=P, n=4, t=8, k=3, kd=1, layout=abi.HNS_GAE_BATCH_MAJOR, dd=abi.HNS_GAE_DONE_U8, g=0.99, l=0.95,
              scale=None, shift=None, success=None, m=0, adv=P, ret=P, mom=None, ws=None)

    def call(**kw):
        a = {**ok, **kw}
        return lib.hns_gae(a["reward"], a["value"], a["done"], a["nv"], a["n"], a["t"], a["k"], a["kd"], a["layout"], a["dd"], a["g"], a["l"],
                           a["scale"], a["shift"], a["success"], a["m"], a["adv"], a["ret"], a["mom"], a["ws"], None)

    for kw, msg in ((dict(reward=None), b"null"), (dict(adv=None), b"null"), (dict(done=None), b"null"), (dict(n=0), b">= 1"), (dict(t=0), b">= 1"),
                    (dict(k=-2), b">= 1"), (dict(kd=2), b"kd"), (dict(layout=2), b"layout"), (dict(dd=5), b"done_dtype"),
                    (dict(scale=P), b"scale"), (dict(m=3), b"success"), (dict(mom=P), b"workspace"), (dict(n=1 << 40), b"too large"),
                    (dict(g=float("nan")), b"gamma")):
        assert call(**kw) == abi.HNS_ERR_INVALID_ARG, kw
        assert msg in lib.hns_last_error(), (kw, lib.hns_last_error())
    assert lib.hns_rollout_normalise(None, 0, None, None, None, 0, None, None, None) == abi.HNS_ERR_INVALID_ARG
    assert lib.hns_rollout_normalise(P, 10, P, None, None, 0, None, None, None) == abi.HNS_ERR_INVALID_ARG
    assert lib.hns_rollout_normalise(None, 10, None, None, None, 10, P, P, None) == abi.HNS_ERR_INVALID_ARG
    assert b"returns" in lib.hns_last_error()


def test_new_kernels_have_no_spills_or_scratch(lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = [k for k in kernel_resources.all_kernels(os.path.join(ROOT, "build", "obj")) if k["object"] == "hns_gae.o"]
    names = {k["demangled"] for k in ks}
    for d in ("true", "false"):
        for m in ("true", "false"):
            assert f"hns_gae_staged_kernel<{d}, {m}>" in names and f"hns_gae_direct_kernel<{d}, {m}>" in names, names
    assert "hns_gae_moments_kernel" in names and "hns_rollout_normalise_kernel" in names, names
    for k in ks:
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hns_gae_is_the_reference_bit_for_bit(golden):
    """Both layouts, Kd = 1 and Kd = K, bool and fp32 dones, with and without ValueNorm1.denormalize folded in."""
    from hns_amd import gae
    g = golden("g_gae")
    scale, shift = torch.from_numpy(g["dn_scale"]).cuda(), torch.from_numpy(g["dn_shift"]).cuda()
    for cid, T, K, E, Kd, (reward, done, value, nv) in _cases(g):
        reward, done, value, nv = reward.cuda(), done.cuda(), value.cuda(), nv.cuda()
        for dn in (done, done.float()):
            for gi, (gamma, lmbda) in enumerate(g["pairs"]):
                gamma, lmbda = float(gamma), float(lmbda)
                adv, ret = gae.compute_gae(reward, dn, value, nv, gamma=gamma, lmbda=lmbda)
                assert _bits_equal(adv, g[f"{cid}_g{gi}_adv"]) and _bits_equal(ret, g[f"{cid}_g{gi}_ret"]), (cid, gi, dn.dtype)
                adv, ret = gae.compute_gae_(_tm(reward), _tm(dn), _tm(value), nv, gamma=gamma, lmbda=lmbda)
                assert _bits_equal(adv, g[f"{cid}_g{gi}_adv_tm"]) and _bits_equal(ret, g[f"{cid}_g{gi}_ret_tm"]), (cid, gi, dn.dtype)
            gamma, lmbda = (float(x) for x in g["pairs"][1])
            for tm in (False, True):
                args = (_tm(reward), _tm(dn), _tm(value)) if tm else (reward, dn, value)
                adv, ret, row = gae._launch_gae(*args, nv, gamma, lmbda, tm, scale, shift, moments=True)
                adv, ret = (_tm(adv), _tm(ret)) if tm else (adv, ret)
                assert _bits_equal(adv, g[f"{cid}_dn_adv"]) and _bits_equal(ret, g[f"{cid}_dn_ret"]), (cid, tm, dn.dtype)


def _row_np(adv, ret, success=None):
    a, r = adv.double().cpu().numpy().ravel(), ret.double().cpu().numpy().ravel()
    s = success.double().cpu().numpy() if success is not None else np.zeros(0)
    return np.array([a.sum(), (a * a).sum(), a.size, s.sum(), s.size, r.sum(), (r * r).sum(), r.size]), \
        np.array([np.abs(a).sum(), (a * a).sum(), 1, np.abs(s).sum(), 1, np.abs(r).sum(), (r * r).sum(), 1])


def _assert_row(row, adv, ret, success=None):
    ref, mag = _row_np(adv, ret, success)
    got = row.cpu().numpy()
    assert np.all(np.abs(got - ref) <= 1e-12 * mag), (got, ref)


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("E,T,K,Kd", [(2048, 64, 3, 1), (65536, 64, 3, 3), (65536, 64, 3, 1), (1, 64, 3, 1), (65, 65, 3, 3), (4097, 65, 3, 1),
                                      (65, 8, 7, 1), (3, 4200, 3, 1), (5, 2, 300, 300)])
def test_hns_gae_is_the_torch_loop_on_the_device(E, T, K, Kd):
    """At the sizes a user runs, ragged ones, and spans too large to stage (T K > 12 288 floats; K > 256 columns): the reference's loop on the same
    device, bit for bit, both layouts; the moment row against fp64 numpy (1e-12 of the magnitudes summed) and identical across two launches."""
    from hns_amd import gae
    gen = torch.Generator(device="cuda").manual_seed(E * 1000 + T + K)
    reward = torch.randn(E, T, K, device="cuda", generator=gen)
    value = torch.randn(E, T, K, device="cuda", generator=gen) * 3
    nv = torch.randn(E, K, device="cuda", generator=gen)
    done = torch.rand(E, T, Kd, device="cuda", generator=gen) < 0.02
    success = (torch.rand(E, device="cuda", generator=gen) < 0.3).float()
    for tm in (False, True):
        args = (_tm(reward), _tm(done), _tm(value)) if tm else (reward, done, value)
        ref = gae._torch_gae(*args, nv, 0.995, 0.95, tm)
        adv, ret, row = gae._launch_gae(*args, nv, 0.995, 0.95, tm, success=success, moments=True)
        assert _bits_equal(adv, ref[0]) and _bits_equal(ret, ref[1]), tm
        _assert_row(row, adv, ret, success)
        again = gae._launch_gae(*args, nv, 0.995, 0.95, tm, success=success, moments=True)[2]
        assert torch.equal(row, again)


@pytest.mark.gpu
def test_rollout_targets_on_the_device_is_the_train_op_block(golden):
    from hns_amd import gae
    g = golden("g_gae")
    gamma, lmbda = (float(x) for x in g["train_gamma_lambda"])
    for done_key in ("dones", "env_done"):                      # [E, T, A, 1] (Kd = K) and the broadcast env done [E, T, 1] -> [E, T, 1, 1]
        vn = _ValueNorm1(float(g["beta"]), device="cuda")
        for r, (reward, done, value, nv) in _train_op_rollouts(g, "cuda", done_key):
            if done.dim() == 3:
                done = done.unsqueeze(-1)
            success = (torch.arange(reward.shape[0], device="cuda") % 3 == 0).float()
            adv, ret, rate = gae.rollout_targets(reward, done, value, nv, gamma, lmbda, value_normalizer=vn, success=success)
            assert rate.is_cuda and rate.dim() == 0
            _check_train_op(g, r, adv.cpu().numpy(), ret.cpu().numpy(), vn, f"rollout {r} ({done_key})")
            assert abs(float(rate) - float(success.double().mean())) < 1e-12


@pytest.mark.gpu
def test_rollout_normalise_is_shardings_expression():
    """Given the same table: (adv - mean.f32) / (std.f32 + eps) as sharding.normalise_advantages forms it, and ValueNorm1.normalize's
    (ret - mean) / sqrt(var), bit for bit; either pair alone; a misaligned tail."""
    from hns_amd import gae, sharding
    gen = torch.Generator(device="cuda").manual_seed(7)
    adv = torch.randn(65536 * 64 * 3 + 3, device="cuda", generator=gen) * 4 + 1
    ret = torch.randn(65536 * 64 * 3 + 3, device="cuda", generator=gen) * 9 - 20
    table = sharding.allgather_moments(sharding.local_moments(adv, None, ret))
    mean, std = sharding.global_mean_std(table)
    mean, std = mean.to(torch.float32), std.to(torch.float32)
    want_a = (adv - mean) / (std + 1e-8)
    vn = _ValueNorm1(0.995, device="cuda")
    sharding.valuenorm1_update(vn, table)
    m, var = vn.running_mean_var()
    want_r = (ret - m) / torch.sqrt(var)
    a, r = adv.clone(), ret.clone()
    gae.rollout_normalise(a, r, mean, std + 1e-8, m, torch.sqrt(var))
    assert _bits_equal(a, want_a) and _bits_equal(r, want_r)
    a, r = adv[1:].clone(), ret[1:].clone()                     # not 16-byte aligned: the scalar path
    gae.rollout_normalise(a, r, mean, std + 1e-8, None, None)
    assert _bits_equal(a, want_a[1:]) and torch.equal(r, ret[1:])
    gae.rollout_normalise(a, r, None, None, m, torch.sqrt(var))
    assert _bits_equal(r, want_r[1:])


@pytest.mark.gpu
def test_split_rollout_rows_sum_to_the_whole():
    """Two halves of the env batch (two ranks' shards) give rows whose sum is the one-piece row to 1e-6."""
    from hns_amd import gae
    gen = torch.Generator(device="cuda").manual_seed(11)
    E, T, K = 4096, 64, 3
    reward, value = torch.randn(E, T, K, device="cuda", generator=gen), torch.randn(E, T, K, device="cuda", generator=gen)
    nv, done = torch.randn(E, K, device="cuda", generator=gen), torch.rand(E, T, 1, device="cuda", generator=gen) < 0.05
    success = (torch.rand(E, device="cuda", generator=gen) < 0.5).float()
    whole = gae._launch_gae(reward, done, value, nv, 0.99, 0.95, False, success=success, moments=True)[2]
    h = E // 2 + 17
    parts = [gae._launch_gae(reward[s].contiguous(), done[s].contiguous(), value[s].contiguous(), nv[s].contiguous(), 0.99, 0.95, False,
                             success=success[s].contiguous(), moments=True)[2] for s in (slice(0, h), slice(h, E))]
    np.testing.assert_allclose((parts[0] + parts[1]).cpu().numpy(), whole.cpu().numpy(), rtol=1e-6, atol=1e-6)


@pytest.mark.gpu
def test_compute_gae_replays_in_a_graph():
    from hns_amd import gae
    gen = torch.Generator(device="cuda").manual_seed(5)
    E, T, K = 2048, 64, 3
    reward, value = torch.randn(E, T, K, device="cuda", generator=gen), torch.randn(E, T, K, device="cuda", generator=gen)
    nv, done = torch.randn(E, K, device="cuda", generator=gen), torch.rand(E, T, 1, device="cuda", generator=gen) < 0.05
    eager = gae.compute_gae(reward, done, value, nv, 0.995, 0.95)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gae.compute_gae(reward, done, value, nv, 0.995, 0.95)          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = gae.compute_gae(reward, done, value, nv, 0.995, 0.95)
    for _ in range(2):
        out[0].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _bits_equal(out[0], eager[0]) and _bits_equal(out[1], eager[1])


@pytest.mark.gpu
def test_python_refuses_bad_tensors():
    from hns_amd import gae
    E, T, K = 8, 4, 3
    r, v, nv = torch.zeros(E, T, K, device="cuda"), torch.zeros(E, T, K, device="cuda"), torch.zeros(E, K, device="cuda")
    d = torch.zeros(E, T, 1, dtype=torch.bool, device="cuda")
    with pytest.raises(TypeError):
        gae.compute_gae(r.double(), d, v.double(), nv.double())
    with pytest.raises(TypeError):
        gae.compute_gae(r, d.int(), v, nv)
    with pytest.raises(ValueError):
        gae.compute_gae(r, d, v[:, :3], nv)
    with pytest.raises(ValueError):
        gae.compute_gae(r, torch.zeros(E, T, 2, dtype=torch.bool, device="cuda"), v, nv)
    with pytest.raises(ValueError):
        gae.compute_gae(r, d, v, nv[:4])
    with pytest.raises(ValueError):
        gae.compute_gae(r, d.squeeze(-1), v, nv)
