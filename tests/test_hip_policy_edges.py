"""hns_policy_forward (through hns_amd.policy.DevicePolicy and through the C ABI) at its shape, stride and mode edges on an MI355X.

The accuracy rule is test_hip_policy.py's (BAR = 8): per output, e_hip <= 8 max(e_32, 2^-24 max|ref_64|), errors as max-abs against the fp64
restatement of tests/policy_reference.py, e_32 the error of the same statements in CPU torch fp32.  Every device output is asserted finite
first and no row is left out of a comparison.  tests/test_policy_net.py shows on the CPU that this gate, on these cases, fails for each of
eight seeded defects of an fp32 emulation of the kernel.

  1. Shape limits (A = 1, 2, 7; K = 1, 16; D = 1, 96; 1, 31, 32 and 33 rows; one env) and a seeded sweep over A, K, D and every residue of
     the row count modulo the kernel's 32-row tile, each in all three call forms (sampling with eps, deterministic, value only): loc and
     value bit-identical across the forms, the sampled and the deterministic outputs through the gate.
  2. Observations as views into NaN-filled parents (wider rows, extra agents and token slots, storage offsets, [N, T, A, ..] parents cut at
     one t, a stride-0 agent dimension): the bits of the contiguous copy, so nothing outside the logical elements is read.  Output buffers
     with 64 guard rows: nothing past `rows` is written; value-only leaves action / log_prob / loc untouched; loc is optional.
  3. The noise contract of include/hns.h restated on the host (policy_reference.philox_normal): per element for four seeds x four counters
     (both halves of each word matter), per component and agent slot moments at 65 536 envs, consecutive calls.
  5. The collector's log_prob and value fed to the learner's kernels on unchanged parameters: ratios of 1 to rounding.

Worst ratios per case: printed by test_report_ratios (RATIOS).  They have not been recorded from an MI355X run yet (the CPU emulation of the
kernel's algorithm reaches 1.38 of 8 on the shape limits; the kernel's known worst elsewhere is 3.86, flat_tokens); the bar is not tuned to
them."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import policy_reference as R
from hns_amd import abi
from hns_amd import actor_train as AT
from hns_amd import critic_train as CT
from hns_amd import policy as P

pytestmark = pytest.mark.gpu

BAR = R.BAR
RATIOS = {}
SEEDS = list(range(int(os.environ.get("HNS_FUZZ_POLICY_SEEDS", 40))))      # HNS_FUZZ_POLICY_SEEDS=2000: the occasional deep run
DEFAULT_SEEDS = 40
TILE = 32                                                                   # kEncRows of csrc/hns_encoder.h


def _dev(d):
    return {k: torch.as_tensor(np.asarray(v)).cuda() for k, v in d.items()}


def _obs_dev(obs):
    return (torch.as_tensor(obs["state_self"]).cuda(), torch.as_tensor(obs["state_others"]).cuda() if "state_others" in obs else None,
            torch.as_tensor(obs["cylinders"]).cuda())


def _np(t):
    return t.cpu().double().numpy()


def _check(tag, form, got, r64, r32):
    ratios = R.gate_ratios(got, r64, r32)
    print(f"  {tag} {form}: " + " ".join(f"{n} {v:.2f}" for n, v in ratios.items()))
    for n, v in ratios.items():
        assert v <= BAR, f"{tag} {form} {n}: ratio {v:.2f} > {BAR}"
    return max(ratios.values())


def three_forms(tag, actor, critic, obs, eps, record=True):
    """Sampling with eps, deterministic and value-only on one policy: loc and value bit-identical across the forms (the same instruction
    stream on the same rows), the sampled and the deterministic outputs through the fp64 gate (the deterministic log_prob against the
    restatement's log-probability at the mode)."""
    pol = P.DevicePolicy(_dev(actor), _dev(critic))
    x = _obs_dev(obs)
    E, A = obs["state_self"].shape[:2]
    s = pol.forward(*x, eps=torch.as_tensor(eps).cuda())
    d = pol.forward(*x, deterministic=True)
    v = pol.forward(*x, value_only=True)
    torch.cuda.synchronize()
    assert v.action is None and v.log_prob is None and v.loc is None
    for o in (s, d):
        assert o.action.shape == (E, A, 4) and o.loc.shape == (E, A, 4) and o.log_prob.shape == (E, A, 1) and o.value.shape == (E, A, 1)
    assert torch.equal(s.loc, d.loc) and torch.equal(d.action, d.loc), tag
    assert torch.equal(s.value, d.value) and torch.equal(s.value, v.value), tag
    worst = _check(tag, "sampled", [_np(s.loc), _np(s.log_prob), _np(s.value)], R.reference_outputs(actor, critic, obs, eps, torch.float64),
                   R.reference_outputs(actor, critic, obs, eps, torch.float32))
    worst = max(worst, _check(tag, "mode", [_np(d.loc), _np(d.log_prob), _np(d.value)], R.reference_outputs(actor, critic, obs, None, torch.float64),
                              R.reference_outputs(actor, critic, obs, None, torch.float32)))
    if record:
        RATIOS[tag] = round(worst, 2)
    return worst


# ---- 1. shape limits and the seeded sweep ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.LIMIT_SHAPES, ids=[R.limit_tag(s) for s in R.LIMIT_SHAPES])
def test_shape_limits(shape):
    """One value at its limit per case (policy_reference.LIMIT_SHAPES, the cases of the CPU defect table): A = 1, 2 and 7, K = 1 and 16,
    self_dim 1 and 96, row counts 1, 31, 32 and 33 around the 32-row tile, one env."""
    three_forms(R.limit_tag(shape), *R.limit_case(shape))


def draw_case(seed):
    """(A, K, D, E) of a sweep seed: A in 1..7, K in 1..16, D in 1..96, and E such that E A = seed (mod 32), so that the default seeds
    leave every number of padding rows in the last tile; E A <= 8 192.  A is redrawn while gcd(A, 32) does not divide the residue."""
    r = np.random.RandomState(7000 + seed)
    want = seed % TILE
    while True:
        A = int(r.randint(1, 8))
        if want % math.gcd(A, TILE) == 0:
            break
    K, D = int(r.randint(1, 17)), int(r.randint(1, 97))
    step = TILE // math.gcd(A, TILE)
    e0 = next(e for e in range(1, TILE + 1) if (e * A) % TILE == want)
    rows_max = int(r.choice([48, 200, 1000, 8192]))
    E = e0 + step * int(r.randint(0, max(0, (rows_max // A - e0) // step) + 1))
    assert E >= 1 and E * A <= 8192 and (E * A) % TILE == want
    return A, K, D, E


def test_the_default_sweep_leaves_every_tail_length():
    """From the seeds alone: over the default seeds E A mod 32 takes every residue, every A occurs, K and D span most of their ranges (their
    ends are test_shape_limits') and the batch sizes reach past 2 048 rows."""
    cases = [draw_case(s) for s in range(DEFAULT_SEEDS)]
    assert {(E * A) % TILE for A, K, D, E in cases} == set(range(TILE))
    assert {A for A, _, _, _ in cases} == set(range(1, 8))
    assert min(K for _, K, _, _ in cases) <= 2 and max(K for _, K, _, _ in cases) == 16
    assert min(D for _, _, D, _ in cases) <= 4 and max(D for _, _, D, _ in cases) >= 85
    assert max(E * A for A, _, _, E in cases) > 2048


@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_shape_sweep(seed):
    A, K, D, E = draw_case(seed)
    actor, critic = R.random_net(D, A, 9000 + seed)
    obs, eps = R.random_obs(E, A, K, D, 9500 + seed)
    w = three_forms(f"sweep{seed}-a{A}k{K}d{D}e{E}", actor, critic, obs, eps, record=False)
    RATIOS["sweep (worst)"] = max(RATIOS.get("sweep (worst)", 0.0), round(w, 2))


# ---- 2. strided views and guarded outputs ---------------------------------------------------------------------------------------------
PATTERN = 0x5CA1AB1E                             # the guard rows' bit pattern (a finite float: a stray read of it would not hide as NaN)
GUARD = 64


def _case(A, K, D, E, seed):
    actor, critic = R.random_net(D, A, seed)
    obs, eps = R.random_obs(E, A, K, D, seed + 1)
    return P.DevicePolicy(_dev(actor), _dev(critic), seed=seed), obs, eps


def _embed(x, t_total, t, pre, post, offset):
    """x [E, A, (n,) w] as a view into a NaN-filled [E, T, A + .., (n + ..,) w + ..] parent cut at step t, behind a storage offset: every
    dimension of the parent is larger than the view's (`pre` / `post` elements before / after), so no stride is the product of the inner
    extents, and every element that is not x's is NaN."""
    E = x.shape[0]
    shape = (E, t_total) + tuple(p + s + q for p, s, q in zip(pre, x.shape[1:], post))
    flat = torch.full((offset + int(np.prod(shape)),), float("nan"), device="cuda")
    parent = flat[offset:].view(shape)
    view = parent[:, t]
    for dim, (p, s) in enumerate(zip(pre, x.shape[1:]), start=1):
        view = view.narrow(dim, p, s)
    view.copy_(x)
    assert not view.is_contiguous() and view.stride(-1) == 1 and view.storage_offset() > 0
    assert int(torch.isnan(flat).sum()) == flat.numel() - x.numel()
    return view


def _equal_outputs(a, b, names=("action", "log_prob", "value", "loc")):
    for n in names:
        x, y = getattr(a, n), getattr(b, n)
        assert torch.isfinite(x).all(), n
        assert torch.equal(x, y), n


@pytest.mark.parametrize("shape", [(3, 5, 35, 11), (1, 5, 20, 37), (7, 16, 96, 9), (2, 1, 1, 40)])
def test_views_into_nan_filled_parents_give_the_bits_of_their_contiguous_copies(shape):
    """A read outside the logical elements would turn an output into NaN (nothing here can fault: every parent is larger than its view)."""
    A, K, D, E = shape
    pol, obs, eps = _case(A, K, D, E, 1200 + A)
    xs, xo, xc = _obs_dev(obs)
    e = torch.as_tensor(eps).cuda()
    want = pol.forward(xs, xo, xc, eps=e)
    vs = _embed(xs, 3, 1, (1, 0, 2), (1, 0, 1), 5)                      # [E, A, 1, D] in [E, 3, A + 2, 1, D + 3]
    vo = _embed(xo, 3, 1, (1, 1, 1), (1, 1, 0), 3) if xo is not None else None   # [E, A, A - 1, 3] in [E, 3, A + 2, A + 1, 4]
    vc = _embed(xc, 4, 2, (2, 2, 1), (0, 1, 1), 7)                      # [E, A, K, 5] in [E, 4, A + 2, K + 3, 7]
    assert vs.stride(0) != A * vs.stride(1) and vc.stride(1) != K * vc.stride(2)
    got = pol.forward(vs, vo, vc, eps=e)
    _equal_outputs(got, want)
    _equal_outputs(pol.forward(vs.contiguous(), vo.contiguous() if vo is not None else None, vc.contiguous(), eps=e), want)
    assert torch.equal(pol.forward(vs, vo, vc, value_only=True).value, want.value)
    _equal_outputs(pol.forward(vs, vo, vc, deterministic=True), pol.forward(xs, xo, xc, deterministic=True))
    # one view at a time beside contiguous others
    _equal_outputs(pol.forward(vs, xo, xc, eps=e), want)
    _equal_outputs(pol.forward(xs, xo, vc, eps=e), want)
    if xo is not None:
        _equal_outputs(pol.forward(xs, vo, xc, eps=e), want)
    # [E, A, 1, D] and [E, A, D] forms of state_self, contiguous and as the view
    _equal_outputs(pol.forward(xs.squeeze(2), xo, xc, eps=e), want)
    _equal_outputs(pol.forward(vs.squeeze(2), vo, vc, eps=e), want)
    # eps as a non-contiguous view
    wide = torch.full((E, A, 9), float("nan"), device="cuda")
    wide[..., 2:6] = e
    assert not wide[..., 2:6].is_contiguous()
    _equal_outputs(pol.forward(xs, xo, xc, eps=wide[..., 2:6]), want)
    _equal_outputs(pol.forward(vs, vo, vc, eps=torch.stack([e, e], dim=1)[:, 1]), want)


def test_a_stride_0_agent_dimension_is_read_as_its_expansion():
    """The ABI accepts strides >= 0: every agent of an env reads the same state_self / cylinders rows (expand), inside NaN-filled parents."""
    A, K, D, E = 3, 5, 35, 11
    pol, obs, eps = _case(A, K, D, E, 1300)
    xs, xo, xc = _obs_dev(obs)
    e = torch.as_tensor(eps).cuda()
    vs = _embed(xs[:, :1], 2, 1, (1, 0, 1), (1, 0, 2), 3).expand(E, A, 1, D)
    vo = _embed(xo[:, :1], 2, 0, (0, 1, 0), (1, 0, 1), 1).expand(E, A, A - 1, 3)
    vc = _embed(xc[:, :1], 2, 1, (1, 1, 1), (0, 2, 1), 9).expand(E, A, K, 5)
    assert vs.stride(1) == 0 and vo.stride(1) == 0 and vc.stride(1) == 0
    want = pol.forward(vs.contiguous(), vo.contiguous(), vc.contiguous(), eps=e)
    _equal_outputs(pol.forward(vs, vo, vc, eps=e), want)
    assert torch.equal(want.loc[:, 0], want.loc[:, 1]) and torch.equal(want.value[:, 0], want.value[:, 2])     # the rows are the same row
    assert not torch.equal(want.loc[0], want.loc[1])
    # a stride-0 env dimension beside it
    v0 = xs[:1].expand(E, A, 1, D)
    _equal_outputs(pol.forward(v0, xo, xc, eps=e), pol.forward(v0.contiguous(), xo, xc, eps=e))


class _Out:
    """Output buffers of rows + GUARD rows, every word PATTERN."""

    def __init__(self, rows):
        self.rows = rows
        mk = lambda n: torch.full(((rows + GUARD) * n,), PATTERN, dtype=torch.int32, device="cuda")
        self.action, self.loc, self.log_prob, self.value = mk(4), mk(4), mk(1), mk(1)

    def get(self, name):
        t = getattr(self, name)
        return t.view(torch.float32)[:self.rows * (t.numel() // (self.rows + GUARD))]

    def untouched(self, name, start=None):
        t = getattr(self, name)
        n = t.numel() // (self.rows + GUARD)
        return bool((t[(self.rows if start is None else start) * n:] == PATTERN).all())


def _abi_forward(pol, xs, xo, xc, out, eps=None, flags=0, loc=True, only_value=False):
    """lib.hns_policy_forward on contiguous observations with the caller's output buffers."""
    pol.refresh()
    E, A, K = xs.shape[0], xs.shape[1], xc.shape[2]
    xs = xs.reshape(E, A, -1)
    io = abi.HnsPolicyIo()
    io.obs_self, io.obs_cylinders, io.obs_others = xs.data_ptr(), xc.data_ptr(), (xo.data_ptr() if xo is not None else None)
    io.self_stride[:] = [xs.stride(0), xs.stride(1)]
    io.others_stride[:] = [xo.stride(0), xo.stride(1), xo.stride(2)] if xo is not None else [0, 0, 0]
    io.cyl_stride[:] = [xc.stride(0), xc.stride(1), xc.stride(2)]
    io.eps = eps.data_ptr() if eps is not None else None
    io.value = out.value.data_ptr()
    if not only_value:
        io.action, io.log_prob = out.action.data_ptr(), out.log_prob.data_ptr()
        io.loc = out.loc.data_ptr() if loc else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = pol._lib.hns_policy_forward(pol.packed.data_ptr(), pol.self_dim, E, A, K, C.byref(io), flags, pol.seed, pol.counter.data_ptr(), st)
    assert rc == abi.HNS_OK, pol._lib.hns_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", [(1, 5, 20, 1), (3, 5, 35, 11), (7, 5, 20, 9), (2, 8, 20, 16), (3, 16, 24, 37), (1, 5, 20, 31)])
@pytest.mark.parametrize("flags", [0, abi.HNS_POLICY_DETERMINISTIC])
def test_nothing_is_written_past_the_last_row(shape, flags):
    """1, 33, 63, 32, 111 and 31 rows: the padding rows of the last tile write nothing (64 guard rows behind every output keep their bits),
    and the rows themselves are DevicePolicy.forward's."""
    A, K, D, E = shape
    pol, obs, eps = _case(A, K, D, E, 1400 + A + K)
    xs, xo, xc = _obs_dev(obs)
    e = torch.as_tensor(eps).cuda()
    det = bool(flags & abi.HNS_POLICY_DETERMINISTIC)
    want = pol.forward(xs, xo, xc, eps=None if det else e, deterministic=det)
    out = _Out(E * A)
    _abi_forward(pol, xs, xo, xc, out, eps=None if det else e, flags=flags)
    for n in ("action", "loc", "log_prob", "value"):
        assert out.untouched(n), n
        got = out.get(n)
        assert torch.isfinite(got).all() and torch.equal(got, getattr(want, n).reshape(-1)), n
    # io.loc = NULL: the call succeeds, action and log_prob are those of the call that had it, the loc buffer keeps its bits
    nol = _Out(E * A)
    _abi_forward(pol, xs, xo, xc, nol, eps=None if det else e, flags=flags, loc=False)
    assert nol.untouched("loc", 0)
    for n in ("action", "log_prob", "value"):
        assert nol.untouched(n) and torch.equal(nol.get(n), out.get(n)), n


@pytest.mark.parametrize("shape", [(3, 5, 35, 11), (1, 5, 20, 31), (7, 5, 20, 9)])
def test_value_only_leaves_action_log_prob_and_loc_untouched(shape):
    """HNS_POLICY_VALUE_ONLY with non-NULL action / log_prob / loc buffers (include/hns.h: "untouched"), alone and beside the
    deterministic flag, and with those pointers NULL."""
    A, K, D, E = shape
    pol, obs, _ = _case(A, K, D, E, 1500 + A)
    xs, xo, xc = _obs_dev(obs)
    want = pol.forward(xs, xo, xc, value_only=True).value.reshape(-1)
    for flags in (abi.HNS_POLICY_VALUE_ONLY, abi.HNS_POLICY_VALUE_ONLY | abi.HNS_POLICY_DETERMINISTIC):
        out = _Out(E * A)
        _abi_forward(pol, xs, xo, xc, out, flags=flags)
        for n in ("action", "log_prob", "loc"):
            assert out.untouched(n, 0), n
        assert out.untouched("value") and torch.isfinite(out.get("value")).all() and torch.equal(out.get("value"), want)
    c0 = int(pol.counter)
    out = _Out(E * A)
    _abi_forward(pol, xs, xo, xc, out, flags=abi.HNS_POLICY_VALUE_ONLY, only_value=True)
    assert torch.equal(out.get("value"), want) and int(pol.counter) == c0           # no noise drawn: the call counter stays


# ---- 3. the noise contract ------------------------------------------------------------------------------------------------------------
NOISE_SEEDS = [0, 5, 2 ** 32 + 5, 2 ** 63 + 1]
NOISE_COUNTERS = [0, 1, 2 ** 32, 2 ** 32 + 1]


def _noise(pol, x):
    """z = (action - loc) / scale in fp64 from the device's fp32 outputs, and the per-element allowance for the two roundings of
    loc + scale eps: 2^-23 (|loc| + |action|) / scale."""
    out = pol.forward(*x)
    loc, act, sc = _np(out.loc), _np(out.action), _np(pol.scale)
    assert np.isfinite(act).all() and np.isfinite(loc).all()
    return ((act - loc) / sc).reshape(-1, 4), (2.0 ** -23 * (np.abs(loc) + np.abs(act)) / sc).reshape(-1, 4)


def _noise_ratio(z, slack, seed, counter):
    """Worst |z - eps_64| / (8 max(e_32, 2^-24 max|eps_64|) + slack) over the elements; e_32 the fp32 restatement's error."""
    e64, e32 = R.philox_normal(seed, counter, z.shape[0]), R.philox_normal(seed, counter, z.shape[0], np.float32)
    bound = BAR * max(float(np.abs(e32 - e64).max()), 2.0 ** -24 * float(np.abs(e64).max())) + slack
    return float((np.abs(z - e64) / bound).max())


@pytest.mark.parametrize("A", [1, 3])
def test_the_noise_is_philox_keyed_by_the_whole_seed_and_counted_by_the_whole_counter_and_row(A):
    """include/hns.h: "the noise of row r is Philox4x32-10 with key `seed` and counter (*counter, r)".  37 envs (37 or 111 rows: a tail),
    four seeds x four counters with bits in the low and the high word of each, every element against the host restatement.  A kernel that
    dropped the high half of the seed or of the counter, keyed by row / 4 or reused a pair for two components would fail it.
    The worst ratio to the bound (1 = at the bound) is recorded in RATIOS."""
    pol, obs, _ = _case(A, 5, 20, 37, 1600 + A)
    x = _obs_dev(obs)
    worst, seen = 0.0, {}
    for seed in NOISE_SEEDS:
        pol.seed = seed
        for counter in NOISE_COUNTERS:
            pol.counter.fill_(counter)
            z, slack = _noise(pol, x)
            assert int(pol.counter) == counter + 1
            r = _noise_ratio(z, slack, seed, counter)
            assert r <= 1.0, f"seed {seed} counter {counter}: {r:.2f} of the bound"
            worst = max(worst, r)
            seen[(seed, counter)] = z
    keys = list(seen)
    for i, a in enumerate(keys):                                # all sixteen streams differ, 5 and 2^32 + 5 and 0 and 2^32 among them
        for b in keys[i + 1:]:
            assert np.abs(seen[a] - seen[b]).max() > 0.5, (a, b)
    assert np.abs(seen[(5, 0)] - seen[(2 ** 32 + 5, 0)]).max() > 0.5
    RATIOS[f"noise a{A} (of its bound)"] = round(worst, 2)


def test_consecutive_calls_count_the_counter_up_by_one():
    """Row r of call c + 1 is the restatement at counter c + 1 (not merely different from call c), across the 2^32 carry."""
    pol, obs, _ = _case(3, 5, 20, 37, 1700)
    pol.seed = 2 ** 40 + 17
    x = _obs_dev(obs)
    start = 2 ** 32 - 2
    pol.counter.fill_(start)
    for k in range(4):
        z, slack = _noise(pol, x)
        assert int(pol.counter) == start + k + 1
        assert _noise_ratio(z, slack, pol.seed, start + k) <= 1.0, k
    pol.forward(*x, deterministic=True), pol.forward(*x, value_only=True), pol.forward(*x, eps=torch.zeros(37, 3, 4, device="cuda"))
    assert int(pol.counter) == start + 4                        # only a call that draws noise bumps it


def test_moments_per_component_and_agent_slot_at_65536_envs():
    """Mean and standard deviation of z for each of the 4 components in each of the 3 agent slots, n = 65 536 draws each: the mean of n
    standard normals has standard deviation 1 / sqrt(n) and their sample standard deviation 1 / sqrt(2 n); both are held to 5 of those
    (two-sided 5.7e-7 each, 24 checks).  The pairs of one row are uncorrelated within 5 / sqrt(n) as well (the product of two independent
    standard normals has variance 1)."""
    n = 65536
    actor, critic = R.random_net(20, 3, 31)
    pol = P.DevicePolicy(_dev(actor), _dev(critic), seed=2024)
    obs, _ = R.random_obs(n, 3, 5, 20, 32)
    z, _ = _noise(pol, _obs_dev(obs))
    z = z.reshape(n, 3, 4)
    for a in range(3):
        for c in range(4):
            v = z[:, a, c]
            assert abs(v.mean()) <= 5.0 / math.sqrt(n), (a, c, v.mean())
            assert abs(v.std() - 1.0) <= 5.0 / math.sqrt(2 * n), (a, c, v.std())
        for c, d in ((0, 1), (2, 3), (0, 2), (1, 3)):
            assert abs((z[:, a, c] * z[:, a, d]).mean()) <= 5.0 / math.sqrt(n), (a, c, d)
    for a, b in ((0, 1), (1, 2)):                               # neighbouring rows: another counter word, independent draws
        assert abs((z[:, a, 0] * z[:, b, 0]).mean()) <= 5.0 / math.sqrt(n)


# ---- 5. the collector's outputs into the learner --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 5, 35, 203), (6, 16, 24, 203)])
def test_the_learner_recomputes_the_collectors_log_prob_and_value(shape):
    """The collector writes action_logp and state_value with hns_policy_forward (fp32 sum, this file's kernel); the first PPO epoch
    recomputes them on unchanged parameters with hns_actor_train_grad (fp64 sum) and hns_critic_train_grad.  609 and 1 218 rows (tails of 1
    and 2).  Each kernel is gated against the same fp64 number with b = 8 max(e_32, 2^-24 max|ref_64|) (ref: R.forward at the collector's
    action), so per row |log_probs - log_prob| <= 2 b, and likewise for the values.  Then every ratio exp(d) is inside the clip, and the
    learner's ESS = (sum_i e^{r_i})^2 / (n sum_i e^{2 r_i}) (mappo.py's statement, r_i the ratios) is within 4 h + 2^-22 of 1 with
    h = e^{2 b} - 1: with every r_i in [1 - h, 1 + h] the numerator is at least n^2 e^{2 - 2 h} and the denominator at most n^2 e^{2 + 2 h},
    so ESS >= e^{-4 h} >= 1 - 4 h, ESS <= 1 by Cauchy-Schwarz, and 2^-22 is the allowance test_hip_actor_train.py gives the fp32 scalar when
    the ratios are exactly 1."""
    A, K, D, E = shape
    assert (E * A) % TILE
    actor, critic = R.random_net(D, A, 1800 + A)
    obs, _ = R.random_obs(E, A, K, D, 1801 + A)
    a_dev, c_dev = _dev(actor), _dev(critic)
    pol = P.DevicePolicy(a_dev, c_dev, seed=77)
    xs, xo, xc = _obs_dev(obs)
    fwd = pol.forward(xs, xo, xc)
    act = fwd.action.cpu().numpy()
    _, _, _, l64, v64 = R.forward(actor, critic, obs, action=act, dtype=torch.float64)
    _, _, _, l32, v32 = R.forward(actor, critic, obs, action=act, dtype=torch.float32)
    bound = lambda r64, r32: BAR * max(float((r32.double() - r64).abs().max()), 2.0 ** -24 * float(r64.abs().max()))
    b_lp, b_v = bound(l64, l32), bound(v64, v32)
    for t in (fwd.action, fwd.log_prob, fwd.value):
        assert torch.isfinite(t).all()
    assert np.abs(_np(fwd.log_prob) - l64.numpy()).max() <= b_lp and np.abs(_np(fwd.value) - v64.numpy()).max() <= b_v
    g = torch.Generator().manual_seed(5)
    adv = torch.randn(E, A, 1, generator=g).cuda()
    out = AT.policy_loss_and_grad(a_dev, xs, xo, xc, fwd.action, fwd.log_prob, adv)
    torch.cuda.synchronize()
    assert out.log_probs.shape == fwd.log_prob.shape and torch.isfinite(out.log_probs).all()
    d = _np(out.log_probs) - _np(fwd.log_prob)
    print(f"  a{A}k{K}d{D}: max |log_probs - log_prob| {np.abs(d).max():.3e} of 2 b = {2 * b_lp:.3e}; ESS - 1 = {float(out.ess) - 1:.3e}")
    assert np.abs(d).max() <= 2 * b_lp
    assert np.abs(_np(out.log_probs) - l64.numpy()).max() <= b_lp
    ratio = np.exp(d)
    assert ratio.min() > 0.9 and ratio.max() < 1.1
    h = math.exp(2 * b_lp) - 1.0
    assert abs(float(out.ess) - 1.0) <= 4 * h + 2.0 ** -22
    ret = torch.randn(E, A, 1, generator=g).cuda()
    vout = CT.value_loss_and_grad(c_dev, xs, xo, xc, fwd.value, ret)
    torch.cuda.synchronize()
    assert vout.values.shape == fwd.value.shape and torch.isfinite(vout.values).all()
    dv = np.abs(_np(vout.values) - _np(fwd.value)).max()
    print(f"  a{A}k{K}d{D}: max |values - value| {dv:.3e} of 2 b = {2 * b_v:.3e}")
    assert dv <= 2 * b_v
    RATIOS[f"learner a{A}k{K}d{D} (log_prob, value; of 2 b)"] = (round(float(np.abs(d).max() / (2 * b_lp)), 2), round(float(dv / (2 * b_v)), 2))
    # the parameters did not move: the next forward pass and DevicePolicy.value give the same bits
    td = {("agents", "observation"): {"state_self": xs, "state_others": xo, "cylinders": xc}}
    assert torch.equal(pol.value(td), fwd.value)
    assert torch.equal(pol.forward(xs, xo, xc, value_only=True).value, fwd.value)
    assert torch.equal(pol.forward(xs, xo, xc, eps=torch.zeros(E, A, 4, device="cuda")).value, fwd.value)


def test_report_ratios():
    print("policy edge ratios:", RATIOS)
