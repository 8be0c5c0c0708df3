"""Shared by test_central_edges.py (CPU) and test_hip_central_edges.py (GPU): the centralised critic's update past one row range of the
weight-gradient kernel and at its edges — the network builder with the three knobs of the numerical edges, ct_plan's central
branch restated from its constants, every update case of the GPU file as numpy with its fp64 / fp32 yardsticks (computed once, never
changed), and the conditions a case must meet on those yardsticks before anything runs on a device.  Imports nothing that needs a GPU."""
import collections
import functools

import numpy as np
import torch

import central_reference as CR


def critic(D, A, seed, weight_scale=1.0, embed_scale=1.0, flat_bias=False):
    """central_reference.random_critic with the three knobs of test_hip_critic_train._net, by its statements: in_proj_weight x weight_scale,
    the embedding weights x embed_scale, flat_bias: the embedding biases 0.3 + linspace(0, 1e-3).  The defaults leave random_critic's bits."""
    c = CR.random_critic(D, A, seed)
    for k in c:
        if "in_proj_weight" in k and weight_scale != 1.0:
            c[k] = (c[k] * np.float32(weight_scale)).astype(np.float32)
        if "split_embed.embed" in k and k.endswith("weight") and embed_scale != 1.0:
            c[k] = (c[k] * np.float32(embed_scale)).astype(np.float32)
        if flat_bias and "split_embed.embed" in k and k.endswith("bias"):
            c[k] = (np.full_like(c[k], 0.3) + np.linspace(0, 1e-3, c[k].size, dtype=np.float32)).astype(np.float32)
    return c


# ---------------------------------------------------------------------------------------------------------------- the plan
# csrc/hns_policy_train.hip restated: kCtRows, kCtMaxSplits, kCtE, kCtMat, kCtGemmOut, kCtMaxBlocks, I_EW, O_EWS, HNS_MAX_AGENTS
ROWS, MAX_SPLITS, E, MAX_BLOCKS, MAX_AGENTS = 32, 48, 128, 4096, 7
MAT, I_EW, O_EWS = E * E, 12 * E * E, 1280 + 3 * E + 5 * E + 4
GEMM_OUT = MAT + E


def central_plan(steps):
    """ct_plan(central = true) for a minibatch of `steps` env-steps: (tiles of 32 env-steps, tiles per row range of the weight-gradient kernel,
    row ranges, tiles in the last range, live rows of the last tile)."""
    tiles = -(-steps // ROWS)
    tps = -(-tiles // MAX_SPLITS)
    ranges = -(-tiles // tps)
    return tiles, tps, ranges, tiles - (ranges - 1) * tps, steps - (tiles - 1) * ROWS


def central_workspace_bytes(steps, D, A, K):
    """hns_critic_train_central_workspace_bytes(steps, D, A, K): the plan's sum of 256-byte aligned arrays — the control floats, five fp64 loss
    partials per tile, the reduce kernel's per-block sums, the packed image, two partial rows (ct_partial_central) per tile, six
    weight-gradient partials per row range, twelve staged operand arrays of 32 rows per tile."""
    up = lambda v: (v + 255) & ~255                                                 # noqa: E731
    tiles, _, ranges, _, _ = central_plan(steps)
    P = O_EWS + D * E + (MAX_AGENTS - 1) * E + 8                                    # ct_partial_central(D)
    img = I_EW + (D + 8) * E                                                        # ct_img_floats(D)
    return (up(64 * 4) + up(tiles * 5 * 8) + up(MAX_BLOCKS * 8) + up(img * 4) + up(tiles * 2 * P * 4) + up(ranges * 6 * GEMM_OUT * 4) +
            up(12 * tiles * ROWS * E * 4))


# (A, K, D, env-steps of the minibatch) -> (tiles, tps, row ranges, tiles in the last range, live rows of the last tile)
PLANS = {
    (3, 5, 35, 1537): (49, 2, 25, 1, 1),           # first tps = 2: the last range is ONE tile with ONE live row
    (7, 16, 96, 1537): (49, 2, 25, 1, 1),          # the limits; read through an index whose last entry is dead: the last range has no live row
    (1, 5, 20, 3073): (97, 3, 33, 1, 1),           # tps = 3, one agent: the obs critic's bits
}

# ---------------------------------------------------------------------------------------------------------------- the cases
# critic, state_drones [S, A, D], cylinders [S, K, 5], b_values / b_returns [S, A, 1], index (int64 [B] or None), loss_and_grad's keywords,
# layout ((N, T) with N T = S, or None: flat)
Case = collections.namedtuple("Case", ["critic", "sd", "cyl", "bv", "ret", "index", "kw", "layout"])


def _plain(A, K, D, S, shift=None, tseed=102, **kw):
    """test_hip_critic_central._case's construction: random_critic(D, A, 100 + A + K), random_state(.., 101), targets(.., 102)."""
    c = critic(D, A, 100 + A + K)
    sd, cyl = CR.random_state(S, A, K, D, 101)
    bv, ret = CR.targets(c, sd, cyl, tseed, shift=shift)
    return Case(c, sd, cyl, bv, ret, None, kw, None)


def _limits_through_a_dead_index():
    """(7, 16, 96): 1 537 positions of a [40, 40] rollout through a permuted index; position 0 is -1, position 768 is 2^40, position 1 536 —
    the one live row of the last tile, which is the whole last row range — is 1 600, one past the rollout."""
    c = _plain(7, 16, 96, 1600, shift=0.3)
    index = np.random.default_rng(5).permutation(1600)[:1537].astype(np.int64)
    index[0], index[768], index[1536] = -1, 2 ** 40, 1600
    return c._replace(index=index, layout=(40, 40))


def _edge(mode):
    """test_hip_critic_train.test_numerical_edges_pass_the_fp64_gate's constructions on the centralised critic at (3, 8, 20): 700 of 1 024
    env-steps through an index; large_obs: the state's magnitudes x 300."""
    seed, net = {"flat_tokens": (21, dict(embed_scale=1e-4, flat_bias=True)), "saturated_softmax": (22, dict(weight_scale=40.0)),
                 "large_obs": (23, {})}[mode]
    c = critic(20, 3, seed, **net)
    sd, cyl = CR.random_state(1024, 3, 8, 20, seed + 1)
    if mode == "large_obs":
        sd, cyl = (sd * np.float32(300.0)).astype(np.float32), (cyl * np.float32(300.0)).astype(np.float32)
    bv, ret = CR.targets(c, sd, cyl, seed + 2)
    index = np.random.default_rng(seed + 3).permutation(1024)[:700].astype(np.int64)
    return Case(c, sd, cyl, bv, ret, index, {}, None)


def _repeated():
    """An index of 70 draws from 40 env-steps (36 of them repeats): a repeated env-step counts as often as it is drawn."""
    c = _plain(3, 5, 35, 40, shift=-0.3)
    index = np.random.default_rng(6).integers(0, 40, 70).astype(np.int64)
    assert 70 - np.unique(index).size == 36
    return c._replace(index=index)


PAST_RANGE = ["a3k5d35s1537", "a7k16d96s1537-dead", "a1k5d20s3073"]
FILLS = [(7, 1, 20, 17), (2, 16, 20, 31), (6, 16, 24, 32), (3, 5, 35, 16), (3, 5, 35, 64), (3, 5, 1, 33), (1, 1, 1, 1)]
EDGES = ["flat_tokens", "saturated_softmax", "large_obs"]
MIXED_DELTA, CLIP = 0.7, 0.1

BUILDERS = {
    "a3k5d35s1537": lambda: _plain(3, 5, 35, 1537),
    "a7k16d96s1537-dead": _limits_through_a_dead_index,
    "a1k5d20s3073": lambda: _plain(1, 5, 20, 3073, shift=-0.3),
    # (one value: with targets' seed 102 it falls in the shift's inside-the-clip half — clipped == v, an exact tie; 103 is the first seed off it)
    **{"a%dk%dd%ds%d" % s: (lambda s=s: _plain(*s, shift=0.3 if s[3] % 2 else -0.3, tseed=103 if s == (1, 1, 1, 1) else 102)) for s in FILLS},
    **{m: (lambda m=m: _edge(m)) for m in EDGES},
    "mixed-huber": lambda: _plain(3, 5, 35, 65, huber_delta=MIXED_DELTA),
    "mixed-mse": lambda: _plain(3, 5, 35, 65, loss="mse"),
    "repeated": _repeated,
}
UPDATE_CASES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


def steps(c):
    """The env-steps the minibatch holds: the plan's `rows`."""
    return c.index.size if c.index is not None else c.sd.shape[0]


def live_positions(c):
    """The minibatch positions whose index entry lies inside the rollout (all of them without an index)."""
    if c.index is None:
        return np.arange(c.sd.shape[0])
    return np.flatnonzero((c.index >= 0) & (c.index < c.sd.shape[0]))


def _restate(c, dtype):
    """The restatement on the live entries; with dead ones (include/hns.h: "contributes nothing") the kernel's means still divide by the whole
    minibatch's B A values: value_loss, grad_norm and every gradient scale by live / B exactly in real arithmetic, explained_var takes n = B A."""
    pos = live_positions(c)
    B, A = steps(c), c.sd.shape[1]
    r = CR.loss_and_grad(c.critic, c.sd, c.cyl, c.bv, c.ret, c.index[pos] if c.index is not None else None, dtype=dtype, **c.kw)
    if pos.size != B:
        f = pos.size / B
        r["value_loss"] *= f
        r["l_orig"] *= f
        r["l_clip"] *= f
        r["grad_norm"] *= f
        r["grads"] = {k: g * f for k, g in r["grads"].items()}
        v, t = r["values"].ravel(), c.ret[c.index[pos]].astype(np.float64).ravel()
        n = float(B * A)
        r["explained_var"] = 1.0 - (((v - t) ** 2).sum() / n) / ((np.sum(t * t) - t.sum() ** 2 / n) / (n - 1.0))
    return r


@functools.lru_cache(maxsize=None)
def references(name):
    """(fp64 yardstick, fp32 restatement) of the case, loss_and_grad's dicts with `values` over the live positions.  Computed once: treat
    them as read-only (copy_refs for a test that edits one)."""
    c = case(name)
    return _restate(c, torch.float64), _restate(c, torch.float32)


def copy_refs(r):
    return {k: ({n: g.copy() for n, g in v.items()} if isinstance(v, dict) else (v.copy() if isinstance(v, np.ndarray) else v)) for k, v in r.items()}


def check_conditions(name, r64, r32):
    """What a gated case must be before a device sees it: off the tie of the max (the two mean losses at least 1e-3 of the loss apart, the
    rule of test_hip_critic_central.py), the same branch in fp32 and fp64, every gradient tensor non-zero — in_proj_bias outside its k third,
    which the softmax cancels —, everything finite."""
    sep = abs(r64["l_orig"] - r64["l_clip"])
    assert sep >= 1e-3 * r64["value_loss"], f"{name}: the two mean losses are {sep:.3e} apart ({sep / r64['value_loss']:.2e} of the loss): the case sits on the tie"
    assert r64["branch"] == r32["branch"] != 2, f"{name}: branch {r64['branch']} in fp64, {r32['branch']} in fp32"
    for r in (r64, r32):
        for n in ("value_loss", "grad_norm"):
            assert np.isfinite(r[n]), (name, n)
        assert np.isfinite(r["values"]).all(), name
        for n, g in r["grads"].items():
            assert np.isfinite(g).all(), (name, n)
            if n.endswith("in_proj_bias"):
                assert g[:E].any() and g[2 * E:].any(), (name, n)
            else:
                assert g.any(), f"{name}: d {n} is identically zero"


def mixed_shares(r64, c, delta=MIXED_DELTA, clip=CLIP):
    """Of the case's env-steps, on the fp64 yardstick: the share that holds both a value in Huber's linear region and one in the quadratic
    region, the share that holds both a clipped and an unclipped value, and the nearest |v - ret| to delta and |v - b_value| to the clip."""
    pos = live_positions(c)
    idx = c.index[pos] if c.index is not None else pos
    v = r64["values"][..., 0]
    dr, dc = np.abs(v - c.ret[idx][..., 0].astype(np.float64)), np.abs(v - c.bv[idx][..., 0].astype(np.float64))
    lin, cut = dr >= delta, dc > clip
    both = lambda m: float((m.any(1) & (~m).any(1)).mean())                          # noqa: E731
    return both(lin), both(cut), float(np.abs(dr - delta).min()), float(np.abs(dc - clip).min())
