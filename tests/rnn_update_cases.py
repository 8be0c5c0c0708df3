"""The cases of the composed recurrent update (hns_amd.rnn_train.policy_loss_and_grad_rnn / value_loss_and_grad_rnn) past one
tile of each of its three ops, for tests/test_rnn_update_edges.py (CPU) and tests/test_hip_rnn_update_edges.py (MI355X).

  * CASES: (A, K, D; N, T, L; B) by tag — B shuffled segment ids, a strict subset of the rollout's N T / L, with segment 0 (a flag at its step 0)
    and the segment with rollout_case's planted mid-segment flag among them (one-segment, B 1: the latter alone);
  * `plan`: the three ops' plans restated from their constants, each named once below beside its source; REACH: what each case is there for,
    as predicates of its plan (a tile size or a grid cap that changes and empties a case fails the CPU file);
  * `build` / `refs`: rollout_reference.rollout_case and the actor's per_row_case unchanged, a critic builder in head_case's manner (`critic_rows`),
    the fp64 and fp32 flows, computed once per (case, network) and never changed;
  * SEEDS: per case and network the first of 900, 901, ... (`find_seed`) at which the preconditions hold and the CPU torch path of rnn_train stays
    at ratio <= SEED_BAR = 4 on every gated item — a second fp32 evaluation in another order uses at most half the bar of 8 and leaves the
    device a factor two.  The search reads nothing from a device;
  * `defect_flow`: the flow in fp32 with the contributions left out that a plan-limited defect of the kernels would lose (DEFECTS);
  * `rescaled` / `rescaled_flow`: the references of a call with an out-of-range segment id (test_hip_rnn_train.py's docstring)."""
import collections
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import policy_reference as R
import rnn_update_reference as U
from per_agent_cases import E, GEMM_OUT, I_EW, MAX_SPLITS, O_EWS, ROWS          # csrc/hns_policy_train.hip: kCtE, kCtGemmOut, I_EW, kCtMaxSplits, O_EWS, kCtRows

H = U.H
GRU_TILE = 16                                                    # csrc/hns_gru.hip: kGruTile, sequences per tile
GRU_GROUPS = 256                                                 # csrc/hns_gru.hip: kGruMaxGroups, workgroups of the forward and backward sweeps
GRU_WG_ROWS = 32                                                 # csrc/hns_gru.hip: kGruWgRows, rows per tile of the weight-gradient kernel
GRU_SPLITS = 256                                                 # csrc/hns_gru.hip: kGruMaxSplits, its row ranges
GRU_GATE = 4 * H                                                 # csrc/hns_gru.hip: kGruGate, floats per row of the gate gradients
GRU_MAX_STEPS = 64                                               # include/hns.h: HNS_GRU_MAX_STEPS
ENC_ROWS, ENC_SPLITS = ROWS, MAX_SPLITS                          # (32-row tiles, 48 row ranges: named in per_agent_cases.py)
ENC_BLOCKS = 4096                                                # csrc/hns_policy_train.hip: kCtMaxBlocks
HEAD_ROWS = 32                                                   # csrc/hns_rnn_train.hip: kRtRows, rows of a workgroup's trip
HEAD_GROUPS = 512                                                # csrc/hns_rnn_train.hip: kRtMaxGroups
ESS_THREADS = 256                                                # csrc/hns_rnn_train.hip: kRtThreads, the ESS kernel's stride over the segments
HEAD_SLOTS = (528, 8, 136)                                       # csrc/hns_rnn_train.hip: kRtActorSlots, kRtSumSlots, kRtCriticSlots
SEED_BAR = 4.0

Case = collections.namedtuple("Case", ["A", "K", "D", "N", "T", "L", "B"])
CASES = {
    "default": Case(3, 5, 35, 8, 32, 16, 11),
    "encoder-ranges": Case(3, 5, 35, 20, 32, 16, 33),
    "longest": Case(2, 5, 20, 70, 64, 64, 65),
    "widest": Case(7, 16, 24, 6, 16, 16, 5),
    "second-trips": Case(1, 5, 20, 4100, 4, 4, 4097),
    "ess-columns": Case(3, 5, 35, 310, 4, 4, 300),
    "one-step": Case(3, 5, 35, 6, 4, 1, 20),
    "one-segment": Case(3, 5, 35, 4, 16, 16, 1),
}
PRESENT = Case(3, 5, 35, 3, 8, 4, 5)                             # test_update_gradients_against_the_independent_flow's shape (A 3)
TAGS = list(CASES)
# the critic's branch of the max: returns on b_values' side of v ("orig": the unclipped mean loss is the larger) or beyond v ("clip": only the
# rows inside the value clip have a gradient).  The table alternates down its rows, so that either branch is held at small and at large
# shapes; the one departure is second-trips, which by that rule would be "orig": with "orig" no seed from 900 to 1499 met the seed rule
# below (the CPU path's sequential LayerNorm sums over 98 000 token rows: smallest ratio 4.14, typically 5 to 15); with "clip" the first
# that does is 1019
BRANCH = {"default": "orig", "encoder-ranges": "clip", "longest": "orig", "widest": "clip", "second-trips": "clip", "ess-columns": "clip",
          "one-step": "orig", "one-segment": "clip"}
# find_seed's results (python tests/rnn_update_cases.py prints them)
SEEDS = {("default", True): 900, ("default", False): 900, ("encoder-ranges", True): 900, ("encoder-ranges", False): 900,
         ("longest", True): 901, ("longest", False): 930, ("widest", True): 900, ("widest", False): 900,
         ("second-trips", True): 903, ("second-trips", False): 1019,
         ("ess-columns", True): 900, ("ess-columns", False): 901, ("one-step", True): 900, ("one-step", False): 900,
         ("one-segment", True): 900, ("one-segment", False): 900}


def _cdiv(a, b):
    return -(-a // b)


def _up(v):
    return (v + 255) & ~255


def plan(case):
    """The plans of the three ops for one call of the composed update, as a dict:
    gru_plan (seqs B A, steps L): tiles of 16 sequences over <= 256 workgroups; the weight-gradient kernel's 32-row tiles, tiles per range, ranges;
    ct_plan_encoder (rows B L A): 32-row tiles, tiles per range, ranges (<= 48);
    the head entries: trips of 32 rows over <= 512 workgroups; ESS columns L A, each over B segments in strides of 256;
    y's strides as _rows_struct hands them over ([B, A, L, 128] view of [B L A, 128]; 0 where the extent is 1); the workspaces' bytes."""
    A, K, D, N, T, L, B = case
    rows, seqs = B * L * A, B * A
    p = {"rows": rows, "seqs": seqs, "segments": N * (T // L)}
    p["gru_tiles"] = _cdiv(seqs, GRU_TILE)
    p["gru_groups"] = min(p["gru_tiles"], GRU_GROUPS)
    p["gru_trips"] = _cdiv(p["gru_tiles"], p["gru_groups"])
    p["gru_last_tile_seqs"] = seqs - GRU_TILE * (p["gru_tiles"] - 1)
    p["gru_wg_tiles"] = _cdiv(rows, GRU_WG_ROWS)
    p["gru_tps"] = _cdiv(p["gru_wg_tiles"], GRU_SPLITS)
    p["gru_splits"] = _cdiv(p["gru_wg_tiles"], p["gru_tps"])
    p["enc_tiles"] = _cdiv(rows, ENC_ROWS)
    p["enc_tps"] = _cdiv(p["enc_tiles"], ENC_SPLITS)
    p["enc_splits"] = _cdiv(p["enc_tiles"], p["enc_tps"])
    p["enc_last_tile_rows"] = rows - ENC_ROWS * (p["enc_tiles"] - 1)
    p["enc_last_range_tiles"] = p["enc_tiles"] - p["enc_tps"] * (p["enc_splits"] - 1)
    p["head_trips"] = _cdiv(rows, HEAD_ROWS)
    p["head_groups"] = min(p["head_trips"], HEAD_GROUPS)
    p["head_last_trip_rows"] = rows - HEAD_ROWS * (p["head_trips"] - 1)
    p["ess_columns"], p["ess_strides"] = L * A, _cdiv(B, ESS_THREADS)
    p["y_stride"] = tuple(s if n > 1 else 0 for s, n in zip((L * A * H, H, A * H), (B, A, L)))
    p["gru_bytes"] = _up(rows * GRU_GATE * 4) + _up(p["gru_splits"] * 6 * (H * H + H) * 4) + _up(p["gru_groups"] * 2 * H * 4)
    img, P = I_EW + (D + 8) * E, O_EWS + D * E                   # ct_img_floats(D), ct_partial_floats(D, 0)
    p["enc_forward_bytes"] = _up(img * 4)
    p["enc_bytes"] = (_up(img * 4) + _up(ENC_BLOCKS * 8) + _up(p["enc_tiles"] * 2 * P * 4) + _up(p["enc_splits"] * 6 * GEMM_OUT * 4) +
                      _up(12 * p["enc_tiles"] * ENC_ROWS * E * 4))
    G = p["head_groups"]
    p["actor_head_bytes"] = _up(G * HEAD_SLOTS[0] * 8) + _up(rows * 4) + _up(L * A * 8)
    p["critic_head_bytes"] = _up(G * HEAD_SLOTS[1] * 8) + _up(G * HEAD_SLOTS[2] * 8) + 256 + _up(rows * 4)
    return p


def _cuts_a_segment(p, A):
    """A GRU tile edge that falls inside a segment's A sequences."""
    return A > 1 and any((GRU_TILE * t) % A for t in range(1, p["gru_tiles"]))


# what each case reaches, as predicates of (its plan, the case): every one is asserted by test_rnn_update_edges.py
REACH = {
    "default": lambda p, c: c.L == 16 and p["seqs"] == 33 and p["gru_tiles"] == 3 and p["gru_last_tile_seqs"] == 1 and _cuts_a_segment(p, c.A) and
    p["enc_tiles"] == 17 and p["enc_last_tile_rows"] == ENC_ROWS // 2 and p["enc_tps"] == 1,
    "encoder-ranges": lambda p, c: p["enc_tiles"] == 50 > ENC_SPLITS and p["enc_tps"] == 2 and p["enc_last_tile_rows"] == 16 and p["gru_tiles"] == 7 and
    p["gru_tps"] == 1,
    "longest": lambda p, c: c.L == GRU_MAX_STEPS and p["gru_wg_tiles"] == 260 > GRU_SPLITS and p["gru_tps"] == 2 and p["enc_tps"] == 6 and
    0 < p["enc_last_range_tiles"] < p["enc_tps"] and p["ess_columns"] == 128,
    "widest": lambda p, c: c.A == 7 and c.K == 16 and p["seqs"] == 35 and p["rows"] == 560 and _cuts_a_segment(p, c.A),
    "second-trips": lambda p, c: p["gru_tiles"] == GRU_GROUPS + 1 and p["gru_trips"] == 2 and p["gru_last_tile_seqs"] == 1 and
    p["head_trips"] == HEAD_GROUPS + 1 and p["head_last_trip_rows"] == 4 and p["ess_strides"] == 17 and p["enc_tps"] == 11 and p["gru_tps"] == 3 and
    c.A == 1 and p["y_stride"][1] == 0,
    "ess-columns": lambda p, c: p["ess_strides"] >= 2 and p["ess_columns"] == 12 and c.B % ESS_THREADS != 0,
    "one-step": lambda p, c: c.L == 1 and p["y_stride"][2] == 0 and p["y_stride"][0] > 0 and p["gru_tiles"] > 1,
    "one-segment": lambda p, c: c.B == 1 and p["y_stride"][0] == 0 and p["y_stride"][1] > 0 and p["y_stride"][2] > 0,
}


# ---------------------------------------------------------------------------------------------------------------- the builder
def flagged_segment(case):
    """The id of the segment that holds rollout_case's planted mid-segment flag, is_init[N - 1, min(L // 2, T - 1)]."""
    return (case.N - 1) * (case.T // case.L) + min(case.L // 2, case.T - 1) // case.L


def minibatch(case, seed):
    """B shuffled ids, a strict subset of the rollout's segments, with segment 0 and the flagged one (B 1: the flagged one alone)."""
    NS, B = case.N * (case.T // case.L), case.B
    assert B < NS
    fixed = [flagged_segment(case)] if B == 1 else [0, flagged_segment(case)]
    g = np.random.default_rng(seed)
    rest = np.setdiff1d(np.arange(NS), fixed)
    seg = np.concatenate([np.array(fixed, np.int64), g.permutation(rest)[:B - len(fixed)]])
    return g.permutation(seg).astype(np.int64)


def critic_rows(case, net, obs, state, is_init, seed, branch="orig", value_bands=((0.0, 0.05), (0.15, 0.40))):
    """[b_values, b_returns], [N, T, A, 1] fp32, in head_case's manner on the recomputed values: v from the fp64 flow over every segment of the
    rollout, b_values = v - d with |d| in `value_bands` (off the value clip 0.1 by >= 0.05), returns 1 to 1.5 away from v, on b_values' side of
    it ("orig": clipping moves the value towards the return, the unclipped mean loss is the larger) or beyond it ("clip")."""
    A, K, D, N, T, L, B = case
    g = np.random.default_rng(seed)
    some = [np.zeros((N, T, A, 1), np.float32), g.standard_normal((N, T, A, 1)).astype(np.float32)]
    _, s = U.flow(net, False, obs, state, is_init, some, np.arange(N * (T // L)), L, torch.float64)
    v = s["values"].reshape(N, T, A, 1)
    pick = g.integers(0, len(value_bands), v.shape)
    lo, hi = np.array([b[0] for b in value_bands])[pick], np.array([b[1] for b in value_bands])[pick]
    d = (lo + (hi - lo) * g.random(v.shape)) * np.where(g.random(v.shape) < 0.5, -1.0, 1.0)
    ret = v + (-1.0 if branch == "orig" else 1.0) * np.sign(d) * (1.0 + 0.5 * g.random(v.shape))
    return [(v - d).astype(np.float32), ret.astype(np.float32)]


Built = collections.namedtuple("Built", ["case", "actor", "net", "obs", "state", "is_init", "rows", "seg", "g64", "s64", "g32", "s32"])


def build(case, actor, seed, branch="orig", seg=None, row_seed=None, present=False):
    """One network's inputs and both flows.  seed: rollout_case's; seed + 1000: the per-row tensors'; seed + 2000: the minibatch's.
    `present`: the inputs of test_update_gradients_against_the_independent_flow (per_row_case for the critic as well)."""
    A, K, D, N, T, L, B = case
    a_net, c_net, obs, states, is_init = U.rollout_case(N, T, A, K, D, L, seed)
    net, state = (a_net, states["actor"]) if actor else (c_net, states["critic"])
    row_seed = seed + 1000 if row_seed is None else row_seed
    if actor or present:
        rows = U.per_row_case(actor, N, T, A, row_seed, net, obs, state, is_init, L)
    else:
        rows = critic_rows(case, net, obs, state, is_init, row_seed, branch)
    seg = minibatch(case, seed + 2000) if seg is None else np.asarray(seg, np.int64)
    g64, s64 = U.flow(net, actor, obs, state, is_init, rows, seg, L, torch.float64)
    g32, s32 = U.flow(net, actor, obs, state, is_init, rows, seg, L, torch.float32)
    return Built(case, actor, net, obs, state, is_init, rows, seg, g64, s64, g32, s32)


_REFS = {}


def refs(tag, actor):
    """build() of a case of the table at its recorded seed, or of "present": computed once per process, never changed."""
    key = (tag, bool(actor))
    if key not in _REFS:
        if tag == "present":
            _REFS[key] = build(PRESENT, actor, 900 + PRESENT.A, seg=[4, 0, 5, 2, 1], row_seed=31, present=True)
        else:
            _REFS[key] = build(CASES[tag], actor, SEEDS[key], BRANCH[tag])
    return _REFS[key]


def preconditions(b):
    """The failures of the existing preconditions, as strings (none: well posed), and the figures: in fp64 no ratio within U.MARGIN of 1 +- 0.1
    and fp32 on the same side of the clip on every row; no |v - b_values| within U.MARGIN of 0.1 and the two mean losses >= 1e-3 of value_loss
    apart."""
    bad, fig = [], {}
    if b.actor:
        d = np.minimum(np.abs(b.s64["ratio"] - 0.9), np.abs(b.s64["ratio"] - 1.1))
        fig["clip distance"] = float(d.min())
        if not d.min() >= U.MARGIN:
            bad.append(f"a ratio is {d.min():.2e} from the clip's bound")
        if not np.array_equal(b.s64["w"], b.s32["w"]):
            bad.append("fp32 takes another side of the clip on some row")
        inside = (b.s64["ratio"] >= 0.9) & (b.s64["ratio"] <= 1.1)
        fig["inside"] = float(inside.mean())
    else:
        fig["clip distance"] = float(b.s64["dist"])
        fig["loss separation"] = abs(float(b.s64["l_orig"] - b.s64["l_clip"])) / float(b.s64["value_loss"])
        if not fig["clip distance"] >= U.MARGIN:
            bad.append(f"a value is {fig['clip distance']:.2e} from the value clip's bound")
        if not fig["loss separation"] >= 1e-3:
            bad.append(f"the two mean losses are {fig['loss separation']:.2e} of value_loss apart")
    return bad, fig


ACTOR_SCALARS, CRITIC_SCALARS = ("policy_loss", "entropy", "ess", "log_probs"), ("value_loss", "explained_var", "values")


def call(b, to, seg=None, live=None, **kw):
    """The library's call on `b`'s inputs: (the live parameters with their .grad set, the result).  `to`: numpy array -> tensor on the device
    under test; seg: other ids than b's; live: the parameters of an earlier call (a bucket= is tied to them); kw: further arguments of
    policy_loss_and_grad_rnn / value_loss_and_grad_rnn."""
    from hns_amd import rnn_train
    live = {k: to(v) for k, v in b.net.items()} if live is None else live
    fn = rnn_train.policy_loss_and_grad_rnn if b.actor else rnn_train.value_loss_and_grad_rnn
    res = fn(live, to(b.obs["state_self"]), to(b.obs["state_others"]) if b.case.A > 1 else None, to(b.obs["cylinders"]), to(b.state), to(b.is_init),
             *(to(r) for r in b.rows), segment=to(b.seg if seg is None else seg), seq_len=b.case.L, **({"entropy_coef": 1e-3} if b.actor else {}), **kw)
    return live, res


def outputs(b, live, res):
    """{name: fp64 numpy} of everything test_rnn_train.py gates: each gradient tensor, the scalars, log_probs / values, grad_norm."""
    np64 = lambda t: t.detach().cpu().double().numpy()            # noqa: E731
    out = {k: np64(live[k].grad) for k in b.net}
    for k in (ACTOR_SCALARS if b.actor else CRITIC_SCALARS):
        v = getattr(res, k)
        out[k] = np64(v.squeeze(-1) if k in ("log_probs", "values") else v)
    out["grad_norm"] = np64(res.grad_norm)
    return out


def items(b, out, r64=None, r32=None, rows=None):
    """U.gate's items of `out` (outputs(), or a flow's (grads, scalars) merged) against b's references (or r64 / r32: (grads, scalars));
    rows: the kept minibatch positions of log_probs / values."""
    g64, s64 = r64 if r64 is not None else (b.g64, b.s64)
    g32, s32 = r32 if r32 is not None else (b.g32, b.s32)
    its = [(k, out[k], g64[k], g32[k]) for k in b.net]
    for k in (ACTOR_SCALARS if b.actor else CRITIC_SCALARS) + ("grad_norm",):
        got = out[k][rows] if rows is not None and k in ("log_probs", "values") else out[k]
        its.append((k, got, s64[k], s32[k]))
    return its


def find_seed(tag, actor, start=900, tries=40, verbose=True):
    """The first seed from `start` at which the case is well posed and rnn_train's CPU torch path stays at ratio <= SEED_BAR on every item."""
    to = lambda v: torch.as_tensor(np.asarray(v)).clone()         # noqa: E731
    for seed in range(start, start + tries):
        b = build(CASES[tag], actor, seed, BRANCH[tag])
        bad, fig = preconditions(b)
        worst = math.inf
        if not bad:
            worst, _ = U.gate(tag, items(b, outputs(b, *call(b, to))), verbose=False)
        if verbose:
            print(f"  {tag} {'actor' if actor else 'critic'} seed {seed}: {bad or 'well posed'}, {fig}, CPU path's worst ratio {worst:.2f}", flush=True)
        if not bad and worst <= SEED_BAR:
            return seed
    raise RuntimeError(f"no seed in [{start}, {start + tries}) for {tag}")


# ---------------------------------------------------------------------------------------------------------------- defects
# What a kernel whose loop stops at its plan's first tile, trip or stride would lose, as masks over the minibatch's rows (b, t, a).  Row orders:
# the GRU's sequence q = b A + a and its gate-gradient row q L + t; the encoder's and the head's row (b L + t) A + a.
DEFECTS = ("gru_first_tile_only", "gru_first_trip_only", "gru_wgrad_one_tile_per_range", "encoder_wgrad_one_tile_per_range", "head_first_trip_only",
           "ess_first_stride_only")
# the encoder tensors that the weight-gradient kernel sums over its row ranges (the six matrices and their biases; the others come from the
# tiles' partial rows)
ENC_GEMM = ("attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias", "linear1.weight", "linear1.bias",
            "linear2.weight", "linear2.bias")
GRU_CELL = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def defect_keep(defect, case):
    """{mask name: what stays}: "gru_seq" [B, A] (sequences whose backward pass runs: the GRU's gradients and dx), "gru_wg" [B, A, L] (rows
    that reach the GRU cell's weight gradients), "enc_wg" [B, L, A] (rows that reach the encoder's six matrices), "head" [B, L, A] (rows the
    head entry sees), "ess" (segments of a column that reach ESS).  Empty: nothing is lost at this shape."""
    A, K, D, N, T, L, B = case
    p = plan(case)
    b, t, a = np.arange(B)[:, None, None], np.arange(L)[None, :, None], np.arange(A)[None, None, :]
    row = (b * L + t) * A + a                                    # [B, L, A]
    q = (b * A + a)[:, 0, :]                                     # [B, A]
    gate_row = (b * A + a).transpose(0, 2, 1) * L + t.transpose(0, 2, 1)            # [B, A, L]
    keep = {"gru_first_tile_only": {"gru_seq": q < GRU_TILE},
            "gru_first_trip_only": {"gru_seq": q < GRU_TILE * GRU_GROUPS},
            "gru_wgrad_one_tile_per_range": {"gru_wg": (gate_row // GRU_WG_ROWS) % p["gru_tps"] == 0},
            "encoder_wgrad_one_tile_per_range": {"enc_wg": (row // ENC_ROWS) % p["enc_tps"] == 0},
            "head_first_trip_only": {"head": row < HEAD_ROWS * HEAD_GROUPS},
            "ess_first_stride_only": {"ess": min(B, ESS_THREADS)}}[defect]
    return {k: v for k, v in keep.items() if not (v == B if k == "ess" else v.all())}


# defect -> the cases it must fail on (the CPU file also checks that these are exactly the cases at which defect_keep loses something, for
# the defects with one named cause, and that nothing is lost at PRESENT)
DEFECT_TABLE = {
    "gru_first_tile_only": ("default", "encoder-ranges", "longest", "widest", "second-trips", "ess-columns", "one-step"),
    "gru_first_trip_only": ("second-trips",),
    "gru_wgrad_one_tile_per_range": ("longest", "second-trips"),
    "encoder_wgrad_one_tile_per_range": ("encoder-ranges", "longest", "second-trips", "ess-columns"),
    "head_first_trip_only": ("second-trips",),
    "ess_first_stride_only": ("second-trips", "ess-columns"),
}


def _masked_critic(y, w, b, bv, ret, m, clip_param, loss, huber_delta):
    """critic_statements over the rows of mask m alone at n = all rows: what the sums hold when the other rows never reach them."""
    values = F.linear(y, w, b)
    clipped = bv + (values - bv).clamp(-clip_param, clip_param)
    lf = (lambda x, t: F.huber_loss(x, t, reduction="none", delta=huber_delta)) if loss == "huber" else (lambda x, t: F.mse_loss(x, t, reduction="none"))
    n = float(values.numel())
    l_clip, l_orig = (lf(ret, clipped) * m).sum() / n, (lf(ret, values) * m).sum() / n
    value_loss = torch.max(l_orig, l_clip)
    with torch.no_grad():
        var = ((ret * ret * m).sum() - (ret * m).sum() ** 2 / n) / (n - 1.0)
        ev = 1 - ((values - ret) ** 2 * m).sum() / n / var
    return value_loss, {"value_loss": value_loss.detach(), "explained_var": ev, "values": (values.detach() * m).squeeze(-1)}


def defect_flow(b, keep, dtype=torch.float32, clip_param=0.1, entropy_coef=1e-3, loss="huber", huber_delta=10.0):
    """U.flow on b's inputs with `keep`'s contributions alone (defect_keep): ({name: gradient}, scalars) as fp64 numpy.  A contribution is
    left out by detaching what it would flow through, never by changing a value of the forward pass: with an empty `keep` the statements, and
    the bits, are U.flow's."""
    A, K, D, N, T, L, B = b.case
    actor = b.actor
    p = {k: U._t(v, dtype).requires_grad_(True) for k, v in b.net.items()}
    seg = np.asarray(b.seg, np.int64)
    idx = torch.as_tensor((seg[:, None] * L + np.arange(L)).reshape(-1))
    o = {k: U._t(v, dtype).reshape(N * T, *v.shape[2:])[idx] for k, v in b.obs.items()}
    prefix = "encoder." if actor else "base."
    x = R.encoder(p, prefix, o, dtype)
    if "enc_wg" in keep:
        lost = {k: (v.detach() if k in [prefix + n for n in ENC_GEMM] else v) for k, v in p.items()}
        x = torch.where(torch.as_tensor(keep["enc_wg"]).reshape(B * L, A, 1), x, R.encoder(lost, prefix, o, dtype))
    x = x.reshape(B, L, A, H)
    cell = nn.GRUCell(H, H).to(dtype)
    cp = {n: p["rnn.cell." + n] for n in GRU_CELL}
    cd = {n: v.detach() for n, v in cp.items()}
    h = U._t(b.state, dtype).reshape(-1, A, H)[torch.as_tensor(seg)]
    flags = U._t(b.is_init, dtype).reshape(-1, L)[torch.as_tensor(seg)]
    outs = []
    for t in range(L):
        h = h * (1 - flags[:, t].reshape(B, 1, 1))
        args = (x[:, t].reshape(B * A, H), h.reshape(B * A, H))
        hn = torch.func.functional_call(cell, cp, args)
        if "gru_wg" in keep:
            hn = torch.where(torch.as_tensor(keep["gru_wg"][:, :, t]).reshape(B * A, 1), hn, torch.func.functional_call(cell, cd, args))
        h = hn.reshape(B, A, H)
        outs.append(h)
    y = F.layer_norm(torch.stack(outs, 1) + x, (H,), p["rnn.layer_norm.weight"], p["rnn.layer_norm.bias"], 1e-5)
    if "gru_seq" in keep:
        y = torch.where(torch.as_tensor(keep["gru_seq"]).reshape(B, 1, A, 1), y, y.detach())
    rows = [U._t(v, dtype).reshape(N * T, A, -1)[idx].reshape(B, L, A, -1) for v in b.rows]
    m = torch.as_tensor(keep["head"]).to(dtype).reshape(B, L, A, 1) if "head" in keep else None
    if actor:
        if m is not None:                                        # a row with advantage 0 adds nothing to the surrogate or to any gradient
            rows[2] = rows[2] * m
        total, scal = U.actor_statements(y, p["act_dist.fc_mean.weight"], p["act_dist.fc_mean.bias"], p["act_dist.log_std"], *rows, clip_param, entropy_coef)
        if m is not None:
            scal["log_probs"] = scal["log_probs"] * m.squeeze(-1)
        if "ess" in keep:
            r = scal["ratio"].unsqueeze(-1)[:keep["ess"]]
            scal["ess"] = (2 * r.logsumexp(0) - (2 * r).logsumexp(0)).exp().mean() / B
    elif m is not None:
        total, scal = _masked_critic(y, p["v_out.weight"], p["v_out.bias"], *rows, m, clip_param, loss, huber_delta)
    else:
        total, scal = U.critic_statements(y, p["v_out.weight"], p["v_out.bias"], *rows, clip_param, loss, huber_delta)
    total.backward()
    grads = {k: v.grad.double().numpy() for k, v in p.items()}
    scal["grad_norm"] = torch.tensor(math.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in grads.values())))
    return grads, U._np(scal)


# ---------------------------------------------------------------------------------------------------------------- an out-of-range id
def explained_var_at(values, ret, n):
    """1 - (sum (v - ret)^2 / n) / var, the unbiased variance from the live rows' sums with n rows: the kernels' statement when rows are dead."""
    var = ((ret * ret).sum() - ret.sum() ** 2 / n) / (n - 1.0)
    return 1.0 - (((values - ret) ** 2).sum() / n) / var


def rescaled(c, keep, dtype, loss="huber"):
    """The head entries' references (U.actor_head_autograd / critic_head_autograd of a head_case) on the kept segments at n = B L A
    (tests/test_hip_rnn_train.py's docstring): every mean by len(keep) / B, the entropy term's constant gradient kept, explained_var from
    the live rows' sums with n = B L A; the dead segments' dy rows zeros."""
    B = c["y"].shape[0]
    sub = {k: (v[keep] if k in ("y", "action", "log_probs_old", "advantages", "b_values", "b_returns") else v) for k, v in c.items()}
    a, v = U.actor_head_autograd(sub, dtype), U.critic_head_autograd(sub, dtype, loss=loss)
    f = len(keep) / B
    n = float(np.prod(c["y"].shape[:3]))
    full = lambda x: np.concatenate([x, np.zeros((B - len(keep),) + x.shape[1:])])[np.argsort(list(keep) + [b for b in range(B) if b not in keep])]   # noqa: E731
    ra = {"dy": full(a["dy"] * f), "d_head_w": a["d_head_w"] * f, "d_head_b": a["d_head_b"] * f, "d_log_std": (a["d_log_std"] + 1e-3) * f - 1e-3,
          "policy_loss": a["policy_loss"] * f, "entropy": a["entropy"], "ess": a["ess"] * f, "log_probs": a["log_probs"], "ratio": a["ratio"], "w": a["w"]}
    val, ret = v["values"], np.asarray(sub["b_returns"], np.float64 if dtype == torch.float64 else np.float32).astype(np.float64)
    rv = {"dy": full(v["dy"] * f), "d_head_w": v["d_head_w"] * f, "d_head_b": v["d_head_b"] * f, "value_loss": v["value_loss"] * f,
          "explained_var": explained_var_at(val, ret, n), "values": v["values"], "l_orig": v["l_orig"], "l_clip": v["l_clip"], "dist": v["dist"]}
    return ra, rv


def rescaled_flow(b, keep, dtype, entropy_coef=1e-3):
    """The whole update's reference when the minibatch positions outside `keep` hold out-of-range ids: U.flow on the kept segments, rescaled
    to n = B L A as `rescaled` does it — every gradient and mean by len(keep) / B (the entropy term's constant gradient on log_std kept whole,
    the entropy itself unchanged), ESS by the same (its columns are divided by B), explained_var from the kept rows' sums with n = B L A,
    grad_norm of the rescaled gradients; log_probs / values of the kept positions alone."""
    A, K, D, N, T, L, B = b.case
    g, s = U.flow(b.net, b.actor, b.obs, b.state, b.is_init, b.rows, b.seg[keep], L, dtype)
    f, n = len(keep) / B, float(B * L * A)
    g = {k: ((v + entropy_coef) * f - entropy_coef if k == "act_dist.log_std" else v * f) for k, v in g.items()}
    s = dict(s)
    if b.actor:
        s["policy_loss"], s["ess"] = s["policy_loss"] * f, s["ess"] * f
    else:
        idx = (b.seg[keep][:, None] * L + np.arange(L)).reshape(-1)
        ret = np.asarray(b.rows[1], np.float64 if dtype == torch.float64 else np.float32).astype(np.float64).reshape(N * T, A)[idx].reshape(len(keep), L, A)
        s["value_loss"], s["explained_var"] = s["value_loss"] * f, np.asarray(explained_var_at(s["values"], ret, n))
    s["grad_norm"] = np.asarray(math.sqrt(sum(float((v ** 2).sum()) for v in g.values())))
    return g, s


if __name__ == "__main__":                                      # the seed search: prints SEEDS.  Arguments: tags, or tag:actor / tag:critic[:first seed to try]
    import sys
    found = {}
    for arg_ in (sys.argv[1:] or TAGS):
        tag_, which_, start_ = (arg_.split(":") + ["", ""])[:3]
        for actor_ in [w == "actor" for w in ([which_] if which_ else ["actor", "critic"])]:
            found[tag_, actor_] = find_seed(tag_, actor_, start=int(start_ or 900), tries=2000)
    print("SEEDS = " + repr(found))
