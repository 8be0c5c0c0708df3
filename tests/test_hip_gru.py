"""The GRU as a differentiable op on the device (hns_gru_forward / hns_gru_backward through hns_amd.rnn) on an MI355X.

Accuracy gate (the rule of test_hip_encoder.py, test_hip_critic_train.py and test_tp_train.py, BAR = 8): for out, h_last, dx, dh0 and EACH of
the six parameter gradients of sum(out dy) + sum(h_last dh), e_hip <= 8 max(e_32, 2^-24 max|ref_64|), errors as max-abs against
tests/gru_reference.py in fp64, e_32 the error of the same statements in CPU fp32 — per PARTITION (gru_reference.gate): the r, z and n thirds
of weight_ih, weight_hh, bias_ih and bias_hh, out and dx per step, the other tensors whole; the bound is the partition's own e_32 and
max|ref_64| (the thirds differ by an order of magnitude: under the whole-tensor bound an error of 100 x fp32's own in the r third passes).  A
partition pass implies the whole-tensor pass.  Every partition's fp64 reference is asserted non-zero first, except the ones that are zero by
construction (dh0 when every sequence starts an episode at step 0, weight_hh's gradient when every step does): those must be exactly zero on
the device.  Inputs: gru_reference.random_case (orthogonal weights, biases 0.1 N, LN weight 1 + 0.1 N, x ~ N, h0 ~ 0.5 N, flags
Bernoulli(0.15), seeded dy and dh; S = 1 runs with is_init[0, 0] = 0, or its dh0 is identically zero).  The kernels' sequence tile is 16:
S = 17 and S = 33 are one more than one and two tiles.  tests/test_gru.py shows on the CPU that the gate has teeth on these cases.

Constants the shapes are derived from (csrc/hns_gru.hip): kGruTile 16 sequences per tile, kGruMaxGroups 256 persistent workgroups (tiles g,
g + 256, ...), kGruWgRows 32 rows (s L + t) per weight-gradient tile, kGruMaxSplits 256 (tps = ceil(tiles / 256) tiles per split).  Past one
trip: (4097, 3) and (8197, 1) and the strided [1366, 3, 3] — a second and third trip of both persistent loops, tps 2, a ragged last split,
256 LayerNorm partial rows and 193 / 129 splits under a NaN-filled workspace.

Measured on an MI355X, worst ratio over a case's tensors, whole tensor / worst partition (whole tensor: the figure recorded before the
partitions, unchanged; both printed by test_report_ratios from WHOLE and RATIOS):
  (S, L): (37, 16) 1.50 / 1.65, (1, 16) 1.83 / 3.08, (15, 2) 1.36 / 1.36, (16, 3) 1.56 / 1.72, (17, 1) 1.53 / 1.53, (33, 1) 1.43 / 1.43,
  (5, 17) 1.50 / 1.97, (3, 64) 1.60 / 2.91;
  flag patterns at (18, 4): first step 1.55 / 1.55, last step 1.59 / 1.59, all 1.59 / 1.59, none 1.65 / 1.83, mixed 1.92 / 2.79;
  past one trip: (4097, 3) 1.18 / 1.25, (8197, 1) 1.29 / 1.29, strided [1366, 3, 3] 1.28 / 1.28;
  encode -> gru -> nn.Linear(128, 1) (values, the head's 2, the GRU's 6 and the encoder's 20 gradient tensors): 1.60 / 1.60."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import gru_reference as GR
import policy_reference as R
from hns_amd import abi
from hns_amd import encoder as EN
from hns_amd import policy as P
from hns_amd import rnn as RN

pytestmark = pytest.mark.gpu

BAR = GR.BAR
RATIOS = {}                                                     # tag -> worst ratio over the case's partitions
WHOLE = {}                                                      # tag -> worst whole-tensor ratio (the figure recorded before the partitions)
CASES = GR.CASES
CANARY = 1234.5
H = 128
# csrc/hns_gru.hip: kGruTile, kGruMaxGroups, kGruWgRows, kGruMaxSplits
TILE, MAX_GROUPS, WG_ROWS, MAX_SPLITS = GR.TILE, GR.MAX_GROUPS, GR.WG_ROWS, GR.MAX_SPLITS
# the smallest shapes past one trip of the persistent loops and with more than one weight-gradient tile per split (derived in
# _assert_past_one_trip); [B, A, L] of the strided case (S = 4 098)
BIG = [(4097, 3), (8197, 1)]
STRIDED = (1366, 3, 3)


@functools.lru_cache(maxsize=None)
def _reference(S, L, agents=None):
    """One case per shape with its fp64 and fp32 references, computed once: (inputs, {dtype: (out, h_last, gradients)}).  agents: the flags
    are env-level (agent 0's for the env's `agents` sequences)."""
    p, x, h0, flags, dy, dh = GR.shape_case(S, L)
    if agents:
        flags = flags.view(S // agents, agents, L)[:, :1].expand(-1, agents, -1).reshape(S, L).contiguous()
    case = (p, x, h0, flags, dy, dh)
    return case, {dt: GR.run(*case, dt) for dt in (torch.float64, torch.float32)}


def _gate(tag, items, zero=()):
    """items: (name, device value, fp64 reference, fp32 reference); every PARTITION (gru_reference.partitions) is held to the bar with its own
    bound; names in `zero` must be exactly zero against an identically zero reference.  Records the worst ratios under `tag`."""
    worst, whole, bad = GR.gate(tag, [(n, np.asarray(h, np.float64), a, b) for n, h, a, b in items], zero=zero, bar=BAR)
    RATIOS[tag], WHOLE[tag] = max(worst, RATIOS.get(tag, 0.0)), max(whole, WHOLE.get(tag, 0.0))
    assert not bad, f"{tag}: " + "; ".join(bad)


def _items(out, h, g, refs, names=GR.GRADS):
    (o64, h64, g64), (o32, h32, g32) = refs[torch.float64], refs[torch.float32]
    return [("out", out.cpu().numpy(), o64, o32), ("h_last", h.cpu().numpy(), h64, h32)] + [(n, g[n].cpu().numpy(), g64[n], g32[n]) for n in names]


def _run(p, x, h0, flags, dy, dh, grad=True):
    """The op on the device from CPU inputs: (out, h_last, {name: gradient}) as device tensors."""
    q = {f: t.cuda().requires_grad_(grad) for f, t in p.items()}
    xl = x.cuda().requires_grad_(grad)
    hl = h0.cuda().requires_grad_(grad) if h0 is not None else None
    out, h = RN.gru(q, xl, hl, flags.cuda() if flags is not None else None)
    if not grad:
        return out, h, {}
    ((out * dy.cuda()).sum() + (h * dh.cuda()).sum()).backward()
    g = {f: t.grad for f, t in q.items()}
    g["dx"], g["dh0"] = xl.grad, (hl.grad if hl is not None else None)
    return out.detach(), h.detach(), g


@pytest.mark.parametrize("S,L", CASES)
def test_outputs_and_gradients_pass_the_fp64_gate(S, L):
    case, refs = _reference(S, L)
    out, h, g = _run(*case)
    assert tuple(out.shape) == (S, L, H) and tuple(h.shape) == (S, H)
    _gate(f"S{S}L{L}", _items(out, h, g, refs))                 # (asserts every partition's fp64 reference non-zero first)


def test_strided_view_of_encoder_features_is_the_contiguous_call_bit_for_bit():
    """[B L A, 128] features read in place as [B, A, L, 128]: out, dx and every gradient against the contiguous call."""
    B, A, L = 5, 3, 3
    p, _, _, _, _, _ = GR.random_case(1, 1, 31)
    g = torch.Generator().manual_seed(32)
    buf = torch.randn(B * L * A, H, generator=g)
    h0, flags = 0.5 * torch.randn(B, A, H, generator=g), torch.rand(B, 1, L, generator=g) < 0.3
    dy, dh = torch.randn(B * L * A, H, generator=g), torch.randn(B, A, H, generator=g)
    view = lambda t: t.view(B, L, A, H).transpose(1, 2)
    res = []
    for contiguous in (False, True):
        q = {f: t.cuda().requires_grad_(True) for f, t in p.items()}
        leaf = buf.cuda().requires_grad_(True)
        hl = h0.cuda().requires_grad_(True)
        x4 = view(leaf).contiguous() if contiguous else view(leaf)
        assert x4.is_contiguous() == contiguous
        out, h = RN.gru(q, x4, hl, flags.cuda())
        assert out.stride() == x4.stride() and tuple(h.shape) == (B, A, H)
        ((out * view(dy.cuda())).sum() + (h * dh.cuda()).sum()).backward()
        res.append((out.detach().contiguous(), h.detach(), leaf.grad, hl.grad, {f: t.grad for f, t in q.items()}))
    (o0, h0_, dx0, dh0, g0), (o1, h1, dx1, dh1, g1) = res
    assert torch.equal(o0, o1) and torch.equal(h0_, h1) and torch.equal(dx0, dx1) and torch.equal(dh0, dh1)
    assert all(torch.equal(g0[f], g1[f]) for f in g0)
    # and the [B, A] index is the flat one: sequence s = b A + a, the env-level flag repeated per agent
    x3 = view(buf).reshape(B * A, L, H)
    o3, h3, g3 = _run(p, x3, h0.reshape(B * A, H), flags.expand(B, A, L).reshape(B * A, L), view(dy).reshape(B * A, L, H), dh.reshape(B * A, H))
    assert torch.equal(o3.view(B, A, L, H), o1) and torch.equal(h3.view(B, A, H), h1) and all(torch.equal(g3[f], g1[f]) for f in g1)
    assert torch.equal(g3["dx"].view(B, A, L, H).transpose(1, 2).reshape(B * L * A, H), dx1)


def test_no_state_and_no_flags_are_zeros_bit_for_bit():
    p, x, h0, flags, dy, dh = GR.random_case(19, 4, 41)
    a = _run(p, x, None, None, dy, dh)
    b = _run(p, x, torch.zeros_like(h0), torch.zeros_like(flags), dy, dh)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(a[2][n], b[2][n]) for n in GR.GRADS if n != "dh0") and a[2]["dh0"] is None
    c, d = _run(p, x, h0, None, dy, dh), _run(p, x, h0, torch.zeros_like(flags), dy, dh)
    assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1]) and all(torch.equal(c[2][n], d[2][n]) for n in GR.GRADS)
    assert not torch.equal(a[0], c[0])


@pytest.mark.parametrize("pattern", ["first", "last", "all", "none", "mixed"])
def test_flags(pattern):
    p, x, h0, flags, dy, dh = GR.flag_case(pattern)
    out, h, g = _run(p, x, h0, flags, dy, dh)
    refs = {dt: GR.run(p, x, h0, flags, dy, dh, dt) for dt in (torch.float64, torch.float32)}
    # every sequence starts an episode at step 0 (first, all): dh0 is identically zero; at every step (all): so is weight_hh's gradient, every
    # operand a masked zero.  Those must be exactly zero on the device; every other partition's reference is asserted non-zero
    _gate("flags-" + pattern, _items(out, h, g, refs), zero=GR.FLAG_ZERO.get(pattern, ()))
    first = flags[:, 0]
    if first.any():
        assert bool((g["dh0"][first.cuda()] == 0).all()), "dh0 of a sequence that starts an episode must be exactly zero"
        zero = h0.clone()
        zero[first] = 0
        oz, hz, _ = _run(p, x, zero, flags, dy, dh, grad=False)
        assert torch.equal(oz, out) and torch.equal(hz, h)
    if (~first).any():
        assert bool((g["dh0"][(~first).cuda()] != 0).any())


def test_chaining_and_row_independence_bit_for_bit():
    S, L = 17, 5
    p, x, h0, flags, dy, dh = GR.random_case(S, L, 61)
    out, h, g = _run(p, x, h0, flags, dy, dh)
    q = {f: t.cuda() for f, t in p.items()}
    xd, fd, hc = x.cuda(), flags.cuda(), h0.cuda()
    for t in range(L):                                          # collection: one step per call, the state handed on
        o1, hc = RN.gru(q, xd[:, t], hc, fd[:, t])
        assert tuple(o1.shape) == (S, H) and torch.equal(o1, out[:, t]), f"step {t}"
    assert torch.equal(hc, h)
    # the [S, 1, 128] form of the one-step call, and chained three- and two-step calls
    o3, h3 = RN.gru(q, xd[:, :3], h0.cuda(), fd[:, :3])
    o2, h2 = RN.gru(q, xd[:, 3:], h3, fd[:, 3:])
    assert torch.equal(torch.cat([o3, o2], 1), out) and torch.equal(h2, h)
    # a sequence's results do not depend on the other sequences of the call: 3 .. 9 alone (another tile position, another tile count)
    sl = slice(3, 10)
    os_, hs_, gs = _run(p, x[sl], h0[sl], flags[sl], dy[sl], dh[sl])
    assert torch.equal(os_, out[sl]) and torch.equal(hs_, h[sl]) and torch.equal(gs["dx"], g["dx"][sl]) and torch.equal(gs["dh0"], g["dh0"][sl])


def _memory_order(t, layout):
    """A logical [S, L, 128] tensor in the encoder's feature order: [B L A, 128], sequence s = b A + a."""
    B, A = layout
    return t.view(B, A, t.shape[1], H).transpose(1, 2).reshape(-1, H)


def _logical(buf, layout, L):
    """The inverse: a flat buffer in [B, L, A, 128] order as a contiguous [S, L, 128]."""
    B, A = layout
    return buf.view(B, L, A, H).transpose(1, 2).reshape(B * A, L, H)


def _raw(p, x, h0, flags, dy, dh, fill, layout=None):
    """hns_gru_forward and hns_gru_backward called directly with canaries around out, h_last, h_hist, dx and dh0 and a workspace filled with
    `fill`: every output as a clone.  layout (B, A): x, dy, out and dx lie in the encoder's feature order [B L A, 128] and are read and written
    in place as [B, A, L, 128]; out and dx come back in the logical order [S L 128]."""
    lib = abi.load_library()
    S, L, _ = x.shape
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if layout is None:
        x4, dyd = x.cuda().unsqueeze(1), dy.cuda().contiguous()
    else:
        xbuf, dyd = _memory_order(x, layout).cuda(), _memory_order(dy, layout).cuda()
        x4 = xbuf.view(layout[0], L, layout[1], H).transpose(1, 2)
        assert not x4.is_contiguous() and tuple(x4.shape) == (layout[0], layout[1], L, H)
    init = flags.to(torch.uint8).cuda()
    h0d = h0.cuda()

    def guarded(n):
        t = torch.full((n + 2 * H,), CANARY, device="cuda")
        return t, t[H:H + n]

    (bo, out), (bh, hl), (bhist, hist), (bdx, dx), (bd0, dh0) = guarded(S * L * H), guarded(S * H), guarded(S * L * H), guarded(S * L * H), guarded(S * H)
    dev = {f: t.cuda() for f, t in p.items()}                   # (kept alive: the structs hold bare pointers)
    net, seq = RN._net(dev), RN._seq(x4, h0d, init)
    assert lib.hns_gru_forward(C.byref(net), C.byref(seq), out.data_ptr(), hl.data_ptr(), hist.data_ptr(), None, 0, st) == abi.HNS_OK
    nb = lib.hns_gru_workspace_bytes(S, L, 1)
    ws = torch.empty(nb // 4, dtype=torch.float32, device="cuda").fill_(fill).view(torch.uint8)
    flat = torch.full((RN.grad_layout()[1] + 64,), CANARY, device="cuda")
    grads = RN._views(flat)
    grd = RN._net(grads)
    dhd = dh.cuda().contiguous()
    assert lib.hns_gru_backward(C.byref(net), C.byref(seq), hist.data_ptr(), dyd.data_ptr(), dhd.data_ptr(), C.byref(grd), dx.data_ptr(),
                                dh0.data_ptr(), ws.data_ptr(), nb, st) == abi.HNS_OK
    torch.cuda.synchronize()
    del dev
    for name, (buf, n) in {"out": (bo, S * L * H), "h_last": (bh, S * H), "h_hist": (bhist, S * L * H), "dx": (bdx, S * L * H), "dh0": (bd0, S * H)}.items():
        assert bool((buf[:H] == CANARY).all()) and bool((buf[H + n:] == CANARY).all()), f"floats around {name} were written"
        assert bool(torch.isfinite(buf[H:H + n]).all()) and bool((buf[H:H + n] != CANARY).all()), name
    assert bool((flat[-64:] == CANARY).all()) and bool(torch.isfinite(flat[:-64]).all()) and bool((flat[:-64] != CANARY).all())
    if layout is not None:
        out, dx = _logical(out, layout, L).reshape(-1), _logical(dx, layout, L).reshape(-1)
    return [t.clone() for t in (out, hl, hist, dx, dh0, flat)]


def test_determinism_workspace_from_scratch_and_canaries():
    S, L = 21, 6                                                # two tiles, the second with five live sequences
    case = GR.random_case(S, L, 71)
    runs = [_raw(*case, fill) for fill in (0.0, float("nan"), 0.0)]
    names = ("out", "h_last", "h_hist", "dx", "dh0", "gradients")
    for k, r in enumerate(runs[1:]):
        differ = [(n, float((a - b).abs().max()), int((a != b).sum())) for n, a, b in zip(names, r, runs[0]) if not torch.equal(a, b)]
        assert not differ, f"run {k + 1} against run 0 (name, max difference, values): {differ}"
    # the hidden states the forward pass leaves: h_hist[:, L - 1] is h_last; and the direct calls are the module's
    out, h, g = _run(*case)
    o, hl, hist, dx, dh0, flat = runs[0]
    assert torch.equal(hist.view(S, L, H)[:, L - 1], hl.view(S, H))
    assert torch.equal(o.view(S, L, H), out) and torch.equal(hl.view(S, H), h) and torch.equal(dx.view(S, L, H), g["dx"]) and torch.equal(dh0.view(S, H), g["dh0"])
    views = RN._views(flat)
    assert all(torch.equal(views[f], g[f]) for f in RN.FIELDS)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Past one trip of the grids.  kGruMaxGroups = 256 persistent workgroups walk the 16-sequence tiles g, g + 256, ...: a second trip needs
# S > 4 096.  The weight-gradient kernel takes tps = ceil(tiles of 32 rows / 256) tiles per split: tps = 2 needs S L > 8 192.
RAW_NAMES = ("out", "h_last", "h_hist", "dx", "dh0", "gradients")


def _assert_past_one_trip(S, L, trips, last_live, wg_tiles, splits, last_rows):
    """The branches (S, L) reaches, derived from S, L and the kernels' constants — and the plan is the library's: its workspace size."""
    tiles = -(-S // TILE)
    assert tiles == (trips - 1) * MAX_GROUPS + 1                # workgroup 0 alone makes a last trip: tiles 0, 256, ...
    assert S - (tiles - 1) * TILE == last_live                  # live sequences of that last tile
    rows = S * L
    assert -(-rows // WG_ROWS) == wg_tiles and wg_tiles > MAX_SPLITS
    tps = -(-wg_tiles // MAX_SPLITS)
    assert tps == 2 and -(-wg_tiles // tps) == splits
    assert wg_tiles - (splits - 1) * tps == 1                   # the ragged last split: one tile, not two ...
    assert rows - (wg_tiles - 1) * WG_ROWS == last_rows         # ... with few live rows
    pl = GR.plan(S, L)
    assert (pl["tiles"], pl["groups"], pl["wg_tiles"], pl["tps"], pl["splits"]) == (tiles, MAX_GROUPS, wg_tiles, tps, splits)
    r256 = lambda n: -(-n // 256) * 256
    want = r256(rows * 4 * H * 4) + r256(splits * 6 * (H * H + H) * 4) + r256(MAX_GROUPS * 2 * H * 4)
    assert abi.load_library().hns_gru_workspace_bytes(S, L, 1) == want


def _assert_the_last_tile_matters(S, case, refs):
    """Before the device is touched: the case can fail.  The fp32 reference gradients of the first 16 floor((S - 1) / 16) sequences only (the
    last tile dropped) must fail the gate for each of the six parameter gradients."""
    keep = TILE * ((S - 1) // TILE)
    p, x, h0, flags, dy, dh = case
    _, _, cut = GR.run(p, x[:keep], h0[:keep], flags[:keep], dy[:keep], dh[:keep], torch.float32)
    g64, g32 = refs[torch.float64][2], refs[torch.float32][2]
    for f in GR.FIELDS:
        worst, _, bad = GR.gate("last tile dropped", [(f, cut[f], g64[f], g32[f])], verbose=False)
        assert bad and worst > BAR, f"{f}: without the last tile's {S - keep} sequences the gate still passes ({worst:.2f}): the case gates nothing"


def _assert_raw_runs_equal_the_module(tag, S, L, case, layout=None):
    """Direct C calls with canaries, the workspace NaN on one run and 0 on another: bit-identical, and the module path's bits."""
    runs = [_raw(*case, fill, layout=layout) for fill in (float("nan"), 0.0)]
    differ = [(n, float((a - b).abs().max()), int((a != b).sum())) for n, a, b in zip(RAW_NAMES, runs[1], runs[0]) if not torch.equal(a, b)]
    assert not differ, f"{tag}: workspace 0 against workspace NaN (name, max difference, values): {differ}"
    out, h, g = _run(*case) if layout is None else _run_layout(case, layout, False)
    o, hl, hist, dx, dh0, flat = runs[0]
    assert torch.equal(hist.view(S, L, H)[:, L - 1], hl.view(S, H))
    assert torch.equal(o.view(S, L, H), out) and torch.equal(hl.view(S, H), h) and torch.equal(dx.view(S, L, H), g["dx"]) and torch.equal(dh0.view(S, H), g["dh0"])
    views = RN._views(flat)
    assert all(torch.equal(views[f], g[f]) for f in RN.FIELDS)
    return out, h, g


@pytest.mark.parametrize("S,L,trips,last_live,wg_tiles,splits,last_rows", [(4097, 3, 2, 1, 385, 193, 3), (8197, 1, 3, 5, 257, 129, 5)])
def test_past_one_trip_of_the_grids_passes_the_partition_gate(S, L, trips, last_live, wg_tiles, splits, last_rows):
    """(4097, 3): 257 tiles, workgroup 0 takes tiles 0 and 256, tile 256 holds the single sequence 4096; 12 291 rows, 385 weight-gradient
    tiles, tps 2, 193 splits, the last one tile with 3 live rows.  (8197, 1), the collection shape: 513 tiles, three trips for workgroup 0,
    5 live sequences in tile 512; 257 weight-gradient tiles, 129 splits, the last tile with 5 rows."""
    assert (S, L) in BIG
    _assert_past_one_trip(S, L, trips, last_live, wg_tiles, splits, last_rows)
    case, refs = _reference(S, L)
    _assert_the_last_tile_matters(S, case, refs)
    out, h, g = _assert_raw_runs_equal_the_module(f"S{S}L{L}", S, L, case)
    _gate(f"S{S}L{L}", _items(out, h, g, refs))


@pytest.mark.parametrize("S,L", BIG)
def test_second_trip_tiles_alone_give_their_bits_inside_the_big_call(S, L):
    """Row independence at the positions where state left over between a workgroup's tiles would break it: the sequences of tile 256 (and
    512), and of tile 0 of the same workgroup, run alone."""
    case, _ = _reference(S, L)
    out, h, g = _run(*case)
    tiles = -(-S // TILE)
    mine = list(range(0, tiles, MAX_GROUPS))                    # workgroup 0's tiles
    assert len(mine) >= 2 and mine[-1] == tiles - 1
    for tile in mine:
        sl = slice(TILE * tile, min(TILE * (tile + 1), S))
        os_, hs_, gs = _run(*(t[sl] if torch.is_tensor(t) else t for t in case))
        for name, a, b in (("out", os_, out[sl]), ("h_last", hs_, h[sl]), ("dx", gs["dx"], g["dx"][sl]), ("dh0", gs["dh0"], g["dh0"][sl])):
            assert torch.equal(a, b), f"tile {tile} alone: {name} differs in {int((a != b).sum())} values, max {float((a - b).abs().max()):.3e}"


def test_chained_one_step_calls_past_one_trip_bit_for_bit():
    S, L = BIG[0]
    (p, x, h0, flags, dy, dh), _ = _reference(S, L)
    q = {f: t.cuda() for f, t in p.items()}
    xd, fd, hc = x.cuda(), flags.cuda(), h0.cuda()
    with torch.no_grad():
        out, h = RN.gru(q, xd, hc, fd)
        for t in range(L):
            o1, hc = RN.gru(q, xd[:, t], hc, fd[:, t])
            assert torch.equal(o1, out[:, t]), f"step {t}: {int((o1 != out[:, t]).sum())} values differ"
    assert torch.equal(hc, h)


def _run_layout(case, layout, contiguous):
    """The module path on the encoder's feature order: x a leaf [B L A, 128] read in place as [B, A, L, 128] (or its .contiguous() copy), the
    flags env-level [B, 1, L].  -> (out, h_last, gradients) in the logical order of _run."""
    p, x, h0, flags, dy, dh = case
    (B, A), (S, L, _) = layout, x.shape
    q = {f: t.cuda().requires_grad_(True) for f, t in p.items()}
    leaf = _memory_order(x, layout).cuda().requires_grad_(True)
    hl = h0.view(B, A, H).cuda().requires_grad_(True)
    view = lambda t: t.view(B, L, A, H).transpose(1, 2)
    x4 = view(leaf).contiguous() if contiguous else view(leaf)
    assert x4.is_contiguous() == contiguous
    env = flags.view(B, A, L)[:, :1]
    assert torch.equal(env.expand(B, A, L).reshape(S, L), flags)
    out, h = RN.gru(q, x4, hl, env.cuda())
    assert out.stride() == x4.stride() and tuple(h.shape) == (B, A, H)
    ((out * view(_memory_order(dy, layout).cuda())).sum() + (h * dh.view(B, A, H).cuda()).sum()).backward()
    g = {f: t.grad for f, t in q.items()}
    g["dx"], g["dh0"] = _logical(leaf.grad, layout, L), hl.grad.view(S, H)
    return out.detach().reshape(S, L, H), h.detach().view(S, H), g


def test_strided_features_past_one_trip_are_the_contiguous_call_and_pass_the_gate():
    """[B, A, L] = [1366, 3, 3] read in place from a [B L A, 128] buffer with env-level flags [B, 1, L]: S = 4 098, 257 tiles, the last with 2
    live sequences."""
    B, A, L = STRIDED
    S = B * A
    assert -(-S // TILE) == MAX_GROUPS + 1 and S - MAX_GROUPS * TILE == 2 and GR.plan(S, L)["tps"] == 2
    case, refs = _reference(S, L, agents=A)
    assert case[3].any() and not case[3].all()
    _assert_the_last_tile_matters(S, case, refs)
    out, h, g = _assert_raw_runs_equal_the_module("strided", S, L, case, layout=(B, A))
    oc, hc, gc = _run_layout(case, (B, A), True)
    assert torch.equal(out, oc) and torch.equal(h, hc)
    differ = [n for n in GR.GRADS if not torch.equal(g[n], gc[n])]
    assert not differ, f"strided against contiguous: {differ}"
    _gate("strided-B1366A3L3", _items(out, h, g, refs))


def test_autograd_semantics():
    p, x, h0, flags, dy, dh = GR.random_case(9, 3, 81)
    out, h, g1 = _run(p, x, h0, flags, dy, dh)
    dev = {f: t.cuda() for f, t in p.items()}
    xd, hd, fd, dyd, dhd = x.cuda(), h0.cuda(), flags.cuda(), dy.cuda(), dh.cuda()
    # a tensor that does not require grad gets none; the others keep their bits
    leaves = {f: t.clone().requires_grad_(f not in ("ln_w", "weight_hh")) for f, t in dev.items()}
    o, hh = RN.gru(leaves, xd, hd, fd)
    ((o * dyd).sum() + (hh * dhd).sum()).backward()
    assert leaves["ln_w"].grad is None and leaves["weight_hh"].grad is None
    assert all(torch.equal(t.grad, g1[f]) for f, t in leaves.items() if t.requires_grad)
    # two passes accumulate to exactly twice one pass; a non-contiguous incoming gradient is laid out as x
    leaves = {f: t.clone().requires_grad_(True) for f, t in dev.items()}
    wide = torch.zeros(9, 3, 256, device="cuda")
    wide[..., ::2] = dyd
    for _ in range(2):
        o, hh = RN.gru(leaves, xd, hd, fd)
        torch.autograd.backward([o, hh], [wide[..., ::2], dhd])
    assert all(torch.equal(t.grad, g1[f] + g1[f]) for f, t in leaves.items())
    # only out used: dh_last arrives as zeros
    xl = xd.clone().requires_grad_(True)
    (RN.gru(dev, xl, hd, fd)[0] * dyd).sum().backward()
    assert bool(torch.isfinite(xl.grad).all()) and not torch.equal(xl.grad, g1["dx"])
    # no_grad, and nothing requiring grad: no node, the same bits
    with torch.no_grad():
        plain = RN.gru(leaves, xd, hd, fd)
    frozen = RN.gru(dev, xd, hd, fd)
    assert plain[0].grad_fn is None and frozen[0].grad_fn is None and torch.equal(plain[0], out) and torch.equal(frozen[1], h)
    # a parameter changed in place between forward and backward: autograd's version check
    loss = (RN.gru(leaves, xd, hd, fd)[0] * dyd).sum()
    with torch.no_grad():
        leaves["bias_hh"].add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()
    # the module form with the reference's call shape, an optimiser of torch's own on top
    mod = RN.GRU().cuda()
    mod.load_state_dict({k: dev[f] for k, f in RN.NAMES.items()})
    o, hp = mod(xd, hd, fd.unsqueeze(-1))
    assert torch.equal(o, out) and tuple(hp.shape) == (9, 3, H) and torch.equal(hp[:, 0], h)
    opt = torch.optim.AdamW(mod.parameters(), lr=1e-3, weight_decay=0.01)
    ((o * dyd).sum() + (hp[:, 0] * dhd).sum()).backward()
    assert torch.equal(mod.cell.weight_ih.grad, g1["weight_ih"]) and torch.equal(mod.layer_norm.bias.grad, g1["ln_b"])
    opt.step()
    assert not torch.equal(mod(xd, hd, fd)[0], out)
    with pytest.raises(ValueError, match="share one device"):
        RN.gru(dev, x, hd, fd)


def test_composition_encode_gru_linear_passes_the_fp64_gate():
    """encode -> gru -> nn.Linear(128, 1) on five 3-step segments (A 3, K 5, D 35): the head's, the GRU's and the encoder's gradients against
    policy_reference.encoder + gru_reference in fp64.  The features [B L A, 128] are read in place as [B, A, L, 128] and dx is the encoder's
    d features."""
    A, K, D, B, L = 3, 5, 35, 5, 3
    _, critic = R.random_net(D, A, 91)
    obs, _ = R.random_obs(B * L, A, K, D, 92)
    o = {k: torch.as_tensor(v) for k, v in obs.items()}
    p, _, _, _, _, _ = GR.random_case(1, 1, 93)
    g = torch.Generator().manual_seed(94)
    h0, flags = 0.5 * torch.randn(B * A, H, generator=g), torch.rand(B, 1, L, generator=g) < 0.3
    hw, hb, dv = 0.1 * torch.randn(1, H, generator=g), torch.randn(1, generator=g), torch.randn(B, A, L, 1, generator=g)
    fl = flags.expand(B, A, L).reshape(B * A, L)

    def ref(dtype):
        q = {k: torch.as_tensor(v).to(dtype).requires_grad_(True) for k, v in critic.items() if k.startswith("base.")}
        r = {f: t.clone().to(dtype).requires_grad_(True) for f, t in p.items()}
        w, b = hw.clone().to(dtype).requires_grad_(True), hb.clone().to(dtype).requires_grad_(True)
        feats = R.encoder(q, "base.", o, dtype)                 # [B L, A, 128]
        x = feats.reshape(B, L, A, H).transpose(1, 2).reshape(B * A, L, H)
        out, _ = GR.forward(r, x, h0.to(dtype), fl.to(dtype))
        v = torch.nn.functional.linear(out, w, b)
        (v * dv.reshape(B * A, L, 1).to(dtype)).sum().backward()
        res = {"values": v.detach().double().numpy(), "head_w": w.grad.double().numpy(), "head_b": b.grad.double().numpy()}
        res.update({"gru." + f: t.grad.double().numpy() for f, t in r.items()})
        res.update({"enc." + P._ENCODER[k[len("base."):]]: t.grad.double().numpy() for k, t in q.items()})
        return res

    r64, r32 = ref(torch.float64), ref(torch.float32)
    for n, a in r64.items():
        assert a.any() or n == "enc.in_proj_b", n
    ep = {f: torch.as_tensor(critic["base." + k]).cuda().requires_grad_(True) for k, f in P._ENCODER.items() if "base." + k in critic}
    gp = {f: t.cuda().requires_grad_(True) for f, t in p.items()}
    head = nn.Linear(H, 1).cuda()
    with torch.no_grad():
        head.weight.copy_(hw)
        head.bias.copy_(hb)
    feats = EN.encode(ep, o["state_self"].cuda(), o["state_others"].cuda(), o["cylinders"].cuda())
    x4 = feats.view(B, L, A, H).transpose(1, 2)
    out, _ = RN.gru(gp, x4, h0.cuda(), flags.cuda())
    assert out.stride() == x4.stride()
    v = head(out)
    (v * dv.cuda()).sum().backward()
    got = {"values": v.detach().reshape(B * A, L, 1), "head_w": head.weight.grad, "head_b": head.bias.grad}
    got.update({"gru." + f: t.grad for f, t in gp.items()})
    got.update({"enc." + f: t.grad for f, t in ep.items()})
    assert set(got) == set(r64)
    _gate("composition", [(n, got[n].cpu().numpy(), r64[n], r32[n]) for n in r64])


def test_c_level_refusals_launch_nothing():
    S, L = 5, 3
    p, x, h0, flags, dy, dh = GR.random_case(S, L, 95)
    lib = abi.load_library()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dev = {f: t.cuda() for f, t in p.items()}
    x4, h0d, init = x.cuda().unsqueeze(1), h0.cuda(), flags.to(torch.uint8).cuda()
    out, hl, hist = (torch.full((n + 4,), CANARY, device="cuda") for n in (S * L * H, S * H, S * L * H))
    dx, dh0 = torch.full((S * L * H + 4,), CANARY, device="cuda"), torch.full((S * H + 4,), CANARY, device="cuda")
    flat = torch.full((RN.grad_layout()[1],), CANARY, device="cuda")
    dyd, dhd = dy.cuda(), dh.cuda()
    nb = lib.hns_gru_workspace_bytes(S, L, 1)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device="cuda")
    net, grd = RN._net(dev), RN._net(RN._views(flat))

    def seq(**kw):
        s = RN._seq(x4, h0d, init)
        for k, v in kw.items():
            if k.startswith("stride"):
                s.x_stride[int(k[-1])] = v
            else:
                setattr(s, k, v)
        return s

    def fwd(s=None, n=None, o=out.data_ptr(), h=hl.data_ptr(), hh=hist.data_ptr(), w=None):
        return lib.hns_gru_forward(C.byref(n if n is not None else net), C.byref(s if s is not None else seq()), o, h, hh, w, 0, st)

    def bwd(s=None, n=None, gr=None, hh=hist.data_ptr(), d=dyd.data_ptr(), dl=dhd.data_ptr(), x_=dx.data_ptr(), d0=dh0.data_ptr(), w=ws.data_ptr(), wb=nb):
        return lib.hns_gru_backward(C.byref(n if n is not None else net), C.byref(s if s is not None else seq()), hh, d, dl,
                                    C.byref(gr if gr is not None else grd), x_, d0, w, wb, st)

    def net_with(field, value, base=net):
        n = abi.HnsGruNet()
        C.memmove(C.byref(n), C.byref(base), C.sizeof(n))
        setattr(n, field, value)
        return n

    cases = [(lambda: lib.hns_gru_forward(None, C.byref(seq()), out.data_ptr(), hl.data_ptr(), None, None, 0, st), "null pointer"),
             (lambda: lib.hns_gru_backward(C.byref(net), None, hist.data_ptr(), dyd.data_ptr(), None, C.byref(grd), dx.data_ptr(), None, ws.data_ptr(), nb, st),
              "null pointer"),
             (lambda: fwd(n=net_with("weight_hh", None)), "parameter pointers"), (lambda: bwd(n=net_with("ln_b", dev["ln_b"].data_ptr() + 4)), "parameter pointers"),
             (lambda: bwd(gr=net_with("bias_ih", None, grd)), "gradient pointers"), (lambda: bwd(gr=net_with("weight_ih", flat.data_ptr() + 8, grd)), "gradient pointers"),
             (lambda: fwd(seq(x=None)), "x must be"), (lambda: bwd(seq(x=x4.data_ptr() + 4)), "x must be"),
             (lambda: fwd(seq(steps=0)), "steps must be in [1, 64]"), (lambda: fwd(seq(steps=65)), "steps must be in [1, 64]"),
             (lambda: bwd(seq(steps=65)), "steps must be in [1, 64]"), (lambda: bwd(seq(steps=-1)), "steps must be in [1, 64]"),
             (lambda: fwd(seq(outer=0)), "outer and inner"), (lambda: bwd(seq(inner=0)), "outer and inner"), (lambda: fwd(seq(inner=-2)), "outer and inner"),
             (lambda: fwd(seq(stride0=-384)), "strides must be"), (lambda: bwd(seq(stride2=-128)), "strides must be"), (lambda: fwd(seq(stride2=130)), "strides must be"),
             (lambda: fwd(seq(h0=h0d.data_ptr() + 4)), "h0 must be"),
             (lambda: fwd(o=None), "out and h_last"), (lambda: fwd(h=hl.data_ptr() + 4), "out and h_last"), (lambda: fwd(hh=hist.data_ptr() + 8), "h_hist must be"),
             (lambda: fwd(w=ws.data_ptr() + 16), "workspace must be"),
             (lambda: bwd(hh=None), "h_hist is required"), (lambda: bwd(d=None), "h_hist, dout and dx"), (lambda: bwd(x_=dx.data_ptr() + 4), "h_hist, dout and dx"),
             (lambda: bwd(dl=dhd.data_ptr() + 4), "dh_last and dh0"), (lambda: bwd(d0=dh0.data_ptr() + 4), "dh_last and dh0"),
             (lambda: bwd(w=None), "workspace must be"), (lambda: bwd(w=ws.data_ptr() + 16), "workspace must be"), (lambda: bwd(wb=nb - 1), "workspace too small")]
    for i, (call, text) in enumerate(cases):
        assert call() == abi.HNS_ERR_INVALID_ARG, (i, text)
        assert text in lib.hns_last_error().decode(), (i, text, lib.hns_last_error().decode())
    torch.cuda.synchronize()
    for t in (out, hl, hist, dx, dh0, flat):
        assert bool((t == CANARY).all())                        # nothing was launched
    # the optional pointers: no h_hist forward; no dh_last and no dh0 backward
    assert fwd(hh=None) == abi.HNS_OK and fwd() == abi.HNS_OK and bwd(dl=None, d0=None) == abi.HNS_OK
    torch.cuda.synchronize()
    assert bool((out[:S * L * H] != CANARY).all()) and bool((out[S * L * H:] == CANARY).all()) and bool((dh0 == CANARY).all())
    assert bool(torch.isfinite(flat).all()) and bool((flat != CANARY).all()) and bool((dx[:S * L * H] != CANARY).all())


def test_report_ratios():
    print("gru gate ratios (worst partition):", {k: round(v, 2) for k, v in RATIOS.items()})
    print("gru gate ratios (worst whole tensor):", {k: round(v, 2) for k, v in WHOLE.items()})
