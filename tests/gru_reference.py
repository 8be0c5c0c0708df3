"""The GRU block (include/hns.h: hns_gru_*; modules/rnn.py:44-89 with nn.GRUCell's statements) restated in torch at a given dtype, with autograd:
the reference of tests/test_gru.py (fp32: the golden fixture, the CPU node's bits) and tests/test_hip_gru.py (fp64: the accuracy gate).

    for t = 0 .. L - 1:  h <- h (1 - is_init[:, t]);  r, z = sigmoid(W_i{r,z} x_t + b_i{r,z} + W_h{r,z} h + b_h{r,z});
                         n = tanh(W_in x_t + b_in + r (W_hn h + b_hn));  h <- (1 - z) n + z h
    out = LayerNorm(stack(h) + x);  h_last = h

This is the project's own restatement; tests/golden/make_golden_gru.py executes the reference's class for the fixture.

Below it: the partition gate both test files use (`gate`), the cases of the device gate (`shape_case`, `flag_case`), and `emulate_kernel`, the
kernels' algorithm in fp32 with nine seedable defects (`DEFECTS`): the teeth of the gate, tests/test_gru.py."""
import numpy as np
import torch
import torch.nn.functional as F

H = 128
FIELDS = ("weight_ih", "weight_hh", "bias_ih", "bias_hh", "ln_w", "ln_b")
GRADS = FIELDS + ("dx", "dh0")


def forward(p, x, h0, is_init):
    """p: {field: tensor}; x [S, L, 128]; h0 [S, 128]; is_init [S, L] of 0 / 1 in x's dtype -> (out [S, L, 128], h_last [S, 128])."""
    h, outs = h0, []
    for t in range(x.shape[1]):
        h = h * (1 - is_init[:, t:t + 1])
        gi, gh = F.linear(x[:, t], p["weight_ih"], p["bias_ih"]), F.linear(h, p["weight_hh"], p["bias_hh"])
        i_r, i_z, i_n = gi.chunk(3, 1)
        h_r, h_z, h_n = gh.chunk(3, 1)
        r, z = torch.sigmoid(i_r + h_r), torch.sigmoid(i_z + h_z)
        n = torch.tanh(i_n + r * h_n)
        h = (1 - z) * n + z * h
        outs.append(h)
    return F.layer_norm(torch.stack(outs, 1) + x, (H,), p["ln_w"], p["ln_b"], 1e-5), h


def random_case(S, L, seed, flag_p=0.15, first_flag=None):
    """The accuracy gate's inputs (fp32 CPU tensors): orthogonal weights, biases 0.1 N(0, 1), LN weight 1 + 0.1 N, x ~ N(0, 1), h0 ~ 0.5 N, flags
    Bernoulli(flag_p), seeded dy and dh.  first_flag: is_init[0, 0] forced to it."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    p = {}
    for f in ("weight_ih", "weight_hh"):
        q, _ = torch.linalg.qr(rn(3 * H, H))                    # [384, 128] with orthonormal columns: what nn.init.orthogonal_ makes
        p[f] = q.contiguous()
    p["bias_ih"], p["bias_hh"] = 0.1 * rn(3 * H), 0.1 * rn(3 * H)
    p["ln_w"], p["ln_b"] = 1.0 + 0.1 * rn(H), 0.1 * rn(H)
    x, h0 = rn(S, L, H), 0.5 * rn(S, H)
    flags = (torch.rand(S, L, generator=g) < flag_p)
    if first_flag is not None:
        flags[0, 0] = bool(first_flag)
    return p, x, h0, flags, rn(S, L, H), rn(S, H)


def run(p, x, h0, flags, dy, dh, dtype):
    """(out, h_last, {gradient name: array}) of sum(out dy) + sum(h_last dh) at `dtype`, as fp64 numpy."""
    q = {f: t.detach().to(dtype).requires_grad_(True) for f, t in p.items()}
    xl, hl = x.detach().to(dtype).requires_grad_(True), h0.detach().to(dtype).requires_grad_(True)
    out, h = forward(q, xl, hl, flags.to(dtype))
    ((out * dy.to(dtype)).sum() + (h * dh.to(dtype)).sum()).backward()
    grads = {f: q[f].grad.double().numpy() for f in FIELDS}
    grads["dx"], grads["dh0"] = xl.grad.double().numpy(), hl.grad.double().numpy()
    return out.detach().double().numpy(), h.detach().double().numpy(), grads


# ---------------------------------------------------------------------------------------------------------------------------------------
# The partition gate: the same rule and the same bar, the bound from the partition's OWN e_32 and max|ref_64|.  The r, z and n thirds of the
# 384-row tensors differ by an order of magnitude in size and in fp32 error, and so do the steps of out and dx: under a whole-tensor bound an
# error of 100 x fp32's own in the smallest partition passes.  A partition pass implies the whole-tensor pass (max over the partitions of e
# <= bar max over the partitions of the bound).
BAR = 8.0
THIRDS = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def partitions(name, shape):
    """[(label, index)] of tensor `name` (a `gru.` prefix allowed): the gate thirds of the 384-row tensors, out and dx ([S, L, 128]) per step,
    the whole tensor for the rest."""
    base = name[len("gru."):] if name.startswith("gru.") else name
    if base in THIRDS:
        assert shape[0] == 3 * H, (name, shape)
        return [(f"{name}[{g}]", slice(k * H, (k + 1) * H)) for k, g in enumerate("rzn")]
    if base in ("out", "dx") and len(shape) == 3:
        return [(f"{name}[t={t}]", (slice(None), t)) for t in range(shape[1])]
    return [(name, Ellipsis)]


def _ratio(e, bound):
    return e / bound if bound > 0 else (0.0 if e == 0 else float("inf"))


def gate_ratios(name, got, r64, r32, zero=False):
    """(whole-tensor ratio, {partition label: ratio}) of e / max(e_32, 2^-24 max|ref_64|).  zero: the fp64 reference must be identically zero
    and `got` exactly zero (ratio 0, else inf); otherwise every partition's reference must be non-zero, or the partition gates nothing."""
    got, r64, r32 = np.asarray(got, np.float64), np.asarray(r64, np.float64), np.asarray(r32, np.float64)
    assert got.shape == r64.shape == r32.shape, (name, got.shape, r64.shape, r32.shape)
    assert np.isfinite(got).all(), f"{name}: not finite"
    if zero:
        assert not r64.any(), f"{name}: expected an identically zero fp64 reference"
        r = 0.0 if not got.any() else float("inf")
        return r, {name: r}
    err, e32 = np.abs(got - r64), np.abs(r32 - r64)
    whole = _ratio(float(err.max()), max(float(e32.max()), 2.0 ** -24 * float(np.abs(r64).max())))
    parts = {}
    for label, idx in partitions(name, r64.shape):
        top = float(np.abs(r64[idx]).max())
        assert top > 0, f"{label}: the fp64 reference is identically zero, the partition gates nothing"
        parts[label] = _ratio(float(err[idx].max()), max(float(e32[idx].max()), 2.0 ** -24 * top))
    return whole, parts


def gate(tag, items, zero=(), bar=BAR, verbose=True):
    """items: (name, value, fp64 reference, fp32 reference).  -> (worst partition ratio, worst whole-tensor ratio, [failures]); names in `zero`
    must be exactly zero against an identically zero reference."""
    worst, worst_whole, bad = 0.0, 0.0, []
    for name, got, r64, r32 in items:
        whole, parts = gate_ratios(name, got, r64, r32, zero=name in zero)
        label, top = max(parts.items(), key=lambda kv: kv[1])
        if verbose:
            a = np.asarray(r64, np.float64)
            e, e32 = np.abs(np.asarray(got, np.float64) - a).max(), np.abs(np.asarray(r32, np.float64) - a).max()
            print(f"  {tag} {name}: e {e:.3e} e_32 {e32:.3e} max|ref| {np.abs(a).max():.3e} ratio {whole:.2f} (whole tensor); worst partition {label} {top:.2f}")
        worst, worst_whole = max(worst, top), max(worst_whole, whole)
        bad += [f"{l}: ratio {r:.3g} > {bar}" for l, r in parts.items() if not r <= bar]
    return worst, worst_whole, bad


# the cases the device gate runs (test_hip_gru.py), shared with the CPU emulation (test_gru.py)
CASES = [(37, 16), (1, 16), (15, 2), (16, 3), (17, 1), (33, 1), (5, 17), (3, 64)]
FLAG_PATTERNS = ("first", "last", "all", "none", "mixed")
FLAG_ZERO = {"first": ("dh0",), "all": ("weight_hh", "dh0")}      # identically zero by construction: every operand is a masked zero


def shape_case(S, L):
    """The (S, L) case of the gate: seed 2000 + 100 S + L; S = 1 with is_init[0, 0] = 0 (or its dh0 is identically zero)."""
    return random_case(S, L, 2000 + 100 * S + L, first_flag=0 if S == 1 else None)


def flag_case(pattern):
    S, L = 18, 4
    p, x, h0, _, dy, dh = random_case(S, L, 51)
    flags = torch.zeros(S, L, dtype=torch.bool)
    if pattern == "first":
        flags[:, 0] = True
    elif pattern == "last":
        flags[:, L - 1] = True
    elif pattern == "all":
        flags[:] = True
    elif pattern == "mixed":
        flags[::3, 0] = True
        flags[1::4, 2] = True
    else:
        assert pattern == "none", pattern
    return p, x, h0, flags, dy, dh


# ---------------------------------------------------------------------------------------------------------------------------------------
# The kernels' algorithm (csrc/hns_gru.hip) in fp32, vectorised over the sequences: not autograd.  It keeps what the kernels decide — the x
# products before the h products on b_i + b_h, 1 / (1 + exp(-a)), the gates recomputed in the backward sweep from h_hist, the LayerNorm
# backward formula, the four gate gradients, the weight gradients as 32-row-tile partials grouped tps per split and summed in fp64 in index
# order, the LayerNorm gradients as per-workgroup partials over the tiles g, g + 256, ... — and not the MFMA's rounding order inside a product.
TILE, MAX_GROUPS, WG_ROWS, MAX_SPLITS, EPS = 16, 256, 32, 256, 1e-5


def plan(S, L):
    """gru_plan's arithmetic: tiles of 16 sequences, workgroups, weight-gradient tiles of 32 rows, tiles per split, splits."""
    tiles = -(-S // TILE)
    wg_tiles = -(-S * L // WG_ROWS)
    tps = -(-wg_tiles // MAX_SPLITS)
    return {"tiles": tiles, "groups": min(tiles, MAX_GROUPS), "rows": S * L, "wg_tiles": wg_tiles, "tps": tps, "splits": -(-wg_tiles // tps)}


DEFECTS = ("mask_after_cell", "dh_unmasked", "hn_from_an", "bhn_outside_r", "dar_without_bhn", "dx_without_ln_term", "stale_state_second_trip",
           "last_split_dropped", "ln_partials_first_trip_only")


def _sigm(a):
    return 1.0 / (1.0 + torch.exp(-a))


def _cell(p, x, hp, defect):
    """One step's gates from x_t and the masked h_{t-1}: (r, z, n, a_hn, h_t)."""
    wi, wh, bi, bh = p["weight_ih"], p["weight_hh"], p["bias_ih"], p["bias_hh"]
    a_r = ((bi[:H] + bh[:H]) + x @ wi[:H].T) + hp @ wh[:H].T
    a_z = ((bi[H:2 * H] + bh[H:2 * H]) + x @ wi[H:2 * H].T) + hp @ wh[H:2 * H].T
    a_in = bi[2 * H:] + x @ wi[2 * H:].T
    if defect == "bhn_outside_r":
        a_hn = hp @ wh[2 * H:].T
        r, z = _sigm(a_r), _sigm(a_z)
        n = torch.tanh(a_in + r * a_hn + bh[2 * H:])
    else:
        a_hn = bh[2 * H:] + hp @ wh[2 * H:].T
        r, z = _sigm(a_r), _sigm(a_z)
        n = torch.tanh(a_in + r * a_hn)
    return r, z, n, a_hn, (1.0 - z) * n + z * hp


def _norm(y):
    mean = y.sum(1, keepdim=True) * (1.0 / H)
    yc = y - mean
    rstd = 1.0 / torch.sqrt((yc * yc).sum(1, keepdim=True) * (1.0 / H) + EPS)
    return yc * rstd, rstd


def emulate_kernel(p, x, h0, flags, dy, dh, defect=None):
    """(out, h_last, {gradient name: array}) as fp64 numpy, the layout of `run`.  `defect` seeds one subtle error (DEFECTS)."""
    assert defect is None or defect in DEFECTS, defect
    f32 = torch.float32
    p = {f: t.detach().to(f32) for f, t in p.items()}
    x, h0, dy, dh = x.detach().to(f32), h0.detach().to(f32), dy.detach().to(f32), dh.detach().to(f32)
    S, L, _ = x.shape
    pl = plan(S, L)
    keep = (~flags).to(f32)                                     # m = 1 - is_init
    trip = torch.arange(S) // (TILE * MAX_GROUPS)               # the trip of its workgroup's loop on which a sequence's tile is reached
    with torch.no_grad():
        # forward (hns_gru_fwd_kernel)
        h = h0.clone()
        hist, outs = [], []
        for t in range(L):
            m = keep[:, t:t + 1]
            hp = h if defect == "mask_after_cell" else h * m
            _, _, _, _, h = _cell(p, x[:, t], hp, defect)
            if defect == "mask_after_cell":
                h = h * m
            xh, _ = _norm(h + x[:, t])
            outs.append(xh * p["ln_w"] + p["ln_b"])
            hist.append(h)
        if defect == "stale_state_second_trip":
            # a later trip's tile starts from what the same lanes of the workgroup's previous tile left in the registers, not from h0
            for k in range(1, -(-pl["tiles"] // MAX_GROUPS)):
                idx = torch.nonzero(trip == k).flatten()
                hs = hist[L - 1][idx - TILE * MAX_GROUPS].clone()
                for t in range(L):
                    _, _, _, _, hs = _cell(p, x[idx, t], hs * keep[idx, t:t + 1], defect)
                    xh, _ = _norm(hs + x[idx, t])
                    outs[t][idx] = xh * p["ln_w"] + p["ln_b"]
                    hist[t][idx] = hs
            h = hist[L - 1]
        out, h_last, hist = torch.stack(outs, 1), h, torch.stack(hist, 1)

        # backward sweep (hns_gru_bwd_kernel): gates recomputed from x_t and h_{t-1}
        d = dh.clone()
        dgate = torch.zeros(S, L, 4, H)
        hprev = torch.zeros(S, L, H)
        dx = torch.zeros(S, L, H)
        dlnw, dlnb = torch.zeros(S, H), torch.zeros(S, H)       # per lane: the sequence's sums over t, then over the workgroup's tiles
        for t in range(L - 1, -1, -1):
            m = keep[:, t:t + 1]
            hp = hist[:, t - 1] if t > 0 else h0
            if defect != "mask_after_cell":
                hp = hp * m
            r, z, n, a_hn, hn = _cell(p, x[:, t], hp, defect)
            xh, rstd = _norm(hn + x[:, t])
            g = dy[:, t] * p["ln_w"]
            dlnw += dy[:, t] * xh
            dlnb += dy[:, t]
            mg, mgx = g.sum(1, keepdim=True) * (1.0 / H), (g * xh).sum(1, keepdim=True) * (1.0 / H)
            dyt = rstd * ((g - mg) - xh * mgx)
            dht = d + dyt
            dn, dz = dht * (1.0 - z), dht * (hp - n)
            dan = dn * (1.0 - n * n)
            daz = dz * (z * (1.0 - z))
            hn_term = a_hn - p["bias_hh"][2 * H:] if defect == "dar_without_bhn" else a_hn
            dar = (dan * hn_term) * (r * (1.0 - r))
            dahn = dan * r
            dgate[:, t, 0], dgate[:, t, 1], dgate[:, t, 2], dgate[:, t, 3] = dar, daz, dan, dahn
            hprev[:, t] = hp
            dxa = torch.cat([dar, daz, dan], 1) @ p["weight_ih"]
            dx[:, t] = dxa if defect == "dx_without_ln_term" else dxa + dyt
            d = torch.cat([dar, daz, dahn], 1) @ p["weight_hh"] + dht * z
            if defect != "dh_unmasked":
                d = d * m
        dh0 = d

        # LayerNorm gradients: workgroup g's lanes accumulate over its tiles g, g + 256, ..., then the 16 sequences; fp64 over the workgroups
        trips = -(-pl["tiles"] // MAX_GROUPS)
        lane = torch.zeros(2, trips * MAX_GROUPS * TILE, H)
        lane[0, :S], lane[1, :S] = dlnw, dlnb
        lane = lane.view(2, trips, MAX_GROUPS, TILE, H)
        acc = lane[:, 0].clone()
        for k in range(1, trips):
            if defect != "ln_partials_first_trip_only":
                acc += lane[:, k]
        ln = acc.sum(2)[:, :pl["groups"]].double().sum(1)        # [2, 128]

        # weight gradients (hns_gru_wgrad_kernel): matrix m's dA block and operand, 32-row tiles, tps tiles per split in one fp32 accumulator
        rows, tps, splits = pl["rows"], pl["tps"], pl["splits"]
        pad = splits * tps * WG_ROWS

        def tiled(a):
            b = torch.zeros(pad, H)
            b[:rows] = a.reshape(rows, H)
            return b.view(splits, tps, WG_ROWS, H)

        ops = (tiled(x), tiled(hprev))
        blocks = [tiled(dgate[:, :, k]) for k in range(4)]
        grads = {}
        use = splits - 1 if defect == "last_split_dropped" and splits > 1 else splits
        for mi in range(6):
            blk = mi if mi < 3 else (3 if mi == 5 and defect != "hn_from_an" else mi - 3)
            da, op = blocks[blk], ops[0 if mi < 3 else 1]
            part, bias = torch.zeros(splits, H, H), torch.zeros(splits, H)
            for j in range(tps):
                part += da[:, j].transpose(1, 2) @ op[:, j]
                bias += da[:, j].sum(1)
            w64, b64 = torch.zeros(H, H, dtype=torch.float64), torch.zeros(H, dtype=torch.float64)
            for s in range(use):
                w64 += part[s].double()
                b64 += bias[s].double()
            grads[mi] = (w64.float(), b64.float())
    res = {"weight_ih": torch.cat([grads[k][0] for k in range(3)]), "weight_hh": torch.cat([grads[k][0] for k in range(3, 6)]),
           "bias_ih": torch.cat([grads[k][1] for k in range(3)]), "bias_hh": torch.cat([grads[k][1] for k in range(3, 6)]),
           "ln_w": ln[0].float(), "ln_b": ln[1].float(), "dx": dx, "dh0": dh0}
    return out.double().numpy(), h_last.double().numpy(), {k: v.double().numpy() for k, v in res.items()}
