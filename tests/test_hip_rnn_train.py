"""The recurrent update's head-and-loss kernels (hns_rnn_actor_head_grad, hns_rnn_critic_head_grad; csrc/hns_rnn_train.hip) and
hns_amd.rnn_train's update functions on an MI355X.

Accuracy gate (the rule of test_hip_critic_train.py, BAR = 8): for every scalar, log_probs / values, dy and each head gradient,
e_hip <= 8 max(e_32, 2^-24 max|ref_64|), errors as max-abs against fp64 autograd of the reference's statements (tests/rnn_update_reference.py),
e_32 the error of the same statements in CPU fp32.  Every case asserts first, in fp64, that no ratio lies within 1e-3 of 1 +- clip_param, that
no |v - b_values| lies within 1e-3 of clip_param and that the two mean value losses are apart (or, in the tie case, equal).

Shapes (csrc: kRtRows = 32 rows per trip of a workgroup, kRtMaxGroups = 512 workgroups): one row; 3 x 5 x 2, a partial workgroup; 2 x 16 x 3;
1 x 64 x 7, the largest L and A; 31, 32 and 33 rows; 512 x 32 + 1 rows, a second trip of workgroup 0.  y is given as the op's strided
[B, A, L, 128] view of [B L A, 128] and as a contiguous [S, L, 128]; segment is NULL, a permutation, and one with an out-of-range id.

The out-of-range id.  The entries take no row count of their own, so "the call without that segment at n = B L A" is checked against the
references: the fp64 / fp32 statements on the remaining segments, rescaled to n = B L A (every mean by (B - 1) / B, the entropy term's
constant gradient kept, explained_var from the live rows' sums with n = B L A), under the same gate; exactly: the bad segment's dy rows are
zeros, and two different bad ids (-1, num_segments + 7) give the same bits in every output.

Worst ratio per case (RATIOS, printed by test_report_ratios), recorded on an MI355X; the view and the contiguous layout of y gave the same
figure in every case:
    1x1x1 4.98   3x5x2 1.61   2x16x3 0.88   1x64x7 1.40   31x1x1 1.77   16x1x2 0.73   11x1x3 1.00   16385x1x1 4.07
    inside 1.00   outside 2.45   orig 1.00   clip 1.00   tie 1.00   mse 1.00   permutation 1.48   bad-id 2.05
    update-actor-a3k5d35 1.18   update-actor-a1k5d20 1.05   update-critic-a3k5d35 2.06   update-critic-a1k5d20 1.70"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import rnn_update_reference as U
from rnn_update_cases import rescaled as _rescaled          # the references on the kept segments at n = B L A (the module docstring)
from hns_amd import abi, rnn_train

pytestmark = pytest.mark.gpu

BAR = U.BAR
RATIOS = {}
R_ROWS, G_MAX = 32, 512                                         # csrc/hns_rnn_train.hip: kRtRows, kRtMaxGroups
H = 128
ACTOR_OUT = ("dy", "d_head_w", "d_head_b", "d_log_std", "policy_loss", "entropy", "ess", "log_probs")
CRITIC_OUT = ("dy", "d_head_w", "d_head_b", "value_loss", "explained_var", "values")


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


class Call:
    """The device tensors of one pair of calls: y in the chosen layout, the per-row arrays laid out as a rollout of `nseg` segments."""

    def __init__(self, c, strided=True, segment=None, nseg=None):
        B, L, A, _ = c["y"].shape
        self.B, self.L, self.A = B, L, A
        seg = np.arange(B) if segment is None else np.asarray(segment, np.int64)
        self.nseg = int(nseg if nseg is not None else B)
        ybuf = _dev(c["y"]) if strided else _dev(c["y"].transpose(0, 2, 1, 3))      # [B, L, A, 128] / [B, A, L, 128] contiguous
        self.y = ybuf.transpose(1, 2) if strided else ybuf                         # both: [B, A, L, 128]
        self.segment = _dev(seg) if segment is not None else None
        self.rows = {}
        for k in ("action", "log_probs_old", "advantages", "b_values", "b_returns"):
            roll = np.zeros((self.nseg * L,) + c[k].shape[2:], np.float32)
            for b, s in enumerate(seg):
                if 0 <= s < self.nseg:
                    roll[s * L:(s + 1) * L] = c[k][b]
            self.rows[k] = _dev(roll)
        self.head = {k: _dev(c[k]) for k in ("head_w", "head_b", "log_std", "v_w", "v_b")}

    def struct(self, y=None):
        y = self.y if y is None else y
        r = abi.HnsRnnRows()
        r.y = y.data_ptr()
        for d in range(3):
            r.y_stride[d] = y.stride(d) if y.shape[d] > 1 else 0
        r.outer, r.inner, r.steps = self.B, self.A, self.L
        r.segment = self.segment.data_ptr() if self.segment is not None else None
        r.num_segments = self.nseg
        return r

    def _dy(self):
        return torch.full_like(self.y, float("nan")) if self.y.is_contiguous() else \
            torch.full((self.B, self.L, self.A, H), float("nan"), device="cuda").transpose(1, 2)

    def actor(self, fill=None):
        lib = abi.load_library()
        nb = lib.hns_rnn_actor_head_workspace_bytes(self.B, self.A, self.L)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        if fill is not None:
            ws.fill_(fill)
        dy = self._dy()
        o = {"d_head_w": torch.empty(4, H, device="cuda"), "d_head_b": torch.empty(4, device="cuda"), "d_log_std": torch.empty(4, device="cuda"),
             "scal": torch.empty(3, device="cuda"), "log_probs": torch.full((self.B, self.L, self.A), float("nan"), device="cuda")}
        h, r, rows = self.head, self.rows, self.struct()
        rc = lib.hns_rnn_actor_head_grad(h["head_w"].data_ptr(), h["head_b"].data_ptr(), h["log_std"].data_ptr(), C.byref(rows), r["action"].data_ptr(),
                                         r["log_probs_old"].data_ptr(), r["advantages"].data_ptr(), 0.1, 1e-3, dy.data_ptr(), o["d_head_w"].data_ptr(),
                                         o["d_head_b"].data_ptr(), o["d_log_std"].data_ptr(), o["scal"][0:].data_ptr(), o["scal"][1:].data_ptr(),
                                         o["scal"][2:].data_ptr(), o["log_probs"].data_ptr(), ws.data_ptr(), nb, None)
        abi.check(rc, "hns_rnn_actor_head_grad")
        s = o.pop("scal").cpu().numpy()
        out = {k: v.cpu().numpy() for k, v in o.items()}
        out.update(dy=dy.transpose(1, 2).cpu().numpy(), policy_loss=s[0], entropy=s[1], ess=s[2])
        return out

    def critic(self, fill=None, loss="huber"):
        lib = abi.load_library()
        nb = lib.hns_rnn_critic_head_workspace_bytes(self.B, self.A, self.L)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        if fill is not None:
            ws.fill_(fill)
        dy = self._dy()
        o = {"d_head_w": torch.empty(1, H, device="cuda"), "d_head_b": torch.empty(1, device="cuda"), "scal": torch.empty(2, device="cuda"),
             "values": torch.full((self.B, self.L, self.A), float("nan"), device="cuda")}
        h, r, rows = self.head, self.rows, self.struct()
        rc = lib.hns_rnn_critic_head_grad(h["v_w"].data_ptr(), h["v_b"].data_ptr(), C.byref(rows), r["b_values"].data_ptr(), r["b_returns"].data_ptr(), 0.1,
                                          critic_loss(loss), 10.0, dy.data_ptr(), o["d_head_w"].data_ptr(), o["d_head_b"].data_ptr(),
                                          o["scal"][0:].data_ptr(), o["scal"][1:].data_ptr(), o["values"].data_ptr(), ws.data_ptr(), nb, None)
        abi.check(rc, "hns_rnn_critic_head_grad")
        s = o.pop("scal").cpu().numpy()
        out = {k: v.cpu().numpy() for k, v in o.items()}
        out.update(dy=dy.transpose(1, 2).cpu().numpy(), value_loss=s[0], explained_var=s[1])
        return out


def critic_loss(loss):
    return abi.HNS_CRITIC_LOSS_HUBER if loss == "huber" else abi.HNS_CRITIC_LOSS_MSE


def _gate(tag, c, tie=False, loss="huber", **call):
    a64, a32 = U.actor_head_autograd(c, torch.float64), U.actor_head_autograd(c, torch.float32)
    c64, c32 = U.critic_head_autograd(c, torch.float64, loss=loss), U.critic_head_autograd(c, torch.float32, loss=loss)
    U.assert_off_the_edges(a64, c64, tie=tie)
    assert np.array_equal(a64["w"], a32["w"]), f"{tag}: fp32 takes another side of the clip on some row"
    k = Call(c, **call)
    a, v = k.actor(), k.critic(loss=loss)
    one = c["y"].shape[0] * c["y"].shape[1] * c["y"].shape[2] == 1
    if one:                                                     # the unbiased variance of one return: NaN in the reference and on the device
        assert np.isnan(c64["explained_var"]) and np.isnan(v["explained_var"])
    items = [("actor." + n, a[n], a64[n], a32[n]) for n in ACTOR_OUT] + \
            [("critic." + n, v[n], c64[n], c32[n]) for n in CRITIC_OUT if not (one and n == "explained_var")]
    worst, bad = U.gate(tag, items)
    RATIOS[tag] = worst
    assert not bad, f"{tag}: " + "; ".join(bad)
    return k, a, v


SHAPES = [(1, 1, 1), (3, 5, 2), (2, 16, 3), (1, 64, 7), (R_ROWS - 1, 1, 1), (16, 1, 2), (11, 1, 3), (G_MAX * R_ROWS + 1, 1, 1)]


@pytest.mark.parametrize("B,L,A", SHAPES)
@pytest.mark.parametrize("strided", [True, False])
def test_head_entries_against_fp64_autograd(B, L, A, strided):
    assert B * L * A < 10 ** 5
    _gate(f"{B}x{L}x{A}-{'view' if strided else 'contiguous'}", U.head_case(B, L, A, 10 * B + L + A), strided=strided)


@pytest.mark.parametrize("variant", ["inside", "outside", "orig", "clip", "tie", "mse"])
def test_head_entries_at_the_clip_the_branches_and_the_tie(variant):
    bands = {"inside": ((0.0, 0.05),), "outside": ((0.15, 0.40),)}.get(variant, ((0.0, 0.05), (0.15, 0.40)))
    c = U.head_case(3, 5, 2, 77, bands=bands, branch=variant if variant in ("orig", "clip", "tie") else "orig")
    _gate(variant, c, tie=variant == "tie", loss="mse" if variant == "mse" else "huber")


def test_a_permutation_of_the_segments_reads_the_rollout_in_place_and_permutes_dy():
    B, L, A = 7, 5, 3
    c = U.head_case(B, L, A, 123)
    perm = np.array([3, 6, 0, 5, 1, 4, 2])
    # the minibatch in its own order b, the rollout holding segment perm[b]'s rows: the gate, with a rollout of more segments than the minibatch
    k, a, v = _gate("permutation", c, segment=perm + 2, nseg=B + 4)
    # the same rollout, the minibatch in another order: row b of the second call is row order[b] of the first
    order = np.array([2, 0, 1, 6, 4, 3, 5])
    c2 = dict(c)
    for name in ("y", "action", "log_probs_old", "advantages", "b_values", "b_returns"):
        c2[name] = c[name][order]
    a2 = Call(c2, segment=(perm + 2)[order], nseg=B + 4).actor()
    assert np.array_equal(a2["dy"], a["dy"][order]) and np.array_equal(a2["log_probs"], a["log_probs"][order])


def test_same_bits_twice_and_with_a_dirty_workspace():
    k = Call(U.head_case(37, 3, 2, 5))
    a1, a2, a3 = k.actor(), k.actor(fill=0xFF), k.actor(fill=0x7F)
    v1, v2, v3 = k.critic(), k.critic(fill=0xFF), k.critic(fill=0x7F)
    for x, y in ((a1, a2), (a1, a3), (v1, v2), (v1, v3)):
        for n in x:
            assert np.array_equal(x[n], y[n]), n


def test_an_out_of_range_segment_id_contributes_nothing():
    B, L, A = 6, 5, 3
    c = U.head_case(B, L, A, 321)
    bad_at, keep = 2, [0, 1, 3, 4, 5]
    (a64, c64), (a32, c32) = _rescaled(c, keep, torch.float64), _rescaled(c, keep, torch.float32)
    U.assert_off_the_edges(a64, c64)
    outs = []
    for bad in (-1, B + 7):
        seg = np.arange(B)
        seg[bad_at] = bad
        k = Call(c, segment=seg, nseg=B)
        outs.append((k.actor(), k.critic()))
    (a, v), (a_, v_) = outs
    for x, y in ((a, a_), (v, v_)):
        for n in x:
            assert np.array_equal(x[n], y[n], equal_nan=True), n    # (log_probs / values of the dead rows keep their NaN fill: not written)
    assert not a["dy"][bad_at].any() and not v["dy"][bad_at].any()
    assert np.isnan(a["log_probs"][bad_at]).all() and np.isnan(v["values"][bad_at]).all()
    items = [("actor." + n, a[n][keep] if n == "log_probs" else a[n], a64[n], a32[n]) for n in ACTOR_OUT] + \
            [("critic." + n, v[n][keep] if n == "values" else v[n], c64[n], c32[n]) for n in CRITIC_OUT]
    worst, bad = U.gate("bad-id", items)
    RATIOS["bad-id"] = worst
    assert not bad, "; ".join(bad)


REFUSALS = ("null_y", "misaligned_y", "misaligned_dy", "misaligned_weight", "misaligned_scalar", "outer_0", "inner_8", "steps_65", "negative_stride",
            "stride_not_4", "short_workspace", "misaligned_workspace", "null_workspace", "null_rows")


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals_return_an_error_and_launch_nothing(what):
    lib = abi.load_library()
    k = Call(U.head_case(3, 5, 2, 9))
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")                     # noqa: E731
    for actor in (True, False):
        size = lib.hns_rnn_actor_head_workspace_bytes if actor else lib.hns_rnn_critic_head_workspace_bytes
        nb = size(k.B, k.A, k.L)
        ws = torch.empty(nb + 256, dtype=torch.uint8, device="cuda")
        pad = nan(3 * 5 * 2 * H + 8)
        dy = pad[:3 * 5 * 2 * H].view(3, 5, 2, H).transpose(1, 2)
        outs = [nan(4 if actor else 1, H), nan(4 if actor else 1), nan(4), nan(4), nan(3, 5, 2)]
        rows = k.struct()
        hw = k.head["head_w" if actor else "v_w"]
        arg = dict(hw=hw.data_ptr(), dy=dy.data_ptr(), scal=outs[3].data_ptr(), ws=ws.data_ptr(), nb=nb, rows=C.byref(rows))
        if what == "null_y":
            rows.y = None
        elif what == "misaligned_y":
            rows.y = k.y.data_ptr() + 4
        elif what == "misaligned_dy":
            arg["dy"] = pad.data_ptr() + 4
        elif what == "misaligned_weight":
            arg["hw"] = torch.cat([hw.reshape(-1), hw.reshape(-1)])[1:].data_ptr()
        elif what == "misaligned_scalar":
            arg["scal"] = outs[3].data_ptr() + 2
        elif what == "outer_0":
            rows.outer = 0
        elif what == "inner_8":
            rows.inner = 8
        elif what == "steps_65":
            rows.steps = 65
        elif what == "negative_stride":
            rows.y_stride[2] = -rows.y_stride[2]
        elif what == "stride_not_4":
            rows.y_stride[0] = rows.y_stride[0] + 2
        elif what == "short_workspace":
            arg["nb"] = nb - 1
        elif what == "misaligned_workspace":
            arg["ws"] = ws.data_ptr() + 128
        elif what == "null_workspace":
            arg["ws"] = None
        elif what == "null_rows":
            arg["rows"] = None
        if what in ("outer_0", "inner_8", "steps_65"):
            assert size(rows.outer, rows.inner, rows.steps) == 0
        h, r = k.head, k.rows
        if actor:
            rc = lib.hns_rnn_actor_head_grad(arg["hw"], h["head_b"].data_ptr(), h["log_std"].data_ptr(), arg["rows"], r["action"].data_ptr(),
                                             r["log_probs_old"].data_ptr(), r["advantages"].data_ptr(), 0.1, 1e-3, arg["dy"], outs[0].data_ptr(),
                                             outs[1].data_ptr(), outs[2].data_ptr(), arg["scal"], outs[3][1:].data_ptr(), outs[3][2:].data_ptr(),
                                             outs[4].data_ptr(), arg["ws"], arg["nb"], None)
        else:
            rc = lib.hns_rnn_critic_head_grad(arg["hw"], h["v_b"].data_ptr(), arg["rows"], r["b_values"].data_ptr(), r["b_returns"].data_ptr(), 0.1,
                                              abi.HNS_CRITIC_LOSS_HUBER, 10.0, arg["dy"], outs[0].data_ptr(), outs[1].data_ptr(), arg["scal"],
                                              outs[3][1:].data_ptr(), outs[4].data_ptr(), arg["ws"], arg["nb"], None)
        assert rc != 0 and lib.hns_last_error().decode().startswith("hns_rnn_actor_head_grad:" if actor else "hns_rnn_critic_head_grad:")
        torch.cuda.synchronize()
        for t in (pad, *outs):
            assert torch.isnan(t).all(), what


# ---------------------------------------------------------------------------------------------------------------------------------------
# the update functions against the independent flow
@pytest.mark.parametrize("A,K,D", [(3, 5, 35), (1, 5, 20)])
@pytest.mark.parametrize("actor", [True, False])
def test_update_gradients_against_the_independent_flow(A, K, D, actor):
    N, T, L = 3, 8, 4
    a_net, c_net, obs, states, is_init = U.rollout_case(N, T, A, K, D, L, 900 + A)
    net = a_net if actor else c_net
    state = states["actor" if actor else "critic"]
    assert is_init[0, 0, 0] and is_init[N - 1, L // 2, 0] and np.abs(state).min() > 0
    rows = U.per_row_case(actor, N, T, A, 31, net, obs, state, is_init, L)
    seg = np.array([4, 0, 5, 2, 1], np.int64)
    g64, s64 = U.flow(net, actor, obs, state, is_init, rows, seg, L, torch.float64)
    g32, s32 = U.flow(net, actor, obs, state, is_init, rows, seg, L, torch.float32)
    if actor:
        d = np.minimum(np.abs(s64["ratio"] - 0.9), np.abs(s64["ratio"] - 1.1))
        assert d.min() >= U.MARGIN and np.array_equal(s64["w"], s32["w"])
    else:
        assert float(s64["dist"]) >= U.MARGIN and abs(float(s64["l_orig"] - s64["l_clip"])) >= 1e-3 * float(s64["value_loss"])
    live = {k: _dev(v) for k, v in net.items()}
    fn = rnn_train.policy_loss_and_grad_rnn if actor else rnn_train.value_loss_and_grad_rnn
    res = fn(live, _dev(obs["state_self"]), _dev(obs["state_others"]) if A > 1 else None, _dev(obs["cylinders"]), _dev(state), _dev(is_init),
             *(_dev(r) for r in rows), segment=_dev(seg), seq_len=L, **({"entropy_coef": 1e-3} if actor else {}))
    items = [(k, live[k].grad.cpu().numpy(), g64[k], g32[k]) for k in net]
    scal = (("policy_loss", res.policy_loss), ("entropy", res.entropy), ("ess", res.ess), ("log_probs", res.log_probs.squeeze(-1))) if actor else \
        (("value_loss", res.value_loss), ("explained_var", res.explained_var), ("values", res.values.squeeze(-1)))
    items += [(k, v.cpu().numpy(), s64[k], s32[k]) for k, v in scal]
    items.append(("grad_norm", res.grad_norm.cpu().numpy(), s64["grad_norm"], s32["grad_norm"]))
    tag = f"update-{'actor' if actor else 'critic'}-a{A}k{K}d{D}"
    worst, bad = U.gate(tag, items)
    RATIOS[tag] = worst
    assert not bad, "; ".join(bad)


def test_report_ratios():
    for tag, worst in sorted(RATIOS.items()):
        print(f"worst ratio {tag}: {worst:.2f}")
    assert all(math.isfinite(w) for w in RATIOS.values())
