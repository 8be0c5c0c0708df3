"""The data-parallel recurrent update's device entries on an MI355X: hns_rnn_critic_head_sums,
hns_rnn_critic_head_grad_global, hns_rnn_actor_head_grad_global, rnn_train's global forms, learner.DataParallelRecurrentLearner.

  one-rank bits        with one rank (global_rows = B L A, entropy_share 1, sums = the call's own hns_rnn_critic_head_sums output) every output
                       of the three entries — dy, the head gradients, the scalars, values, log_probs — has the bits of the two local entries:
                       1 x 1 x 1; 5 x 4 x 3 (60 rows, inside one trip); 11 x 3 x 7 (231 rows, no multiple of 32); 2 x 64 x 2; 172 x 16 x 6
                       (16 512 rows > 512 x 32: past one trip of the grid) — through the op's strided [B, A, L, 128] view and through the
                       contiguous layout; guard rows around dy and around sums keep their fill.
  two emulated ranks   B split 5 + 11 (L 4, A 3) and 1 + 171 (L 16, A 6): the parts' sums added in fp64, global_rows the union's row count.
                       value_loss and explained_var are equal on both parts bit for bit; the concatenated dy, log_probs and values, the
                       summed head gradients (entropy_share 1/2 each) and the summed policy_loss shares meet the gate
                       e <= 8 max(e_32, 2^-24 max|ref_64|) against fp64 autograd of the reference's statements over the union
                       (rnn_update_reference); once more with a dead segment id in part 1: n stays global_rows, the reference is rescaled
                       (dp_rnn_reference.rescale_dead).  assert_off_the_edges holds on every union in fp64.
  branch               dp_rnn_reference.branch_flip_case: part 0's dy follows the union's branch (the precondition asserted first).
  refusals             NULL or misaligned sums, global_rows < rows, a NaN / infinite entropy_share, and the local entries' own refusals
                       spot-checked on the new names: an error, the outputs keep their fill.
  learner              a one-rank gloo group (file store) against RecurrentDeviceLearner without a group: the info row and every parameter
                       bit-identical; two real ranks on one card over gloo (tests/dp_rnn_learner_job.py, one child process a rank, each
                       under its own time limit): the ranks end bit-identical with equal info rows."""
import ctypes as C
import importlib.util
import json
import os
import queue
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import dp_rnn_reference as DU
import rnn_update_reference as U
import test_hip_rnn_train as TR
from hns_amd import abi, collector, learner, tp_train
from hns_amd import policy as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 128
GUARD = 64                                                      # guard floats around dy (16-byte aligned), guard doubles: 2
FILL = -7.5
_dev = TR._dev


class GCall(TR.Call):
    """TR.Call with the three global entries.  dy lies between two guard runs, sums between two guard pairs; `check_guards` asserts them."""

    def _guarded_dy(self):
        n = self.B * self.L * self.A * H
        buf = torch.full((n + 2 * GUARD,), FILL, device="cuda")
        body = buf[GUARD:GUARD + n]
        dy = body.view(self.B, self.A, self.L, H) if self.y.is_contiguous() else body.view(self.B, self.L, self.A, H).transpose(1, 2)
        assert dy.data_ptr() % 16 == 0
        return buf, dy

    @staticmethod
    def check_guards(buf, n):
        assert (buf[:GUARD] == FILL).all() and (buf[GUARD + n:] == FILL).all(), "a guard row was written"

    def _critic_ws(self, fill):
        lib = abi.load_library()
        nb = lib.hns_rnn_critic_head_workspace_bytes(self.B, self.A, self.L)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        if fill is not None:
            ws.fill_(fill)
        return lib, nb, ws

    def sums(self, fill=0xFF, loss="huber"):
        lib, nb, ws = self._critic_ws(fill)
        box = torch.full((9,), FILL, dtype=torch.float64, device="cuda")
        sums = box[2:7]
        values = torch.full((self.B, self.L, self.A), float("nan"), device="cuda")
        h, r, rows = self.head, self.rows, self.struct()
        rc = lib.hns_rnn_critic_head_sums(h["v_w"].data_ptr(), h["v_b"].data_ptr(), C.byref(rows), r["b_values"].data_ptr(), r["b_returns"].data_ptr(), 0.1,
                                          TR.critic_loss(loss), 10.0, sums.data_ptr(), values.data_ptr(), ws.data_ptr(), nb, None)
        abi.check(rc, "hns_rnn_critic_head_sums")
        torch.cuda.synchronize()
        assert (box[:2] == FILL).all() and (box[7:] == FILL).all(), "a guard around sums was written"
        return sums.clone(), values.cpu().numpy()

    def critic_global(self, sums, global_rows, fill=0x7F, loss="huber"):
        lib, nb, ws = self._critic_ws(fill)                     # its own workspace, dirty: the call stands alone
        buf, dy = self._guarded_dy()
        o = {"d_head_w": torch.empty(1, H, device="cuda"), "d_head_b": torch.empty(1, device="cuda"), "scal": torch.empty(2, device="cuda")}
        values = torch.full((self.B, self.L, self.A), float("nan"), device="cuda")
        h, r, rows = self.head, self.rows, self.struct()
        rc = lib.hns_rnn_critic_head_grad_global(h["v_w"].data_ptr(), h["v_b"].data_ptr(), C.byref(rows), r["b_values"].data_ptr(), r["b_returns"].data_ptr(),
                                                 0.1, TR.critic_loss(loss), 10.0, dy.data_ptr(), o["d_head_w"].data_ptr(), o["d_head_b"].data_ptr(),
                                                 o["scal"][0:].data_ptr(), o["scal"][1:].data_ptr(), values.data_ptr(), ws.data_ptr(), nb, None,
                                                 sums.data_ptr(), int(global_rows))
        abi.check(rc, "hns_rnn_critic_head_grad_global")
        torch.cuda.synchronize()
        self.check_guards(buf, self.B * self.L * self.A * H)
        assert torch.isnan(values).all()                         # `values` is not written by the global entry
        s = o.pop("scal").cpu().numpy()
        out = {k: v.cpu().numpy() for k, v in o.items()}
        out.update(dy=dy.transpose(1, 2).cpu().numpy(), value_loss=s[0], explained_var=s[1])
        return out

    def actor_global(self, global_rows, share, fill=0x7F):
        lib = abi.load_library()
        nb = lib.hns_rnn_actor_head_workspace_bytes(self.B, self.A, self.L)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda").fill_(fill)
        buf, dy = self._guarded_dy()
        o = {"d_head_w": torch.empty(4, H, device="cuda"), "d_head_b": torch.empty(4, device="cuda"), "d_log_std": torch.empty(4, device="cuda"),
             "scal": torch.empty(3, device="cuda"), "log_probs": torch.full((self.B, self.L, self.A), float("nan"), device="cuda")}
        h, r, rows = self.head, self.rows, self.struct()
        rc = lib.hns_rnn_actor_head_grad_global(h["head_w"].data_ptr(), h["head_b"].data_ptr(), h["log_std"].data_ptr(), C.byref(rows), r["action"].data_ptr(),
                                                r["log_probs_old"].data_ptr(), r["advantages"].data_ptr(), 0.1, 1e-3, dy.data_ptr(), o["d_head_w"].data_ptr(),
                                                o["d_head_b"].data_ptr(), o["d_log_std"].data_ptr(), o["scal"][0:].data_ptr(), o["scal"][1:].data_ptr(),
                                                o["scal"][2:].data_ptr(), o["log_probs"].data_ptr(), ws.data_ptr(), nb, None, int(global_rows), float(share))
        abi.check(rc, "hns_rnn_actor_head_grad_global")
        torch.cuda.synchronize()
        self.check_guards(buf, self.B * self.L * self.A * H)
        s = o.pop("scal").cpu().numpy()
        out = {k: v.cpu().numpy() for k, v in o.items()}
        out.update(dy=dy.transpose(1, 2).cpu().numpy(), policy_loss=s[0], entropy=s[1], ess=s[2])
        return out


def _bits(tag, got, want, names):
    for n in names:
        assert got[n].shape == want[n].shape and got[n].tobytes() == want[n].tobytes(), f"{tag}: {n} differs from the local entry"


SHAPES = [(1, 1, 1), (5, 4, 3), (11, 3, 7), (2, 64, 2), (172, 16, 6)]
_CASES = {}


def _case(B, L, A):
    if (B, L, A) not in _CASES:
        _CASES[(B, L, A)] = U.head_case(B, L, A, 10 * B + L + A)
    return _CASES[(B, L, A)]


@pytest.mark.parametrize("B,L,A", SHAPES)
@pytest.mark.parametrize("strided", [True, False])
def test_one_rank_global_entries_have_the_bits_of_the_local_entries(B, L, A, strided):
    rows = B * L * A
    assert (rows > TR.G_MAX * TR.R_ROWS) == (B == 172) and (rows % TR.R_ROWS != 0) == ((B, L, A) in ((1, 1, 1), (5, 4, 3), (11, 3, 7)))
    k = GCall(_case(B, L, A), strided=strided)
    a, v = k.actor(), k.critic()
    sums, values = k.sums()
    vg = k.critic_global(sums, rows)
    ag = k.actor_global(rows, 1.0)
    tag = f"{B}x{L}x{A}-{'view' if strided else 'contiguous'}"
    _bits(tag + " actor", ag, a, TR.ACTOR_OUT)
    _bits(tag + " critic", vg, v, [n for n in TR.CRITIC_OUT if n != "values"])
    assert values.tobytes() == v["values"].tobytes(), f"{tag}: values of the sums entry"
    assert torch.isfinite(sums).all()
    # the same inputs give the same bits, whatever the workspace held
    s2, _ = k.sums(fill=0x11)
    assert torch.equal(sums, s2)
    _bits(tag + " again", k.critic_global(sums, rows, fill=0x11), vg, [n for n in TR.CRITIC_OUT if n != "values"])


def _two_parts(c, sizes, dead=None):
    """The parts' calls of one emulated two-rank update; `dead`: (part, b) whose segment id is out of range.  Returns what a SUM all-reduce
    and a concatenation give, and the parts' scalars."""
    parts, ids = DU.split(c, sizes), DU.segment_ids(sizes)
    B = sum(sizes)
    rows = int(np.prod(c["y"].shape[:3]))
    calls = []
    for r, (p, seg) in enumerate(zip(parts, ids)):
        seg = seg.copy()
        if dead is not None and dead[0] == r:
            seg[dead[1]] = B + 3
        calls.append(GCall(p, segment=seg, nseg=B))
    own = [k.sums() for k in calls]
    union = own[0][0] + own[1][0]                                # the all-reduce of two ranks: one fp64 addition per value
    v = [k.critic_global(union, rows) for k in calls]
    a = [k.actor_global(rows, 0.5) for k in calls]
    cat = lambda xs: np.concatenate(xs)                          # noqa: E731
    add = lambda x, y: (x.astype(np.float32) + y.astype(np.float32))      # noqa: E731  (the all-reduce: one fp32 addition per entry)
    out_a = {"dy": cat([x["dy"] for x in a]), "log_probs": cat([x["log_probs"] for x in a]),
             "policy_loss": np.float64(a[0]["policy_loss"]) + np.float64(a[1]["policy_loss"]), "entropy": a[0]["entropy"]}
    out_a.update({n: add(a[0][n], a[1][n]) for n in ("d_head_w", "d_head_b", "d_log_std")})
    out_v = {"dy": cat([x["dy"] for x in v]), "values": cat([x[1] for x in own]), "value_loss": v[0]["value_loss"], "explained_var": v[0]["explained_var"]}
    out_v.update({n: add(v[0][n], v[1][n]) for n in ("d_head_w", "d_head_b")})
    return out_a, out_v, a, v


@pytest.mark.parametrize("sizes,L,A", [((5, 11), 4, 3), ((1, 171), 16, 6)])
def test_two_emulated_ranks_meet_the_gate_over_the_union(sizes, L, A):
    c = _case(sum(sizes), L, A) if sum(sizes) == 172 else U.head_case(sum(sizes), L, A, 2024)
    a64, a32 = U.actor_head_autograd(c, torch.float64), U.actor_head_autograd(c, torch.float32)
    c64, c32 = U.critic_head_autograd(c, torch.float64), U.critic_head_autograd(c, torch.float32)
    U.assert_off_the_edges(a64, c64)
    assert np.array_equal(a64["w"], a32["w"])
    out_a, out_v, a, v = _two_parts(c, sizes)
    assert v[0]["value_loss"].tobytes() == v[1]["value_loss"].tobytes() and v[0]["explained_var"].tobytes() == v[1]["explained_var"].tobytes()
    assert a[0]["entropy"].tobytes() == a[1]["entropy"].tobytes()
    items = [("actor." + n, out_a[n], a64[n], a32[n]) for n in ("dy", "d_head_w", "d_head_b", "d_log_std", "policy_loss", "entropy", "log_probs")] + \
            [("critic." + n, out_v[n], c64[n], c32[n]) for n in ("dy", "d_head_w", "d_head_b", "value_loss", "explained_var", "values")]
    worst, bad = U.gate(f"{sizes[0]}+{sizes[1]}", items)
    assert not bad, "; ".join(bad)


def test_a_dead_segment_in_one_part_leaves_n_at_global_rows():
    sizes, L, A = (5, 11), 4, 3
    c = U.head_case(sum(sizes), L, A, 2024)
    rows = sum(sizes) * L * A
    dead_b = sizes[0] + 4                                        # segment 4 of part 1
    keep = [b for b in range(sum(sizes)) if b != dead_b]
    (a64, c64), (a32, c32) = DU.rescale_dead(c, keep, rows, torch.float64), DU.rescale_dead(c, keep, rows, torch.float32)
    U.assert_off_the_edges(a64, c64)
    assert np.array_equal(a64["w"], a32["w"])
    out_a, out_v, a, v = _two_parts(c, sizes, dead=(1, 4))
    assert not out_a["dy"][dead_b].any() and not out_v["dy"][dead_b].any()
    assert np.isnan(out_a["log_probs"][dead_b]).all() and np.isnan(out_v["values"][dead_b]).all()          # a dead row's are not written
    assert v[0]["value_loss"].tobytes() == v[1]["value_loss"].tobytes() and v[0]["explained_var"].tobytes() == v[1]["explained_var"].tobytes()
    live = lambda x: x[keep]                                     # noqa: E731
    full = U.actor_head_autograd(c, torch.float64), U.critic_head_autograd(c, torch.float64)
    full32 = U.actor_head_autograd(c, torch.float32), U.critic_head_autograd(c, torch.float32)
    items = [("actor." + n, out_a[n], a64[n], a32[n]) for n in ("dy", "d_head_w", "d_head_b", "d_log_std", "policy_loss", "entropy")] + \
            [("critic." + n, out_v[n], c64[n], c32[n]) for n in ("dy", "d_head_w", "d_head_b", "value_loss", "explained_var")] + \
            [("actor.log_probs", live(out_a["log_probs"]), live(full[0]["log_probs"]), live(full32[0]["log_probs"])),
             ("critic.values", live(out_v["values"]), live(full[1]["values"]), live(full32[1]["values"]))]
    worst, bad = U.gate("dead segment", items)
    assert not bad, "; ".join(bad)


def test_part_0_follows_the_unions_branch():
    sizes = (5, 11)
    c, parts = DU.branch_flip_case(sizes, 4, 3, 4242)
    c64 = DU.assert_branch_precondition(c, parts)
    c32 = U.critic_head_autograd(c, torch.float32)
    rows = int(np.prod(c["y"].shape[:3]))
    calls = [GCall(p, segment=seg, nseg=sum(sizes)) for p, seg in zip(parts, DU.segment_ids(sizes))]
    own = [k.sums()[0] for k in calls]
    v = [k.critic_global(own[0] + own[1], rows) for k in calls]
    B0 = sizes[0]
    items = [("dy part 0", v[0]["dy"], c64["dy"][:B0], c32["dy"][:B0]), ("dy part 1", v[1]["dy"], c64["dy"][B0:], c32["dy"][B0:]),
             ("value_loss", v[0]["value_loss"], c64["value_loss"], c32["value_loss"]),
             ("explained_var", v[1]["explained_var"], c64["explained_var"], c32["explained_var"])]
    worst, bad = U.gate("branch flip", items)
    assert not bad, "; ".join(bad)
    wrong = calls[0].critic_global(own[0], rows)                 # part 0 deciding on its own sums: the other branch, far outside the bar
    worst, _ = U.gate("per-part decision", [("dy", wrong["dy"], c64["dy"][:B0], c32["dy"][:B0])], verbose=False)
    assert worst > U.BAR, worst


REFUSALS = ("null_sums", "misaligned_sums", "global_rows_short", "nan_share", "inf_share", "null_y", "misaligned_dy", "steps_65", "short_workspace",
            "null_rows")


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals_return_an_error_and_launch_nothing(what):
    lib = abi.load_library()
    k = GCall(U.head_case(3, 5, 2, 9))
    rows_n = 3 * 5 * 2
    fill = lambda *s, dtype=torch.float32: torch.full(s, FILL, dtype=dtype, device="cuda")      # noqa: E731
    own, _ = k.sums()
    for entry in ("sums", "critic", "actor"):
        if (what in ("nan_share", "inf_share") and entry != "actor") or (what in ("null_sums", "misaligned_sums") and entry == "actor") or \
                (what == "global_rows_short" and entry == "sums") or (what == "misaligned_dy" and entry == "sums"):
            continue
        actor = entry == "actor"
        size = lib.hns_rnn_actor_head_workspace_bytes if actor else lib.hns_rnn_critic_head_workspace_bytes
        nb = size(k.B, k.A, k.L)
        ws = torch.empty(nb + 256, dtype=torch.uint8, device="cuda")
        pad = fill(rows_n * H + 8)
        dy = pad[:rows_n * H].view(3, 5, 2, H).transpose(1, 2)
        outs = [fill(4 if actor else 1, H), fill(4 if actor else 1), fill(4), fill(4), fill(3, 5, 2)]
        box = fill(8, dtype=torch.float64)
        if entry == "critic":
            box[:5] = own
        rows = k.struct()
        arg = dict(dy=dy.data_ptr(), ws=ws.data_ptr(), nb=nb, rows=C.byref(rows), sums=box.data_ptr(), n=rows_n, share=1.0)
        if what == "null_sums":
            arg["sums"] = None
        elif what == "misaligned_sums":
            arg["sums"] = box.data_ptr() + 4
        elif what == "global_rows_short":
            arg["n"] = rows_n - 1
        elif what == "nan_share":
            arg["share"] = float("nan")
        elif what == "inf_share":
            arg["share"] = float("inf")
        elif what == "null_y":
            rows.y = None
        elif what == "misaligned_dy":
            arg["dy"] = pad.data_ptr() + 4
        elif what == "steps_65":
            rows.steps = 65
        elif what == "short_workspace":
            arg["nb"] = nb - 1
        elif what == "null_rows":
            arg["rows"] = None
        h, r = k.head, k.rows
        before = box.clone()
        if actor:
            rc = lib.hns_rnn_actor_head_grad_global(h["head_w"].data_ptr(), h["head_b"].data_ptr(), h["log_std"].data_ptr(), arg["rows"],
                                                    r["action"].data_ptr(), r["log_probs_old"].data_ptr(), r["advantages"].data_ptr(), 0.1, 1e-3, arg["dy"],
                                                    outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), outs[3][1:].data_ptr(),
                                                    outs[3][2:].data_ptr(), outs[4].data_ptr(), arg["ws"], arg["nb"], None, arg["n"], arg["share"])
            name = "hns_rnn_actor_head_grad_global:"
        elif entry == "critic":
            rc = lib.hns_rnn_critic_head_grad_global(h["v_w"].data_ptr(), h["v_b"].data_ptr(), arg["rows"], r["b_values"].data_ptr(), r["b_returns"].data_ptr(),
                                                     0.1, abi.HNS_CRITIC_LOSS_HUBER, 10.0, arg["dy"], outs[0].data_ptr(), outs[1].data_ptr(),
                                                     outs[3].data_ptr(), outs[3][1:].data_ptr(), outs[4].data_ptr(), arg["ws"], arg["nb"], None, arg["sums"],
                                                     arg["n"])
            name = "hns_rnn_critic_head_grad_global:"
        else:
            rc = lib.hns_rnn_critic_head_sums(h["v_w"].data_ptr(), h["v_b"].data_ptr(), arg["rows"], r["b_values"].data_ptr(), r["b_returns"].data_ptr(), 0.1,
                                              abi.HNS_CRITIC_LOSS_HUBER, 10.0, arg["sums"], outs[4].data_ptr(), arg["ws"], arg["nb"], None)
            name = "hns_rnn_critic_head_sums:"
        assert rc != 0 and lib.hns_last_error().decode().startswith(name), (what, entry, lib.hns_last_error())
        torch.cuda.synchronize()
        for t in (pad, *outs):
            assert (t == FILL).all(), (what, entry)
        assert torch.equal(box, before), (what, entry)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the learner
SEQ = 4
CFG = {"ppo_epochs": 2, "num_minibatches": 2, "TP_epochs": 2, "use_TP_net": 1, "actor": {"rnn": {"train_seq_len": SEQ}}, "critic": {"rnn": {"train_seq_len": SEQ}}}


def _example():
    spec = importlib.util.spec_from_file_location("recurrent_policy_example", os.path.join(ROOT, "examples", "recurrent_policy.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _to(x, dev):
    if torch.is_tensor(x):
        return x.to(dev)
    if isinstance(x, (tuple, list)):
        return tuple(_to(v, dev) for v in x)
    return x


def _rollout(N=5, T=8):
    """The small CPU shapes (tests/test_rnn_train.py's), collected on the CPU and moved to the device."""
    ex = _example()
    ex.SEQ = SEQ
    torch.manual_seed(N * 100 + T)
    env = ex.StandInEnv(N, max_episode_length=5)
    actor, critic = ex.Network(env.D, env.A, True, 0), ex.Network(env.D, env.A, False, 1)
    pol = P.RecurrentDevicePolicy(actor.names(), critic.names(), seed=0)
    col = collector.DeviceCollector(env, pol, T, rnn_seq_len=SEQ)
    col.collect()
    st = col.collect()
    kw, rk = {**st.learner_kwargs(), "tp": U.predictor_rollout(N, T, 3, N + T)}, st.recurrent_kwargs()
    params = ({k: v.detach().clone() for k, v in actor.names().items()}, {k: v.detach().clone() for k, v in critic.names().items()})
    return params, {k: _to(v, "cuda") for k, v in kw.items()}, {k: _to(v, "cuda") for k, v in rk.items()}


def _snapshot(lrn):
    out = [v.detach().clone() for v in (*lrn.actor.values(), *lrn.critic.values(), *tp_train.parameters(lrn.tp_net))]
    for opt in (lrn.actor_opt, lrn.critic_opt, lrn.tp_opt):
        for st in opt.state_dict()["state"].values():
            out += [st["step"].clone().cuda(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
    vn = lrn.value_normalizer
    return out + [vn.running_mean.clone(), vn.running_mean_sq.clone(), vn.debiasing_term.clone()]


@pytest.fixture
def one_rank_group(tmp_path):
    import torch.distributed as dist
    assert not dist.is_initialized()
    dist.init_process_group("gloo", rank=0, world_size=1, store=dist.FileStore(str(tmp_path / "store"), 1))
    yield dist.group.WORLD
    dist.destroy_process_group()


def test_a_one_rank_group_trains_as_the_recurrent_learner_without_one(one_rank_group):
    params, kw, rk = _rollout()
    runs = []
    for group in (None, one_rank_group):
        actor, critic = ({k: v.clone().cuda() for k, v in p.items()} for p in params)
        args = dict(tp_net=U.predictor(3, 41).cuda(), value_normalizer=learner.ValueNorm1().cuda(), generator=torch.Generator(device="cuda").manual_seed(7))
        lrn = learner.RecurrentDeviceLearner(actor, critic, CFG, **args) if group is None else \
            learner.DataParallelRecurrentLearner(actor, critic, CFG, group=group, **args)
        info = lrn.train_rollout(**kw, **rk)
        torch.cuda.synchronize()
        runs.append((info, _snapshot(lrn)))
    (i0, s0), (i1, s1) = runs
    assert list(i0) == list(i1) == [f"drone/{k}" for k in learner.INFO_KEYS]
    for k in i0:
        assert np.float32(i0[k]) == np.float32(i1[k]) and np.isfinite(i0[k]), (k, i0[k], i1[k])
    assert len(s0) == len(s1) and all(torch.equal(x, y) for x, y in zip(s0, s1))
    assert not torch.equal(s0[0], next(iter(params[0].values())).cuda())                      # the parameters moved


@pytest.mark.timeout(400)
def test_two_ranks_on_one_gpu_over_gloo(tmp_path):
    """tests/dp_rnn_learner_job.py, one child process a rank, each under its own time limit; both ranks share cuda:0 and the collectives run
    over gloo — a correctness run.  The parent stops at the first non-zero status.  The ranks end with one sha256 over their parameters,
    Adam states and ValueNorm1, and with equal info rows."""
    job = os.path.join(ROOT, "tests", "dp_rnn_learner_job.py")
    logs = [open(tmp_path / f"rank{r}.log", "w+") for r in range(2)]
    procs = [subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, job, "--rank", str(r), "--world", "2", "--store", str(tmp_path / "store"),
                               "--out", str(tmp_path)], stdout=logs[r], stderr=subprocess.STDOUT, cwd=ROOT) for r in range(2)]
    done, status = queue.Queue(), [None, None]
    waiters = [threading.Thread(target=lambda r=r, p=p: done.put((r, p.wait())), daemon=True) for r, p in enumerate(procs)]
    for w in waiters:
        w.start()
    try:
        for _ in procs:
            r, code = done.get(timeout=300)                      # (the children end under their own time limits first)
            status[r] = code
            if code != 0:
                break                                            # nothing goes on after a failed rank
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
            p.wait()

    def tail(r):
        logs[r].seek(0)
        return logs[r].read()[-3000:]
    assert status == [0, 0], f"statuses {status}\nrank 0:\n{tail(0)}\nrank 1:\n{tail(1)}"
    reps = [json.load(open(tmp_path / f"rank{r}.json")) for r in range(2)]
    assert reps[0]["digest"] == reps[1]["digest"] and reps[0]["start"] == reps[1]["start"] != reps[0]["digest"]
    assert reps[0]["infos"] == reps[1]["infos"] and len(reps[0]["infos"]) == 2
    assert [r["envs"] for r in reps] == [3, 5]                   # unequal shards
    for info in reps[0]["infos"]:
        assert list(info) == [f"drone/{k}" for k in learner.INFO_KEYS] and all(np.isfinite(v) for v in info.values()), info
