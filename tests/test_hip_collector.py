"""hns_rollout_store and hns_amd.collector on an MI355X.  Bit identity throughout, no tolerance: the kernel is a copy, and the collector is
compared with the same loop driven by hand (torch `copy_` into [N, T, ...] tensors, a read-back of `done` on every step).

Kernel against numpy: row lengths 1 .. 1240 bytes, source and destination bases 0, 1 and 4 bytes off a 16-byte boundary (so the 16-, 4- and
1-byte units all occur), tight and padded strides, 1 / 33 / 1000 envs (one partial workgroup .. several), one slot and the first / last of
five, 16 mixed segments in one call.  Every destination is prefilled with a byte pattern and followed by 64 guard bytes: the target rows equal
the source and every other byte keeps the pattern.

Collector against the hand loop: two envs from one cfg and seed and two DevicePolicy objects from one seed; every tensor of learner_kwargs()
equal; with short episodes also `done` from before the reset, the post-reset observation in the slot behind a boundary, next_obs_last from
before the reset and the episode statistics.  Collector plus learner: two iterations of collect -> train_rollout give the info rows and
parameters of the hand-driven pair."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import learner_cases as LC
from hns_amd import abi, collector, config, learner
from hns_amd import policy as P
from hns_amd.tensordict_shim import TensorDict

pytestmark = pytest.mark.gpu

PATTERN, GUARD = 0xA5, 64
ROW_BYTES = [1, 3, 4, 12, 16, 20, 140, 1240]
OFFSETS = [0, 1, 4]


def _unit(*values):
    bits = 0
    for v in values:
        bits |= int(v)
    return 16 if bits % 16 == 0 else 4 if bits % 4 == 0 else 1


class _Case:
    """One segment's device buffers and its expected destination image."""

    def __init__(self, g, row, num_envs, num_slots, slot, src_off, dst_off, src_pad, dst_pad):
        self.row, self.slot = row, slot
        self.src_stride, self.dst_stride = row + src_pad, num_slots * row + dst_pad
        src_host = torch.randint(0, 256, (src_off + num_envs * self.src_stride,), dtype=torch.uint8, generator=g)
        self.src_buf = src_host.cuda()
        self.dst_buf = torch.full((dst_off + num_envs * self.dst_stride + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        assert self.src_buf.data_ptr() % 16 == 0 and self.dst_buf.data_ptr() % 16 == 0
        self.src_ptr, self.dst_ptr = self.src_buf.data_ptr() + src_off, self.dst_buf.data_ptr() + dst_off
        self.unit = _unit(self.src_ptr, self.dst_ptr, self.src_stride, self.dst_stride, row)
        want = np.full(self.dst_buf.numel(), PATTERN, np.uint8)
        s = src_host.numpy()
        for e in range(num_envs):
            at = dst_off + e * self.dst_stride + slot * row
            want[at:at + row] = s[src_off + e * self.src_stride:src_off + e * self.src_stride + row]
        self.want = want

    def fill(self, seg):
        seg.src, seg.dst, seg.src_stride, seg.dst_stride, seg.row_bytes = self.src_ptr, self.dst_ptr, self.src_stride, self.dst_stride, self.row

    def check(self, what):
        got = self.dst_buf.cpu().numpy()
        assert np.array_equal(got, self.want), f"{what}: {int((got != self.want).sum())} bytes differ, the first at {int(np.argmax(got != self.want))}"


def _launch(cases, num_envs, slot, num_slots):
    lib = abi.load_library()
    segs = (abi.HnsRolloutSegment * abi.HNS_ROLLOUT_MAX_SEGMENTS)()
    for seg, c in zip(segs, cases):
        c.fill(seg)
    rc = lib.hns_rollout_store(segs, len(cases), num_envs, slot, num_slots, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.hns_last_error()


@pytest.mark.parametrize("num_envs", [1, 33, 1000])
@pytest.mark.parametrize("row", ROW_BYTES)
def test_store_against_numpy_bit_for_bit(row, num_envs):
    """Per (row length, env count): 3 x 3 base offsets x (tight | 16-byte-keeping pad | 4-byte pad) x (one slot | first of five | last of
    five), one segment per call."""
    g = torch.Generator().manual_seed(row * 1009 + num_envs)
    pads = [(0, 0), ((-row) % 16 + 16, 16), (4, 0)]
    cases = []
    for src_off in OFFSETS:
        for dst_off in OFFSETS:
            for src_pad, dst_pad in pads:
                for num_slots, slot in ((1, 0), (5, 0), (5, 4)):
                    c = _Case(g, row, num_envs, num_slots, slot, src_off, dst_off, src_pad, dst_pad)
                    _launch([c], num_envs, slot, num_slots)
                    cases.append((c, f"offsets {src_off}/{dst_off} pads {src_pad}/{dst_pad} slot {slot} of {num_slots}"))
    torch.cuda.synchronize()
    for c, what in cases:
        c.check(f"row {row} envs {num_envs} {what} unit {c.unit}")
    want_units = {1, 4, 16} if row % 16 == 0 else {1, 4} if row % 4 == 0 else {1}
    assert {c.unit for c, _ in cases} == want_units


@pytest.mark.parametrize("num_envs, num_slots, slot", [(33, 5, 4), (1000, 1, 0), (1, 5, 0)])
def test_sixteen_mixed_segments_in_one_call(num_envs, num_slots, slot):
    g = torch.Generator().manual_seed(num_envs)
    cases = []
    for i in range(16):
        row = ROW_BYTES[i % len(ROW_BYTES)]
        # the first pass over the row lengths walks the base offsets, the second keeps the bases at 0 / 4 bytes: units 1, 4 and 16
        src_off, dst_off = (OFFSETS[i % 3], OFFSETS[(i // 3) % 3]) if i < 8 else ((0, 0) if i % 2 == 0 else (4, 0))
        src_pad, dst_pad = [(0, 0), ((-row) % 16 + 16, 16), (4, 0)][i % 3]
        cases.append(_Case(g, row, num_envs, num_slots, slot, src_off, dst_off, src_pad, dst_pad))
    assert {c.unit for c in cases} == {1, 4, 16}
    _launch(cases, num_envs, slot, num_slots)
    torch.cuda.synchronize()
    for i, c in enumerate(cases):
        c.check(f"segment {i} row {c.row} unit {c.unit}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# the collector against a hand-driven loop
def _make_env(task, use_tp, seed=0):
    from hns_amd.env import HideAndSeek
    torch.manual_seed(seed + 100)                                # the predictor's initial weights come from the global generator
    cfg = config.make_cfg(task, algo={"use_TP_net": int(use_tp)})
    env = HideAndSeek(cfg, headless=True)
    env.set_seed(seed)
    return env


class HandLoop:
    """What a user writes without the collector: torch copy_ into [N, T, ...] tensors, `done.any()` read back on every step, the statistics
    of the done envs taken from env.stats before the reset and averaged on the host in fp64.  tools/collector_cost.py times its own copy
    of this loop: a change to the loop's order belongs in both."""

    def __init__(self, env, pol, T):
        self.env, self.pol, self.T, self.cur, self.buf, self.last = env, pol, T, None, None, None
        self.sums, self.count = {}, 0

    def _alloc(self, name, t):
        self.buf[name] = torch.empty(t.shape[0], self.T, *t.shape[1:], dtype=t.dtype, device=t.device)

    def collect(self):
        env, T = self.env, self.T
        if self.cur is None:
            self.cur = env.reset()
        cur = self.cur
        first = self.buf is None
        if first:
            self.buf = {}
        for t in range(T):
            obs = cur[("agents", "observation")]
            xs, xo, xc = obs["state_self"], obs.get("state_others", None), obs["cylinders"]
            out = self.pol.forward(xs, xo, xc)
            pre = {"obs_self": xs, "obs_others": xo, "obs_cylinders": xc, "action": out.action, "log_probs": out.log_prob, "state_value": out.value}
            for k, v in pre.items():
                if v is not None:
                    if first and t == 0:
                        self._alloc(k, v)
                    self.buf[k][:, t].copy_(v)
            nxt = env.step(env.rand_step_input(out.action))["next"]
            post = {"reward": nxt[("agents", "reward")], "done": nxt["done"]}
            if env.use_TP_net:
                post.update({k: nxt[("agents", "TP", k)] for k in collector.TP_KEYS})
            for k, v in post.items():
                if first and t == 0:
                    self._alloc(k, v)
                self.buf[k][:, t].copy_(v)
            if t == T - 1:
                nobs = nxt[("agents", "observation")]
                self.last = (nobs["state_self"].clone(), nobs["state_others"].clone() if xo is not None else None, nobs["cylinders"].clone())
            done = nxt["done"]
            if bool(done.any()):
                mask = done.clone().reshape(-1)
                for k in env.stats.keys():
                    self.sums[k] = self.sums.get(k, 0.0) + float(env.stats[k].reshape(-1)[mask].double().cpu().numpy().sum())
                self.count += int(mask.sum())
                cur = env.reset(TensorDict({"_reset": mask.reshape(-1, 1)}, env.batch_size))
            else:
                cur = nxt
        self.cur = cur
        b = self.buf
        kw = {k: b.get(k) for k in ("obs_self", "obs_others", "obs_cylinders", "action", "log_probs", "state_value", "reward", "done")}
        kw["next_obs_last"] = self.last
        if env.use_TP_net:
            kw["tp"] = tuple(b[k] for k in collector.TP_KEYS)
        return kw

    def episode_stats(self):
        n = self.count
        means = {k: float(np.float32(v / n)) for k, v in self.sums.items()} if n else {}
        self.sums, self.count = {}, 0
        return means, n


def _same(a, b, what):
    if a is None or b is None:
        assert a is None and b is None, what
    elif isinstance(a, tuple):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
    else:
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), what


def _same_kwargs(got, want, what):
    assert set(got) == set(want), (what, set(got) ^ set(want))
    for k in want:
        _same(got[k], want[k], f"{what}: {k}")


def _pair(task, use_tp, T, seed=0):
    """(collector, hand loop) over two envs of one cfg and seed and two policies of one seed."""
    out = []
    for _ in range(2):
        env = _make_env(task, use_tp, seed)
        D = abi.self_dim(env.num_targets) + (3 * env.tp_future_step * env.num_targets if use_tp else 0)
        actor, critic = P.random_parameters(D, env.num_agents, seed=seed + 1)
        pol = P.DevicePolicy(actor, critic, device=env.device, seed=seed + 2)
        out.append((env, pol))
    (e1, p1), (e2, p2) = out
    return collector.DeviceCollector(e1, p1, T), HandLoop(e2, p2, T)


CASES = [
    ("64 envs, A = 3, T = 5", {"num_agents": 3, "env": {"num_envs": 64}}, 0, 5),
    ("33 envs, A = 1, T = 1", {"num_agents": 1, "env": {"num_envs": 33}}, 0, 1),
    ("64 envs, A = 3, T = 8, predictor", {"num_agents": 3, "env": {"num_envs": 64}}, 1, 8),
    ("64 envs, A = 3, two evaders, predictor, T = 3", {"num_agents": 3, "num_targets": 2, "env": {"num_envs": 64}}, 1, 3),
]


@pytest.mark.parametrize("what, task, use_tp, T", CASES, ids=[c[0] for c in CASES])
def test_collect_equals_the_hand_driven_loop(what, task, use_tp, T):
    col, hand = _pair(task, use_tp, T)
    try:
        for call in range(2):
            st = col.collect()
            _same_kwargs(st.learner_kwargs(), hand.collect(), f"{what}, collect {call}")
        assert st.launches == 2 * (2 * T + 1)                    # two stores per step and the next observation once per collect
        assert col.done_reads == 0                               # (the default episode is far longer than these rollouts)
        assert ("obs_others" in st.data) == (task["num_agents"] > 1) and ("TP_input" in st.data) == bool(use_tp)
    finally:
        col.env.close()
        hand.env.close()


def test_boundaries_inside_and_at_the_end_of_a_rollout():
    """Episodes of 6 steps, rollouts of 8, three collects: the boundaries fall at slot 5 of the first, slot 3 of the second, slots 1 and 7 (the
    last) of the third."""
    L, T, N = 6, 8, 64
    col, hand = _pair({"num_agents": 3, "env": {"num_envs": N, "max_episode_length": L}}, 1, T)
    try:
        for call in range(3):
            st = col.collect()
            kw, want = st.learner_kwargs(), hand.collect()
            _same_kwargs(kw, want, f"collect {call}")
            steps = torch.arange(call * T + 1, call * T + T + 1, device=kw["done"].device)
            assert torch.equal(kw["done"], (steps % L == 0).view(1, T, 1).expand(N, T, 1))          # done as it was before the reset
            got, ref = col.episode_stats(), hand.episode_stats()
            assert got[1] == ref[1] == N * int((steps % L == 0).sum())
            assert set(got[0]) == set(ref[0]) == set(abi.STAT_NAMES)
            g, r = (np.array([d[k] for k in abi.STAT_NAMES], np.float32) for d in (got[0], ref[0]))
            assert np.array_equal(g, r, equal_nan=True), {k: (got[0][k], ref[0][k]) for k in abi.STAT_NAMES if not got[0][k] == ref[0][k]}
        # the third collect ended on a boundary: next_obs_last is the step's own next observation, the carried one is the reset's
        cur = col._cur[("agents", "observation")]["state_self"]
        assert not torch.equal(kw["next_obs_last"][0], cur)
        assert col.done_reads == 4                               # lock-step episodes: one read per episode (steps 6, 12, 18, 24)
    finally:
        col.env.close()
        hand.env.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# collector plus learner
def test_two_iterations_of_collect_and_train_equal_the_hand_driven_pair():
    N, T, A = 64, 8, 3
    cfg = copy.deepcopy(LC.CFG)
    cfg.update(ppo_epochs=1, num_minibatches=16)
    task = {"num_agents": A, "env": {"num_envs": N}}
    cpu = LC.make_state(A, 71)
    sides = []
    for kind in ("collector", "hand"):
        env = _make_env(task, 1, seed=3)
        assert env.tp_future_step == LC.FUTURE
        state = LC.clone_state(cpu, "cuda")
        pol = P.DevicePolicy(state["actor"], state["critic"], cfg, seed=4)
        L = learner.DeviceLearner(state["actor"], state["critic"], cfg, tp_net=env.TP, value_normalizer=state["vn"],
                                  generator=torch.Generator(device="cuda").manual_seed(5), device_policy=pol)
        loop = collector.DeviceCollector(env, pol, T) if kind == "collector" else HandLoop(env, pol, T)
        sides.append((env, state, L, loop))
    try:
        for it in range(2):
            infos = []
            for env, state, L, loop in sides:
                got = loop.collect()
                infos.append(L.train_rollout(**(got.learner_kwargs() if isinstance(got, collector.RolloutStorage) else got)))
            assert set(infos[0]) == set(infos[1]) == {f"drone/{k}" for k in learner.INFO_KEYS}
            a, b = (np.array([i[k] for k in sorted(i)], np.float64) for i in infos)
            assert np.array_equal(a, b, equal_nan=True), (it, infos)
            tensors = []
            for env, state, L, loop in sides:
                state = dict(state, tp=env.TP)
                tensors.append(LC.state_tensors(state, LC.learner_opts(L)))
            LC.assert_same_state(tensors[0], tensors[1], f"iteration {it}")
    finally:
        for env, *_ in sides:
            env.close()
