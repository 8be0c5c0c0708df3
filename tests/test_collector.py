"""hns_amd.collector on the CPU and hns_rollout_store's refusals (no GPU needed).

Refusals: every argument hns_rollout_store refuses, through ctypes with stream = None — HNS_ERR_INVALID_ARG before any launch, and
hns_last_error() names the argument.  Storage: `store(t, ...)` fills slot t and nothing else; `learner_kwargs()` is what
DeviceLearner.train_rollout takes, and training from the storage's views equals training from the raw tensors bit for bit (A = 1, without
state_others, and A = 3).  The loop: a stub env that rewrites its buffers in place, as the real one does, pins which observation lands in
which slot, `done` from before the reset, next_obs_last from before the reset, the episode statistics — and the read-back rule: no read of
`done` before max_episode_length steps, one on every step after that until a reset covers every env."""
import collections
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import learner_cases as LC
from hns_amd import abi, collector, learner
from hns_amd.tensordict_shim import _ShimTensorDict as TD


# ---------------------------------------------------------------------------------------------------------------------------------------
# hns_rollout_store: refusals
@pytest.fixture(scope="module")
def lib():
    return abi.load_library()


def _segments(n=1, **kw):
    """n valid segments over host memory (nothing is ever launched here: every call below is refused first)."""
    keep = np.zeros(4096, np.uint8)
    segs = (abi.HnsRolloutSegment * abi.HNS_ROLLOUT_MAX_SEGMENTS)()
    for i in range(n):
        segs[i].src, segs[i].dst = keep.ctypes.data, keep.ctypes.data + 2048
        segs[i].src_stride, segs[i].dst_stride, segs[i].row_bytes = 16, 64, 16
    for k, v in kw.items():
        setattr(segs[n - 1], k, v)
    return segs, keep


REFUSALS = [
    # (what, segment overrides, count, num_envs, slot, num_slots, word in the message)
    ("count 0", {}, 0, 4, 0, 4, "count"),
    ("count 17", {}, 17, 4, 0, 4, "count"),
    ("num_envs 0", {}, 1, 0, 0, 4, "num_envs"),
    ("num_slots 0", {}, 1, 4, 0, 0, "num_slots"),
    ("slot -1", {}, 1, 4, -1, 4, "slot"),
    ("slot == num_slots", {}, 1, 4, 4, 4, "slot"),
    ("null src", {"src": None}, 1, 4, 0, 4, "src"),
    ("null dst", {"dst": None}, 1, 4, 0, 4, "dst"),
    ("row_bytes 0", {"row_bytes": 0}, 1, 4, 0, 4, "row_bytes"),
    ("row_bytes 2^20 + 1", {"row_bytes": 2 ** 20 + 1, "src_stride": 2 ** 21, "dst_stride": 2 ** 23}, 1, 4, 0, 4, "row_bytes"),
    ("src_stride < row_bytes", {"src_stride": 15}, 1, 4, 0, 4, "src_stride"),
    ("dst_stride < num_slots row_bytes", {"dst_stride": 63}, 1, 4, 0, 4, "dst_stride"),
    ("num_envs dst_stride past int64", {"dst_stride": 2 ** 40}, 1, 2 ** 40, 0, 4, "dst_stride"),
]


@pytest.mark.parametrize("what, over, count, num_envs, slot, num_slots, word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_rollout_store_refuses(lib, what, over, count, num_envs, slot, num_slots, word):
    segs, keep = _segments(1, **over)
    assert lib.hns_rollout_store(segs, count, num_envs, slot, num_slots, None) == abi.HNS_ERR_INVALID_ARG, what
    msg = lib.hns_last_error().decode()
    assert msg.startswith("hns_rollout_store: ") and word in msg, msg


def test_rollout_store_refuses_null_segments_and_names_the_faulty_segment(lib):
    assert lib.hns_rollout_store(None, 1, 4, 0, 4, None) == abi.HNS_ERR_INVALID_ARG
    assert "segments" in lib.hns_last_error().decode()
    segs, keep = _segments(3, row_bytes=0)                       # two good segments in front of the bad one
    assert lib.hns_rollout_store(segs, 3, 4, 0, 4, None) == abi.HNS_ERR_INVALID_ARG
    assert "segments[2].row_bytes" in lib.hns_last_error().decode()


def test_the_segment_struct_is_the_headers():
    assert C.sizeof(abi.HnsRolloutSegment) == 40 and abi.HnsRolloutSegment.row_bytes.offset == 32
    assert abi.HNS_ROLLOUT_MAX_SEGMENTS == 16


# ---------------------------------------------------------------------------------------------------------------------------------------
# RolloutStorage on the CPU
def _names(ro):
    """The rollout's tensors under the storage's names: {name: [N, T, ...]} and the next observation {name: [N, ...]}."""
    full = {"obs_self": ro["obs_self"], "obs_others": ro["obs_others"], "obs_cylinders": ro["obs_cylinders"], "action": ro["action"],
            "log_probs": ro["log_probs"], "state_value": ro["state_value"], "reward": ro["reward"], "done": ro["done"],
            "TP_input": ro["tp"][0], "TP_groundtruth": ro["tp"][1], "TP_done": ro["tp"][2]}
    last = dict(zip(collector.LAST_NAMES, ro["next_obs_last"]))
    return {k: v for k, v in full.items() if v is not None}, {k: v for k, v in last.items() if v is not None}


def _filled(ro, N, T, order=None):
    full, last = _names(ro)
    st = collector.RolloutStorage(N, T, {k: v[:, 0] for k, v in full.items()})
    for t in (order if order is not None else range(T)):
        st.store(t, {k: v[:, t] for k, v in full.items()})
    st.store_last(last)
    return st


@pytest.mark.parametrize("A", [1, 3])
def test_store_fills_its_slot_and_nothing_else(A):
    N, T = 5, 4
    ro = LC.make_rollout(LC.make_state(A, 3), N, T, A, 4)
    full, last = _names(ro)
    st = collector.RolloutStorage(N, T, {k: v[:, 0] for k, v in full.items()})
    assert set(st.data) == set(full) and set(st.last) == set(last) and ("obs_others" in st.data) == (A > 1)
    for k, v in st.data.items():
        assert v.shape == full[k].shape and v.dtype == full[k].dtype, k
        v.fill_(True if v.dtype == torch.bool else 7)
    assert st.data["done"].dtype == torch.bool
    before = {k: v.clone() for k, v in st.data.items()}
    st.store(2, {k: v[:, 2] for k, v in full.items()})
    for k, v in st.data.items():
        assert torch.equal(v[:, 2], full[k][:, 2]), k
        keep = [0, 1, 3]
        assert torch.equal(v[:, keep], before[k][:, keep]), k
    st.store_last(last)
    for k, v in last.items():
        assert torch.equal(st.last[k], v), k
    with pytest.raises(IndexError):
        st.store(T, {"reward": full["reward"][:, 0]})
    with pytest.raises(ValueError):
        st.store(0, {"reward": full["reward"][:, 0, :, :0]})
    with pytest.raises(ValueError):
        st.store(0, {"done": full["done"][:, 0].to(torch.uint8)})


@pytest.mark.parametrize("A", [1, 3])
def test_learner_kwargs_are_train_rollouts_arguments_as_views(A):
    N, T = 5, 6
    ro = LC.make_rollout(LC.make_state(A, 5), N, T, A, 6)
    st = _filled(ro, N, T, order=reversed(range(T)))
    kw = st.learner_kwargs()
    params = inspect.signature(learner.DeviceLearner.train_rollout).parameters
    required = {k for k, p in params.items() if k != "self" and p.default is inspect.Parameter.empty}
    assert required <= set(kw) <= set(params) - {"self"}
    D, K = LC.D, LC.K
    want = {"obs_self": (N, T, A, 1, D), "obs_cylinders": (N, T, A, K, 5), "action": (N, T, A, 4), "log_probs": (N, T, A, 1),
            "state_value": (N, T, A, 1), "reward": (N, T, A, 1), "done": (N, T, 1)}
    for k, s in want.items():
        assert tuple(kw[k].shape) == s, k
    assert (kw["obs_others"] is None) == (A == 1) and (A == 1 or tuple(kw["obs_others"].shape) == (N, T, A, A - 1, 3))
    xs, xo, xc = kw["next_obs_last"]
    assert tuple(xs.shape) == (N, A, 1, D) and tuple(xc.shape) == (N, A, K, 5) and ((xo is None) if A == 1 else tuple(xo.shape) == (N, A, A - 1, 3))
    assert [tuple(t.shape) for t in kw["tp"]] == [(N, T, LC.HIST, 7 + 3 * A), (N, T, 3), (N, T, 1)]
    # views of the storage, no copies
    flat = [v for v in kw.values() if torch.is_tensor(v)] + [t for t in (*kw["next_obs_last"], *kw["tp"]) if t is not None]
    owned = {t.data_ptr() for t in (*st.data.values(), *st.last.values())}
    assert all(t.data_ptr() in owned for t in flat)
    # and the rollout itself, whatever the order the slots were written in
    full, last = _names(ro)
    for k, v in full.items():
        assert torch.equal(st.data[k], v), k


@pytest.mark.parametrize("A", [1, 3])
def test_training_from_the_storage_equals_training_from_the_raw_tensors(A):
    N, T = 4, 8
    start = LC.make_state(A, 21)
    ro = LC.make_rollout(start, N, T, A, 22)
    st = _filled(ro, N, T)
    sa, sb = LC.clone_state(start), LC.clone_state(start)
    La, Lb = LC.make_learner(sa, seed=9), LC.make_learner(sb, seed=9)
    info_a = La.train_rollout(**st.learner_kwargs())
    info_b = Lb.train_rollout(**ro)
    assert info_a == info_b and set(info_a) == {f"drone/{k}" for k in learner.INFO_KEYS}
    LC.assert_same_state(LC.state_tensors(sa, LC.learner_opts(La)), LC.state_tensors(sb, LC.learner_opts(Lb)), "storage views against raw tensors")


# ---------------------------------------------------------------------------------------------------------------------------------------
# DeviceCollector over a stub env
class CountedDone(torch.Tensor):
    """The stub's `done`: counts the reductions a host read-back of it goes through."""
    reads = 0

    def _read(self, fn, *a, **k):
        CountedDone.reads += self.dtype == torch.bool            # (a float result computed FROM the mask inherits the class: not a read of done)
        return getattr(self.as_subclass(torch.Tensor), fn)(*a, **k)

    def sum(self, *a, **k):
        return self._read("sum", *a, **k)

    def any(self, *a, **k):
        return self._read("any", *a, **k)

    def all(self, *a, **k):
        return self._read("all", *a, **k)


class StubEnv:
    """N envs of one agent; env e's episode ends when its progress reaches lengths[e] (>= max_episode_length = min(lengths)).  Every tensor
    handed out is a persistent buffer rewritten in place by step() and reset(), as HideAndSeek's are.  Observation row: (env, progress,
    episode); reward: progress + 100 episode; the statistic `return` sums the rewards of the running episode."""

    def __init__(self, lengths, A=1):
        N = len(lengths)
        self.lengths = torch.tensor(lengths, dtype=torch.float32)
        self.max_episode_length, self.num_envs, self.batch_size, self.A = int(min(lengths)), N, torch.Size([N]), A
        self.progress, self.episode, self.ret = torch.zeros(N), torch.full((N,), -1.0), torch.zeros(N, 1)
        self.xs, self.xc, self.xo = torch.zeros(N, A, 1, 3), torch.zeros(N, A, 2, 5), torch.zeros(N, A, A - 1, 3)
        self.reward = torch.zeros(N, A, 1)
        self.done = torch.zeros(N, 1, dtype=torch.bool).as_subclass(CountedDone)
        self.masks, self.actions = [], []
        self.next = self._tree()
        self.next.set(("agents", "reward"), self.reward)
        self.next.set("done", self.done)

    def _tree(self):
        obs = {"state_self": self.xs, "cylinders": self.xc}
        if self.A > 1:
            obs["state_others"] = self.xo
        return TD({"agents": {"observation": obs}}, self.batch_size)

    def _write(self):
        row = torch.stack([torch.arange(self.num_envs, dtype=torch.float32), self.progress, self.episode], -1)
        self.xs[:] = row[:, None, None, :]
        self.xc[:] = (self.progress + 1000 * self.episode)[:, None, None, None]
        self.xo[:] = -self.progress[:, None, None, None]

    def reset(self, td=None):
        mask = torch.ones(self.num_envs, dtype=torch.bool) if td is None else td["_reset"].as_subclass(torch.Tensor).reshape(-1).clone()
        self.masks.append(mask.tolist())
        stats = TD({"return": self.ret.clone()}, self.batch_size)
        self.progress[mask], self.ret[mask] = 0, 0
        self.episode[mask] += 1
        self.done.as_subclass(torch.Tensor)[mask] = False
        self._write()
        out = self._tree()
        out.set("stats", stats)
        return out

    def step(self, td):
        self.actions.append(td[("agents", "action")].clone())
        self.progress += 1
        self.reward[:] = (self.progress + 100 * self.episode)[:, None, None]
        self.ret += self.reward[:, 0]
        self.done.as_subclass(torch.Tensor)[:] = (self.progress >= self.lengths)[:, None]
        self._write()
        td.set("next", self.next)
        return td


Out = collections.namedtuple("Out", ["action", "log_prob", "value"])


class StubPolicy:
    def forward(self, xs, xo, xc):
        key = xs[:, :, 0, 1:2] + 10 * xs[:, :, 0, 2:3]           # progress + 10 episode
        return Out(key.expand(-1, -1, 4) + torch.arange(4.0), key * 2, key * 3)


def _simulate(lengths, steps):
    """The stub's episodes step by step in plain Python: per step, per env (progress, episode) before the step, after it, done, and after
    the reset; and the (return, env) of every episode that ended."""
    N = len(lengths)
    prog, epi, ret = [0] * N, [0] * N, [0.0] * N
    rows, ended = [], []
    for _ in range(steps):
        before = list(zip(prog, epi))
        prog = [p + 1 for p in prog]
        ret = [r + p + 100 * e for r, p, e in zip(ret, prog, epi)]
        done = [p >= L for p, L in zip(prog, lengths)]
        after = list(zip(prog, epi))
        for e in range(N):
            if done[e]:
                ended.append(ret[e])
                prog[e], epi[e], ret[e] = 0, epi[e] + 1, 0.0
        rows.append((before, after, done, list(zip(prog, epi))))
    return rows, ended


@pytest.mark.parametrize("lengths, A", [([4, 4, 4, 4], 1), ([3, 3, 5, 3], 1), ([4, 4, 4, 4, 4], 3)])
def test_collect_puts_each_observation_done_and_next_observation_in_its_slot(lengths, A):
    """Two collects of 6 steps: boundaries fall inside both, and (lengths 3, 3, 5, 3) never cover every env at once."""
    N, T = len(lengths), 6
    env = StubEnv(lengths, A)
    col = collector.DeviceCollector(env, StubPolicy(), T)
    rows, ended = _simulate(lengths, 2 * T)
    seen = 0
    for call in range(2):
        st = col.collect()
        assert st is col.storage
        kw = st.learner_kwargs()
        for t in range(T):
            before, after, done, _ = rows[call * T + t]
            for e in range(N):
                p, k = before[e]
                assert kw["obs_self"][e, t, 0, 0].tolist() == [e, p, k], (call, t, e)          # the observation the policy saw
                assert kw["obs_cylinders"][e, t].eq(p + 1000 * k).all()
                assert kw["action"][e, t, 0].tolist() == [p + 10 * k + i for i in range(4)]
                assert kw["log_probs"][e, t, 0, 0] == 2 * (p + 10 * k) and kw["state_value"][e, t, 0, 0] == 3 * (p + 10 * k)
                assert kw["reward"][e, t, 0, 0] == after[e][0] + 100 * after[e][1]
                assert bool(kw["done"][e, t, 0]) == done[e]                                      # as it was before the reset
                if A > 1:
                    assert kw["obs_others"][e, t].eq(-p).all()
        before, after, done, _ = rows[call * T + T - 1]
        xs, xo, xc = kw["next_obs_last"]
        assert (xo is None) == (A == 1)
        for e in range(N):                                       # the step's own next observation, not what the reset put there
            assert xs[e, 0, 0].tolist() == [e, after[e][0], after[e][1]]
        means, n = col.episode_stats()
        upto = sum(sum(r[2]) for r in rows[:(call + 1) * T])
        assert n == upto - seen
        want = float(np.float32(np.sum(np.array(ended[seen:upto], np.float64)) / n))
        assert means == {"return": want}
        seen = upto
    assert col.episode_stats() == ({}, 0)
    # the env saw exactly the actions the policy gave and the masks of the done envs
    assert len(env.actions) == 2 * T and all(torch.equal(a, kw_a) for a, kw_a in zip(env.actions[T:], kw["action"].unbind(1)))
    assert env.masks == [[True] * N] + [r[2] for r in rows if any(r[2])]


def test_done_is_read_back_only_once_an_episode_can_have_ended():
    """Lock-step episodes of 4 steps: reads at steps 4, 8, 12 only (each followed by a reset of every env).  Lengths (4, 4, 7): the first
    boundary resets two envs of three, so from step 4 on every step reads."""
    for lengths, want in (([4, 4, 4], [4, 8, 12]), ([4, 4, 7], list(range(4, 15)))):
        env = StubEnv(lengths)
        col = collector.DeviceCollector(env, StubPolicy(), 1)
        CountedDone.reads, reads_at = 0, []
        for step in range(1, 15):
            col.collect()
            if CountedDone.reads:
                assert CountedDone.reads == 1
                reads_at.append(step)
                CountedDone.reads = 0
        assert reads_at == want and col.done_reads == len(want), (lengths, reads_at)
