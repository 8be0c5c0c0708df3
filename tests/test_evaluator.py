"""hns_amd.evaluator on the CPU, and the refusals of hns_policy_act and hns_eval_means (no GPU needed).

Refusals: every argument the two entry points refuse, through ctypes on made-up pointers — HNS_ERR_INVALID_ARG before any launch, the message
names the argument.  `DevicePolicy.act` on the CPU equals `forward(deterministic=True).action`.  `stat_means`, the kernel's definition on the
host, against math.fsum within the derived bound (eval_cases.py).  The loop: a stub env (truncation at L = 5, 7 envs, statistics that depend
on env, step and action) pins what `evaluate()` returns, what it calls, and what it puts back — the env's `training` flag, seed and reset
epoch, torch's CPU generator — that an env which is not done after L steps raises, and how a collector on the same env is restarted."""
import collections
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import eval_cases as EC
import policy_reference as R
from hns_amd import abi, collector, evaluator
from hns_amd import policy as P
from hns_amd.env import HnsError
from hns_amd.tensordict_shim import _ShimTensorDict as TD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 20                                   # a made-up, 16-byte aligned address: every call below is refused by argument checking alone


@pytest.fixture(scope="module")
def lib():
    return abi.load_library()


# ---------------------------------------------------------------------------------------------------------------------------------------
# hns_policy_act: refusals
def _io(**kw):
    """An hns_policy_io that passes every check of hns_policy_act (contiguous strides of A = 3, K = 5, D = 35; log_prob, value, loc and eps
    NULL: the call ignores them), then `kw` on top."""
    io = abi.HnsPolicyIo()
    io.obs_self, io.obs_others, io.obs_cylinders = FAKE, FAKE + 4096, FAKE + 8192
    io.self_stride[:], io.others_stride[:], io.cyl_stride[:] = [105, 35], [18, 6, 3], [75, 25, 5]
    io.action = FAKE + 16384
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(io, k)[v[0]] = v[1]
        else:
            setattr(io, k, v)
    return io


ACT_REFUSALS = [
    ("null image", b"null or misaligned packed image", dict(packed=None), {}),
    ("image 8 bytes off 16-byte alignment", b"null or misaligned packed image", dict(packed=FAKE + 8), {}),
    ("null io", b"null or misaligned packed image", dict(io=None), {}),
    ("self_dim 0", b"self_dim must be in [1, 96]", dict(D=0), {}),
    ("self_dim 97", b"self_dim must be in [1, 96]", dict(D=97), {}),
    ("num_agents 0", b"num_agents must be in [1, 7]", dict(A=0), {}),
    ("num_agents 8", b"num_agents must be in [1, 7]", dict(A=8), {}),
    ("num_cylinders 0", b"num_cylinders must be in [1, 16]", dict(K=0), {}),
    ("num_cylinders 17", b"num_cylinders must be in [1, 16]", dict(K=17), {}),
    ("num_envs 0", b"num_envs must be in [1, 2^31 / 7]", dict(E=0), {}),
    ("num_envs negative", b"num_envs must be in [1, 2^31 / 7]", dict(E=-1), {}),
    ("num_envs 2^31 / 7 + 1", b"num_envs must be in [1, 2^31 / 7]", dict(E=(1 << 31) // 7 + 1), {}),
    ("obs_self missing", b"observation pointer missing", {}, dict(obs_self=None)),
    ("obs_cylinders missing", b"observation pointer missing", {}, dict(obs_cylinders=None)),
    ("obs_others missing with A = 3", b"observation pointer missing", {}, dict(obs_others=None)),
    ("obs_self 2 bytes off", b"misaligned observation", {}, dict(obs_self=FAKE + 2)),
    ("obs_others 2 bytes off", b"misaligned observation", {}, dict(obs_others=FAKE + 4098)),
    ("obs_others 2 bytes off with A = 1", b"misaligned observation", dict(A=1), dict(obs_others=FAKE + 4098)),
    ("obs_cylinders 2 bytes off", b"misaligned observation", {}, dict(obs_cylinders=FAKE + 8194)),
    ("self_stride[0] < 0", b"negative stride", {}, dict(self_stride=(0, -105))),
    ("self_stride[1] < 0", b"negative stride", {}, dict(self_stride=(1, -1))),
    ("others_stride[0] < 0", b"negative stride", {}, dict(others_stride=(0, -18))),
    ("others_stride[1] < 0", b"negative stride", {}, dict(others_stride=(1, -6))),
    ("others_stride[2] < 0", b"negative stride", {}, dict(others_stride=(2, -3))),
    ("cyl_stride[0] < 0", b"negative stride", {}, dict(cyl_stride=(0, -75))),
    ("cyl_stride[1] < 0", b"negative stride", {}, dict(cyl_stride=(1, -25))),
    ("cyl_stride[2] < 0", b"negative stride", {}, dict(cyl_stride=(2, -5))),
    ("action missing", b"action output missing or misaligned", {}, dict(action=None)),
    ("action 2 bytes off", b"action output missing or misaligned", {}, dict(action=FAKE + 16386)),
]


@pytest.mark.parametrize("row", ACT_REFUSALS, ids=[r[0].replace(" ", "_") for r in ACT_REFUSALS])
def test_every_refusal_branch_of_hns_policy_act(lib, row):
    """One wrong argument at a time on an otherwise valid call.  Every pointer is made up: a row that were NOT refused must never be committed."""
    _, fragment, call, fields = row
    a = dict(packed=FAKE + 65536, D=35, E=4, A=3, K=5, io=_io(**fields))
    a.update(call)
    io = ctypes.byref(a["io"]) if a["io"] is not None else None
    assert lib.hns_policy_act(a["packed"], a["D"], a["E"], a["A"], a["K"], io, None) == abi.HNS_ERR_INVALID_ARG
    err = lib.hns_last_error()
    assert err.startswith(b"hns_policy_act: ") and fragment in err, err


def test_the_act_entry_is_exported_and_declared():
    assert "hns_policy_act" in abi.EXPORTED_SYMBOLS and "hns_eval_means" in abi.EXPORTED_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "hns.h")).read()
    assert re.search(r"\bint hns_policy_act\(const void \*packed, int32_t self_dim, int64_t num_envs, int32_t num_agents,\s*int32_t num_cylinders, "
                     r"const hns_policy_io \*io,\s*void \*stream\);", hdr)


# ---------------------------------------------------------------------------------------------------------------------------------------
# hns_eval_means: refusals, the struct
def _rows(n=1, **kw):
    """n valid rows over host memory (nothing is ever launched here), `kw` on the last one; (rows, mean, used, what keeps them alive)."""
    keep = np.zeros(4096, np.float32)
    rows = (abi.HnsEvalRow * abi.HNS_EVAL_MAX_ROWS)()
    for i in range(n):
        rows[i].src, rows[i].stride = keep.ctypes.data + 64 * i, 1
    for k, v in kw.items():
        setattr(rows[n - 1], k, v)
    return rows, keep.ctypes.data + 8192, keep.ctypes.data + 12288, keep


MEANS_REFUSALS = [
    # (what, row overrides, keyword overrides of the call, word in the message)
    ("count 0", {}, dict(count=0), "count"),
    ("count 65", {}, dict(count=65), "count"),
    ("num_envs 0", {}, dict(num_envs=0), "num_envs"),
    ("num_envs negative", {}, dict(num_envs=-3), "num_envs"),
    ("null rows", {}, dict(rows=None), "rows"),
    ("null mean", {}, dict(mean=None), "mean"),
    ("null used", {}, dict(used=None), "used"),
    ("mean 2 bytes off", {}, dict(mean_off=2), "mean"),
    ("used 4 bytes off 8-byte alignment", {}, dict(used_off=4), "used"),
    ("null src", {"src": None}, {}, "rows[0].src"),
    ("src 2 bytes off", {"src": FAKE + 2}, {}, "rows[0].src"),
    ("stride 0", {"stride": 0}, {}, "rows[0].stride"),
    ("stride negative", {"stride": -1}, {}, "rows[0].stride"),
    ("num_envs stride past int64", {"stride": 2 ** 40}, dict(num_envs=2 ** 40), "rows[0].stride"),
]


@pytest.mark.parametrize("what, over, call, word", MEANS_REFUSALS, ids=[r[0] for r in MEANS_REFUSALS])
def test_eval_means_refuses(lib, what, over, call, word):
    rows, mean, used, keep = _rows(1, **over)
    call = dict(call)                                            # (the offsets are popped: the table's row stays whole)
    a = dict(rows=rows, count=1, num_envs=4, mean=mean + call.pop("mean_off", 0), used=used + call.pop("used_off", 0))
    a.update(call)
    assert lib.hns_eval_means(a["rows"], a["count"], a["num_envs"], None, a["mean"], a["used"], None) == abi.HNS_ERR_INVALID_ARG, what
    msg = lib.hns_last_error().decode()
    assert msg.startswith("hns_eval_means: ") and word in msg, msg


def test_eval_means_names_the_faulty_row(lib):
    rows, mean, used, keep = _rows(3, stride=0)                  # two good rows in front of the bad one
    assert lib.hns_eval_means(rows, 3, 4, None, mean, used, None) == abi.HNS_ERR_INVALID_ARG
    assert "rows[2].stride" in lib.hns_last_error().decode()


def test_the_row_struct_and_the_macro_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "hns.h")).read()
    assert int(re.search(r"#define HNS_EVAL_MAX_ROWS (\d+)", hdr).group(1)) == abi.HNS_EVAL_MAX_ROWS == 64
    body = re.search(r"typedef struct hns_eval_row \{(.*?)\} hns_eval_row;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(const float \*|int64_t )(\w+);", body, re.M)
    assert [(t.strip(), n) for t, n in fields] == [("const float *", "src"), ("int64_t", "stride")]
    assert [n for n, _ in abi.HnsEvalRow._fields_] == ["src", "stride"]
    assert ctypes.sizeof(abi.HnsEvalRow) == 16 and abi.HnsEvalRow.stride.offset == 8 and abi.HnsEvalRow.stride.size == 8


# ---------------------------------------------------------------------------------------------------------------------------------------
# DevicePolicy.act on the CPU
@pytest.mark.parametrize("tag", ["a1k5d20", "a3k5d35"])
def test_cpu_act_is_the_deterministic_forwards_action(tag):
    gp = np.load(os.path.join(ROOT, "tests", "golden", "g_policy.npz"))
    actor, critic, obs, _, _ = R.golden_case(gp, tag)
    t = lambda p: {k: torch.from_numpy(v) for k, v in p.items()}          # noqa: E731
    pol = P.DevicePolicy(t(actor), t(critic))
    xs, xc = torch.from_numpy(obs["state_self"]), torch.from_numpy(obs["cylinders"])
    xo = torch.from_numpy(obs["state_others"]) if "state_others" in obs else None
    want = pol.forward(xs, xo, xc, deterministic=True).action
    got = pol.act(xs, xo, xc)
    assert got.shape == want.shape == (xs.shape[0], xs.shape[1], 4) and torch.equal(got, want)
    out = torch.full_like(want, 7.0)
    assert pol.act(xs, xo, xc, out=out) is out and torch.equal(out, want)
    for bad in (out[:, :, :3], out.double(), out.transpose(0, 1).contiguous().transpose(0, 1) if xs.shape[1] > 1 else out[:-1]):
        with pytest.raises(ValueError, match="out must be"):
            pol.act(xs, xo, xc, out=bad)
    with pytest.raises(ValueError, match="cylinders must be"):            # the same checks as forward
        pol.act(xs, xo, torch.zeros(xs.shape[0], xs.shape[1], 17, 5))


# ---------------------------------------------------------------------------------------------------------------------------------------
# stat_means against math.fsum
@pytest.mark.parametrize("kind", [None, "partial", "zero"])
@pytest.mark.parametrize("count, n", [(1, 1), (5, 63), (24, 257), (7, 4097)])
def test_stat_means_against_fsum(count, n, kind):
    rows, mask = EC.make_rows(count, n, seed=100 * count + n), EC.make_mask(kind, n, seed=n)
    mean, used, masked = evaluator.stat_means(torch.from_numpy(rows), None if mask is None else torch.from_numpy(mask))
    assert mean.dtype == np.float32 and mean.shape == (count,) and used.dtype == np.int64
    assert masked == (n if mask is None else int((mask != 0).sum()))
    for i in range(count):
        assert used[i] == EC.check_mean(mean[i], rows[i], mask, f"row {i}")
    if count > 1:
        assert used[1] == 0 and math.isnan(mean[1])              # the all-NaN row
    if kind == "zero":
        assert masked == 0 and not used.any() and np.isnan(mean).all()


def test_stat_means_takes_lists_and_bool_masks_and_propagates_infinities():
    mean, used, masked = evaluator.stat_means([torch.tensor([1.0, float("nan"), 3.0, 100.0]), torch.tensor([[math.inf], [1.0], [-math.inf], [2.0]]),
                                               torch.tensor([math.inf, 1.0, -math.inf, -math.inf])], torch.tensor([True, True, True, False]))
    assert masked == 3 and used.tolist() == [2, 3, 3]
    assert mean[0] == 2.0 and math.isnan(mean[1]) and math.isnan(mean[2])
    mean, _, _ = evaluator.stat_means([torch.tensor([math.inf, 1.0, -math.inf, -math.inf])], torch.tensor([False, True, True, True]))
    assert mean[0] == -math.inf


# ---------------------------------------------------------------------------------------------------------------------------------------
# DeviceEvaluator over a stub env
class StubEnv:
    """N envs of one agent, env e done when its progress reaches lengths[e].  Every tensor handed out is a persistent buffer rewritten in
    place, as HideAndSeek's are.  Statistics: `score` += (e + 1) progress action[e, 0, 0] per step; `gap` = progress / 2 for even envs and
    NaN for odd ones; `wide` has two values per env (not a per-env statistic: the evaluator leaves it out).  set_seed seeds torch and clears
    the reset epoch, reset draws from torch's global generator: what HideAndSeek does to the caller's random streams."""

    def __init__(self, lengths, L):
        N = len(lengths)
        self.lengths = torch.tensor(lengths, dtype=torch.float32)
        self.max_episode_length, self.num_envs, self.batch_size = L, N, torch.Size([N])
        self.training, self.seed, self.reset_epoch = False, 11, 3
        self.progress = torch.zeros(N)
        self.xs, self.xc = torch.zeros(N, 1, 1, 3), torch.zeros(N, 1, 2, 5)
        self.reward, self.done = torch.zeros(N, 1, 1), torch.zeros(N, 1, dtype=torch.bool)
        self.stats = {"score": torch.zeros(N, 1), "gap": torch.zeros(N, 1), "wide": torch.zeros(N, 2)}
        self.full_resets = self.masked_resets = self.steps = 0
        self.seeds, self.modes, self.clears = [], [], []
        obs = {"state_self": self.xs, "cylinders": self.xc}
        self.next = TD({"agents": {"observation": obs, "reward": self.reward}, "done": self.done}, self.batch_size)

    def set_seed(self, seed=-1):
        self.seed, self.reset_epoch = seed, 0
        torch.manual_seed(seed)
        self.seeds.append(seed)

    def train(self, mode=True):
        self.training = mode
        return self

    def clear_carried_state(self):
        self.clears.append(self.full_resets)

    def _write(self):
        self.xs[:, 0, 0, 0], self.xs[:, 0, 0, 1] = torch.arange(float(self.num_envs)), self.progress

    def reset(self, td=None):
        mask = torch.ones(self.num_envs, dtype=torch.bool) if td is None else td["_reset"].reshape(-1).clone()
        self.full_resets += td is None
        self.masked_resets += td is not None
        self.reset_epoch += 1
        torch.rand(3)
        self.progress[mask] = 0
        self.done[mask] = False
        for v in self.stats.values():
            v[mask] = 0
        self._write()
        return TD({"agents": {"observation": {"state_self": self.xs, "cylinders": self.xc}}}, self.batch_size)

    def step(self, td):
        a = td[("agents", "action")]
        self.steps += 1
        self.modes.append(self.training)
        self.progress += 1
        e = torch.arange(float(self.num_envs))
        self.stats["score"][:, 0] += (e + 1) * self.progress * a[:, 0, 0]
        self.stats["gap"][:, 0] = torch.where(e % 2 == 0, self.progress / 2, torch.full_like(e, float("nan")))
        self.reward[:] = 1.0
        self.done[:] = (self.progress >= self.lengths)[:, None]
        self._write()
        td.set("next", self.next)
        return td


Out = collections.namedtuple("Out", ["action", "log_prob", "value"])


class StubPolicy:
    """action = the progress the observation shows (so the statistics depend on what the policy saw), written into `out` when given."""
    acts = 0

    def act(self, xs, xo, xc, out=None):
        self.acts += 1
        a = xs[:, :, 0, 1:2].expand(-1, -1, 4)
        if out is None:
            return a.clone()
        self.same_out = getattr(self, "out", out) is out
        self.out = out
        return out.copy_(a)

    def forward(self, xs, xo, xc):
        a = xs[:, :, 0, 1:2].expand(-1, -1, 4).clone()
        return Out(a, a[..., :1] * 2, a[..., :1] * 3)


def test_evaluate_on_a_stub_env_returns_the_first_done_means_and_puts_everything_back():
    L, N = 5, 7
    env, pol = StubEnv([L] * N, L), StubPolicy()
    ev = evaluator.DeviceEvaluator(env, pol)
    torch.manual_seed(1234)
    torch.rand(5)
    before = torch.get_rng_state().clone()
    info = ev.evaluate(seed=3)
    assert torch.equal(torch.get_rng_state(), before)            # set_seed's torch.manual_seed and the reset's draws are undone
    score = [(e + 1) * sum(p * (p - 1) for p in range(1, L + 1)) for e in range(N)]       # the action at progress p is p - 1
    assert set(info) == {"eval/stats.score", "eval/stats.gap"}   # `wide` is no per-env statistic
    assert info["eval/stats.score"] == float(np.float32(math.fsum(score) / N))
    assert info["eval/stats.gap"] == L / 2                       # nanmean: the odd envs' NaNs are skipped
    assert set(ev.stats) == {"score", "gap"} and ev.stats["score"].tolist() == score
    assert ev.stats["score"].data_ptr() != env.stats["score"].data_ptr()                  # a clone
    assert (ev.steps, env.steps, env.full_resets, env.masked_resets, ev.done_reads, pol.acts) == (L, L, 1, 0, 1, L)
    assert pol.same_out                                          # one persistent action tensor
    assert env.seeds == [3] and env.modes == [True] * L          # seeded, and stepped in training mode (views, no per-step clones)
    assert env.clears == [0]                                     # carried-over state is cleared once, in front of the full reset
    assert (env.training, env.seed, env.reset_epoch) == (False, 11, 3)
    info2 = ev.evaluate(seed=3)
    assert info2 == info and (ev.steps, ev.done_reads, env.full_resets) == (2 * L, 2, 2)
    assert torch.equal(torch.get_rng_state(), before) and (env.training, env.seed, env.reset_epoch) == (False, 11, 3)


def test_an_env_that_is_not_done_after_the_episode_length_raises_and_is_still_restored():
    L = 5
    env = StubEnv([L] * 6 + [9], L)
    ev = evaluator.DeviceEvaluator(env, StubPolicy())
    before = torch.get_rng_state().clone()
    with pytest.raises(HnsError, match="1 of 7 envs were not done after max_episode_length = 5 steps"):
        ev.evaluate(seed=1)
    assert torch.equal(torch.get_rng_state(), before) and (env.training, env.seed, env.reset_epoch) == (False, 11, 3)


def test_restart_and_the_evaluators_handling_of_a_collector():
    L, N, T = 5, 7, 2
    env, pol = StubEnv([L] * N, L), StubPolicy()
    col = collector.DeviceCollector(env, pol, T)
    col.collect()
    col.collect()
    assert env.full_resets == 1                                  # the observation is carried from one collect() to the next
    col.restart()
    col.collect()
    assert env.full_resets == 2 and col._since_full_reset == T   # restart(): the next collect() begins with a full reset
    ev = evaluator.DeviceEvaluator(env, pol, collector=col)
    ev.evaluate()
    assert env.full_resets == 3
    st = col.collect()
    assert env.full_resets == 4 and col._since_full_reset == T   # ... and so it does after an evaluation on the collector's env
    assert st.data["obs_self"][:, 0, 0, 0, 1].tolist() == [0.0] * N and st.data["obs_self"][:, 1, 0, 0, 1].tolist() == [1.0] * N
    with pytest.raises(ValueError, match="another env"):
        evaluator.DeviceEvaluator(StubEnv([L] * N, L), pol, collector=col)
    env2 = StubEnv([L] * 6 + [9], L)                             # a run that raises restarts the collector as well
    col2 = collector.DeviceCollector(env2, pol, T)
    col2.collect()
    with pytest.raises(HnsError):
        evaluator.DeviceEvaluator(env2, pol, collector=col2).evaluate()
    assert col2._cur is None
