"""The cases the recurrent policy step is held to, shared by the CPU emulation (test_policy_rnn.py) and the device
(test_hip_policy_rnn.py, test_hip_policy_rnn_edges.py): every case is a CHAIN

    (actor, critic, obs per step, eps per step, flags per step, the actor's start state, the critic's)

in numpy, run with each side's own states feeding its next step.  `case(tag)` builds a chain once per process, `references(tag)` gives the
fp64 and fp32 restatements' outputs per step (policy_rnn_reference.forward, each chain feeding itself), CASE_TAGS names every chain the
device gate runs.

Shapes are (E, A, K, D).  The kernels work on tiles of 32 rows (rows = E A, row = env A + agent), so what a shape exercises is its tile
count, the live rows of its last tile and where the env boundaries fall inside the tiles:
  SHAPES          the four of test_hip_policy_rnn.py: 3, 33, 5 and 21 rows, 5-step chains with flags at steps 0 and 3
  sweep_shape     32 seeds, E A mod 32 == seed: every tail length, A 1..7, 1 to 7 tiles; 2-step chains, half of the envs flagged at step 2
  FULL_TILES      32, 64 and 96 rows: residue 0 with one, two and three tiles
  STRADDLE_SHAPES A in (3, 5, 6, 7) with 40 envs: tiles that do not start on an env boundary; one step, `straddling_envs` flagged
  EDGES           the encoder's three numerical edges behind a GRU, and the GRU step's own four; 3-step chains of envs chosen so that the
                  reference itself is well posed
  LONG_CHAIN      64 steps at 33 rows"""
import functools
import math
import os

import numpy as np
import torch

import policy_reference as R
import policy_rnn_reference as RR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TILE = RR.TILE

# ---- the four shapes of test_hip_policy_rnn.py: three rows of a 32-row tile; 33 rows (a second tile with one live row); no state_others;
# every limit at its maximum
SHAPES = [(1, 3, 5, 35), (11, 3, 5, 35), (5, 1, 5, 20), (3, 7, 16, 96)]
STEPS = 5


def shape_tag(shape):
    return "e%da%dk%dd%d" % tuple(shape)


def random_chain(E, A, K, D, seed, steps=STEPS):
    """(obs per step, eps per step, flags per step, h0 actor, h0 critic): flags for some envs at steps 0 and 3 (E = 1: at step 3)."""
    g = np.random.default_rng(seed)
    obs, eps, flags = [], [], []
    for t in range(steps):
        o, e = R.random_obs(E, A, K, D, seed + 10 * t + 1)
        obs.append(o)
        eps.append(e)
        f = np.zeros(E, bool)
        if t in (0, 3):
            f = g.random(E) < 0.4
            f[0] = t == 3
            if E > 1:
                f[-1] = t == 0
        flags.append(f)
    ha, hc = RR.random_states(E, A, seed + 5)
    return obs, eps, flags, ha, hc


def shape_case(shape):
    E, A, K, D = shape
    return (*RR.random_net(D, A, 300 + E + A), *random_chain(E, A, K, D, 400 + E))


def golden_chain(tag):
    gp, gg, z = (np.load(os.path.join(GOLDEN, n)) for n in ("g_policy.npz", "g_gru.npz", "g_policy_rnn.npz"))
    actor, critic = RR.golden_params(gp, gg, tag)
    case = RR.golden_case(z, tag)
    T = int(case["shape"][4])
    return actor, critic, [RR.step_obs(case, t) for t in range(T)], list(case["eps"]), list(case["is_init"]), case["h0:actor"], case["h0:critic"]


# ---- the seeded sweep
SWEEP_SEEDS = range(32)
MAX_SWEEP_TILES = 7


def tiles_of(shape):
    return -(-shape[0] * shape[1] // TILE)


def sweep_shape(seed):
    """(E, A, K, D) with E A mod 32 == seed: A drawn from the agent counts that can reach the residue (gcd(A, 32) divides it), E from the env
    counts that do with at most MAX_SWEEP_TILES tiles (E <= 32 always does), K in 1..16, D in 1..96."""
    g = np.random.default_rng(7000 + seed)
    A = 4 if seed % 8 == 4 else int(g.choice([a for a in range(1, 8) if seed % math.gcd(a, TILE) == 0]))     # (four agents reach 0, 4, .., 28 only)
    E = int(g.choice([e for e in range(1, MAX_SWEEP_TILES * TILE // A + 1) if e * A % TILE == seed]))
    return E, A, int(g.integers(1, 17)), int(g.integers(1, 97))


def sweep_case(shape, seed):
    """A 2-step chain at `shape`: random start states, no flag at step 1, a random half of the envs flagged at step 2 (E = 1: its env)."""
    E, A, K, D = shape
    actor, critic = RR.random_net(D, A, 7100 + seed)
    g = np.random.default_rng(7200 + seed)
    obs, eps = zip(*(R.random_obs(E, A, K, D, 7300 + 10 * seed + t) for t in range(2)))
    half = np.zeros(E, bool)
    half[g.permutation(E)[:(E + 1) // 2]] = True
    return actor, critic, list(obs), list(eps), [np.zeros(E, bool), half], *RR.random_states(E, A, 7400 + seed)


# residue 0 with one, two and three tiles (the seeds give residue 0 once)
FULL_TILES = [(8, 4, 5, 35), (32, 2, 3, 20), (32, 3, 5, 35)]

# ---- tiles that do not start on an env boundary
STRADDLE_SHAPES = [(40, A, 5, 35) for A in (3, 5, 6, 7)]


def straddling_envs(E, A):
    """The envs whose agents' rows fall in two tiles."""
    return [e for e in range(E) if e * A // TILE != (e * A + A - 1) // TILE]


def straddle_case(shape):
    """One step with exactly the straddling envs flagged."""
    E, A, K, D = shape
    actor, critic = RR.random_net(D, A, 7500 + A)
    obs, eps = R.random_obs(E, A, K, D, 7510 + A)
    flags = np.zeros(E, bool)
    flags[straddling_envs(E, A)] = True
    return actor, critic, [obs], [eps], [flags], *RR.random_states(E, A, 7520 + A)


# ---- numerical edges: the encoder's three (policy_reference.EDGES) with a random GRU behind each network, and the step's own: saturated
# gates (both GRU weight matrices x 40: 1 / (1 + expf(-a)) at its overflow end), large caller-supplied states (x 60), an update gate that is
# exactly one (`carry`: b_iz + 30, so h' = h bit for bit), LayerNorm(h' + f) on a nearly flat sum (`near_flat_norm`: carry with
# h0 = 0.3 - f_32 + 1e-2 N(0, 1), the same observation at every step so that the sum stays flat).
#
# An edge is only a check where the REFERENCE is well posed: the gate's bound max(e_32, 2^-24 max|ref_64|) must stay below POSED_CAP
# max|ref_64| at every step of the self-fed chain, or an error of 1e-3 passes.  A saturated softmax has rows near a tie (scores x 1600) and
# weights x 40 amplify a state's fp32 error from step to step, and the bound is a maximum over rows: so each edge draws a pool of EDGE_POOL
# times its envs and keeps, in order, the first envs whose own rows stay below POSED_SELECT (half the cap: flat tokens and x 40 gates sit
# at 3e-5 to 5e-5 in the bulk of their rows) in the two CPU restatements alone.  Envs do not interact, so the kept envs' references are the pool's.
EDGES = R.EDGES + ("saturated_gates", "large_state", "carry", "near_flat_norm")
EDGE_STEPS, EDGE_POOL = 3, 3
POSED_CAP, POSED_SELECT = 1e-4, 5e-5
EDGE_SHAPES = {name: (64, 3, 8, 20) if name in R.EDGES else (43, 3, 5, 35) for name in EDGES}      # 192 rows: six full tiles; 129: four and a row


def _edge_pool(name):
    """The edge's chain over EDGE_POOL times its envs; a random third of the envs flagged at step 1."""
    k = EDGES.index(name)
    E, A, K, D = EDGE_SHAPES[name]
    E *= EDGE_POOL
    ha, hc = RR.random_states(E, A, 7620 + k)
    if name in R.EDGES:
        actor, critic, obs, _ = R.edge_case(name)
        assert obs["state_self"].shape[1:] == (A, 1, D) and obs["cylinders"].shape[2] == K
        actor, critic = RR.add_random_gru(actor, critic, 7600 + k)
        obs = [{key: v[t * E:(t + 1) * E] for key, v in obs.items()} for t in range(EDGE_STEPS)]          # other envs of the case per step
    else:
        actor, critic = RR.random_net(D, A, 7600 + k)
        obs = [R.random_obs(E, A, K, D, 7630 + 10 * k + t)[0] for t in range(EDGE_STEPS)]
        if name == "saturated_gates":
            for p in (actor, critic):
                for n in ("rnn.cell.weight_ih", "rnn.cell.weight_hh"):
                    p[n] = p[n] * np.float32(40.0)
        elif name == "large_state":
            ha, hc = ha * np.float32(60.0), hc * np.float32(60.0)
        else:
            for p in (actor, critic):
                p["rnn.cell.bias_ih"] = p["rnn.cell.bias_ih"].copy()
                p["rnn.cell.bias_ih"][RR.H:2 * RR.H] += np.float32(30.0)
            if name == "near_flat_norm":
                obs = [obs[0]] * EDGE_STEPS
                t = lambda p: {key: torch.as_tensor(np.asarray(v)) for key, v in p.items()}
                g = np.random.default_rng(7640)
                f32 = [R.encoder(t(p), prefix, t(obs[0]), torch.float32).numpy() for p, prefix in ((actor, "encoder."), (critic, "base."))]
                ha, hc = ((np.float32(0.3) - f + np.float32(1e-2) * g.standard_normal(f.shape).astype(np.float32)).astype(np.float32) for f in f32)
    g = np.random.default_rng(7650 + k)
    eps = [g.standard_normal((E, A, 4)).astype(np.float32) for _ in range(EDGE_STEPS)]
    flags = [np.zeros(E, bool) for _ in range(EDGE_STEPS)]
    flags[1][g.permutation(E)[:E // 3]] = True
    return actor, critic, obs, eps, flags, ha, hc


def posedness(refs):
    """Per env, the largest over steps and outputs of max(e_32 of the env's rows, 2^-24 max|ref_64|) / max|ref_64| (the maxima of the
    reference over all rows of the step): the gate's bound relative to the output's size."""
    worst = 0.0
    for r64, r32 in refs:
        for name in RR.OUTPUTS:
            a, b = r64[name], r32[name]
            assert np.isfinite(a).all() and np.isfinite(b).all(), name
            top = float(np.abs(a).max())
            e = np.abs(b - a).reshape(a.shape[0], -1).max(1)
            worst = np.maximum(worst, np.maximum(e, 2.0 ** -24 * top) / top)
    return worst


def take_envs(chain, envs):
    actor, critic, obs, eps, flags, ha, hc = chain
    return (actor, critic, [{k: v[envs] for k, v in o.items()} for o in obs], [e[envs] for e in eps], [f[envs] for f in flags], ha[envs], hc[envs])


def edge_case(name):
    """A 3-step chain at EDGE_SHAPES[name]: the first envs of the edge's pool that are well posed in the reference alone."""
    assert name in EDGES, name
    pool = _edge_pool(name)
    keep = np.nonzero(posedness(chain_references(pool)) <= POSED_SELECT)[0]
    E = EDGE_SHAPES[name][0]
    assert len(keep) >= E, f"{name}: only {len(keep)} of {len(pool[5])} envs of the pool are well posed"
    return take_envs(pool, keep[:E])


# ---- the long chain: 64 steps (a segment is 16, the device gate's other chains 5) with flags on some envs around the segment boundary
LONG_CHAIN = (11, 3, 5, 35)
LONG_STEPS, LONG_FLAG_STEPS, LONG_CPU_STEPS = 64, (0, 15, 16, 17, 40, 63), 8


def long_case(steps=LONG_STEPS):
    E, A, K, D = LONG_CHAIN
    actor, critic = RR.random_net(D, A, 7700)
    g = np.random.default_rng(7701)
    obs, eps = zip(*(R.random_obs(E, A, K, D, 7710 + t) for t in range(LONG_STEPS)))
    flags = [(g.random(E) < 0.4) if t in LONG_FLAG_STEPS else np.zeros(E, bool) for t in range(LONG_STEPS)]
    for t in LONG_FLAG_STEPS:
        flags[t][t % E] = True                                   # at least one env flagged, at least one not
        flags[t][(t + 1) % E] = False
    ha, hc = RR.random_states(E, A, 7702)
    return actor, critic, list(obs)[:steps], list(eps)[:steps], flags[:steps], ha, hc


# ---- every chain the device gate runs
def sweep_tag(seed):
    return "sweep-%02d-" % seed + shape_tag(sweep_shape(seed))


@functools.lru_cache(maxsize=None)
def case(tag):
    """The chain of a tag of CASE_TAGS (built once per process; treat it as read-only)."""
    kind, _, rest = tag.partition("-")
    if tag in RR.CASES:
        return golden_chain(tag)
    if kind == "random":
        return shape_case(next(s for s in SHAPES if shape_tag(s) == rest))
    if kind == "sweep":
        seed = int(rest[:2])
        return sweep_case(sweep_shape(seed), seed)
    if kind == "full":
        shape = next(s for s in FULL_TILES if shape_tag(s) == rest)
        return sweep_case(shape, 100 + tiles_of(shape))
    if kind == "straddle":
        return straddle_case(next(s for s in STRADDLE_SHAPES if shape_tag(s) == rest))
    if kind == "long":
        return long_case(LONG_CPU_STEPS if rest == "first%d" % LONG_CPU_STEPS else LONG_STEPS)
    return edge_case(tag)


OLD_SHAPE_TAGS = ["random-" + shape_tag(s) for s in SHAPES]
SWEEP_TAGS = [sweep_tag(s) for s in SWEEP_SEEDS]
FULL_TAGS = ["full-" + shape_tag(s) for s in FULL_TILES]
STRADDLE_TAGS = ["straddle-" + shape_tag(s) for s in STRADDLE_SHAPES]
LONG_CPU_TAG = "long-first%d" % LONG_CPU_STEPS
# what the CPU emulation is run on: all of the device gate's chains, the long one over its first steps
CASE_TAGS = list(RR.CASES) + OLD_SHAPE_TAGS + SWEEP_TAGS + FULL_TAGS + STRADDLE_TAGS + list(EDGES) + [LONG_CPU_TAG]


def chain_references(chain, mode=False):
    """[(fp64 outputs, fp32 outputs)] per step of a chain, {name: fp64 numpy}: policy_rnn_reference.forward at both dtypes, each chain feeding
    itself.  mode: eps None (the log-probability at the mode; nothing else changes)."""
    actor, critic, obs, eps, flags, ha, hc = chain
    h = {torch.float64: (ha, hc), torch.float32: (ha, hc)}
    out = []
    for t in range(len(obs)):
        step = []
        for dtype in (torch.float64, torch.float32):
            r = RR.forward(actor, critic, obs[t], *h[dtype], flags[t], None if mode else eps[t], dtype)
            h[dtype] = (r["actor_state"], r["critic_state"])
            step.append({k: v.double().numpy() for k, v in r.items()})
        out.append(tuple(step))
    return out


@functools.lru_cache(maxsize=None)
def references(tag, mode=False):
    """chain_references of the chain `tag`, computed once per process (read-only)."""
    return chain_references(case(tag), mode)
