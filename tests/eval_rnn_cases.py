"""What the recurrent evaluation's tests share (test_evaluator_rnn.py on the CPU, test_hip_evaluator_rnn.py on the GPU): the chains
`act_step` is run over beside `forward(deterministic=True)`, and the two hand-written evaluation loops `DeviceEvaluator` is compared with.

A chain is STEPS policy calls in which the pass's own state feeds its next call; env-level flags are set at steps 0 and 3 and nowhere else.
At step 0 the last env is flagged and, with more than one env, the first is not (so the random start state reaches the outputs); at step 3
the first env is flagged and, with more than one env, the last is not; the envs between draw their flag with probability 0.4."""
import numpy as np

import policy_reference as R
import policy_rnn_reference as RR

# (E, A, K, D): three rows of a 32-row tile; 33 rows (a second tile with one live row); no state_others; every limit at its maximum
SHAPES = [(1, 3, 5, 35), (11, 3, 5, 35), (5, 1, 5, 20), (3, 7, 16, 96)]
STEPS = 5


def chain_flags(E, seed):
    """The flags [E] bool of every step of a chain."""
    g = np.random.default_rng(seed)
    flags = []
    for t in range(STEPS):
        f = np.zeros(E, bool)
        if t in (0, 3):
            f = g.random(E) < 0.4
            f[-1] = t == 0
            f[0] = t == 3 or E == 1
        flags.append(f)
    assert flags[0].any() and flags[3].any() and not any(flags[t].any() for t in (1, 2, 4))
    return flags


def random_chain(E, A, K, D, seed):
    """(observation dict per step, flags [E] bool per step, the actor's start state [E, A, 128]) in numpy."""
    obs = [R.random_obs(E, A, K, D, seed + 10 * t + 1)[0] for t in range(STEPS)]
    return obs, chain_flags(E, seed), RR.random_states(E, A, seed + 5)[0]


def hand_loop(env, pol, seed, step_input, stateful=True, stacked=None):
    """The evaluation a user writes without DeviceEvaluator: a seeded full reset, then max_episode_length times
    forward(deterministic=True) -> step, both states carried out of place (stateful) or dropped after every step (not stateful: every step
    starts from zeros).  step_input(action) -> the tensordict env.step takes.  stacked: {statistic: []} filled with a clone per step, and
    "done" likewise.  Returns the tensordict after the last step."""
    env.set_seed(seed)
    if hasattr(env, "clear_carried_state"):
        env.clear_carried_state()
    cur = env.reset()
    ha = hc = None
    for _ in range(int(env.max_episode_length)):
        obs = cur[("agents", "observation")]
        out = pol.forward(obs["state_self"], obs.get("state_others", None), obs["cylinders"], actor_state=ha, critic_state=hc, deterministic=True)
        if stateful:
            ha, hc = out.actor_state, out.critic_state
        cur = env.step(step_input(out.action))["next"]
        if stacked is not None:
            for k in stacked:
                stacked[k].append((cur["done"] if k == "done" else env.stats[k]).clone())
    return cur
