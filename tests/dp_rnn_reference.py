"""Test-side helpers of the data-parallel recurrent update on top of tests/rnn_update_reference.py:

  * `split` / `union` / `segment_ids`: the ranks' parts of a head case and their union.  The parts of one update share the head's tensors, so a
    union of B_0 + B_1 + ... segments is built as ONE `head_case` and cut along B: the union is the concatenation of the parts, part r's
    segment ids are offset by the segments before it;
  * `branch_flip_case`: part 0 holds `head_case(branch="orig")` rows, part 1 — more of them — `branch="clip"` rows, over one head (the two
    cases differ in b_returns alone: the same seed draws the same y, head and b_values), so part 0 alone takes the unclipped branch of the max
    and the union the clipped one; `assert_branch_precondition` asserts exactly that in fp64, both separations >= 1e-3 of the loss;
  * `rescale_dead`: the fp64 / fp32 references of a union with dead segments — the statements on the live segments, rescaled to n = global_rows;
  * `split_rollout`: the ranks' env slices of a `rollout_case` and the union's segment ids of rank-local ones."""
import numpy as np
import torch

import rnn_update_reference as U

PER_ROW = ("y", "action", "log_probs_old", "advantages", "b_values", "b_returns")


def split(case, sizes):
    """The ranks' parts of a head case: consecutive runs of `sizes` segments, the head's tensors shared."""
    assert sum(sizes) == case["y"].shape[0]
    edges = np.concatenate([[0], np.cumsum(sizes)])
    return [{k: (v[lo:hi] if k in PER_ROW else v) for k, v in case.items()} for lo, hi in zip(edges[:-1], edges[1:])]


def union(parts):
    """The concatenation of the parts along B (the head's tensors are part 0's: all parts share them)."""
    for p in parts[1:]:
        assert all(np.array_equal(p[k], parts[0][k]) for k in p if k not in PER_ROW)
    return {k: (np.concatenate([p[k] for p in parts]) if k in PER_ROW else v) for k, v in parts[0].items()}


def segment_ids(sizes):
    """Part r's segment ids in the union's rollout: its own 0 .. B_r - 1, offset by the segments of the parts before it."""
    edges = np.concatenate([[0], np.cumsum(sizes)])
    return [np.arange(lo, hi, dtype=np.int64) for lo, hi in zip(edges[:-1], edges[1:])]


def branch_flip_case(sizes, L, A, seed):
    """(union, parts): part 0's rows push the unclipped mean loss up, part 1's — more rows — the clipped one."""
    B = sum(sizes)
    orig, clip = U.head_case(B, L, A, seed, branch="orig"), U.head_case(B, L, A, seed, branch="clip")
    assert all(np.array_equal(orig[k], clip[k]) for k in orig if k != "b_returns")
    c = dict(orig)
    c["b_returns"] = np.concatenate([orig["b_returns"][:sizes[0]], clip["b_returns"][sizes[0]:]])
    return c, split(c, sizes)


def assert_branch_precondition(c, parts):
    """In fp64: part 0 alone picks the other branch than the union, both separations >= 1e-3 of the loss."""
    alone, whole = U.critic_head_autograd(parts[0], torch.float64), U.critic_head_autograd(c, torch.float64)
    for tag, r in (("part 0", alone), ("the union", whole)):
        sep = abs(float(r["l_orig"]) - float(r["l_clip"]))
        assert sep >= 1e-3 * float(r["value_loss"]), f"{tag}: the two mean losses are {sep:.3e} apart"
    assert float(alone["l_orig"]) > float(alone["l_clip"]), "part 0 alone must take the unclipped branch"
    assert float(whole["l_clip"]) > float(whole["l_orig"]), "the union must take the clipped branch"
    return whole


def rescale_dead(c, keep, global_rows, dtype, entropy_coef=1e-3, loss="huber"):
    """The references of the union `c` when only the segments `keep` are live and every mean divides by n = global_rows (the entries' rule: a
    dead segment contributes nothing and n stays): the statements on the live segments, every mean rescaled by live rows / n, the entropy
    term's constant gradient kept, explained_var from the live rows' sums at n.  dy has the union's B with zeros at the dead segments."""
    B = c["y"].shape[0]
    sub = {k: (v[keep] if k in PER_ROW else v) for k, v in c.items()}
    a, v = U.actor_head_autograd(sub, dtype, entropy_coef=entropy_coef), U.critic_head_autograd(sub, dtype, loss=loss)
    n = float(global_rows)
    f = float(np.prod(sub["y"].shape[:3])) / n

    def full(x):
        out = np.zeros((B,) + x.shape[1:])
        out[keep] = x
        return out
    ra = {"dy": full(a["dy"] * f), "d_head_w": a["d_head_w"] * f, "d_head_b": a["d_head_b"] * f, "d_log_std": (a["d_log_std"] + entropy_coef) * f - entropy_coef,
          "policy_loss": a["policy_loss"] * f, "entropy": a["entropy"], "ratio": a["ratio"], "w": a["w"]}
    val, ret = v["values"], np.asarray(sub["b_returns"], np.float64 if dtype == torch.float64 else np.float32).astype(np.float64)
    var = ((ret * ret).sum() - ret.sum() ** 2 / n) / (n - 1.0)
    rv = {"dy": full(v["dy"] * f), "d_head_w": v["d_head_w"] * f, "d_head_b": v["d_head_b"] * f, "value_loss": v["value_loss"] * f,
          "explained_var": 1.0 - (((val - ret) ** 2).sum() / n) / var, "l_orig": v["l_orig"], "l_clip": v["l_clip"], "dist": v["dist"]}
    return ra, rv


def split_rollout(obs, states, is_init, per_row, envs):
    """The ranks' env slices of a rollout_case (and of per-row tensors [N, T, A, k]): `envs` envs each, in order."""
    edges = np.concatenate([[0], np.cumsum(envs)])
    assert edges[-1] == is_init.shape[0]
    out = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        out.append(({k: v[lo:hi] for k, v in obs.items()}, {k: v[lo:hi] for k, v in states.items()}, is_init[lo:hi],
                    {k: [r[lo:hi] for r in rows] for k, rows in per_row.items()}))
    return out


def union_segments(local, envs, segments_per_env):
    """Rank-local segment ids (lists, one per rank) -> the union's: rank r's are offset by the segments of the envs before it."""
    edges = np.concatenate([[0], np.cumsum(envs)]) * segments_per_env
    return np.concatenate([np.asarray(s, np.int64) + int(o) for s, o in zip(local, edges[:-1])])
