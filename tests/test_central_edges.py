"""The centralised critic's edge cases (tests/central_cases.py) on the CPU: what tests/test_hip_central_edges.py relies on
before it runs anything on a device.

The plans: ct_plan's central branch restated from its constants (32 rows a tile, 48 row ranges) gives the three PLANS shapes tps 2, 2 and 3
with a last row range of ONE tile holding ONE live row — a change of kCtMaxSplits or of the rule fails here.  Every smaller shape of the GPU
file stays at tps 1.

The conditions: every update case of the GPU file is off the tie of the max (>= 1e-3 of the loss), takes one branch in fp32 and fp64, has no
identically zero gradient tensor (in_proj_bias outside its k third) and is finite; the mixed-region case holds both Huber regions in 62 % of
its env-steps and both sides of the clip in 66 %, nearest gaps 1.1e-3 and 4.2e-4.

The gate has teeth at these shapes: central_reference.gate_update raises on the fp32 restatement of four wrong computations, each built by
changing the restatement's inputs or outputs (ratios e / max(e_32, 2^-24 max|ref_64|) against the bar of 8):
  (a) (3, 5, 35; 1537), the last tile's one live row left out of the sums, the means over 1 537: d embed state_drones.weight 1.1e5,
      d v_out.bias 6.6e4; all 20 gradients, grad_norm and value_loss (the least, 8.2e3) over the bar;
  (b) (3, 5, 35; 16), d embed state_drones from drone 0's token alone: its bias 1.3e6, its weight 8.5e5, nothing else;
  (c) (3, 5, 35; 16), the cylinders from agent 1's rows of the wide [S, A, K, 5] tensor: d v_out.bias 4.4e6, values 4.4e5, every output
      and gradient over the bar;
  (d) (7, 1, 20; 17), d v_out.bias from the first 16-row half of the tile: d v_out.bias 1.5e6, nothing else.

The package's CPU path (critic_train.value_loss_and_grad_central on CPU tensors) with check_index=False at the index cases: an entry outside
the rollout — negative, past 2^32, one past the end — contributes nothing and the means divide by the whole minibatch, include/hns.h's
contract for hns_critic_batch.index and what the kernel does; a repeated entry counts as often as it is drawn.  With the default
check_index=True the same index is refused with an IndexError that names the range.  Both cases are held to the gate against the yardstick
on the same index (worst ratios 1.34 and 1.40 with eight threads, 2.01 and 3.25 with one).

One tensor of the 1 537-position case is gated otherwise.  The CPU path is torch's own statements: F.layer_norm's native backward sums
d weight over all 1 534 x 23 = 35 282 token rows in fp32, in chunks that follow the thread count, where the restatement's written-out
LayerNorm lets autograd sum them another way.  d split_embed.layer_norm.weight is 13.67 / 7.28 / 9.92 / 8.18 / 5.53 / 4.97 / 4.97 x the
restatement's fp32 error with 1 / 2 / 3 / 4 / 5 / 8 / 16 threads (bar 8): over the bar with 1, 3 and 4.  The all-live statements, which this
file's change does not touch, have the same error on the live entries alone: 16.47 / 8.02 / 8.34 / 9.10 / 6.44 / 7.14 / 7.14 — it is
torch's summation over the rows, not the handling of the index.  That ONE tensor of that ONE case (OWN_YARDSTICK) is therefore held to 8 x
the all-live CPU path's own error, computed in the same process.  No other tensor was measured over the bar at any of those thread counts
(the nearest: split_embed.layer_norm.bias 7.54 and norm2.bias 5.02 with one thread), and all 19 other gradients, the scalars and the
values keep the rule above (DESIGN-open-items.md, item 16).  On the device every tensor of the case passes the unchanged gate
(tests/test_hip_central_edges.py: 1.42)."""
import numpy as np
import pytest
import torch

import central_cases as CE
import central_reference as CR
import policy_reference as R
from hns_amd import critic_train as CT

BAR = CR.BAR


def test_the_plans_are_what_the_cases_were_built_for():
    for (A, K, D, S), want in CE.PLANS.items():
        assert CE.central_plan(S) == want, ((A, K, D, S), CE.central_plan(S), want)
        tiles, tps, ranges, last, live = want
        assert tiles > CE.MAX_SPLITS and tps >= 2 and last == 1 and live == 1 and (ranges - 1) * tps + last == tiles
    assert [p[1] for p in CE.PLANS.values()] == [2, 2, 3]
    # the smallest batches with tps 2 and tps 3, and the first of each with one live row in the last tile
    assert CE.central_plan(1536)[1] == 1 and CE.central_plan(3072)[1] == 2
    # every other update case stays inside one tile per row range, as every shape of test_hip_critic_central.py does
    for name in CE.UPDATE_CASES:
        if name not in CE.PAST_RANGE:
            assert CE.central_plan(CE.steps(CE.case(name)))[1] == 1, name
    assert [CE.steps(CE.case(n)) for n in CE.PAST_RANGE] == [1537, 1537, 3073]
    # the restated workspace (the GPU file holds hns_critic_train_central_workspace_bytes to it): 25 row ranges' weight-gradient partials in
    # place of 48 outweigh the 49th tile, so the first tps 2 plan needs LESS than the last tps 1 plan
    assert CE.central_workspace_bytes(1536, 35, 3, 5) > CE.central_workspace_bytes(1537, 35, 3, 5) > CE.central_workspace_bytes(32, 35, 3, 5)
    assert (CE.central_workspace_bytes(1537, 35, 3, 5), CE.central_workspace_bytes(1537, 96, 7, 16), CE.central_workspace_bytes(3073, 20, 1, 5)) == \
        (23349760, 26441728, 37366272)


def test_the_dead_index_kills_the_last_range_and_the_fills_are_what_they_say():
    c = CE.case("a7k16d96s1537-dead")
    assert c.index[0] == -1 and c.index[768] == 2 ** 40 and c.index[1536] == 1600 == c.sd.shape[0] and c.layout == (40, 40)
    pos = CE.live_positions(c)
    assert pos.size == 1534 and pos.max() == 1535 and np.unique(c.index[pos]).size == 1534         # the last tile (position 1 536 alone) is dead
    r = CE.case("repeated")
    assert r.index.size == 70 and r.index.min() >= 0 and r.index.max() < 40 and np.unique(r.index).size == 34
    for name in CE.EDGES:
        e = CE.case(name)
        assert e.index.size == 700 and e.sd.shape == (1024, 3, 20) and e.cyl.shape == (1024, 8, 5)
    assert float(np.abs(CE.case("large_obs").sd).max()) > 600.0
    # a half exactly full, a half with one live row at A = 7, exactly full tiles, D = 1, one value
    assert [(CE.steps(CE.case("a%dk%dd%ds%d" % s)) - 1) % 32 + 1 for s in CE.FILLS] == [17, 31, 32, 16, 32, 1, 1]


@pytest.mark.parametrize("name", CE.UPDATE_CASES)
def test_every_case_meets_its_conditions(name):
    r64, r32 = CE.references(name)
    if name == "a1k1d1s1":                                      # the variance of one return: NaN on every side
        assert np.isnan(r64["explained_var"]) and np.isnan(r32["explained_var"])
    else:
        assert np.isfinite(r64["explained_var"]) and np.isfinite(r32["explained_var"])
    CE.check_conditions(name, r64, r32)


def test_the_mixed_case_holds_both_regions_inside_one_env_step():
    for name in ("mixed-huber", "mixed-mse"):
        c = CE.case(name)
        lin, cut, gap_delta, gap_clip = CE.mixed_shares(CE.references(name)[0], c)
        print(f"  {name}: {lin:.0%} of the env-steps hold both Huber regions, {cut:.0%} both sides of the clip; nearest gaps {gap_delta:.1e}, {gap_clip:.1e}")
        assert lin > 0.25 and cut > 0.25 and gap_delta > 1e-5 and gap_clip > 1e-5
    assert CE.case("mixed-huber").kw == {"huber_delta": 0.7} and CE.case("mixed-mse").kw == {"loss": "mse"}


def test_the_default_critic_keeps_random_critics_bits_and_the_knobs_are_critic_trains():
    a, b = CE.critic(20, 3, 21), CR.random_critic(20, 3, 21)
    assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)
    f = CE.critic(20, 3, 21, weight_scale=40.0, embed_scale=1e-4, flat_bias=True)
    for k in b:
        if "in_proj_weight" in k:
            assert np.array_equal(f[k], b[k] * np.float32(40.0))
        elif "split_embed.embed" in k and k.endswith("weight"):
            assert np.array_equal(f[k], b[k] * np.float32(1e-4))
        elif "split_embed.embed" in k and k.endswith("bias"):
            assert f[k][0] == np.float32(0.3) and abs(float(f[k][-1]) - 0.301) < 1e-6 and np.all(np.diff(f[k]) >= 0)
        else:
            assert np.array_equal(f[k], b[k])


# ---------------------------------------------------------------------------------------------------------------- the gate's teeth
def _over_the_bar(tag, got, r64, r32, named):
    """gate_update must raise on `got` and name `named`; returns {tensor: ratio} of everything over the bar."""
    with pytest.raises(AssertionError, match=named.replace(".", r"\.") + ": ratio"):
        CR.gate_update(tag, got, r64, r32, log=lambda s: None)
    items = [(n, got[n], r64[n], r32[n]) for n in ("value_loss", "explained_var", "grad_norm", "values")]
    items += [(n, got["grads"][n], r64["grads"][n], r32["grads"][n]) for n in r64["grads"]]
    over = {n: x for n, x in ((n, CR.ratio(h, a, b)) for n, h, a, b in items) if not x <= BAR}
    print(f"  {tag}: over the bar: " + ", ".join(f"{n} {x:.3g}" for n, x in sorted(over.items(), key=lambda kv: -kv[1])))
    return over


def test_teeth_a_the_last_tiles_one_live_row_left_out_of_the_sums():
    name = "a3k5d35s1537"
    c, (r64, r32) = CE.case(name), CE.references(name)
    part = CR.loss_and_grad(c.critic, c.sd, c.cyl, c.bv, c.ret, np.arange(1536), dtype=torch.float32, **c.kw)
    assert part["branch"] == r32["branch"]
    f = 1536.0 / 1537.0                                         # the mean still divides by the full count
    got = CE.copy_refs(r32)
    got.update(value_loss=part["value_loss"] * f, grad_norm=part["grad_norm"] * f, grads={k: g * f for k, g in part["grads"].items()})
    over = _over_the_bar("teeth-a", got, r64, r32, "v_out.bias")
    assert over["v_out.bias"] > 100 and len(over) >= 10


def test_teeth_b_d_embed_state_drones_from_drone_0_alone(monkeypatch):
    name = "a3k5d35s16"
    c, (r64, r32) = CE.case(name), CE.references(name)
    w, b = "base.split_embed.embed.state_drones.weight", "base.split_embed.embed.state_drones.bias"
    # the same encoder with the embedding's two tensors as two leaves each: drone 0's token through the first, drones 1 .. A - 1 through a
    # copy (policy_reference.encoder's state_others slot), so autograd hands the first leaf drone 0's part alone
    split = {**c.critic, w.replace("state_drones", "state_others"): c.critic[w].copy(), b.replace("state_drones", "state_others"): c.critic[b].copy()}

    def features(p, sd, cyl, dtype):
        q = {k.replace("embed.state_drones.", "embed.state_self."): v for k, v in p.items()}
        return R.encoder(q, "base.", {"state_self": sd[..., :1, :], "state_others": sd[..., 1:, :], "cylinders": cyl}, dtype)

    monkeypatch.setattr(CR, "features", features)
    wrong = CR.loss_and_grad(split, c.sd, c.cyl, c.bv, c.ret, None, dtype=torch.float32, **c.kw)
    monkeypatch.undo()
    assert CR.ratio(wrong["values"], r64["values"], r32["values"]) <= BAR          # the same forward pass
    got = CE.copy_refs(r32)
    got["grads"][w], got["grads"][b] = wrong["grads"][w], wrong["grads"][b]
    over = _over_the_bar("teeth-b", got, r64, r32, w)
    assert set(over) == {w, b} and over[w] > 100


def test_teeth_c_the_cylinders_of_agent_1():
    name = "a3k5d35s16"
    c, (r64, r32) = CE.case(name), CE.references(name)
    wide = np.repeat(c.cyl[:, None], 3, axis=1)
    wide[:, 1:] += 1.0                                          # the wide tensor of the device tests: the other agents' rows hold something else
    got = CR.loss_and_grad(c.critic, c.sd, wide[:, 1], c.bv, c.ret, None, dtype=torch.float32, **c.kw)
    over = _over_the_bar("teeth-c", got, r64, r32, "values")
    assert over["values"] > 100


def test_teeth_d_d_v_out_bias_from_the_first_half_of_the_tile():
    name = "a7k1d20s17"
    c, (r64, r32) = CE.case(name), CE.references(name)
    first = np.flatnonzero(np.arange(17) % 32 < 16)
    part = CR.loss_and_grad(c.critic, c.sd, c.cyl, c.bv, c.ret, first, dtype=torch.float32, **c.kw)
    assert part["branch"] == r32["branch"] and first.size == 16
    got = CE.copy_refs(r32)
    got["grads"]["v_out.bias"] = part["grads"]["v_out.bias"] * (16.0 / 17.0)
    over = _over_the_bar("teeth-d", got, r64, r32, "v_out.bias")
    assert set(over) == {"v_out.bias"} and over["v_out.bias"] > 100


# ---------------------------------------------------------------------------------------------------------------- the package's CPU path
# the ONE tensor of the 1 537-position CPU case measured over the bar (the module docstring's last paragraph)
OWN_YARDSTICK = "base.split_embed.layer_norm.weight"


def _cpu_call(c, **kw):
    t = torch.as_tensor
    crit = {k: t(v) for k, v in c.critic.items()}
    lay = (lambda x: t(x).reshape(*c.layout, *x.shape[1:])) if c.layout else t
    out = CT.value_loss_and_grad_central(crit, lay(c.sd), lay(c.cyl), lay(c.bv), lay(c.ret), t(c.index) if c.index is not None else None, **c.kw, **kw)
    return crit, out


@pytest.mark.parametrize("name", ["a7k16d96s1537-dead", "repeated"])
def test_the_cpu_path_follows_the_index_contract(name):
    """hns_critic_batch.index: "an index outside [0, N T) contributes nothing" — torch's own gather would read -1 from the end of the rollout
    and raise on 2^40.

    d split_embed.layer_norm.weight of the 1 537-position case alone has another yardstick (the module docstring's last paragraph): the CPU
    path's OWN error on the live entries — the all-live statements this change does not touch, scaled by live / B."""
    c, (r64, r32) = CE.case(name), CE.references(name)
    pos = CE.live_positions(c)
    crit, out = _cpu_call(c, check_index=False)
    v = out.values.numpy()
    assert v.shape == (c.index.size, c.sd.shape[1], 1)
    dead = np.setdiff1d(np.arange(c.index.size), pos)
    assert dead.size == (3 if name.endswith("dead") else 0) and not v[dead].any()
    got = {"value_loss": float(out.value_loss), "explained_var": float(out.explained_var), "grad_norm": float(out.grad_norm), "values": v[pos],
           "grads": {k: p.grad.double().numpy() for k, p in crit.items()}}
    if dead.size:
        live, _ = _cpu_call(c._replace(index=c.index[pos]))                              # check_index on: every entry is inside
        r32 = CE.copy_refs(r32)
        n = OWN_YARDSTICK
        own = live[n].grad.double().numpy() * (pos.size / c.index.size)
        print(f"  cpu path {name} {n}: {CR.ratio(got['grads'][n], r64['grads'][n], r32['grads'][n]):.2f} x the restatement's fp32 error, the all-live "
              f"path {CR.ratio(own, r64['grads'][n], r32['grads'][n]):.2f} x")
        r32["grads"][n] = own
    worst = CR.gate_update(f"cpu-{name}", got, r64, r32)
    print(f"  cpu path {name}: worst ratio {worst:.2f}")


def test_the_cpu_path_refuses_an_out_of_range_index_when_it_checks():
    c = CE.case("a7k16d96s1537-dead")
    with pytest.raises(IndexError, match=r"index values \[-1, 1099511627776\] outside the 1600 env-steps"):
        _cpu_call(c)
