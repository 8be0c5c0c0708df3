"""The per-agent actor update (hns_actor_train_grad_agents) past one row range and with padding tiles, CPU part: the plan that
tests/test_hip_per_agent_edges.py's shapes rest on, and the teeth of its gate — both from the restatements alone, without a device.

The plan: per_agent_cases.agents_plan restates ct_plan_agents (csrc/hns_policy_train.hip) and EDGE_PLANS pins it at every shape the device file
runs; agents_workspace_bytes restates the workspace's byte count and is held to the library's own size query over A 1..7, the B around every
threshold and two (D, K) pairs, so a change of kCtMaxSplits, of the rule or of a layout fails here instead of emptying the device file's coverage.

Teeth: every case is well posed (off the clip, the same side of it in fp64 and fp32) and every agent's last live tile holds a row that has a
gradient; then four defects the padded plan could have, emulated IN fp64 by leaving rows out of the reference, must exceed the gate's bar of
test_hip_per_agent.gate (e_defect / max(e_32, 2^-24 max|ref_64|) > 8) on the scalars and slices named below.  Measured (printed by
test_report_teeth; the weakest figure over the cases, as multiples of the bound, the bar being 8):
  last live tile of every agent lost      policy_loss 807 (a2k8d20-s780b769; 8.4e4 to 1.4e6 elsewhere); an agent's worst slice, weakest over
                                          the agents and cases, 355 (a7k16d24-s400b385, agent 1; 2.6e3 the next); ESS 1.2e3
                                          (a1k5d20-s1540b1537; not asserted)
  tps loop stops after one tile           the weakest of all slices of all agents 3.0e5 (a7k16d24-s260b256, log_std of agent 1), the worst
                                          4.9e6; policy_loss 6.8e5 (a2k8d20-s780b769)
  loss merge stops at 64 tiles (7; 385)   policy_loss 2.3e6, ESS 2.0e6 (agents 5 and 6 counted as adding nothing; the kernel would divide
                                          0 by 0 there)
  nothing left out                        the reference itself: equal but for log_std, whose entropy term is added apart (a rounding of fp64)"""
import ctypes as C

import numpy as np
import pytest
import torch

import actor_per_agent_reference as UA
import actor_update_reference as U
import per_agent_cases as PC

BAR = 8.0                                                        # test_hip_per_agent.BAR
TEETH = {}
TPS2 = [c for c, p in PC.EDGE_PLANS.items() if p[1] >= 2]


# ---------------------------------------------------------------------------------------------------------------- the plan
def test_the_table_is_the_plan_and_reaches_what_it_claims():
    for case, plan in PC.EDGE_PLANS.items():
        A, B = case[0], PC.edge_positions(case)
        tpa, tps, spa, pad, tiles = plan
        assert PC.agents_plan(B, A) == plan, (case, PC.agents_plan(B, A))
        assert tpa == -(-B // 32) and spa * tps == tpa + pad and tiles == A * (tpa + pad) and A * spa <= PC.MAX_SPLITS and B * A <= 2800
        assert (pad == 0) == (case in PC.EXACT_FIT or tps == 1)
    P = PC.EDGE_PLANS
    assert P[7, 16, 24, 200, 192][1] == 1 and PC.agents_plan(193, 7)[1] == 2                  # the threshold between tps 1 and 2 at A = 7
    assert 193 - 32 * (P[7, 16, 24, 200, 193][0] - 1) == 1 and P[7, 16, 24, 200, 193][3] == 1   # a one-row live tile and a padding tile, one range
    assert P[7, 16, 24, 400, 385][1:4] == (3, 5, 2) and P[7, 16, 24, 400, 385][4] > 64         # the loss merge's second trip
    assert PC.MAX_SPLITS % 5 and PC.MAX_SPLITS % 7                                             # 48 / A not exact
    assert {c[0] for c in PC.EDGE_CASES} == {1, 2, 3, 5, 7} and sum(c[4] is None for c in PC.EDGE_CASES) == 1
    # the shapes test_hip_per_agent.py runs (B <= 33) and its learner (32 positions a minibatch) reach none of it
    assert all(PC.agents_plan(B, A)[1:4:2] == (1, 0) for B in (1, 5, 17, 32, 33) for A in range(1, 8))
    # a real minibatch: 8 192 positions x 3 agents fit exactly, one position more pads 14 tiles per agent
    assert PC.agents_plan(8192, 3) == (256, 16, 16, 0, 768) and PC.agents_plan(8193, 3)[1:4] == (17, 16, 15)


def test_the_workspace_bytes_restated_equal_the_librarys_size_query():
    import __graft_entry__ as g
    lib = C.CDLL(g.build())
    query = lib.hns_actor_train_agents_workspace_bytes
    query.restype, query.argtypes = C.c_size_t, [C.c_int64, C.c_int32, C.c_int32, C.c_int32]
    table = {PC.edge_positions(c) for c in PC.EDGE_CASES}
    Bs = sorted({1, 31, 32, 33} | table | {b - 1 for b in table} | {b + 1 for b in table})
    for D, K in ((35, 5), (24, 16)):
        for A in range(1, 8):
            for B in Bs:
                assert query(B * A, D, A, K) == PC.agents_workspace_bytes(B, D, A, K) > 0, (B, D, A, K)
    for A, K, D, _, _ in PC.EDGE_CASES:                          # ... and at every case's own (D, K)
        assert all(query(B * A, D, A, K) == PC.agents_workspace_bytes(B, D, A, K) for B in Bs)


# ---------------------------------------------------------------------------------------------------------------- teeth
_REFS = {}


def _refs(case):
    """(the case's data, its fp64 and fp32 references): computed once, never changed."""
    if case not in _REFS:
        data = PC.edge_case(case)
        _REFS[case] = (data, UA.loss_and_grad(*data, dtype=torch.float64), UA.loss_and_grad(*data, dtype=torch.float32))
    return _REFS[case]


def _ratio(h, a, b):
    """test_hip_per_agent._check's figure: max|h - a| over max(max|b - a|, 2^-24 max|a|)."""
    h, a, b = np.asarray(h, np.float64), np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(h - a).max()) / max(float(np.abs(b - a).max()), 2.0 ** -24 * float(np.abs(a).max()))


def _without(case, keep, entropy_coef=0.001):
    """What the kernels would give if the minibatch positions outside `keep` (bool [B], the same for every agent) never reached the sums: the
    fp64 reference over the kept positions alone, its row sums rescaled to the full n = B A, the entropy term's constant gradient whole, ESS
    over the kept ratios divided by the full B."""
    (actors, obs, action, lpo, adv, index), r64, _ = _refs(case)
    A, B = case[0], PC.edge_positions(case)
    assert keep.shape == (B,) and 0 < keep.sum()
    steps = (index if index is not None else np.arange(B))[keep]
    r = UA.loss_and_grad(actors, obs, action, lpo, adv, steps, entropy_coef=0.0)
    share = keep.sum() / B
    grads = {k: v * share for k, v in r["grads"].items()}
    grads["act_dist.log_std"] = grads["act_dist.log_std"] - entropy_coef / A
    return {"policy_loss": r["policy_loss"] * share, "ess": r["ess"] * share, "grads": grads}


def _slice_ratios(h, r64, r32):
    """{(name, agent): the gate's figure of that slice}."""
    A = r64["log_probs"].shape[1]
    return {(n, a): _ratio(h["grads"][n][a], r64["grads"][n][a], r32["grads"][n][a]) for n in r64["grads"] for a in range(A)}


@pytest.mark.parametrize("case", PC.EDGE_CASES, ids=PC.edge_tag)
def test_the_case_is_well_posed_and_every_last_live_tile_has_a_gradient(case):
    """(a) off the clip with rows of every kind, and fp32 on the same side of it on every row; (b) each agent's last live tile (positions
    >= 32 (tpa - 1)) holds a row with w = 1 and a non-zero advantage — a clipped row has no gradient, and a kernel that lost it would show
    nothing.  Asserted for the exact-fit cases too (their last tiles are full)."""
    _, r64, r32 = _refs(case)
    A, B = case[0], PC.edge_positions(case)
    assert U.assert_off_the_clip(r64, 0.1, need_all=True) >= 1e-3
    assert np.array_equal(r64["w"], r32["w"])
    assert r64["w"].shape == (B, A, 1)
    tail = slice(32 * (PC.EDGE_PLANS[case][0] - 1), None)
    live = [int(((r64["w"][tail, a, 0] == 1) & (r64["adv"][tail, a, 0] != 0)).sum()) for a in range(A)]
    print(f"  {PC.edge_tag(case)}: rows with a gradient in each agent's last live tile {live} of {B - tail.start}")
    assert min(live) >= 1, live


def test_leaving_nothing_out_is_the_reference():
    """The emulation of the defects with no defect: exactly the reference, so what the next tests measure is the defect's alone."""
    case = (3, 5, 35, 513, None)
    _, r64, r32 = _refs(case)
    h = _without(case, np.ones(513, bool))
    assert h["policy_loss"] == r64["policy_loss"] and h["ess"] == r64["ess"]
    assert all(np.array_equal(h["grads"][n], r64["grads"][n]) for n in r64["grads"] if n != "act_dist.log_std")
    assert max(_slice_ratios(h, r64, r32).values()) <= 1e-3      # (log_std: the entropy term added apart, a rounding of fp64)


@pytest.mark.parametrize("case", PC.EDGE_CASES, ids=PC.edge_tag)
def test_losing_each_agents_last_live_tile_fails_the_gate(case):
    """(c) positions >= 32 (tpa - 1) never reach the sums: policy_loss and at least one gradient slice of EVERY agent exceed the bar."""
    _, r64, r32 = _refs(case)
    A, B = case[0], PC.edge_positions(case)
    h = _without(case, np.arange(B) < 32 * (PC.EDGE_PLANS[case][0] - 1))
    loss, ess = _ratio(h["policy_loss"], r64["policy_loss"], r32["policy_loss"]), _ratio(h["ess"], r64["ess"], r32["ess"])
    sl = _slice_ratios(h, r64, r32)
    worst = [max(v for (n, a), v in sl.items() if a == ag) for ag in range(A)]
    print(f"  {PC.edge_tag(case)}: policy_loss {loss:.3g}, ESS {ess:.3g}, each agent's worst slice {['%.3g' % w for w in worst]} x the bound")
    TEETH.setdefault("last live tile lost: policy_loss", []).append((loss, PC.edge_tag(case)))
    TEETH.setdefault("last live tile lost: ESS (not asserted)", []).append((ess, PC.edge_tag(case)))
    TEETH.setdefault("last live tile lost: an agent's worst slice", []).append((min(worst), PC.edge_tag(case)))
    assert loss > BAR and min(worst) > BAR, (loss, worst)


@pytest.mark.parametrize("case", TPS2, ids=PC.edge_tag)
def test_a_tps_loop_that_stops_after_one_tile_fails_the_gate_on_every_slice(case):
    """(d) of each row range only the first tile is summed — positions with (position // 32) % tps == 0: EVERY slice of EVERY agent exceeds
    the bar, and policy_loss."""
    _, r64, r32 = _refs(case)
    B, tps = PC.edge_positions(case), PC.EDGE_PLANS[case][1]
    h = _without(case, (np.arange(B) // 32) % tps == 0)
    sl = _slice_ratios(h, r64, r32)
    loss = _ratio(h["policy_loss"], r64["policy_loss"], r32["policy_loss"])
    weakest = min(sl, key=sl.get)
    print(f"  {PC.edge_tag(case)}: policy_loss {loss:.3g}, the weakest of {len(sl)} slices {weakest} {sl[weakest]:.3g}, the worst {max(sl.values()):.3g} x the bound")
    TEETH.setdefault("tps loop stops after one tile: the weakest slice", []).append((sl[weakest], f"{PC.edge_tag(case)} {weakest}"))
    TEETH.setdefault("tps loop stops after one tile: policy_loss", []).append((loss, PC.edge_tag(case)))
    assert len(sl) == case[0] * (23 if case[0] > 1 else 21)     # every stacked tensor (state_others' two absent at A = 1), every agent
    assert loss > BAR and sl[weakest] > BAR, (weakest, sl[weakest])


def test_a_loss_merge_that_stops_at_64_tiles_fails_the_gate():
    """(e) at (7; 385): 15 tiles per agent, 13 live, numbered agent-major; only tiles 0..63 reach the scalars — agents 0-3 whole, agent 4's
    positions < 128, agents 5 and 6 not at all (they add nothing to ESS here; the kernel's a1^2 / a2 would be 0 / 0).  ESS and policy_loss
    exceed the bar."""
    case = (7, 16, 24, 400, 385)
    _, r64, r32 = _refs(case)
    A, B = 7, 385
    tpa, tps, spa, pad, tiles = PC.EDGE_PLANS[case]
    tile = np.arange(A)[None, :] * (tpa + pad) + (np.arange(B) // 32)[:, None]                # [B, A]: agent-major tile numbers
    keep = tile < 64
    assert tiles > 64 and keep[:, :4].all() and keep[:, 4].sum() == 128 and not keep[:, 5:].any()
    ratio, adv = r64["ratio"][..., 0], r64["adv"][..., 0]
    surr = np.minimum(ratio * adv, np.clip(ratio, 0.9, 1.1) * adv)
    assert abs(-4.0 * surr.sum() / (B * A) - r64["policy_loss"]) <= 1e-12 * max(1.0, abs(r64["policy_loss"]))
    # exp(2 logsumexp(r) - logsumexp(2 r)) per agent, of the ratio itself, as the reference writes it
    ess_of = lambda k: sum(np.exp(ratio[k[:, a], a]).sum() ** 2 / np.exp(2 * ratio[k[:, a], a]).sum() for a in range(A) if k[:, a].any()) / A / B   # noqa: E731
    assert abs(ess_of(np.ones_like(keep)) - r64["ess"]) <= 1e-12
    loss = _ratio(-4.0 * surr[keep].sum() / (B * A), r64["policy_loss"], r32["policy_loss"])
    ess = _ratio(ess_of(keep), r64["ess"], r32["ess"])
    print(f"  loss merge stops at 64 tiles: policy_loss {loss:.3g}, ESS {ess:.3g} x the bound")
    TEETH["loss merge stops at 64 tiles: policy_loss"] = [(loss, PC.edge_tag(case))]
    TEETH["loss merge stops at 64 tiles: ESS"] = [(ess, PC.edge_tag(case))]
    assert loss > BAR and ess > BAR


def test_report_teeth():
    for what, figures in TEETH.items():
        print(f"  {what}: weakest {min(figures)[0]:.3g} ({min(figures)[1]}) x the bound, bar {BAR}")
