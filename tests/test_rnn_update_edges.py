"""The composed recurrent update (hns_amd.rnn_train) past one tile of each of its ops, CPU part: the plans that
tests/test_hip_rnn_update_edges.py's cases rest on, their well-posedness, and the teeth of its gate — without a device.

Plans: rnn_update_cases.plan restates gru_plan, ct_plan_encoder and the head entries' geometry from the kernels' constants; its byte counts are
held to the library's own size queries at every case (and one sequence / row / segment to either side of it), and REACH asserts from the plan
what each case is there for, so a tile size or a grid cap that changes fails here instead of emptying the device file's coverage.

Well-posedness: every case and network, at its recorded seed, is off both clips by U.MARGIN, takes the same side of the clip in fp32, has its
two mean value losses apart, and rnn_train's CPU torch path — a second fp32 evaluation in another summation order — stays at ratio <= 4 on
every gated item (each gradient tensor, the scalars, log_probs / values, grad_norm), half the device's bar of 8.

Teeth (DEFECT_TABLE): six defects a kernel's plan could hide, emulated in fp32 by rnn_update_cases.defect_flow — the flow with the lost
contributions detached, bit for bit the flow when nothing is lost.  Each fails U.gate (bar 8) on its named cases and loses nothing at the
present shape of test_update_gradients_against_the_independent_flow (N 3, T 8, L 4, 5 segments), where its bits are the fp32 flow's: that
test cannot see it.  The smallest of the named cases' worst ratios, per defect (actor / critic; test_report_teeth prints them):
    gru_first_tile_only               1.6e6 (one-step) / 2.8e6 (widest)
    gru_first_trip_only               8.2e4 / 6.9e4 (second-trips: one sequence of 4 097)
    gru_wgrad_one_tile_per_range      1.6e6 (second-trips) / 1.9e6 (longest)
    encoder_wgrad_one_tile_per_range  2.2e6 (second-trips) / 1.3e6 (encoder-ranges)
    head_first_trip_only              3.0e6 / 1.1e7 (second-trips: four rows of 16 388)
    ess_first_stride_only             4.1e5 (ess-columns), on ESS alone / the critic has no ESS"""
import ctypes as C

import numpy as np
import pytest
import torch

import rnn_update_cases as RC
import rnn_update_reference as U

TEETH = {}
NETS = [True, False]
net_id = lambda actor: "actor" if actor else "critic"           # noqa: E731


# ---------------------------------------------------------------------------------------------------------------- the plans
def _queries():
    import __graft_entry__ as g
    lib = C.CDLL(g.build())
    sig = {"hns_gru_workspace_bytes": [C.c_int64, C.c_int32, C.c_int32], "hns_encoder_workspace_bytes": [C.c_int64] + [C.c_int32] * 4,
           "hns_rnn_actor_head_workspace_bytes": [C.c_int64, C.c_int32, C.c_int32], "hns_rnn_critic_head_workspace_bytes": [C.c_int64, C.c_int32, C.c_int32]}
    for name, args in sig.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = C.c_size_t, args
    return lib


def test_every_plan_agrees_with_the_librarys_size_queries():
    lib = _queries()
    shapes = list(RC.CASES.values()) + [RC.PRESENT]
    shapes += [c._replace(B=c.B + d) for c in RC.CASES.values() for d in (-1, 1) if c.B + d >= 1]
    for c in shapes:
        p = RC.plan(c)
        assert lib.hns_gru_workspace_bytes(c.B * c.A, c.L, 1) == p["gru_bytes"] > 0, c
        assert lib.hns_gru_workspace_bytes(c.B * c.A, c.L, 0) == 0
        assert lib.hns_encoder_workspace_bytes(c.B * c.L * c.A, c.D, c.A, c.K, 1) == p["enc_bytes"] > 0, c
        assert lib.hns_encoder_workspace_bytes(c.B * c.L * c.A, c.D, c.A, c.K, 0) == p["enc_forward_bytes"] > 0, c
        assert lib.hns_rnn_actor_head_workspace_bytes(c.B, c.A, c.L) == p["actor_head_bytes"] > 0, c
        assert lib.hns_rnn_critic_head_workspace_bytes(c.B, c.A, c.L) == p["critic_head_bytes"] > 0, c


def test_the_size_queries_move_where_the_plan_says_its_counts_move():
    """The byte counts above contain every count of the plan — the GRU's ranges and workgroups, the encoder's tiles and ranges, the head's
    workgroups — so the equalities pin them; here the thresholds themselves: one more range, workgroup or tile changes the library's answer by
    the restated amount exactly at the restated size."""
    lib = _queries()
    L, A = 4, 1
    for seqs in (RC.GRU_TILE * RC.GRU_GROUPS, RC.GRU_TILE * RC.GRU_GROUPS + 1, RC.GRU_WG_ROWS * RC.GRU_SPLITS // L, RC.GRU_WG_ROWS * RC.GRU_SPLITS // L + 1):
        c = RC.Case(A, 5, 20, seqs + 1, L, L, seqs)
        assert lib.hns_gru_workspace_bytes(seqs, L, 1) == RC.plan(c)["gru_bytes"], seqs
    for rows in (RC.ENC_ROWS * RC.ENC_SPLITS, RC.ENC_ROWS * RC.ENC_SPLITS + 1, RC.HEAD_ROWS * RC.HEAD_GROUPS, RC.HEAD_ROWS * RC.HEAD_GROUPS + 1):
        c = RC.Case(A, 5, 20, rows + 1, 1, 1, rows)
        p = RC.plan(c)
        assert lib.hns_encoder_workspace_bytes(rows, 20, A, 5, 1) == p["enc_bytes"], rows
        assert lib.hns_rnn_actor_head_workspace_bytes(rows, A, 1) == p["actor_head_bytes"] and lib.hns_rnn_critic_head_workspace_bytes(rows, A, 1) == p["critic_head_bytes"]
    assert RC.plan(RC.Case(1, 5, 20, 2, 1, 1, RC.ENC_ROWS * RC.ENC_SPLITS + 1))["enc_tps"] == 2
    assert RC.plan(RC.Case(1, 5, 20, 2, 1, 1, RC.HEAD_ROWS * RC.HEAD_GROUPS + 1))["head_trips"] == RC.HEAD_GROUPS + 1


@pytest.mark.parametrize("tag", RC.TAGS)
def test_the_case_reaches_what_its_row_of_the_table_says(tag):
    c, p = RC.CASES[tag], RC.plan(RC.CASES[tag])
    assert RC.REACH[tag](p, c), (tag, p)
    assert c.T % c.L == 0 and 1 <= c.L <= RC.GRU_MAX_STEPS and c.B < p["segments"]
    seg = RC.minibatch(c, RC.SEEDS[tag, True] + 2000)
    assert len(seg) == c.B == len(set(seg.tolist())) and seg.min() >= 0 and seg.max() < p["segments"]
    assert RC.flagged_segment(c) in seg and (c.B == 1 or 0 in seg)
    assert c.B == 1 or not np.array_equal(seg, np.sort(seg))    # shuffled
    _, _, _, _, is_init = U.rollout_case(c.N, c.T, c.A, c.K, c.D, c.L, 0)
    f = is_init.reshape(p["segments"], c.L)
    assert f[0, 0] and f[RC.flagged_segment(c), min(c.L // 2, c.T - 1) % c.L]


def test_the_present_shape_reaches_none_of_it():
    p = RC.plan(RC.PRESENT)
    assert p["seqs"] == 15 < RC.GRU_TILE and p["rows"] == 60 and p["enc_tiles"] == 2 and p["enc_tps"] == p["gru_tps"] == 1
    assert p["head_trips"] == 2 and p["gru_trips"] == 1 and p["ess_strides"] == 1
    assert all(not RC.defect_keep(d, RC.PRESENT) for d in RC.DEFECTS)


# ---------------------------------------------------------------------------------------------------------------- the gathers
@pytest.mark.parametrize("tag", ["one-segment", "one-step", "default"])
def test_the_gathered_states_and_flags_lie_as_the_kernels_index_them(tag):
    """_gathered's h0 [B A, 128] and flags [B A, L] are what the GRU kernels index without strides (h0[s 128 + u], flags[s L + t]): contiguous,
    and the stored values.  At B 1 the reshape of the expanded flags is a view with stride 0 over the agents — the device read the flags of
    agents 1 .. A - 1 behind the segment's L bytes until _gathered made them contiguous (found by `one-segment` on an MI355X: every output off
    by 1e5 to 2e6 x the gate's bound)."""
    from hns_amd import rnn, rnn_train
    c = RC.CASES[tag]
    b = RC.refs(tag, True)
    NS = RC.plan(c)["segments"]
    h0, flags = rnn_train._gathered(torch.as_tensor(b.state), torch.as_tensor(b.is_init), torch.as_tensor(b.seg), NS, c.A, c.L)
    assert h0.is_contiguous() and flags.is_contiguous() and flags.dtype == torch.uint8
    assert h0.shape == (c.B * c.A, 128) and flags.shape == (c.B * c.A, c.L)
    assert np.array_equal(h0.numpy().reshape(c.B, c.A, 128), b.state.reshape(NS, c.A, 128)[b.seg])
    want = np.repeat(b.is_init.reshape(NS, 1, c.L)[b.seg], c.A, axis=1)
    assert np.array_equal(flags.numpy().reshape(c.B, c.A, c.L), want.astype(np.uint8))
    x4 = torch.zeros(c.B, c.A, c.L, 128)
    view = flags[:1].expand(c.B * c.A, c.L) if c.B * c.A > 1 else None
    if view is not None:                                         # the GRU op refuses what it would misread
        with pytest.raises(ValueError, match="contiguous"):
            rnn._seq(x4, h0, view)
        with pytest.raises(ValueError, match="contiguous"):
            rnn._seq(x4, h0[:1].expand(c.B * c.A, 128), flags)
        with pytest.raises(ValueError, match="sequences"):       # ... and one of another extent
            rnn._seq(x4, h0[1:], flags)
        with pytest.raises(ValueError, match="sequences"):
            rnn._seq(x4, h0, flags[1:])
    assert rnn._seq(x4, h0, flags).steps == c.L


# ---------------------------------------------------------------------------------------------------------------- well-posedness
@pytest.mark.parametrize("actor", NETS, ids=net_id)
@pytest.mark.parametrize("tag", RC.TAGS)
def test_the_case_is_well_posed_and_the_cpu_path_stays_within_half_the_bar(tag, actor):
    b = RC.refs(tag, actor)
    bad, fig = RC.preconditions(b)
    print(f"  {tag} {net_id(actor)}: {fig}")
    assert not bad, bad
    if not actor:                                                # the builder's branch of the max
        assert (b.s64["l_orig"] > b.s64["l_clip"]) == (RC.BRANCH[tag] == "orig")
    else:                                                        # rows on both sides of the clip, unless a handful of rows
        assert b.case.B * b.case.L * b.case.A < 64 or 0.05 < fig["inside"] < 0.95
    f = b.is_init.reshape(-1, b.case.L)[b.seg]
    assert (b.case.B == 1 or f[:, 0].any()) and (b.case.L == 1 or f[:, 1:].any()) and np.abs(b.state).min() > 0
    to = lambda v: torch.as_tensor(np.asarray(v)).clone()        # noqa: E731
    out = RC.outputs(b, *RC.call(b, to))
    worst, bad = U.gate(f"{tag}-{net_id(actor)}", RC.items(b, out), bar=RC.SEED_BAR)
    assert not bad, "; ".join(bad)


def test_the_recorded_seeds_are_the_first_that_qualify():
    """The search itself is `python tests/rnn_update_cases.py` (minutes: the large critic cases took 31 and 120 seeds).  Here: the table is
    complete, and for the two cheapest entries whose seed is not 900 the seed before it does fail the rule."""
    assert set(RC.SEEDS) == {(t, a) for t in RC.TAGS for a in NETS} and all(s >= 900 for s in RC.SEEDS.values())
    late = sorted((RC.plan(RC.CASES[k[0]])["rows"], k) for k, s in RC.SEEDS.items() if s > 900)
    assert late
    to = lambda v: torch.as_tensor(np.asarray(v)).clone()        # noqa: E731
    for _, (tag, actor) in late[:2]:
        b = RC.build(RC.CASES[tag], actor, RC.SEEDS[tag, actor] - 1, RC.BRANCH[tag])
        bad, _ = RC.preconditions(b)
        worst = U.gate(tag, RC.items(b, RC.outputs(b, *RC.call(b, to))), verbose=False)[0] if not bad else np.inf
        print(f"  {tag} {net_id(actor)} seed {RC.SEEDS[tag, actor] - 1}: {bad or worst}")
        assert bad or worst > RC.SEED_BAR, (tag, actor)


# ---------------------------------------------------------------------------------------------------------------- teeth
def test_the_table_names_the_cases_at_which_each_defect_loses_something():
    assert set(RC.DEFECT_TABLE) == set(RC.DEFECTS) and len(RC.DEFECTS) == 6
    for d, tags in RC.DEFECT_TABLE.items():
        losing = tuple(t for t in RC.TAGS if RC.defect_keep(d, RC.CASES[t]))
        assert tags == losing, (d, losing)
        for t in tags:                                           # ... and not everything: a mask that keeps nothing is another defect
            for k, v in RC.defect_keep(d, RC.CASES[t]).items():
                assert (0 < v < RC.CASES[t].B) if k == "ess" else (v.any() and not v.all()), (d, t, k)
    one = RC.defect_keep("gru_first_trip_only", RC.CASES["second-trips"])["gru_seq"]
    assert (~one).sum() == 1                                     # one sequence of 4 097
    head = RC.defect_keep("head_first_trip_only", RC.CASES["second-trips"])["head"]
    assert (~head).sum() == 4                                    # four rows of 16 388


@pytest.mark.parametrize("actor", NETS, ids=net_id)
def test_leaving_nothing_out_is_the_fp32_flow_bit_for_bit(actor):
    """The emulation with no defect: U.flow's bits, at the present shape (where every defect of the table is this) and at a case."""
    for tag in ("present", "default"):
        b = RC.refs(tag, actor)
        g, s = RC.defect_flow(b, {})
        assert all(np.array_equal(g[k], b.g32[k]) for k in b.g32)
        assert all(np.array_equal(s[k], b.s32[k]) for k in s)
        _, bad = U.gate(tag, RC.items(b, {**g, **s}), verbose=False)
        assert not bad


# every defect on both networks, but for ESS, which the critic does not have
TEETH_RUNS = [(d, a) for d in RC.DEFECTS for a in NETS if a or d != "ess_first_stride_only"]


@pytest.mark.parametrize("defect,actor", TEETH_RUNS, ids=[f"{d}-{net_id(a)}" for d, a in TEETH_RUNS])
def test_each_defect_fails_the_gate_on_its_named_cases_and_is_invisible_at_the_present_shape(defect, actor):
    assert "ess" in RC.ACTOR_SCALARS and "ess" not in RC.CRITIC_SCALARS
    b = RC.refs("present", actor)
    keep = RC.defect_keep(defect, b.case)
    assert keep == {}
    g, s = RC.defect_flow(b, keep)
    assert not U.gate("present", RC.items(b, {**g, **s}), verbose=False)[1]
    for tag in RC.DEFECT_TABLE[defect]:
        b = RC.refs(tag, actor)
        g, s = RC.defect_flow(b, RC.defect_keep(defect, b.case))
        worst, bad = U.gate(tag, RC.items(b, {**g, **s}), verbose=False)
        print(f"  {defect} {net_id(actor)} {tag}: worst ratio {worst:.3g}; fails on {len(bad)} items")
        TEETH.setdefault((defect, net_id(actor)), []).append((worst, tag))
        assert bad and worst > U.BAR, (defect, tag, worst)


def test_report_teeth():
    for (defect, net), figures in sorted(TEETH.items()):
        print(f"  {defect} {net}: smallest failing ratio {min(figures)[0]:.3g} ({min(figures)[1]}), bar {U.BAR}")
