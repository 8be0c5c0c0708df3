"""Every step and reset kernel instantiation the library ships, launched and compared with the oracle (tests/kernel_matrix.py).

CPU: the matrix names exactly the step, contact, small-mapping and reset kernels built into build/obj (code-object metadata, as
tools/kernel_resources.py reads it), so an instantiation added to csrc/hns_inst.hip without a matrix entry fails here.
GPU: for every entry, hns_selected_kernels reports the expected step kernel, stamped twin and reset kernel (the selection rule), and a short run
across episode ends — a NaN and a saturating action, full, masked and partial resets — is bit for bit the oracle's on every buffer (the contact
response: tests/contact_reference.py).  Every stamped twin runs the same loop with a phase-profile buffer attached: the same bits, and stamps
that are non-zero and non-decreasing per wave in the order the kernel writes them.  The tile mapping's priority boost runs on and off at a
shape where it is on by default."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest

import kernel_matrix as KM
from hns_amd import abi, config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PROF_SLOTS = 16            # csrc/hns_common.h: kProfSlots
GUARD_WAVES = 4            # rows behind the documented size that no kernel may write
# Phase stamps per wave role in the order the kernel writes them (csrc/hns_step_body.inc, csrc/hns_step_small_kernel.h): shader-clock slots,
# then the 100 MHz clock slots 14 (first) and 15 (last).
STAMPS = {
    ("tile", "pursuer"): (0, 1, 2, 12, 3, 8, 9, 4, 5, 6, 7),
    ("tile", "env"): (0, 1, 2, 12, 3, 8, 4, 5, 6, 7),
    ("small", "owner"): (0, 1, 2, 12, 3, 8, 9, 4, 5, 6, 7),
    ("small", "env"): (0, 1, 2, 12, 3, 8, 4, 5, 10, 11, 6, 7),
    ("small", "helper"): (0, 2, 3, 8, 10, 9, 4, 5, 6, 7),
}
LAUNCHED = {}              # kernel name -> the entry whose run launched it and matched the oracle (this session)


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def built():
    import kernel_resources
    objdir = os.path.join(ROOT, "build", "obj")
    if not os.path.isdir(objdir) or not any(f.endswith(".o") for f in os.listdir(objdir)):
        import __graft_entry__
        __graft_entry__.build(force=True)
    return KM.built_names(kernel_resources.all_kernels(objdir))


def test_matrix_names_every_built_step_and_reset_kernel(built):
    expected = KM.expected_names()
    missing = sorted(built - expected - set(KM.EXEMPT))
    assert not missing, "built but selected by no entry of tests/kernel_matrix.py: " + "; ".join(missing)
    stale = sorted(expected - built)
    assert not stale, "expected by tests/kernel_matrix.py but not built: " + "; ".join(stale)
    assert not set(KM.EXEMPT) & expected, "exempt kernels that an entry selects after all"
    assert len(built) == 230                                    # 125 tile + 49 contact + 28 small-mapping step kernels, 28 reset kernels


def test_matrix_entries_are_valid_configurations():
    ids = [e.id for e in KM.MATRIX]
    assert len(ids) == len(set(ids))
    for e in KM.MATRIX:
        c = config.resolve_hns_cfg(config.make_cfg(e.task()), env_index_offset=e.offset)
        assert (c.num_agents, c.num_targets, c.num_cylinders, c.obs_max_cylinder, c.num_envs) == (e.A, e.NT, e.C, e.K, e.E)
        assert c.contact_response == e.contact and (c.action_input == abi.HNS_ACTION_MOTOR) == e.motor
        assert 8 <= e.E <= 160, "keep the matrix's batches small"
    for cs in KM.FIXED_SHAPES:                                   # every fixed shape: all slots active somewhere, some inactive somewhere
        fixed = [e for e in KM.MATRIX if e.expect["step"].endswith(f", {cs}, false>")]
        assert any(e.min_num == e.C for e in fixed) and any(e.min_num < e.C for e in fixed), cs
    assert sum(bool(e.offset) for e in KM.MATRIX) >= len(KM.MATRIX) // 4


def test_selected_kernels_refuses_a_null_env():
    lib = abi.load_library()
    buf = C.create_string_buffer(64)
    assert lib.hns_selected_kernels(None, buf, buf, buf, 64, None) == abi.HNS_ERR_INVALID_ARG
    assert b"hns_selected_kernels" in lib.hns_last_error()


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------------

def assert_same(host, dev, what):
    for k in host:
        if host[k] is None or (k == "state_drones" and not host[k].size):
            continue
        np.testing.assert_array_equal(host[k], dev[k], err_msg=f"{what}: buffer {k}")


def make_env(entry, monkeypatch):
    from hns_amd.env import HideAndSeek
    monkeypatch.setenv("HNS_STEP_MAPPING", entry.mapping)
    monkeypatch.delenv("HNS_STEP_PRIO", raising=False)
    env = HideAndSeek(config.make_cfg(entry.task()), headless=True, env_index_offset=entry.offset, write_critic_state=True)
    assert env.hcfg.env_index_offset == entry.offset and not env.use_TP_net
    return env


def run_loop(env, entry, seed, steps=14, full_reset_at=9):
    """Reset, then `steps` steps against the oracle: a NaN action at step 2, saturating ones at step 4, a full reset at `full_reset_at`,
    masked resets of the done envs otherwise (every other one partial: a third of them left done).  Every buffer compared after each call."""
    import torch
    import hns_oracle as O
    c = env.hcfg
    ref_step = O.step
    if entry.contact:
        import contact_reference as CR
        ref_step = CR.composed_step
    O.set_threads(8 if c.num_envs > 4096 else 1)
    env.set_seed(seed)
    env.reset()
    host = O.alloc_buffers(c)
    O.reset(c, host, None, env.seed, 0)
    assert_same(host, env.export_state(), "after reset")
    if entry.contact:                                            # bodies inside and next to each other and the cylinders (contact stages active)
        from test_hip_contact import dense_scene
        env.import_state(dense_scene(env.export_state(), np.random.default_rng(seed)))
        host = env.export_state()
    g = torch.Generator().manual_seed(seed)
    E, A = env.num_envs, env.num_agents
    dev = lambda x: x.to(env.device)                                         # noqa: E731
    for t in range(steps):
        action = (torch.rand(E, A, 4, generator=g) * 2 - 1) if entry.motor else torch.randn(E, A, 4, generator=g) * 0.7
        if t == 2:
            action[0] = float("nan")
        if t == 4:
            action[E - 1], action[E // 2, 0] = 50.0, -50.0
        if entry.motor:                                          # rotor commands + the controller transform's keys (include/hns.h)
            from hns_amd.tensordict_shim import TensorDict
            pa, ae = torch.rand(E, A, 4, generator=g) * 2 - 1, torch.rand(E, A, generator=g)
            env.step(TensorDict({"agents": {"action": dev(action)}, "info": {"prev_action": dev(pa)}, "stats": {"action_error_order1": dev(ae)}},
                                env.batch_size))
            host["prev_action"][:], host["action_error"][:] = pa.numpy(), ae.numpy()
        else:
            env.step(env.rand_step_input(dev(action)))
        ref_step(c, host, action.numpy())
        assert_same(host, env.export_state(), f"step {t}")
        mask = None
        if t == full_reset_at:
            epoch = env.reset_epoch
            env.reset()
            O.reset(c, host, None, env.seed, epoch)
        elif host["done"].any():
            mask = host["done"].copy()
            if t % 2:
                mask[::3] = 0
            td = env.rand_step_input()
            td.set("_reset", torch.as_tensor(mask.astype(bool), device=env.device))
            epoch = env.reset_epoch
            env.reset(td)
            O.reset(c, host, mask, env.seed, epoch)
        if t == full_reset_at or mask is not None:
            assert_same(host, env.export_state(), f"{'full' if mask is None else 'masked'} reset after step {t}")
    assert env.reset_epoch >= 3, "the run must cross episode ends"
    return host


def check_selection(env, entry, stamped=False):
    sel = env.selected_kernels()
    assert (sel["step"], sel["step_prof"], sel["reset"]) == (entry.expect["step"], entry.expect["step_prof"], entry.expect["reset"]), sel
    assert sel["stamped"] == stamped and not sel["prio_boost"]
    assert env.step_mapping == entry.mapping


@pytest.mark.gpu
@pytest.mark.parametrize("entry", KM.MATRIX, ids=lambda e: e.id)
def test_instantiation_selected_and_bit_exact(entry, monkeypatch):
    env = make_env(entry, monkeypatch)
    check_selection(env, entry)
    run_loop(env, entry, seed=zlib.crc32(entry.id.encode()) % 10007)
    for name in (entry.expect["step"], entry.expect["reset"]):
        LAUNCHED.setdefault(name, entry.id)


def stamp_roles(entry):
    """Role of every wave of one workgroup, in wave order (csrc/hns_common.h Geo / csrc/hns_step_small_kernel.h GeoSmall)."""
    if entry.mapping == "small":
        return [("small", "owner")] * entry.A + [("small", "env")] + [("small", "helper")] * entry.A
    return [("tile", "pursuer")] * entry.A + [("tile", "env")]


@pytest.mark.gpu
@pytest.mark.parametrize("entry", [e for e in KM.MATRIX if e.expect["step_prof"]], ids=lambda e: e.id)
def test_stamped_twin_bit_exact(entry, monkeypatch):
    import torch
    env = make_env(entry, monkeypatch)
    roles = stamp_roles(entry)
    waves = (entry.E + KM.EPB - 1) // KM.EPB * len(roles)       # include/hns.h: ceil(E/64) (A + 1), (2 A + 1) in the small mapping
    buf = torch.zeros((waves + GUARD_WAVES) * PROF_SLOTS, dtype=torch.int64, device=env.device)
    assert env._lib.hns_set_phase_profile(env._env, C.c_void_p(buf.data_ptr())) == 0
    try:
        check_selection(env, entry, stamped=True)
        run_loop(env, entry, seed=zlib.crc32(entry.id.encode()) % 10007 + 1)
        stamps = buf.view(-1, PROF_SLOTS).cpu().numpy().view(np.uint64)
    finally:
        assert env._lib.hns_set_phase_profile(env._env, None) == 0
    assert not stamps[waves:].any(), "a stamp landed behind the documented buffer size"
    for w in range(waves):
        role = roles[w % len(roles)]
        order, row = STAMPS[role], stamps[w]
        written = set(np.flatnonzero(row).tolist())
        assert written == set(order) | {14, 15}, f"wave {w} ({role[1]}): slots {sorted(written)} written"
        seq = row[list(order)]
        assert (np.diff(seq.astype(np.int64)) >= 0).all(), f"wave {w} ({role[1]}): stamps {seq.tolist()} decrease in the order {order}"
        assert row[14] <= row[15], f"wave {w}: 100 MHz stamps decrease"
    # detached: the plain kernel serves the next step, and nothing is stamped any more
    check_selection(env, entry, stamped=False)
    buf.zero_()
    env.step(env.rand_step_input())
    torch.cuda.synchronize()
    assert not buf.any()
    LAUNCHED.setdefault(entry.expect["step_prof"], entry.id)


@pytest.mark.gpu
def test_priority_boost_on_and_off_is_bit_exact(monkeypatch):
    """3v1, 8 slots, a grid in (3 CUs, 8 CUs]: the pursuer waves start at a raised priority by default (csrc/hns_inst.hip).  HNS_STEP_PRIO=0
    and =1 must give the same bits as the oracle, and the export must report what serves the env."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    E = KM.EPB * (3 * cus + 1)
    step, prof, rst = KM.expected_kernels(3, 1, 8, 3, E, False, False, "tile")
    entry = KM.Entry(3, 1, 8, 3, E, 8, kind="prio", expect={"step": step, "step_prof": prof, "reset": rst})
    monkeypatch.delenv("HNS_STEP_MAPPING", raising=False)
    monkeypatch.delenv("HNS_STEP_PRIO", raising=False)
    from hns_amd.env import HideAndSeek
    env = HideAndSeek(config.make_cfg(entry.task()), headless=True, write_critic_state=True)
    sel = env.selected_kernels()
    assert sel["prio_boost"] and sel["step"] == step and sel["reset"] == rst and env.step_mapping == "tile"
    del env
    for flag in ("0", "1"):
        monkeypatch.setenv("HNS_STEP_PRIO", flag)
        env = HideAndSeek(config.make_cfg(entry.task()), headless=True, write_critic_state=True)
        assert env.selected_kernels()["prio_boost"] == (flag == "1")
        run_loop(env, entry, seed=5, steps=10, full_reset_at=8)
        del env


@pytest.mark.gpu
def test_all_step_and_reset_instantiations_launched_and_compared(monkeypatch, capsys):
    """Runs last: every expected kernel was launched by a test above (or here, when they were deselected) and matched the oracle."""
    for entry in KM.MATRIX:
        if entry.expect["step"] not in LAUNCHED or entry.expect["reset"] not in LAUNCHED:
            test_instantiation_selected_and_bit_exact(entry, monkeypatch)
        if entry.expect["step_prof"] and entry.expect["step_prof"] not in LAUNCHED:
            test_stamped_twin_bit_exact(entry, monkeypatch)
    expected = KM.expected_names()
    assert set(LAUNCHED) == expected, sorted(expected - set(LAUNCHED))
    fam = {f.rstrip("<"): sum(n.startswith(f) for n in LAUNCHED) for f in KM.FAMILIES}
    with capsys.disabled():
        print(f"\nkernel matrix: {len(LAUNCHED)} step and reset instantiations launched and compared bit for bit with the oracle "
              f"({', '.join(f'{v} {k}' for k, v in fam.items())}; {len(KM.MATRIX)} entries)")
