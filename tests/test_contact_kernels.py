"""The contact response's kernels are in the library (CPU test: the objects are cross-compiled here): every hns_step_contact_kernel instantiation
the selection in csrc/hns_inst.hip can pick, and the headline one within the register budget of four 4-wave workgroups per CU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def kernels():
    import kernel_resources
    import __graft_entry__
    __graft_entry__.build()
    return {k["demangled"]: k for k in kernel_resources.all_kernels(os.path.join(ROOT, "build", "obj"))}


def selectable():
    for a in range(1, 8):
        for cs in (0, 5, 8):
            yield f"hns_step_contact_kernel<{a}, 1, false, 4, {cs}, false>"       # tuned tile mapping: whole tiles, k <= 4, policy input
        for km in (4, 16):
            for motor in ("false", "true"):
                yield f"hns_step_contact_kernel<{a}, 1, true, {km}, 0, {motor}>"   # generic: ragged, wide k, motor input


def test_every_selectable_contact_kernel_is_built_without_spills(kernels):
    for name in selectable():
        assert name in kernels, f"{name} is not in the library's objects"
        k = kernels[name]
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, name


def test_headline_contact_kernel_register_budget(kernels):
    assert kernels["hns_step_contact_kernel<3, 1, false, 4, 8, false>"]["vgpr_count"] <= 128
