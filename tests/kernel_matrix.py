"""One configuration per selectable step-kernel instantiation of the library (csrc/hns_inst.hip), with the kernels it must select.

A plain helper module (not a conftest): tests/test_kernel_matrix.py checks on the CPU that the names the matrix expects are exactly the step,
contact, small-mapping and reset kernels built into build/obj, and on the GPU that every entry selects them (hns_selected_kernels) and that
they compute every buffer bit for bit as the oracle does.

Each entry is built from one tuple (pursuers, evaders, shape, input, contact, mapping); the expected names are derived from that tuple by
`expected_kernels`, a restatement of the selection rule in hns_inst.hip, so a change of either side shows up as a mismatch."""
from dataclasses import dataclass, field

FAMILIES = ("hns_step_v4_kernel<", "hns_step_contact_kernel<", "hns_step_small_kernel<", "hns_reset_kernel<")
MAX_K, WIDE_K, EPB = 4, 16, 64            # csrc/hns_common.h: kMaxK, kWideK, kEPB
FIXED_SHAPES = (5, 8, 16)                 # cylinder counts with a fixed-shape tile instantiation (k = 3)
SMALL_FIXED_SHAPES = (5, 8)               # ... in the small-batch mapping and with the contact response

# built kernels that no configuration selects, with the reason: empty — keep it that way or say why here
EXEMPT = {}


def _b(x):
    return "true" if x else "false"


def v4(A, NT, gen, km, prof, cs=0, motor=False):
    return f"hns_step_v4_kernel<{A}, {NT}, {_b(gen)}, {km}, {_b(prof)}, {cs}, {_b(motor)}>"


def contact(A, gen, km, cs, motor):
    return f"hns_step_contact_kernel<{A}, 1, {_b(gen)}, {km}, {cs}, {_b(motor)}>"


def small(A, prof, cs):
    return f"hns_step_small_kernel<{A}, {_b(prof)}, {cs}>"


def reset(A, NT, km):
    return f"hns_reset_kernel<{A}, {NT}, {km}>"


@dataclass(frozen=True)
class Entry:
    A: int                       # pursuers
    NT: int                      # evaders (num_targets)
    C: int                       # cylinder slots (cylinder.max_num)
    K: int                       # obs_max_cylinder
    E: int                       # envs
    min_num: int                 # cylinder.min_num (= C: every slot active)
    motor: bool = False          # task.action_input: motor
    contact: bool = False        # task.contact_response: 1
    mapping: str = "tile"        # HNS_STEP_MAPPING
    offset: int = 0              # env_index_offset (the reset kernel's global Philox key)
    kind: str = ""               # what the entry is there for (its test id)
    expect: dict = field(default_factory=dict, compare=False, hash=False)

    @property
    def id(self):
        return (f"{self.kind}-A{self.A}T{self.NT}C{self.C}K{self.K}E{self.E}" + ("-motor" if self.motor else "") +
                (f"-off{self.offset}" if self.offset else ""))

    def task(self, max_len=7):
        """The task overrides of config.make_cfg for this entry."""
        t = {"num_agents": self.A, "cylinder": {"max_num": self.C, "min_num": self.min_num, "obs_max_cylinder": self.K},
             "env": {"num_envs": self.E, "max_episode_length": max_len}}
        if self.NT == 2:
            t["num_targets"] = 2
        if self.motor:
            t["action_input"] = "motor"
        if self.contact:
            t["contact_response"] = 1
        return t


def expected_kernels(A, NT, C, K, E, motor, contact_on, mapping):
    """(step, stamped twin or None, reset) that hns_create selects for this shape (csrc/hns_inst.hip)."""
    wide, ragged = K > MAX_K, E % EPB != 0
    km = WIDE_K if wide else MAX_K
    cs = C if K == 3 and C in FIXED_SHAPES else 0
    rst = reset(A, NT, km)
    if contact_on:                                                   # no stamped twin, never the small mapping
        if motor:
            return contact(A, True, km, 0, True), None, rst
        if wide or ragged:
            return contact(A, True, km, 0, False), None, rst
        return contact(A, False, MAX_K, cs if cs in SMALL_FIXED_SHAPES else 0, False), None, rst
    if motor:
        return v4(A, NT, True, km, False, 0, True), None, rst
    if wide or ragged:
        return v4(A, NT, True, km, False), None, rst
    if mapping == "small":
        assert NT == 1
        return small(A, False, cs if cs in SMALL_FIXED_SHAPES else 0), small(A, True, 0), rst
    if A == 7 and NT == 2 and cs == 8:
        cs = 0                       # the one fixed shape whose instantiation spilled: its shape-generic twin serves it (hns_inst.hip)
    return v4(A, NT, False, MAX_K, False, cs), v4(A, NT, False, MAX_K, True), rst


def _entry(i, A, NT, C, K, E, kind, *, motor=False, contact_on=False, mapping="tile", min_num=None):
    step, prof, rst = expected_kernels(A, NT, C, K, E, motor, contact_on, mapping)
    offset = 1000 * (i + 1) + 17 if i % 3 == 1 else 0                # every third entry: a nonzero global env index
    return Entry(A, NT, C, K, E, C if min_num is None else min_num, motor, contact_on, mapping, offset, kind,
                 {"step": step, "step_prof": prof, "reset": rst})


def _shapes(A, NT):
    """Tile-mapping shapes for one pursuer / evader count: (C, K, E, kind, min_num, motor)."""
    whole = EPB * (1 + (A + NT) % 2)                                 # 64 or 128 envs
    ragged = EPB + 9 * A + 3 * NT                                    # 76 ... 133: never a whole number of tiles
    # slots where the fixed-shape kernels see inactive cylinders: the two-pursuer entries; every other fixed-shape entry has all slots active
    part = (lambda C: 2) if A == 2 else (lambda C: C)
    cs0 = [(6, 3), (16, 4), (3, 3), (12, 2), (8, 4), (9, 1), (16, 1)][A - 1]     # k = 3 with 5 / 8 / 16 slots would be a fixed shape
    wide_c = 8 if NT == 1 else 12
    wide_k = 5 + A % 4
    out = [(cs0[0], cs0[1], whole, "cs0", min(4, cs0[0]), False)]
    out += [(cs, 3, whole, f"cs{cs}", part(cs), False) for cs in FIXED_SHAPES]
    out += [(8, 3, ragged, "ragged", 4, False),
            (wide_c, wide_k, whole if A % 2 == 0 else ragged, "wide", 3, False),
            (FIXED_SHAPES[A % 3], 3, whole, "motor", FIXED_SHAPES[A % 3], True),
            (6, 3, ragged, "motor-ragged", 4, True),
            (wide_c, wide_k, whole, "motor-wide", 3, True)]
    return out


def _contact_shapes(A):
    """Contact-response shapes for one pursuer count (one evader): (C, K, E, kind, min_num, motor)."""
    whole = EPB * (1 + A % 2)
    full = (lambda C: 2) if A == 2 else (lambda C: C)
    return [(16 if A % 2 else 6, 3, whole, "contact-cs0", 4, False),      # 16 slots: a fixed shape of the plain step, not of the contact one
            (5, 3, whole, "contact-cs5", full(5), False),
            (8, 3, whole, "contact-cs8", full(8), False),
            (8, 3, EPB + 9 * A, "contact-ragged", 4, False),
            (8, 5 + A % 3, whole, "contact-wide", 3, False),
            (5, 3, whole if A % 2 else EPB + 5 * A, "contact-motor", 5, True),
            (12, 6, whole, "contact-motor-wide", 3, True)]


def _small_shapes(A):
    """Small-batch mapping shapes for one pursuer count (one evader, whole tiles, k <= 4): (C, K, E, kind, min_num, motor)."""
    whole = EPB * (1 + A % 2)
    cs0 = [(8, 4), (6, 3), (16, 3), (3, 2), (12, 3), (5, 4), (10, 3)][A - 1]
    return [(cs0[0], cs0[1], whole, "small-cs0", min(4, cs0[0]), False),
            (5, 3, whole, "small-cs5", 2 if A == 3 else 5, False),
            (8, 3, whole, "small-cs8", 2 if A == 3 else 8, False)]


def build_matrix():
    """[Entry]: A = 1 ... 7 x evaders 1 / 2 x every tile shape, the contact response and the small-batch mapping."""
    rows = []
    for A in range(1, 8):
        for NT in (1, 2):
            rows += [(A, NT, s, False, "tile") for s in _shapes(A, NT)]
        rows += [(A, 1, s, True, "tile") for s in _contact_shapes(A)]
        rows += [(A, 1, s, False, "small") for s in _small_shapes(A)]
    return [_entry(i, A, NT, C, K, E, kind, motor=motor, contact_on=con, mapping=mp, min_num=mn)
            for i, (A, NT, (C, K, E, kind, mn, motor), con, mp) in enumerate(rows)]


MATRIX = build_matrix()


def expected_names():
    """Every kernel name the matrix expects some entry to select (step, stamped twin, reset)."""
    return {n for e in MATRIX for n in e.expect.values() if n}


def built_names(kernels):
    """The step, contact, small-mapping and reset kernels among tools/kernel_resources.all_kernels()."""
    return {k["demangled"] for k in kernels if k["demangled"].startswith(FAMILIES)}
