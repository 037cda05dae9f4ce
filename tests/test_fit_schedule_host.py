"""The schedule of the fp64 factorisation, checked without a GPU: csrc/factor_plan.h decides the outer steps, the panel
launches, the inversions of the wide diagonal blocks and the shape of every step launch from plain integers, and
agp_debug_factor_plan / agp_debug_step_launch_shape (csrc/debug_api.hip) show those decisions with no context and no
device.  Here they are compared with the independent restatement in tests/fit_schedule_cases.py at EVERY n up to 20480
(and every 97th up to 70000) under each switch set, and checked for the structure every schedule must have.
tests/test_fit_schedules_gpu.py proves on the device that a factorisation runs what the plan says."""
import pytest

import fit_schedule_cases as fc
from fit_schedule_cases import MERGED, STEP, THROTTLED, SINGLE, INV_EARLY, INV_LAST_STEP, INV_TAIL, NB

BW = 512  # width of the inverted diagonal blocks of a fit's back substitution (csrc/api.hip: backsolve_width)
# what agp_debug_schedule reports on an MI355X with the default environment
DEFAULT = {"panel_fused": 1, "step_below": 4608, "merge_above": 8704, "fp64_nbo": 0, "masked_stream": 1, "step_slots": 512,
           "cus": 256}
STEP_SLOTS_NEEDED = 10 + DEFAULT["step_below"] // 64 + 64  # for a step tail of step_below rows
# name -> (changes of the record, step_buffers_ready, headcnt_ready)
SWITCH_SETS = {
    "default": ({}, True, True),
    "step_below0": ({"step_below": 0}, True, True),
    "panel_fused0": ({"panel_fused": 0}, True, True),
    "merge_above0": ({"merge_above": 0}, True, True),
    "fp64_nbo1024": ({"fp64_nbo": 1024}, True, True),
    "no_masked_stream": ({"masked_stream": 0}, True, True),
    "step_slots_one_short": ({"step_slots": STEP_SLOTS_NEEDED - 1}, True, True),
    "step_slots_just_enough": ({"step_slots": STEP_SLOTS_NEEDED}, True, True),
    "no_headcnt": ({}, True, False),
    "no_step_buffers": ({}, False, True),
}
SIZES = list(range(1, 20481)) + list(range(20480 + 97, 70001, 97))


def check_structure(n, rec, plan):
    outer, intents = plan["outer"], plan["intents"]
    ends = [e for e, _ in outer]
    assert plan["steps_dropped"] == 0
    assert all(a < b for a, b in zip(ends, ends[1:])) and ends[-1] == n
    assert all(e % NB == 0 or e == n for e in ends)
    assert all(not b & (STEP | SINGLE) for _, b in outer[:-1])
    merged = 0
    for (e, b), begin in zip(outer, [0] + ends):
        if b & MERGED:
            merged += 1
            assert not b & (STEP | THROTTLED | SINGLE) and n - begin > rec["merge_above"] > 0
    assert merged <= 256
    # the wide blocks each inversion names: [first, last) in units of BW
    named = {INV_EARLY: [], INV_LAST_STEP: [], INV_TAIL: []}
    for (end, _), begin, (at_last, first, count, mark_after, bit) in zip(outer, [0] + ends, intents):
        if at_last:
            named[INV_LAST_STEP].append((0, at_last))
            assert end == n and at_last * BW <= begin  # final when the last step begins
        if count:
            assert bit == (INV_EARLY if begin == 0 else INV_TAIL) and end == n
            named[bit].append((first, first + count))
            # the marked panel is one of this step's own, and the blocks lie left of the panel after it
            assert begin <= mark_after < n and mark_after % NB == 0 and (first + count) * BW == mark_after + NB
        else:
            assert mark_after == -1 and bit == 0
    assert all(len(v) <= 1 for v in named.values())
    blocks = sorted(r for v in named.values() for r in v)
    assert all(a[1] <= b[0] for a, b in zip(blocks, blocks[1:]))  # disjoint
    assert all(0 <= a < b <= (n - 1) // BW for a, b in blocks)     # never the last wide block
    assert plan["inv"] == sum(bit for bit, v in named.items() if v)
    assert plan["bs_done"] == (blocks[-1][1] if blocks else 0)


@pytest.mark.parametrize("name", SWITCH_SETS)
def test_plan_equals_restatement_at_every_size(name):
    changes, step_buffers_ready, headcnt_ready = SWITCH_SETS[name]
    rec = dict(DEFAULT, **changes)
    seen = 0
    for n in SIZES:
        plan = fc.factor_plan(n, fc.plan_switches(n, rec, step_buffers_ready, headcnt_ready, bs_bw=BW))
        outer, panels = fc.expected_schedule(n, rec, step_buffers_ready, headcnt_ready)
        assert plan["outer"] == outer, (n, plan, outer)
        assert plan["panels"] == panels, (n, plan, panels)
        check_structure(n, rec, plan)
        for _, b in outer:
            seen |= b
    # the sweep reaches every kind of step the switch set allows
    want = fc.MASKED | THROTTLED
    want |= STEP if rec["step_below"] and rec["panel_fused"] and step_buffers_ready else SINGLE
    want |= MERGED if rec["merge_above"] and rec["panel_fused"] and headcnt_ready else 0
    want &= ~(0 if rec["masked_stream"] else fc.MASKED)
    assert seen & want == want, (seen, want)


def test_step_slot_edge_moves_the_step_tail():
    """one slot short of what step_below rows need: the step tail starts one outer block later"""
    n = 3 * DEFAULT["step_below"]
    short, enough = (fc.factor_plan(n, fc.plan_switches(n, dict(DEFAULT, step_slots=s))) for s in (STEP_SLOTS_NEEDED - 1, STEP_SLOTS_NEEDED))
    assert n - enough["outer"][-2][0] == DEFAULT["step_below"] and enough["outer"][-1][1] & STEP
    assert n - short["outer"][-2][0] < DEFAULT["step_below"] and short["outer"][-1][1] & STEP
    assert 10 + (n - short["outer"][-2][0]) // 64 + 64 <= STEP_SLOTS_NEEDED - 1


@pytest.mark.parametrize("n,want", [(2048, (3, INV_EARLY)), (4608, (8, INV_EARLY)), (5120, (9, INV_LAST_STEP | INV_TAIL)),
                                    (9216, (17, INV_LAST_STEP | INV_TAIL)), (2049, (0, 0)), (12289, (0, 0))])
def test_inversion_intents_of_the_fit_cases(n, want):
    """the (bs_done, inversion bits) of FIT_CASES in tests/test_fit_schedules_gpu.py; a fit requests the inversion where
    its back substitution uses the wide blocks (csrc/api.hip: backsolve_width)"""
    bw = BW if n >= 4 * BW and n % BW == 0 else 0
    plan = fc.factor_plan(n, fc.plan_switches(n, DEFAULT, bs_bw=bw))
    assert (plan["bs_done"], plan["inv"]) == want, plan
    if bw == 0:  # not requested: no intent at any step
        assert all(i == (0, 0, 0, -1, 0) for i in plan["intents"]), plan


BELOWS = sorted({b + d for b in range(0, 4609, 64) for d in (-1, 0, 1) if b + d >= 0})


@pytest.mark.parametrize("step_slots", [146, 256, 512, 1024])
def test_step_launch_shape_equals_restatement(step_slots):
    cus = 256
    trailing = 0
    for below in BELOWS:
        for panels_done in (1, 7):
            got = fc.planned_step_launch_shape(below, panels_done, step_slots, cus)
            assert got == fc.step_launch_shape(below, panels_done, step_slots, cus), (below, panels_done, got)
        if below == 0:
            assert got["grid"] == 10 and got["trail_first"] == fc.NO_WORKGROUP and got["hold_count"] == 0
            continue
        trailing += 1
        nt = -(-below // 64)
        critical, tiles = 10 + nt, nt * (nt + 1) // 2 + 2 * nt
        assert got["trail_first"] == critical and got["trail_tiles"] == tiles and got["rowcnt_expect"] == 2 * panels_done
        assert min(2 * nt, tiles) <= got["trail_workers"] <= tiles
        assert got["hold_count"] in (0, critical, 10)
        assert got["hold_index"] == (cus if got["hold_count"] > 0 else fc.NO_WORKGROUP)
        assert got["grid"] == critical + got["trail_workers"] + got["hold_count"]
    assert trailing == len(BELOWS) - 1
