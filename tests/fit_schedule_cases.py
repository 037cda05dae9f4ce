"""The schedule of the fp64 factorisation restated in Python, independently of csrc/factor_plan.h: what the outer steps,
the panel launches and the shape of a step launch must be for given n and switches.  Shared by
tests/test_fit_schedules_gpu.py (the record of a real factorisation equals the restatement at every regime edge) and
tests/test_fit_schedule_host.py (the plan of agp_debug_factor_plan equals it at every n, without a device).

The restatements follow what the launch code has to do (csrc/chol.hip: factor_lower, panel_phase), in Python's own
terms and NOT transcribed from the plan header; they are the reference, so a change of the schedule changes BOTH sides
on purpose.
"""
import ctypes as C

import numpy as np

from albatross_amd import _capi as capi

NB = 128
# ---- the schedule record (csrc/debug_api.hip: agp_debug_schedule, which documents the layout) -----------------------
SCHED_HEADER, SCHED_STEPS = 20, 256
MERGED, STEP, THROTTLED, MASKED, SINGLE = 1, 2, 4, 8, 16
INV_EARLY, INV_LAST_STEP, INV_TAIL = 1, 2, 4
NO_WORKGROUP = 0xffffffff  # trail_first / hold_index of a launch without trailing / placeholder workgroups


def step_fits(rec, rows):
    """chol.hip: step_fits (with step_ready: the step launches need the fused panel kernel's buffers)."""
    return (rec["panel_fused"] == 1 and rec["step_below"] > 0 and rows <= rec["step_below"]
            and rec["step_slots"] >= 10 + rows // 64 + 64)


def expected_schedule(n, rec, step_buffers_ready=True, headcnt_ready=True):
    """factor_lower's outer steps and panel launches for an n x n fp64 factorisation under the switches in force (read
    from the record), restated from chol.hip: (outer [(end, bits)], panel counts {step, fused, split}).
    step_buffers_ready / headcnt_ready: what the record does not show - False if the second tile image and the row
    counters of the step launches, or the counters of the merged launches, could not be set up (then none of those run);
    by default both are there whenever the fused panel kernel is on, as on a device with memory to spare."""
    wide = rec["fp64_nbo"]

    def pick_nbo(r):
        if wide > 512 and r > 8192:
            return wide
        return 512 if r > 2048 else 256 if r > 1024 else NB

    def fits(rows):
        return step_buffers_ready and step_fits(rec, rows)

    fused_on = rec["panel_fused"] == 1
    headcnt = headcnt_ready and fused_on and rec["merge_above"] > 0 and n > rec["merge_above"]
    blocks = []  # (K0, kend, step mode)
    kend = min(pick_nbo(n), n)
    step_all = fits(n)
    if step_all:
        kend = n
    outer = [(kend, STEP if step_all else 0)]
    blocks.append((0, kend, step_all))
    idx = 0
    while kend < n:
        r = n - kend
        ne = min(kend + pick_nbo(r), n)
        step = fits(r)
        single = not step and r <= 1536
        if step or single:
            ne = n
        masked = rec["masked_stream"] == 1 and r <= 8704
        merged = (not step and ne < n and headcnt and r > rec["merge_above"] and idx < SCHED_STEPS
                  and (ne - kend) % NB == 0)
        idx += 1
        if merged:
            outer.append((ne, MERGED | (MASKED if masked else 0)))
        else:
            throttle = ne < n and r <= 8192
            outer.append((ne, (STEP if step else 0) | (THROTTLED if throttle else 0) | (SINGLE if single else 0)
                          | (MASKED if ne < n and masked else 0)))
        blocks.append((kend, ne, step))
        kend = ne
    panels = {"step": 0, "fused": 0, "split": 0}
    for k0, k1, step_mode in blocks:
        count = -(-(k1 - k0) // NB)
        step_mode = step_mode and k1 == n
        if fused_on and ((n - k0) <= 4608 or step_mode):
            panels["fused"] += 1 if step_mode else count
            panels["step"] += count - 1 if step_mode else 0
        else:
            panels["split"] += count
    return outer, panels


def step_launch_shape(below, panels_done, step_slots, cus):
    """The grid of one step launch (panel_fused_kernel<true>) with `below` rows under its panel, restated from panel_phase:
    the factoring workgroup, the nine that update its diagonal block and one per 64 rows below are CRITICAL and come
    first; then the trailing workgroups, which share the 64 x 64 tiles of the trailing triangle plus two row tiles per
    64 rows; then placeholders that keep trailing workgroups off the CUs of the critical ones (workgroup cus + i lands
    next to workgroup i)."""
    row_blocks = -(-below // 64)
    critical = 10 + row_blocks
    shape = {"grid": critical, "trail_first": NO_WORKGROUP, "trail_tiles": 0, "trail_workers": 1,
             "hold_index": NO_WORKGROUP, "hold_count": 0, "rowcnt_expect": 0}
    if below <= 0:
        return shape
    tiles = row_blocks * (row_blocks + 1) // 2 + 2 * row_blocks
    held = 0
    if critical < cus < critical + tiles:  # the launch wraps round the chip: placeholders next to the critical workgroups
        held = critical if tiles <= 1200 else 10
        workers = min(tiles, step_slots - critical - held)
        if critical + workers <= cus:
            held = 0
    else:
        workers = min(tiles, step_slots - critical)
    workers = max(workers, min(2 * row_blocks, tiles))  # every row tile has a workgroup of its own up front
    shape.update(trail_first=critical, trail_tiles=tiles, trail_workers=workers, rowcnt_expect=2 * panels_done,
                 grid=critical + workers + held)
    if held:
        shape.update(hold_index=cus, hold_count=held)
    return shape


# ---- the plan of the library, without a device (csrc/debug_api.hip: agp_debug_factor_plan) --------------------------
PLAN_WORDS = SCHED_HEADER + 7 * SCHED_STEPS
SHAPE_FIELDS = ("grid", "trail_first", "trail_tiles", "trail_workers", "hold_index", "hold_count", "rowcnt_expect")


def plan_switches(n, rec, step_buffers_ready=True, headcnt_ready=True, bs_bw=0):
    """The FactorSwitches an fp64 factor_lower of n rows would see on a context with the switches of `rec`: the buffers of
    the fused kernel are there when it is on, the merged launches' counters are zeroed when any merged launch is possible
    (chol.hip: panel_fused_plan); bs_bw > 0 requests the inversion of the wide diagonal blocks."""
    fused = rec["panel_fused"] == 1
    return [int(fused), rec["step_below"], rec["merge_above"], 0, rec["fp64_nbo"], -1, rec["step_slots"], rec["cus"],
            rec["masked_stream"], int(headcnt_ready and fused and rec["merge_above"] > 0 and n > rec["merge_above"]),
            int(fused and step_buffers_ready), int(fused), int(bs_bw > 0), bs_bw, 0]


def factor_plan(n, switches):
    """agp_debug_factor_plan: {'outer': [(end, bits)], 'panels': {...}, 'bs_done', 'inv', 'steps_dropped',
    'intents': per step (inv_last_step, inv_first, inv_count, mark_after, inv_bit)}."""
    fn = capi.load_debug().agp_debug_factor_plan
    sw = np.array(switches, np.int64)
    w = np.zeros(PLAN_WORDS, np.int64)
    assert fn(C.c_void_p(sw.ctypes.data), n, C.c_void_p(w.ctypes.data), w.size) == 0
    assert w[0] == n
    steps = int(w[1])
    table = w[SCHED_HEADER:SCHED_HEADER + 2 * steps].reshape(steps, 2).tolist()
    first = SCHED_HEADER + 2 * SCHED_STEPS
    return {"outer": [tuple(r) for r in table], "steps_dropped": int(w[2]),
            "panels": {"step": int(w[3]), "fused": int(w[4]), "split": int(w[5])}, "bs_done": int(w[7]), "inv": int(w[8]),
            "intents": [tuple(r) for r in w[first:first + 5 * steps].reshape(steps, 5).tolist()]}


def planned_step_launch_shape(below, panels_done, step_slots, cus):
    """agp_debug_step_launch_shape: factor_plan.h's step_launch_shape as a dict like step_launch_shape above."""
    w = np.zeros(len(SHAPE_FIELDS), np.int64)
    assert capi.load_debug().agp_debug_step_launch_shape(below, panels_done, step_slots, cus, C.c_void_p(w.ctypes.data)) == 0
    return dict(zip(SHAPE_FIELDS, w.tolist()))
