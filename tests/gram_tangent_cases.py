"""Shared by tests/test_gram_tangent_host.py, tests/test_gram_tangent_gpu.py and tests/test_iterative_gradient_gpu.py: the
shapes, the references and the derived bounds for the tangent bilinear forms (csrc/gram_tangent.hip, agp_gram_tangent_forms)
and for the probe gradient of the matrix-free fit (csrc/iterative.hip, agp_iterative_nll_gradient).  Nothing here is measured
on a GPU.

THE FORMS.  forms[c, p] = sum_ij U[i, c] dk_ij(p) V[j, c].

Reference.  contraction_cases.eval_tangent in np.longdouble on the lower triangle (row i >= column j, the argument order the
kernel evaluates), mirrored; then sum_ij U_ic dk_ij V_jc in np.longdouble.

Scale.  sum_ij |U_ic| |dk|*_ij |V_jc| with |dk|* of contraction_cases (absolute values at every sum and at both halves of every
product rule).  It is the sum over the pairs i >= j the kernel visits of mult (|U_ic V_jc| + |V_ic U_jc|) |dk|*_ij with
mult = 1 below the diagonal and 1/2 on it: it cannot cancel.

Bound.  |got - ref| <= (d_sum + c_eval) 2^-53 scale, c_eval as contraction_cases derives it (the same eval_pair_tangent).

  d_sum, the roundings one term U_ic dk_ij V_jc can pass through in gram_tangent_kernel and gram_tangent_sum_kernel:
      3   the symmetric weight w = U_ic V_jc + V_ic U_jc: two products and one addition, relative to |U_ic V_jc| + |V_ic U_jc|
          (the halving of the diagonal pair and the selection above the diagonal are exact)
      1   the product w dk (none when it is fused into the addition, as the kernel spells it)
   walk   the serial column walk of a lane: it adds one column after the other over its whole slice,
          walk = min(tiles per slice, the longest tile list) * TF_COLS additions at most (both row blocks of a unit included)
      6   butterfly steps over the 64 lanes of a wave
      3   additions across the four waves
      ceil(W / 4)   serial additions of a thread of the sum kernel over the W = units * slices workgroup blocks, then
      3   the four strided sums in order
  d_sum(n) = 16 + walk + ceil(W / 4), every quantity read from agp_debug_gram_tangent_plan (plan(); plan_restated() is the
  same arithmetic in Python and the host file asserts that the two agree).

Shapes.  n in N_BASE plus one below, at and one above every row-block, column-tile and slice edge up to N_MAX: every n at
which the plan's row blocks, units, slices or longest tile list change, i.e. every multiple of TF_COLS = 64 (edge_sizes():
read from the probe); ncols in NCOLS around the chunk widths; n_slots in N_SLOTS, the GRAD_GROUP edges
(the first slots of contraction_cases' nine-slot tree); dim in DIMS.  The forms entry takes ONE feature set, so equality ids
exist on both views or on none; the "one view" variant of the contraction tests has no counterpart here.

THE GRADIENT.  See gradient_restated(), dense_gradient_nll() and the tests; the bars: 1e-8 s_p against the dense gradient
with identity probes at a fit tolerance of 1e-12 and cond(A) <= 2e3 (asserted by identity_case), 1e-8 of the sample's own
scale for a sample, 4 standard errors for the estimate.
"""
import ctypes as C
import functools
import math

import numpy as np

import albatross_amd as ab
from albatross_amd import _capi as capi
import contraction_cases as cc
import gram_path_cases as gp
import iterative_fit_cases as ic
import prediction_score_cases as ps

U = cc.U
LD = cc.LD
HAVE_LONGDOUBLE = cc.HAVE_LONGDOUBLE
N_MAX = 777
N_BASE = [1, 2, 63, 64, 65, 128, 129, 200]
NCOLS = [1, 2, 15, 16, 17, 33]
N_SLOTS = [1, 4, 5, 9]
DIMS = [1, 3, 8]


# ---- the plan ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def debug_lib():
    lib = capi.load_debug()
    lib.agp_debug_gram_tangent_plan.restype = C.c_int
    lib.agp_debug_gram_tangent_plan.argtypes = [C.c_int64, C.c_int64, C.c_void_p]
    return lib


@functools.lru_cache(maxsize=None)
def plan(n, ncols=1):
    """agp_debug_gram_tangent_plan (no device): dict of row_blocks, units, slices, tiles_per_slice, max_tiles, rows, cols,
    max_pairs, group, first_chunk"""
    out = np.full(10, -1, dtype=np.int64)
    st = debug_lib().agp_debug_gram_tangent_plan(n, ncols, C.c_void_p(out.ctypes.data))
    assert st == 0, st
    keys = ["row_blocks", "units", "slices", "tiles_per_slice", "max_tiles", "rows", "cols", "max_pairs", "group", "first_chunk"]
    return dict(zip(keys, out.tolist()))


TARGET_WGS, MIN_SLICE_TILES = 1024, 4  # csrc/gram_tangent.h


def col_tiles(b, n, rows, cols):
    return -(-min((b + 1) * rows, n) // cols)


def plan_restated(n, rows=256, cols=64):
    nb = -(-n // rows)
    units = (nb + 1) // 2
    longest = max(col_tiles(q, n, rows, cols) + (col_tiles(nb - 1 - q, n, rows, cols) if nb - 1 - q > q else 0) for q in range(units))
    want = -(-TARGET_WGS // units)
    tps = max(MIN_SLICE_TILES, -(-longest // want))
    return dict(row_blocks=nb, units=units, slices=-(-longest // tps), tiles_per_slice=tps, max_tiles=longest)


@functools.lru_cache(maxsize=1)
def edge_sizes():
    """every n <= N_MAX with another (row blocks, units, slices, longest tile list) than n - 1, with its two neighbours below: n - 1 is
    the last size of the old plan - a full last column tile, row block or slice - and n the first of the new one.  The tile list
    grows at every multiple of the column tile, so every such edge of the kernel up to N_MAX is here."""
    key = lambda n: tuple(plan(n)[k] for k in ("row_blocks", "units", "slices", "max_tiles"))  # noqa: E731
    out = set()
    for n in range(2, N_MAX + 1):
        if key(n) != key(n - 1):
            out.update(m for m in (n - 2, n - 1, n) if 1 <= m <= N_MAX)
    return sorted(out)


def chunks(ncols, max_pairs):
    """the (first column, width of the kernel, columns in use) of the chunks of launch_gram_tangent_forms"""
    out, c0 = [], 0
    while c0 < ncols:
        left = ncols - c0
        T = max_pairs if left >= 5 else (4 if left >= 2 else 1)
        out.append((c0, T, min(left, T)))
        c0 += min(left, T)
    return out


def d_sum(n):
    p = plan(n)
    walk = min(p["tiles_per_slice"], p["max_tiles"]) * p["cols"]
    return 3 + 1 + walk + 6 + 3 + -(-(p["units"] * p["slices"]) // 4) + 3


# ---- cases ------------------------------------------------------------------------------------------------------------------
def _const_poly():
    return ab.Constant(0.7) + ab.Polynomial(2, 0.4)


# name: (contraction_cases tree or a builder of its own, what the issue names it)
TREES = {
    "se+noise": "se_e+noise",
    "m32_r*m32_a": "m32_r*m32_a",          # a product of two radials + noise (integer norms, dim 3)
    "m52_e*m52_e": "m52_e*m52_e",
    "meas(noise)": "m52_e+meas(noise)",
    "scaling": "scaling",
    "const+poly": _const_poly,
    "slots": "nine_slots",
    "dims": "m32_e+noise3",
}


class FormCase:
    pass


@functools.lru_cache(maxsize=None)
def form_case(tree, n, ncols, n_slots=None, dim=3, ids=False, meas=True):
    seed = cc._stable(f"forms/{tree}/{n}/{ncols}/{n_slots}/{dim}/{ids}/{meas}")
    src = TREES[tree]
    if callable(src):
        cov = src()
        x, _ = gp.planted_symmetric(n, 1, seed)
        fs = gp.features(cov, x, meas=meas)
    else:
        cov, fs, x = cc.make_features(src, n, dim, seed, meas, ids)
    c = FormCase()
    c.name = f"{tree}:n{n}:c{ncols}:s{n_slots}:d{fs.dim}" + (":ids" if ids else "") + ("" if meas else ":plain")
    c.cov, c.fs, c.n, c.ncols, c.nodes = cov, fs, n, ncols, cc.plain_nodes(cov)
    slots = cc.slot_table(cov)
    c.slots = slots if n_slots is None else slots[:n_slots]
    assert n_slots is None or len(c.slots) == n_slots, (tree, len(slots))
    c.tang = cc.elevation_tangents(cov, x)
    rng = cc.rng_of("uv", seed)
    c.U, c.V = rng.standard_normal((n, ncols)), rng.standard_normal((n, ncols))
    c.ld, c.ldt = n + 3, n + 2
    c.uflat = _padded_columns(c.U, c.ld)
    c.vflat = _padded_columns(c.V, c.ld)
    c.tflat = cc.padded_tangents(c.tang, c.ldt)
    return c


def _padded_columns(M, ld):
    """n x cols at ld > n with one more column, everything else NaN"""
    n, cols = M.shape
    flat = np.full(ld * (cols + 1), np.nan)
    flat.reshape((ld, cols + 1), order="F")[:n, :cols] = M
    return flat


def form_specs():
    """keyword sets of form_case: every n with a rotating tree and column count; every ncols, every slot count, every dim and
    every tree variant at one small n at least"""
    sizes = sorted(set(N_BASE) | set(edge_sizes()))
    rot = ["se+noise", "m32_r*m32_a", "meas(noise)", "scaling", "const+poly", "m52_e*m52_e"]
    specs = []
    for k, n in enumerate(sizes):
        small = n <= 330
        specs.append(dict(tree=rot[k % len(rot)], n=n, ncols=NCOLS[k % len(NCOLS)] if small else (1, 2, 17)[k % 3], ids=k % 2 == 1))
    specs += [dict(tree="se+noise", n=129, ncols=nc) for nc in NCOLS]
    specs += [dict(tree="slots", n=65, ncols=2, n_slots=s) for s in N_SLOTS]
    specs += [dict(tree="slots", n=257, ncols=17, n_slots=9)]
    specs += [dict(tree="dims", n=65, ncols=5, dim=d) for d in DIMS] + [dict(tree="dims", n=257, ncols=16, dim=8)]
    specs += [dict(tree="m32_r*m32_a", n=200, ncols=3, ids=i) for i in (True, False)]
    specs += [dict(tree="meas(noise)", n=129, ncols=4, meas=m) for m in (True, False)]
    specs += [dict(tree="scaling", n=n, ncols=16) for n in (65, 257)]
    specs += [dict(tree="const+poly", n=n, ncols=4) for n in (64, 200)]
    seen, out = set(), []
    for s in specs:
        key = tuple(sorted(s.items()))
        if key not in seen:
            seen.add(key)
            out.append(s)
    return out


HOST_SPECS = [dict(tree="se+noise", n=129, ncols=17), dict(tree="scaling", n=257, ncols=16), dict(tree="m32_r*m32_a", n=200, ncols=3, ids=True),
              dict(tree="meas(noise)", n=129, ncols=4, meas=False), dict(tree="const+poly", n=200, ncols=4),
              dict(tree="slots", n=257, ncols=17, n_slots=9), dict(tree="dims", n=65, ncols=5, dim=8),
              dict(tree="se+noise", n=513, ncols=2), dict(tree="se+noise", n=1, ncols=1), dict(tree="m52_e*m52_e", n=321, ncols=9)]


def spec_id(s):
    return ":".join(f"{k}={v}" for k, v in sorted(s.items()))


# ---- reference, scale, bound --------------------------------------------------------------------------------------------------
def _lower_mirrored(a):
    return np.tril(a) + np.tril(a, -1).T


def tangents(case, T):
    """(dk, |dk|*, largest exponent argument of a visited pair): per slot n x n arrays, the lower triangle mirrored"""
    dk, dka, _, tt = cc.eval_tangent(case.nodes, case.slots, case.fs, case.fs, case.tang, case.tang, T)
    n = case.n
    return ([_lower_mirrored(np.broadcast_to(a, (n, n))) for a in dk], [_lower_mirrored(np.broadcast_to(a, (n, n))) for a in dka],
            float(np.max(np.tril(np.broadcast_to(tt, (n, n))), initial=0.)))


_REFS = {}


def reference(case):
    """(ref (ncols x n_slots, longdouble), scale (float64), gamma): computed once per case, read-only"""
    if case.name not in _REFS:
        dk, dka, tmax = tangents(case, LD)
        Ul, Vl = case.U.astype(LD), case.V.astype(LD)
        ref = np.stack([np.sum(Ul * (d @ Vl), axis=0) for d in dk], axis=1)
        scale = np.stack([np.sum(np.abs(Ul) * (d @ np.abs(Vl)), axis=0) for d in dka], axis=1).astype(np.float64)
        assert tmax <= cc.T_CAP, (case.name, tmax)
        t_cap = float(max(1, math.ceil(tmax)))
        gamma = (d_sum(case.n) + cc.c_eval(case.nodes, case.fs.dim, t_cap)) * U
        for a in (ref, scale):
            a.setflags(write=False)
        _REFS[case.name] = (ref, scale, gamma)
    return _REFS[case.name]


def ratio(got, case):
    ref, scale, gamma = reference(case)
    got = np.asarray(got)
    if not np.all(np.isfinite(got)):
        return np.inf
    err = np.abs(got.astype(LD) - ref).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0., 0., err / (gamma * scale))
    return float(np.max(r)) if r.size else 0.


# ---- the fp64 restatement in the kernel's order ----------------------------------------------------------------------------------
def kernel_order_forms(case, mut=()):
    """forms (ncols x n_slots) in float64 in the order of gram_tangent_kernel and gram_tangent_sum_kernel.  mut: the planted
    defects of the host file - 'drop_tile' (the last column tile of the first workgroup is skipped), 'one_way' (an
    off-diagonal pair applied as U_i V_j alone), 'diag_twice' (the diagonal pair at full weight), 'next_column' (column c of V
    read as column c + 1)."""
    n, ncols, P = case.n, case.ncols, len(case.slots)
    p = plan(n)
    rows, cols, G = p["rows"], p["cols"], p["group"]
    dk, _, _ = tangents(case, np.float64)
    Uf, Vf = case.U, case.V
    if "next_column" in mut:
        Vf = np.roll(case.V, -1, axis=1)
    out = np.zeros((ncols, P))
    nb = p["row_blocks"]
    lane = np.arange(rows)
    for g0 in range(0, P, G):
        gs = list(range(g0, min(P, g0 + G)))
        for c0, T, cn in chunks(ncols, p["max_pairs"]):
            blocks = []
            for q in range(p["units"]):
                bA, bB = q, nb - 1 - q
                tA = col_tiles(bA, n, rows, cols)
                tB = col_tiles(bB, n, rows, cols) if bB > bA else 0
                for s in range(p["slices"]):
                    t0, t1 = s * p["tiles_per_slice"], min((s + 1) * p["tiles_per_slice"], tA + tB)
                    acc = np.zeros((rows, cn, len(gs)))
                    for t in range(t0, t1):
                        if "drop_tile" in mut and q == 0 and s == 0 and t == t1 - 1:
                            continue
                        blk, ct = (bA, t) if t < tA else (bB, t - tA)
                        r = blk * rows + lane
                        ok = r < n
                        rc = np.minimum(r, n - 1)
                        ui, vi = np.where(ok[:, None], Uf[rc, c0:c0 + cn], 0.), np.where(ok[:, None], Vf[rc, c0:c0 + cn], 0.)
                        for j in range(ct * cols, min((ct + 1) * cols, n)):
                            if j > min(blk * rows + rows - 1, n - 1):
                                break
                            half = 1. if "diag_twice" in mut else 0.5
                            f = np.where(ok & (j < r), 1., np.where(ok & (j == r), half, 0.))
                            d = np.stack([dk[g][rc, j] for g in gs], axis=1) * f[:, None]
                            if "one_way" in mut:
                                w = np.where((j == r)[:, None], ui * Vf[j, c0:c0 + cn] + vi * Uf[j, c0:c0 + cn], ui * Vf[j, c0:c0 + cn])
                            else:
                                w = ui * Vf[j, c0:c0 + cn] + vi * Uf[j, c0:c0 + cn]
                            acc = acc + w[:, :, None] * d[:, None, :]
                    a4 = acc.reshape(4, 64, cn, len(gs))
                    off, ln = 32, np.arange(64)
                    while off > 0:
                        a4 = a4 + a4[:, ln ^ off]
                        off //= 2
                    v = a4[0, 0]
                    for wv in range(1, 4):
                        v = v + a4[wv, 0]
                    blocks.append(v)
            red = [np.zeros((cn, len(gs))) for _ in range(4)]
            for b, v in enumerate(blocks):
                red[b % 4] = red[b % 4] + v
            out[c0:c0 + cn, g0:g0 + len(gs)] = ((red[0] + red[1]) + red[2]) + red[3]
    return out


# ---- the public entry ---------------------------------------------------------------------------------------------------------------
def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


FORMS_EXTRA = 2  # canary rows and one canary column behind the forms


def run_forms(ctx, case, location=capi.HOST, **override):
    """agp_gram_tangent_forms on the case's NaN-padded buffers: (status, forms (ncols x n_slots), the whole canary buffer,
    ldf)"""
    P = len(case.slots)
    ldf = case.ncols + FORMS_EXTRA
    buf = gp.canaries(ldf * (P + 1))
    s = case.fs.as_struct()
    a = dict(n_slots=P, ldt=case.ldt, ldu=case.ld, ldv=case.ld, ncols=case.ncols, ldf=ldf, slots=case.slots)
    a.update(override)
    keep = []
    if location == capi.DEVICE:
        def dev(flat):
            if flat is None:
                return None
            d = ctx.to_device(flat)
            keep.append(d)
            return C.c_void_p(d.ptr)
        tp, up, vp = dev(case.tflat), dev(case.uflat), dev(case.vflat)
    else:
        tp, up, vp = _p(case.tflat), _p(case.uflat), _p(case.vflat)
    st = ctx._lib.agp_gram_tangent_forms(ctx._h, ctx.kernel(case.cov), C.byref(s), a["n_slots"], cc.slot_array(a["slots"]), tp, a["ldt"], up,
                                         a["ldu"], vp, a["ldv"], a["ncols"], _p(buf), a["ldf"], location)
    view = buf.reshape((ldf, P + 1), order="F")
    return st, view[:case.ncols, :P].copy(), buf, ldf


def untouched(buf, ldf, ncols, P):
    """the canaries of run_forms' buffer outside its ncols x P block keep their bits"""
    view = buf.reshape((ldf, -1), order="F")
    return gp.all_canary(np.ascontiguousarray(view[ncols:, :])) and gp.all_canary(np.ascontiguousarray(view[:, P:]))


# ---- the gradient -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gradient_inputs(name):
    """(cov, x, y) of iterative_fit_cases: 'n65_3d', 'n777_2d', or 'n130_3d' - the generator of n65_3d at n = 130"""
    if name == "n130_3d":
        n = 130
        x = ic._uniform(n, 3, 4., 3)
        rng = np.random.default_rng(1000 + n)
        y = np.sin(x).sum(axis=1) + 0.1 * rng.standard_normal(n)
        for a in (x, y):
            a.setflags(write=False)
        return ic._se_noise(), x, y
    cov, x, y, _ = ic.inputs(name)
    return cov, x, y


COND_MAX = 2e3


@functools.lru_cache(maxsize=None)
def dense_system(name):
    """(A, dA {name: n x n}, alpha) in float64 numpy: A = cov(x, x) as measurements from the tangent restatement's value, the
    analytic tangents of contraction_cases summed per parameter name"""
    cov, x, y = gradient_inputs(name)
    fs = gp.features(cov, x, meas=True)
    nodes = cc.plain_nodes(cov)
    slot3 = cov.param_slots()[0]
    slots = [(node, param) for node, param, _ in slot3]
    dk, _, K, _ = cc.eval_tangent(nodes, slots, fs, fs, None, None, np.float64)
    n = fs.n
    A = _lower_mirrored(np.broadcast_to(K, (n, n)))
    dA = {}
    for (_, _, nm), d in zip(slot3, dk):
        dA[nm] = dA.get(nm, 0.) + _lower_mirrored(np.broadcast_to(d, (n, n)))
    alpha = np.linalg.solve(A, y)
    return A, dA, alpha


def identity_case(name):
    """asserts cond(A) <= COND_MAX: with a fit tolerance of 1e-12, tolerance * cond ~ 1e-9 sits a decade under the 1e-8 bar"""
    A, _, _ = dense_system(name)
    cond = float(np.linalg.cond(A))
    assert cond <= COND_MAX, (name, cond)
    return cond


def rademacher(seed, n, t):
    """the documented probes: +1 where agp_standard_normal(seed)[i, c] >= 0, else -1"""
    return np.where(ps.standard_normal(seed, n, 0, t) >= 0., 1., -1.)


def gradient_restated(name, Z):
    """(grad_nll {name}, stderr {name}, samples {name: t}, sample scale {name: t}) in float64 numpy with exact solves"""
    A, dA, alpha = dense_system(name)
    t = Z.shape[1]
    W = np.linalg.solve(A, Z)
    grad, stderr, samples, scales = {}, {}, {}, {}
    for nm, d in dA.items():
        s = np.sum(W * (d @ Z), axis=0)
        tau = s.sum() / t
        grad[nm] = 0.5 * tau - 0.5 * float(alpha @ d @ alpha)
        stderr[nm] = 0.5 * math.sqrt(((s - tau) ** 2).sum() / (t * (t - 1))) if t > 1 else float("nan")
        samples[nm] = s
        scales[nm] = np.sum(np.abs(W) * (np.abs(d) @ np.abs(Z)), axis=0)
    return grad, stderr, samples, scales


def dense_gradient_nll(name):
    """({name: d NLL / d name}, {name: s_p}) exactly in numpy: s_p = 1/2 sum |A^-1_ij dA_ij| + 1/2 |alpha^T dA alpha|, the
    scale of tests/test_nll_gradient_gpu.py"""
    A, dA, alpha = dense_system(name)
    Ainv = np.linalg.inv(A)
    Ainv = 0.5 * (Ainv + Ainv.T)
    grad, scale = {}, {}
    for nm, d in dA.items():
        q = float(alpha @ d @ alpha)
        grad[nm] = 0.5 * np.sum(Ainv * d) - 0.5 * q
        scale[nm] = 0.5 * np.sum(np.abs(Ainv * d)) + 0.5 * abs(q)
    return grad, scale
