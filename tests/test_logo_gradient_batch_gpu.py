"""GPU tests of agp_logo_nll_gradient_batch: the leave-one-group-out likelihood (Joint and Marginal) and its exact gradient
for many problems of any mix of sizes in lock step, the group blocks of ALL problems pooled into one chain per size class;
at the C-ABI and through ab.leave_one_group_out_likelihood_gradient_batch, the pooled helper and the parameter-set methods.

References and bounds are the project's own (test_logo_gradient_gpu.py, test_logo_marginal_gpu.py,
test_ragged_gradient_batch_gpu.py): the numpy closed forms on each problem's own n_b points, the value to 1e-10 relative,
|g - g_ref| <= 1e-7 s_p with those files' s_p; against agp_logo_nll_gradient_typed called alone 1e-10 and 1e-9 s_p; the
value-only call against the full one 1e-12 relative.  Every tree has a noise sigma, so one phantom diagonal pair leaking
into the contraction would show far outside 1e-7 s_p.

At the C-ABI every input column carries NaN behind its n_b values and every output a sentinel behind what may be written."""
import ctypes as C

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
from albatross_amd import gp as abgp
from conftest import synthetic_3d
from test_logo_gradient_gpu import _dataset, _variance, ragged_groups
from test_logo_gradient_gpu import reference as joint_reference
from test_logo_gradient_host import indefinite_problem
from test_logo_marginal_gpu import reference as marginal_reference
from test_loo_gradient_gpu import reference as loo_reference
from test_nll_gradient_batch_gpu import _config3, _copy, _p, _sets
from test_nll_gradient_gpu import LEAVES, _data, _elevation_model
from test_ragged_gradient_batch_gpu import Ragged

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
TYPES = ["joint", "marginal"]
PTYPE = {"joint": capi.PREDICT_JOINT, "marginal": capi.PREDICT_MARGINAL}


def random_groups(n, seed, sizes=(1, 1, 2, 3, 4, 7, 16, 17, 33, 64), cover=0.9):
    """ragged groups of the given sizes from a random permutation until `cover` of the n points are used"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    groups, at = [], 0
    while at < cover * n:
        m = int(min(n - at, rng.choice(sizes)))
        groups.append(perm[at:at + m].tolist())
        at += m
    return groups


class Batch:
    """the arguments of one call, built from (model, x, y, s, groups) problems of any sizes (groups: a list of index lists),
    with every array kept alive; ld: the leading dimension of y, y_var, the tangents and the mean weights"""

    def __init__(self, ctx, problems, ld=None):
        self.ctx = ctx
        self.problems = problems
        self.models = [p[0] for p in problems]
        self.probs = [abgp._gradient_problem(m, _dataset(x, y, s)) for m, x, y, s, _ in problems]
        self.count = len(problems)
        self.sizes = [p.fs.n for p in self.probs]
        self.n = max(self.sizes)
        self.ld = self.n if ld is None else ld
        self.structs = [p.fs.as_struct() for p in self.probs]
        self.Y = np.full((self.count, self.ld), np.nan)  # row b: column b of the column-major argument
        self.V = np.full((self.count, self.ld), np.nan) if any(p.yv is not None for p in self.probs) else None
        self.T = []
        for b, p in enumerate(self.probs):
            nb = p.fs.n
            self.Y[b, :nb] = p.y
            if self.V is not None:
                self.V[b, :nb] = 0. if p.yv is None else p.yv
            if p.tangents is None:
                self.T.append(None)
            else:
                t = np.full((p.tangents.shape[1], self.ld), np.nan)
                t[:, :nb] = p.tangents.T
                self.T.append(t)
        self.ldg = max(1, max(len(p.slots) for p in self.probs))
        self.n_slots = (C.c_int * self.count)(*[len(p.slots) for p in self.probs])
        self.tables = (C.c_void_p * self.count)(*[C.addressof(p.table) for p in self.probs])
        self.tang = (C.c_void_p * self.count)(*[None if t is None else t.ctypes.data for t in self.T])
        self.set_groups([p[4] for p in problems])

    def set_groups(self, groups):
        self.groups = groups
        self.offs = [np.concatenate([[0], np.cumsum([len(g) for g in gs])]).astype(np.int64) for gs in groups]
        self.inds = [np.asarray([i for g in gs for i in g], dtype=np.int64) for gs in groups]
        self.n_groups = (C.c_int64 * self.count)(*[len(gs) for gs in groups])
        self.offsets = (C.c_void_p * self.count)(*[o.ctypes.data for o in self.offs])
        self.indices = (C.c_void_p * self.count)(*[i.ctypes.data if len(i) else None for i in self.inds])

    def call(self, ptype="joint", weights=True, value_only=False, terms=None, **over):
        """(rc, value, grad, vec, status, group terms) of the entry, every output sentinel-filled before the call.
        value_only: no slots, no mean weights; terms: None (no table), or the problems that get a group_nll array"""
        ctx = self.ctx
        value = np.full(self.count, SENTINEL)
        grad = np.full((self.count, self.ldg), SENTINEL)
        vec = np.full((self.count, self.ld), SENTINEL)
        status = (C.c_int * self.count)(*([-5] * self.count))
        gn = [np.full(max(1, len(gs)) + 1, SENTINEL) for gs in self.groups]
        table = None
        if terms is not None:
            table = (C.c_void_p * self.count)(*[gn[b].ctypes.data if b in terms else None for b in range(self.count)])
        n_slots = (C.c_int * self.count)() if value_only else self.n_slots
        handles = [ctx.private_kernel(m.covariance_function_) for m in self.models]
        try:
            kernels = (C.c_void_p * self.count)(*handles)
            fptrs = (C.c_void_p * self.count)(*[C.addressof(s) for s in self.structs])
            rc = ctx._lib.agp_logo_nll_gradient_batch(
                ctx._h, over.get("count", self.count), kernels, fptrs, over.get("y", _p(self.Y)), over.get("ldy", self.ld),
                over.get("y_var", None if self.V is None else _p(self.V)), over.get("ldv", self.ld), self.n_groups, self.offsets,
                self.indices, over.get("predict_type", PTYPE[ptype]), n_slots, self.tables, over.get("tangents", self.tang),
                over.get("ldt", self.ld), _p(value), _p(grad), over.get("ldg", self.ldg),
                _p(vec) if weights and not value_only else None, over.get("ldw", self.ld), table, status)
        finally:
            for h in handles:
                ctx._lib.agp_kernel_destroy(h)
        return rc, value, grad, vec, list(status), gn

    def result(self, b, out):
        m, p = self.models[b], self.probs[b]
        return out[1][b], m._leave_one_out_gradient_dict(p.slots, out[2][b, :len(p.slots)], out[3][b, :p.fs.n], p.fs)

    def check_sentinels(self, out, failed=()):
        _, value, grad, vec, _, gn = out
        for b in range(self.count):
            assert (grad[b, self.n_slots[b]:] == SENTINEL).all(), b
            assert (vec[b, self.sizes[b]:] == SENTINEL).all(), b
            assert gn[b][-1] == SENTINEL
            if b in failed:
                assert (vec[b] == SENTINEL).all(), b
            else:
                assert not (vec[b, :self.sizes[b]] == SENTINEL).any(), b

    def reference(self, b, ptype):
        m, x, y, s, groups = self.problems[b]
        ref = joint_reference if ptype == "joint" else marginal_reference
        return ref(m, x, y, s, groups)[:3]  # gradient, s_p, value

    def check_problem(self, b, out, ptype, single=True):
        """problem b against numpy on its own n_b points and (single) against agp_logo_nll_gradient_typed alone"""
        m, x, y, s, groups = self.problems[b]
        value, grad = self.result(b, out)
        assert set(grad) == set(m.get_params())
        want, scale, ref_value = self.reference(b, ptype)
        rel = abs(value - ref_value) / abs(ref_value) if ref_value else abs(value)
        print(f"{ptype} b={b} n_b={len(y)} groups={len(groups)} value rel err {rel:.2e} gradient err / s_p "
              f"{max([abs(grad[k] - want[k]) / scale[k] for k in want if scale[k] > 0.] or [0.]):.2e}")
        assert abs(value - ref_value) <= 1e-10 * abs(ref_value), (b, value, ref_value)
        for name in want:
            assert abs(grad[name] - want[name]) <= 1e-7 * scale[name], (b, name, grad[name], want[name], scale[name])
        if single:
            v1, g1 = m.leave_one_group_out_likelihood_gradient(_dataset(x, y, s), dict(enumerate(groups)), predict_type=ptype)
            assert abs(value - v1) <= 1e-10 * abs(v1), (b, value, v1)
            for name in g1:
                assert abs(grad[name] - g1[name]) <= 1e-9 * scale[name], (b, name, grad[name], g1[name], scale[name])
        return scale

    def check_value_only(self, out, ptype):
        only = self.call(ptype, value_only=True)
        assert only[0] == capi.AGP_OK and only[4] == out[4]
        assert (only[2] == SENTINEL).all() and (only[3] == SENTINEL).all()
        for b in range(self.count):
            if out[4][b] == capi.AGP_OK:
                assert abs(only[1][b] - out[1][b]) <= 1e-12 * abs(out[1][b]), (b, only[1][b], out[1][b])


def _ok(raw, out):
    assert out[0] == capi.AGP_OK and out[4] == [0] * raw.count, (out[0], out[4])


def _config3_problems(ctx, sizes, seed, with_variance="alternate", groups=None):
    """one copy of the SE + noise model with parameters of its own per size; groups: per problem, or random ragged ones"""
    model = _config3(ctx)
    out = []
    for b, (n, o) in enumerate(zip(sizes, _sets(model, len(sizes), seed))):
        x, y = synthetic_3d(n, seed + 13 * b + n)
        s = _variance(n, seed + b) if (with_variance is True or (with_variance == "alternate" and b % 2)) else None
        out.append((_copy(model, o), x, y, s, groups[b] if groups else random_groups(n, seed + 7 * b)))
    return out


# ---- factor paths by padded size ------------------------------------------------------------------------------------------
FACTOR_PATHS = {128: [100, 128], 256: [129, 256], 512: [400, 512], 640: [600, 640]}


@pytest.mark.parametrize("with_variance", [False, True])
@pytest.mark.parametrize("ptype", TYPES)
@pytest.mark.parametrize("padded", list(FACTOR_PATHS))
def test_factor_paths_by_padded_size(ctx, padded, ptype, with_variance):
    """128 one block; 256 beside 129 rows: the second panel almost all phantom; 512 the fused panels; 640 past the outer block"""
    raw = Batch(ctx, _config3_problems(ctx, FACTOR_PATHS[padded], 300 + padded, with_variance))
    out = raw.call(ptype)
    _ok(raw, out)
    raw.check_sentinels(out)
    for b in range(raw.count):
        raw.check_problem(b, out, ptype)
    raw.check_value_only(out, ptype)


# ---- group shapes, pooled across problems ----------------------------------------------------------------------------------
def _shapes_problems(ctx):
    sizes = [300, 256, 256, 200, 300, 150, 210]
    perm = np.random.default_rng(19).permutation(300)
    groups = [
        ragged_groups(300, 41, [64, 40, 33, 17, 16, 9, 8, 7, 5, 4, 3, 2, 1] + [1] * 91),  # several size classes
        [list(range(4 * g, 4 * g + 4)) for g in range(64)],                                    # equal groups of 4
        [np.random.default_rng(5).permutation(256)[:130].tolist()],                            # past one 128 block
        [],                                                                                    # no groups
        [perm[:40].tolist(), [], perm[40:45].tolist(), perm[45:46].tolist(), perm[46:180].tolist()],  # partial cover
        [np.random.default_rng(3).permutation(150).tolist()],                                  # one group: everything
        random_groups(210, 77),
    ]
    groups[0] = list(groups[0].values())
    problems = _config3_problems(ctx, sizes, 51, groups=groups)
    m, x, y, _, g = problems[5]
    problems[5] = (m, x, y, None, g)  # without a target variance: the group of everything is the log-likelihood
    return problems


@pytest.mark.parametrize("ptype", TYPES)
def test_group_shapes_pooled_in_one_call(ctx, ptype):
    raw = Batch(ctx, _shapes_problems(ctx))
    out = raw.call(ptype)
    _ok(raw, out)
    raw.check_sentinels(out)
    for b in range(raw.count):
        if b == 3:
            assert out[1][3] == 0. and (out[2][3, :raw.n_slots[3]] == 0.).all() and (out[3][3, :200] == 0.).all()
            continue
        raw.check_problem(b, out, ptype)
    if ptype == "joint":
        m, x, y, _, _ = raw.problems[5]
        want = -m.log_likelihood(_dataset(x, y, None))
        assert abs(out[1][5] - want) <= 1e-10 * abs(want), (out[1][5], want)
    raw.check_value_only(out, ptype)


@pytest.mark.parametrize("ptype", TYPES)
def test_singletons_equal_the_leave_one_out_batch(ctx, ptype):
    sizes = [100, 130, 77]
    problems = _config3_problems(ctx, sizes, 9, groups=[[[i] for i in range(n)] for n in sizes])
    raw = Batch(ctx, problems)
    out = raw.call(ptype)
    _ok(raw, out)
    loo = Ragged(ctx, [p[:4] for p in problems])
    ref = loo.call("loo")
    assert ref[0] == capi.AGP_OK
    for b, (m, x, y, s, _) in enumerate(problems):
        _, scale, _, _ = loo_reference(m, x, y, s)
        value, grad = raw.result(b, out)
        v1, g1 = loo.result("loo", b, ref)
        assert abs(value - v1) <= 1e-10 * abs(v1), (b, value, v1)
        for name in g1:
            assert abs(grad[name] - g1[name]) <= 1e-7 * scale[name], (b, name, grad[name], g1[name])


@pytest.mark.parametrize("ptype", TYPES)
def test_indefinite_blocks_as_one_member(ctx, ptype):
    problems = _config3_problems(ctx, [200, 300, 260], 23)
    x, y, s = indefinite_problem(300)
    model = ab.gp_from_covariance(ab.SquaredExponential(1.3, 0.9) + ab.IndependentNoise(0.2), context=ctx)
    problems[1] = (model, x, y, s, list(ragged_groups().values()))
    raw = Batch(ctx, problems)
    out = raw.call(ptype)
    _ok(raw, out)
    blocks = (joint_reference if ptype == "joint" else marginal_reference)(model, x, y, s, problems[1][4])[4]
    assert min(np.linalg.eigvalsh(b).min() for b in blocks) < -0.1
    for b in range(raw.count):
        raw.check_problem(b, out, ptype)


def test_two_chunks_from_one_size_class_across_problems(ctx):
    """8 problems x 512 singletons: 4096 groups of one size against the 3640 groups one chunk's images hold"""
    sizes = [512] * 8
    problems = _config3_problems(ctx, sizes, 88, groups=[[[i] for i in range(512)]] * 8)
    raw = Batch(ctx, problems)
    out = raw.call("joint")
    _ok(raw, out)
    loo = Ragged(ctx, [p[:4] for p in problems])
    ref = loo.call("loo")
    for b in range(8):
        assert abs(out[1][b] - ref[1][b]) <= 1e-10 * abs(ref[1][b]), (b, out[1][b], ref[1][b])
    for b in (0, 7):  # the first chunk's first problem and the problem of the second chunk
        raw.check_problem(b, out, "joint", single=False)


# ---- the terms per group --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ptype", TYPES)
def test_group_nll_in_the_callers_order(ctx, ptype):
    sizes = [300, 140, 257]
    perm = np.random.default_rng(5).permutation(300)
    cut = [7, 130, 0, 1, 33, 2, 0, 65, 3, 17, 1, 16]
    edges = np.concatenate([[0], np.cumsum(cut)])
    groups = [[perm[edges[g]:edges[g + 1]].tolist() for g in range(len(cut))], random_groups(140, 1) + [[]], random_groups(257, 2)]
    raw = Batch(ctx, _config3_problems(ctx, sizes, 6, groups=groups))
    for value_only in (False, True):
        out = raw.call(ptype, value_only=value_only, terms=(0, 1, 2))
        _ok(raw, out)
        if not value_only:
            raw.check_sentinels(out)
        for b, (m, x, y, s, gs) in enumerate(raw.problems):
            got = out[5][b][:len(gs)]
            scores = ab.LeaveOneGroupOutLikelihood(dict(enumerate(gs)), ptype).group_scores(_dataset(x, y, s), m)
            for g, t in scores.items():
                assert abs(got[g] - t) <= 1e-10 * max(1., abs(t)), (b, g, got[g], t)
                assert (got[g] == 0.) == (len(gs[g]) == 0)
            assert abs(got.sum() - out[1][b]) <= 1e-12 * abs(out[1][b]), (b, got.sum(), out[1][b])
    some = raw.call(ptype, terms=(1,))  # some per-problem pointers NULL
    _ok(raw, some)
    assert (some[5][0] == SENTINEL).all() and (some[5][2] == SENTINEL).all()
    assert some[5][1][:len(groups[1])].tobytes() == raw.call(ptype, terms=(0, 1, 2))[5][1][:len(groups[1])].tobytes()


# ---- every leaf -----------------------------------------------------------------------------------------------------------
def _fours():
    return [list(range(4 * g, 4 * g + 4)) for g in range(64)]


@pytest.mark.parametrize("label,make,dim", LEAVES)
def test_every_leaf_in_a_batch_of_three(ctx, label, make, dim):
    problems = []
    for b in range(3):
        x, y = _data(256, dim, 267 + b)
        problems.append((ab.gp_from_covariance(make(), context=ctx), x, y, _variance(256, 5 + b), _fours()))
    raw = Batch(ctx, problems)
    for ptype in TYPES:
        out = raw.call(ptype)
        _ok(raw, out)
        for b in range(3):
            raw.check_problem(b, out, ptype, single=b == 0)


def test_scaling_term_and_linear_mean_in_a_batch_of_three(ctx):
    _, model = _elevation_model(ctx)
    model.set_param_values({"slope": 0.2, "offset": -0.4})
    problems = []
    for b, o in enumerate(_sets(model, 3, 31, spread=0.2)):
        x, y = _data(256, 3, 259 + b)
        problems.append((_copy(model, o), x, y + 0.3 * x[:, 0], _variance(256, 6 + b), _fours()))
    raw = Batch(ctx, problems, ld=300)  # leading dimensions above the padded size
    for ptype in TYPES:
        out = raw.call(ptype)
        _ok(raw, out)
        raw.check_sentinels(out)
        for b in range(3):
            assert {"elevation_scaling_center", "elevation_scaling_factor", "slope", "offset"} <= set(raw.result(b, out)[1])
            raw.check_problem(b, out, ptype)


# ---- failures ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ptype", TYPES)
def test_failed_problems_are_reported_and_isolated(ctx, ptype):
    sizes = [300, 210, 260, 140, 290, 257]
    problems = _config3_problems(ctx, sizes, 4)
    _, xs, ys, _, gs = problems[1]
    xs = xs.copy()
    xs[5] = xs[0]  # no noise, no variance and a duplicated point: singular
    problems[1] = (ab.gp_from_covariance(ab.SquaredExponential(1., 1.), context=ctx), xs, ys, None, gs)
    m4, xn, yn, s4, g4 = problems[4]
    yn = yn.copy()
    yn[17] = np.nan  # a NaN target
    problems[4] = (m4, xn, yn, s4, g4)
    raw = Batch(ctx, problems)
    out = raw.call(ptype, terms=(0, 1, 4))
    rc, value, grad, vec, status, gn = out
    assert rc == capi.AGP_OK
    assert status[1] == capi.AGP_ERR_NOT_POSITIVE_DEFINITE and status[4] == capi.AGP_ERR_NAN_INPUT, status
    raw.check_sentinels(out, failed=(1, 4))
    for b in (1, 4):
        assert np.isnan(value[b]) and np.isnan(grad[b, :raw.n_slots[b]]).all()
        assert np.isnan(gn[b][:len(raw.groups[b])]).all()
    for b in (0, 2, 3, 5):
        assert status[b] == capi.AGP_OK
        raw.check_problem(b, out, ptype)
    raw.check_value_only(out, ptype)


def test_malformed_calls_write_nothing(ctx):
    sizes = [100, 70, 90, 60, 80]
    raw = Batch(ctx, _config3_problems(ctx, sizes, 2))
    _ok(raw, raw.call())
    good = raw.groups

    def rejected(**over):
        rc, value, grad, vec, status, gn = raw.call(terms=tuple(range(5)), **over)
        assert rc == capi.AGP_ERR_INVALID_ARGUMENT, over
        assert (value == SENTINEL).all() and (grad == SENTINEL).all() and (vec == SENTINEL).all() and status == [-5] * 5, over
        assert all((g == SENTINEL).all() for g in gn)

    for bad_index in (60, 99, -1):  # problem 3 has 60 rows: 60 and 99 are below the padded size 100
        bad = [list(map(list, gs)) for gs in good]
        bad[3][0][0] = bad_index
        raw.set_groups(bad)
        rejected()
    bad = [list(map(list, gs)) for gs in good]
    bad[3][1] = bad[3][1] + [bad[3][0][0]]  # an index in two groups
    raw.set_groups(bad)
    rejected()
    raw.set_groups(good)
    rejected(ldg=raw.ldg - 1)
    rejected(predict_type=2)
    rejected(predict_type=-1)
    rejected(count=0)
    rejected(ldy=99)
    rejected(ldw=99)
    _ok(raw, raw.call())


def test_deterministic_and_device_resident_inputs(ctx):
    _, model = _elevation_model(ctx)
    problems = []
    for b, (n, o) in enumerate(zip((150, 300), _sets(model, 2, 31, spread=0.2))):
        x = np.random.default_rng(n).uniform(0., 10., (n, 3))
        problems.append((_copy(model, o), x, np.sin(x).sum(axis=1) + 0.3 * x[:, 0], _variance(n, 100 + b), random_groups(n, b)))
    problems += _config3_problems(ctx, [77], 3, with_variance=True)
    raw = Batch(ctx, problems)
    for ptype in TYPES:
        host, again = raw.call(ptype, terms=(0, 1, 2)), raw.call(ptype, terms=(0, 1, 2))
        _ok(raw, host)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(host[1:4] + tuple(host[5]), again[1:4] + tuple(again[5])))
    keep = []

    def dev(a):  # a device copy with the host array's memory layout
        keep.append(ctx.to_device(np.ravel(a, order="K")))
        return keep[-1].ptr

    for s, p in zip(raw.structs, raw.probs):
        s.coords = dev(p.fs.coords)
        if p.fs.scales is not None:
            s.scales = dev(p.fs.scales)
        s.location = capi.DEVICE
    over = dict(y=C.c_void_p(dev(raw.Y)), y_var=C.c_void_p(dev(raw.V)),
                tangents=(C.c_void_p * raw.count)(*[None if t is None else dev(t) for t in raw.T]))
    out = raw.call("marginal", terms=(0, 1, 2), **over)
    _ok(raw, out)
    raw.check_sentinels(out)
    for h, d in zip(host[1:4] + tuple(host[5]), out[1:4] + tuple(out[5])):
        assert h.tobytes() == d.tobytes()
    for d in keep:
        d.free()


# ---- the Python surfaces ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ptype", TYPES)
def test_python_batch_across_size_classes_and_pooled(ctx, ptype):
    sizes = [60, 300, 128, 257, 17, 200]
    problems = _config3_problems(ctx, sizes, 55)
    assert len(abgp._size_classes(sizes)) == 3
    models = [p[0] for p in problems]
    datasets = [_dataset(x, y, s) for _, x, y, s, _ in problems]
    groupers = [dict(enumerate(p[4])) for p in problems]
    out = ab.leave_one_group_out_likelihood_gradient_batch(models, datasets, groupers, ptype)
    assert len(out) == len(models)
    raw = Batch(ctx, problems)
    for b, ((m, x, y, s, gs), ds, (value, grad, status)) in enumerate(zip(problems, datasets, out)):
        assert status == capi.AGP_OK
        v1, g1 = m.leave_one_group_out_likelihood_gradient(ds, groupers[b], predict_type=ptype)
        scale = raw.reference(b, ptype)[1]
        assert abs(value - v1) <= 1e-10 * abs(v1), (b, value, v1)
        assert set(grad) == set(g1)
        for name in g1:
            assert abs(grad[name] - g1[name]) <= 1e-9 * scale[name], (b, name)
    # one grouper for all: a callable on the feature
    def octant(f):
        return int(f[0] > 5.) + 2 * int(f[1] > 5.)
    model = _config3(ctx)
    total, grad = ab.pooled_leave_one_group_out_likelihood_gradient(model, datasets, octant, ptype)
    parts = [model.leave_one_group_out_likelihood_gradient(ds, octant, predict_type=ptype) for ds in datasets]
    want = sum(v for v, _ in parts)
    assert abs(total - want) <= 1e-10 * abs(want)
    for name in grad:
        terms = [g[name] for _, g in parts]
        assert abs(grad[name] - sum(terms)) <= 1e-8 * sum(abs(t) for t in terms), name
    with pytest.raises(ValueError):
        ab.leave_one_group_out_likelihood_gradient_batch(models, datasets, groupers[:2], ptype)


def test_parameter_sets_against_the_loop(ctx):
    n = 200
    x, y = synthetic_3d(n, 12)
    s = _variance(n, 13)
    ds = _dataset(x, y, s)
    model = _config3(ctx)
    indexer = dict(enumerate(random_groups(n, 14)))
    sets = _sets(model, 5, 15)
    for ptype in TYPES:
        values, grads = model.leave_one_group_out_likelihood_gradients(ds, indexer, sets, ptype)
        only = model.leave_one_group_out_likelihoods(ds, indexer, sets, ptype)
        assert len(values) == len(grads) == len(only) == 5
        for o, v, g, v0 in zip(sets, values, grads, only):
            m = _copy(model, o)
            v1, g1 = m.leave_one_group_out_likelihood_gradient(ds, indexer, predict_type=ptype)
            scale = (joint_reference if ptype == "joint" else marginal_reference)(m, x, y, s, list(indexer.values()))[1]
            assert abs(v - v1) <= 1e-10 * abs(v1) and abs(v0 - v) <= 1e-12 * abs(v)
            for name in g1:
                assert abs(g[name] - g1[name]) <= 1e-9 * scale[name], name
    assert len(model.leave_one_group_out_likelihoods(ds, indexer, [])) == 0
