"""GPU tests of agp_nll_gradient_batch_ragged and agp_loo_nll_gradient_batch_ragged: the batched exact gradients over
problems of UNEQUAL sizes, at the C-ABI and through ab.log_likelihood_gradient_batch,
ab.leave_one_out_likelihood_gradient_batch and the pooled helpers.

Reference and bounds are the ones the equal-size batches are held to (test_nll_gradient_batch_gpu.py,
test_loo_gradient_batch_gpu.py): the numpy closed forms `reference_gradient` and `reference`, evaluated per problem on its
own n_b points; the value to 1e-10 relative, |g - g_ref| <= 1e-7 s_p with their s_p (the sum of the magnitudes of the
terms a gradient adds up); against the single call 1e-9 s_p and 1e-10; the leave-one-out value-only path against the
full one 1e-12 relative.  Every tree has a noise sigma, whose dK_ii / dsigma is not zero: one phantom diagonal pair that
leaked into the contraction would add (n - n_b) sigma to that gradient, far outside 1e-7 s_p.

At the C-ABI every input column carries NaN behind its n_b values (never read) and every output column a sentinel behind
its n_b values (never written).

Factor paths by padded size: up to 128 one block; 256 a second panel that is phantom rows only, bar one; 512 the fused
panels; 640 past the 512-row outer block; 64 problems of 1030..1100 the two-stream look-ahead schedule."""
import ctypes as C

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
from albatross_amd import gp as abgp
from conftest import synthetic_3d
from test_loo_gradient_gpu import _dataset, _variance, reference
from test_nll_gradient_batch_gpu import _config3, _copy, _heterogeneous, _p, _sets
from test_nll_gradient_gpu import _elevation_model, reference_gradient

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
ENTRIES = ["nll", "loo"]


class Ragged:
    """the arguments of one ragged call, built from (model, x, y, s) problems of any sizes (s: the target variance or
    None - then zeros beside problems that have one; the NLL entry is called without variances, as log_likelihood is),
    with every array kept alive.  ld: the leading dimension of y, y_var, the tangents and the vector output."""

    def __init__(self, ctx, problems, ld=None):
        self.ctx = ctx
        self.problems = problems
        self.models = [p[0] for p in problems]
        self.probs = [abgp._gradient_problem(m, _dataset(x, y, s)) for m, x, y, s in problems]
        self.count = len(problems)
        self.sizes = [p.fs.n for p in self.probs]
        self.n = max(self.sizes)
        self.ld = self.n if ld is None else ld
        self.structs = [p.fs.as_struct() for p in self.probs]
        # row b of these C-ordered arrays is column b of the column-major argument
        self.Y = np.full((self.count, self.ld), np.nan)
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

    def call(self, entry, weights=True, twin=False, **over):
        """(rc, value, grad, vector, status) of agp_<entry>_gradient_batch_ragged (twin: of the equal-size entry), the
        outputs sentinel-filled before the call"""
        ctx = self.ctx
        value = np.full(self.count, SENTINEL)
        grad = np.full((self.count, self.ldg), SENTINEL)
        vec = np.full((self.count, self.ld), SENTINEL)
        status = (C.c_int * self.count)(*([-5] * self.count))
        fn = getattr(ctx._lib, ("agp_nll_gradient_batch" if entry == "nll" else "agp_loo_nll_gradient_batch") + ("" if twin else "_ragged"))
        y_var = None if entry == "nll" or self.V is None else _p(self.V)
        handles = [ctx.private_kernel(m.covariance_function_) for m in self.models]
        try:
            kernels = (C.c_void_p * self.count)(*handles)
            fptrs = (C.c_void_p * self.count)(*[C.addressof(s) for s in self.structs])
            rc = fn(ctx._h, over.get("count", self.count), kernels, fptrs, over.get("y", _p(self.Y)), over.get("ldy", self.ld),
                    over.get("y_var", y_var), over.get("ldv", self.ld), over.get("n_slots", self.n_slots),
                    over.get("slots", self.tables), over.get("tangents", self.tang), over.get("ldt", self.ld), _p(value), _p(grad),
                    over.get("ldg", self.ldg), _p(vec) if weights else None, over.get("ldvec", self.ld), status)
        finally:
            for h in handles:
                ctx._lib.agp_kernel_destroy(h)
        return rc, value, grad, vec, list(status)

    def result(self, entry, b, out):
        """(value, {name: gradient}) of problem b as the Python surface reports it (log p for the NLL entry)"""
        _, value, grad, vec, _ = out
        m, p = self.models[b], self.probs[b]
        g, v = grad[b, :len(p.slots)], vec[b, :p.fs.n]
        if entry == "nll":
            return -value[b], m._log_likelihood_gradient_dict(p.slots, g, v, p.fs)
        return value[b], m._leave_one_out_gradient_dict(p.slots, g, v, p.fs)

    def check_sentinels(self, out, failed=()):
        _, value, grad, vec, _ = out
        for b in range(self.count):
            assert (grad[b, self.n_slots[b]:] == SENTINEL).all(), b
            assert (vec[b, self.sizes[b]:] == SENTINEL).all(), b
            if b in failed:
                assert (vec[b] == SENTINEL).all(), b
            else:
                assert not (vec[b, :self.sizes[b]] == SENTINEL).any(), b

    def check_problem(self, entry, b, out, single=True):
        """problem b against numpy on its own n_b points and (single) against the single entry"""
        m, x, y, s = self.problems[b]
        value, grad = self.result(entry, b, out)
        assert set(grad) == set(m.get_params())
        if entry == "nll":
            want, scale, ref_value = reference_gradient(m, x, y)
        else:
            want, scale, ref_value, _ = reference(m, x, y, s)
        print(f"{entry} b={b} n_b={len(y)} value rel err {abs(value - ref_value) / abs(ref_value):.2e} gradient err / s_p "
              f"{max(abs(grad[k] - want[k]) / scale[k] for k in want if scale[k] > 0.):.2e}")
        assert abs(value - ref_value) <= 1e-10 * abs(ref_value), (b, value, ref_value)
        for name in want:
            assert abs(grad[name] - want[name]) <= 1e-7 * scale[name], (b, name, grad[name], want[name], scale[name])
        if single:
            ds = _dataset(x, y, s)
            v1, g1 = m.log_likelihood_gradient(ds) if entry == "nll" else m.leave_one_out_likelihood_gradient(ds)
            assert abs(value - v1) <= 1e-10 * abs(v1), (b, value, v1)
            for name in g1:
                assert abs(grad[name] - g1[name]) <= 1e-9 * scale[name], (b, name, grad[name], g1[name], scale[name])


def _config3_problems(ctx, sizes, seed):
    """one copy of the config-3 model (SE + noise: the one-launch Gram) with parameters of its own per size, every second
    problem with a target variance"""
    model = _config3(ctx)
    out = []
    for b, (n, o) in enumerate(zip(sizes, _sets(model, len(sizes), seed))):
        x, y = synthetic_3d(n, seed + 13 * b + n)
        out.append((_copy(model, o), x, y, _variance(n, seed + b) if b % 2 else None))
    return out


def _ok(raw, out):
    assert out[0] == capi.AGP_OK and out[4] == [0] * raw.count, (out[0], out[4])


def _value_only(raw, out):
    """the leave-one-out value-only path (no slots, no mean weights) against the full one"""
    only = raw.call("loo", weights=False, n_slots=(C.c_int * raw.count)())
    _ok(raw, only)
    assert (only[2] == SENTINEL).all()
    for b in range(raw.count):
        assert abs(only[1][b] - out[1][b]) <= 1e-12 * abs(out[1][b]), (b, only[1][b], out[1][b])


SIZE_SETS = {
    "one block": [1, 63, 64, 65, 127, 128],
    "second panel of phantoms": [129, 191, 192, 200, 256],
    "fused panels": [385, 448, 500, 512],
    "past the outer block": [513, 577, 640],
    "across classes": [7, 130, 300],
}


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("label", list(SIZE_SETS))
def test_sizes_match_numpy_and_single_calls(ctx, label, entry):
    sizes = SIZE_SETS[label]
    raw = Ragged(ctx, _config3_problems(ctx, sizes, 100 + sum(sizes)))
    out = raw.call(entry)
    _ok(raw, out)
    raw.check_sentinels(out)
    for b in range(raw.count):
        raw.check_problem(entry, b, out)
    again = raw.call(entry)  # two identical calls: the same bits
    assert all(a.tobytes() == b.tobytes() for a, b in zip(out[1:4], again[1:4]))
    if entry == "loo":
        _value_only(raw, out)


@pytest.mark.parametrize("entry", ENTRIES)
def test_look_ahead_schedule_with_phantom_rows(ctx, entry):
    """64 problems drawn from 1030..1100: count n^2 >= 6e7, the two-stream look-ahead factorisation.  numpy on the smallest,
    the largest and one more; the single call on the smallest."""
    rng = np.random.default_rng(64)
    sizes = rng.integers(1030, 1101, 64).tolist()
    sizes[5], sizes[40] = 1030, 1100
    raw = Ragged(ctx, _config3_problems(ctx, sizes, 9))
    out = raw.call(entry)
    _ok(raw, out)
    raw.check_sentinels(out)
    for b in (5, 40, 63):
        raw.check_problem(entry, b, out, single=b == 5)
    if entry == "loo":
        _value_only(raw, out)


def _heterogeneous_ragged(ctx):
    """_heterogeneous's six models (mixed operators, dimensions 1-3, 1 to 9 slots: a Gram launch per problem), each on a
    dataset of its own size, every second one with a target variance"""
    sizes = [130, 300, 257, 77, 200, 191]
    return [(*_heterogeneous(ctx, n)[b], _variance(n, 40 + b) if b % 2 else None) for b, n in enumerate(sizes)]


@pytest.mark.parametrize("entry", ENTRIES)
def test_heterogeneous_trees(ctx, entry):
    raw = Ragged(ctx, _heterogeneous_ragged(ctx))
    out = raw.call(entry)
    _ok(raw, out)
    raw.check_sentinels(out)
    for b in range(raw.count):
        raw.check_problem(entry, b, out)


def _elevation_problems(ctx, sizes=(150, 300, 210)):
    """ScalingTerm tangent columns, a linear mean, parameters and a target variance of its own per problem"""
    _, model = _elevation_model(ctx)
    model.set_param_values({"slope": 0.2, "offset": -0.4})
    out = []
    for b, (n, o) in enumerate(zip(sizes, _sets(model, len(sizes), 31, spread=0.2))):
        x = np.random.default_rng(n).uniform(0., 10., (n, 3))
        out.append((_copy(model, o), x, np.sin(x).sum(axis=1) + 0.3 * x[:, 0], _variance(n, 100 + b)))
    return out


@pytest.mark.parametrize("entry", ENTRIES)
def test_elevation_model_with_tangent_columns(ctx, entry):
    raw = Ragged(ctx, _elevation_problems(ctx), ld=333)  # leading dimensions above the padded size
    out = raw.call(entry)
    _ok(raw, out)
    raw.check_sentinels(out)
    for b in range(raw.count):
        assert {"elevation_scaling_center", "elevation_scaling_factor", "slope", "offset"} <= set(raw.result(entry, b, out)[1])
        raw.check_problem(entry, b, out)


def test_duplicated_points_with_a_target_variance(ctx):
    """a point twice in a problem with phantom rows: the noise couples the two (equal features), the target variance keeps K
    definite.  The leave-one-out entry, whose reference carries the variance."""
    problems = _config3_problems(ctx, [140, 90, 200], 77)
    m, x, y, _ = problems[1]
    x = x.copy()
    x[11] = x[3]
    problems[1] = (m, x, y, _variance(90, 5))
    raw = Ragged(ctx, problems)
    out = raw.call("loo")
    _ok(raw, out)
    for b in range(raw.count):
        raw.check_problem("loo", b, out)


@pytest.mark.parametrize("entry", ENTRIES)
def test_equal_sizes_give_the_bits_of_the_equal_size_entry(ctx, entry):
    n = 300
    problems = [(*p, _variance(n, 40 + b) if b % 2 else None) for b, p in enumerate(_heterogeneous(ctx, n))]
    raw = Ragged(ctx, problems)
    ragged, twin = raw.call(entry), raw.call(entry, twin=True)
    _ok(raw, ragged)
    _ok(raw, twin)
    for a, b in zip(ragged[1:4], twin[1:4]):
        assert a.tobytes() == b.tobytes()
    if entry == "loo":
        zero = (C.c_int * raw.count)()
        a, b = raw.call(entry, weights=False, n_slots=zero), raw.call(entry, weights=False, n_slots=zero, twin=True)
        assert a[0] == capi.AGP_OK and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("entry", ENTRIES)
def test_device_resident_inputs_give_the_same_bits(ctx, entry):
    problems = _elevation_problems(ctx, (150, 300)) + _config3_problems(ctx, [77], 3)
    raw = Ragged(ctx, problems)
    host = raw.call(entry)
    _ok(raw, host)
    keep = []

    def dev(a):  # a device copy with the host array's memory layout
        keep.append(ctx.to_device(np.ravel(a, order="K")))
        return keep[-1].ptr

    for s, p in zip(raw.structs, raw.probs):
        s.coords = dev(p.fs.coords)
        if p.fs.scales is not None:
            s.scales = dev(p.fs.scales)
        s.location = capi.DEVICE
    over = dict(y=C.c_void_p(dev(raw.Y)), tangents=(C.c_void_p * raw.count)(*[None if t is None else dev(t) for t in raw.T]))
    if entry == "loo":
        over["y_var"] = C.c_void_p(dev(raw.V))
    out = raw.call(entry, **over)
    _ok(raw, out)
    raw.check_sentinels(out)
    for h, d in zip(host[1:4], out[1:4]):
        assert h.tobytes() == d.tobytes()
    for d in keep:
        d.free()


def test_shared_vectors(ctx):
    """ldy = ldv = 0: one vector of n values, of which problem b uses the first n_b"""
    sizes = [300, 140, 257]
    x, y = synthetic_3d(300, 5)
    s = _variance(300, 8)
    model = _config3(ctx)
    problems = [(_copy(model, o), x[:n], y[:n], s[:n]) for n, o in zip(sizes, _sets(model, 3, 21))]
    raw = Ragged(ctx, problems)
    for entry in ENTRIES:
        rep = raw.call(entry)
        one = raw.call(entry, y=_p(np.ascontiguousarray(y)), ldy=0, y_var=None if entry == "nll" else _p(np.ascontiguousarray(s)), ldv=0)
        _ok(raw, rep)
        _ok(raw, one)
        for a, b in zip(rep[1:4], one[1:4]):
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("entry", ENTRIES)
def test_failed_problems_are_reported_and_isolated(ctx, entry):
    sizes = [300, 210, 260, 140, 290, 257]
    problems = _config3_problems(ctx, sizes, 4)
    _, xs, ys, _ = problems[1]
    xs = xs.copy()
    xs[5] = xs[0]  # no noise, no variance and a duplicated point: singular
    problems[1] = (ab.gp_from_covariance(ab.SquaredExponential(1., 1.), context=ctx), xs, ys, None)
    m4, xn, yn, s4 = problems[4]
    xn = xn.copy()
    xn[17, 1] = np.nan  # a real row
    problems[4] = (m4, xn, yn, s4)
    raw = Ragged(ctx, problems)
    out = raw.call(entry)
    rc, value, grad, vec, status = out
    assert rc == capi.AGP_OK
    assert status[1] == capi.AGP_ERR_NOT_POSITIVE_DEFINITE and status[4] == capi.AGP_ERR_NAN_INPUT
    raw.check_sentinels(out, failed=(1, 4))
    for b in (1, 4):
        assert np.isnan(value[b]) and np.isnan(grad[b, :raw.n_slots[b]]).all()
    for b in (0, 2, 3, 5):
        assert status[b] == capi.AGP_OK
        raw.check_problem(entry, b, out)


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors_write_nothing(ctx, entry):
    _, elev = _elevation_model(ctx)
    rng = np.random.default_rng(2)
    xa, xb = rng.uniform(0., 10., (100, 3)), rng.uniform(0., 10., (70, 3))
    problems = [(_config3(ctx), xa, np.sin(xa).sum(axis=1), _variance(100, 1)), (elev, xb, np.cos(xb).sum(axis=1), _variance(70, 2))]
    raw = Ragged(ctx, problems)
    _ok(raw, raw.call(entry))
    n = raw.n

    def rejected(r=raw, **over):
        rc, value, grad, vec, status = r.call(entry, **over)
        assert rc == capi.AGP_ERR_INVALID_ARGUMENT, over
        assert (value == SENTINEL).all() and (grad == SENTINEL).all() and (vec == SENTINEL).all() and status == [-5, -5], over

    rejected(count=0)
    rejected(ldy=n - 1)
    if entry == "loo":
        rejected(ldv=n - 1)
    rejected(ldvec=n - 1)  # ldi / ldw
    rejected(ldt=n - 1)    # problem 1 has tangent slots
    rejected(ldt=raw.sizes[1])  # its own size is not enough: the padded size counts
    rejected(ldg=raw.ldg - 1)
    rejected(tangents=None)
    for size in (0, -3):
        bad = Ragged(ctx, problems)
        bad.structs[1].n = size
        rejected(bad)
    mixed = Ragged(ctx, problems)
    mixed.structs[1].location = capi.DEVICE
    rejected(mixed)


def test_count_above_the_grid_limit_is_rejected(ctx):
    count = 65536
    x, y = synthetic_3d(8, 1)
    model = _config3(ctx)
    p = abgp._gradient_problem(model, ab.RegressionDataset(x, y))
    st = p.fs.as_struct()
    kh = ctx.private_kernel(model.covariance_function_)
    try:
        kernels = (C.c_void_p * count)(*([kh] * count))
        fptrs = (C.c_void_p * count)(*([C.addressof(st)] * count))
        n_slots = (C.c_int * count)(*([len(p.slots)] * count))
        tables = (C.c_void_p * count)(*([C.addressof(p.table)] * count))
        for name in ("agp_nll_gradient_batch_ragged", "agp_loo_nll_gradient_batch_ragged"):
            value, grad, vec = np.full(count, SENTINEL), np.full((count, len(p.slots)), SENTINEL), np.full((count, 8), SENTINEL)
            status = (C.c_int * count)(*([-5] * count))
            rc = getattr(ctx._lib, name)(ctx._h, count, kernels, fptrs, _p(np.ascontiguousarray(y)), 0, None, 0, n_slots, tables, None, 0,
                                         _p(value), _p(grad), len(p.slots), _p(vec), 8, status)
            assert rc == capi.AGP_ERR_INVALID_ARGUMENT
            assert (value == SENTINEL).all() and (grad == SENTINEL).all() and (vec == SENTINEL).all() and set(status) == {-5}
    finally:
        ctx._lib.agp_kernel_destroy(kh)


# ---- the Python surfaces -------------------------------------------------------------------------------------------
def _shuffled_datasets(ctx):
    """12 datasets spanning three size classes in shuffled order, every second one with a target variance, and one model
    with parameters of its own each"""
    sizes = [60, 300, 128, 257, 17, 200, 129, 384, 90, 256, 330, 100]
    problems = _config3_problems(ctx, sizes, 55)
    assert len(abgp._size_classes(sizes)) == 3
    return [p[0] for p in problems], [_dataset(x, y, s) for _, x, y, s in problems], problems


def test_python_batches_across_size_classes(ctx):
    models, datasets, problems = _shuffled_datasets(ctx)
    for batch, single in ((ab.log_likelihood_gradient_batch, "log_likelihood_gradient"),
                          (ab.leave_one_out_likelihood_gradient_batch, "leave_one_out_likelihood_gradient")):
        out = batch(models, datasets)
        assert len(out) == len(models)
        for (m, x, y, s), ds, (value, grad) in zip(problems, datasets, out):  # the caller's order
            v1, g1 = getattr(m, single)(ds)
            scale = reference_gradient(m, x, y)[1] if batch is ab.log_likelihood_gradient_batch else reference(m, x, y, s)[1]
            assert abs(value - v1) <= 1e-10 * abs(v1), (len(y), value, v1)
            assert set(grad) == set(g1)
            for name in g1:
                assert abs(grad[name] - g1[name]) <= 1e-9 * scale[name], (len(y), name)


def test_pooled_helpers_equal_the_sums(ctx):
    _, datasets, _ = _shuffled_datasets(ctx)
    model = _config3(ctx)
    for pooled, batch in ((ab.pooled_log_likelihood_gradient, ab.log_likelihood_gradient_batch),
                          (ab.pooled_leave_one_out_likelihood_gradient, ab.leave_one_out_likelihood_gradient_batch)):
        total, grad = pooled(model, datasets)
        parts = batch([model] * len(datasets), datasets)
        want = sum(v for v, _ in parts)
        assert abs(total - want) <= 1e-12 * abs(want)
        assert set(grad) == set(model.get_params())
        for name in grad:
            terms = [g[name] for _, g in parts]
            assert abs(grad[name] - sum(terms)) <= 1e-12 * sum(abs(t) for t in terms), name
    # one failing dataset: NaN throughout
    x = np.random.default_rng(1).uniform(0., 10., (50, 3))
    x[3, 0] = np.nan
    total, grad = ab.pooled_log_likelihood_gradient(model, datasets[:3] + [ab.RegressionDataset(x, np.zeros(50))])
    assert np.isnan(total) and all(np.isnan(v) for v in grad.values())
