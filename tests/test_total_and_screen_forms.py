"""The two kernels that decide what a chain accepts, at every form of their
launches (-m gpu): the flat total k_ll_total (bnpc_ll_total_issue / _wait)
and the screen of a parameter batch k_mh_screen (bnpc_mh_screen).

k_ll_total: blocks = min(ceil(K*M / 256), 256); a thread's strided loop makes
a second trip only past K*M = 65536; the last block is ragged; elements
without counts are skipped; trial slots e >= E are padded; the partial sums
come back through pinned memory written in place or through a device buffer
(BNPC_ZERO_COPY=0).  SHAPES puts K*M on each of these edges, with counts that
hold empty rows (whole blocks skip) and single isolated elements at the first
and last index of the array and at the last index of every trip.  Every trial
is compared with an extended-precision reference (oracle.likelihood) under a
bound DERIVED from the kernel's arithmetic (total_ll_bound), not tuned: the
CPU suite shows a float64 evaluation in the kernel's grouping well inside it
(tests/test_oracle_golden.py).  Then the bits: a rate pair gives the same
value alone and in every slot beside other pairs, on either result route, on
a second call, and whatever theta holds where there are no counts; one more
count at one element moves the total by that element's term.

k_mh_screen against the two segments of the last bnpc_view_counts
(counts_src = 1, a third row = their sum): the decisions of the SciPy-level
arithmetic (CRP._mh_math) on the counts passed explicitly, as
test_gpu_parity.py does for the per-cluster counts; the guards that leave an
element to the host, each fed on purpose; and what the entry points refuse.
"""
import collections

import numpy as np
import pytest

from bnpc_amd import _lib, model as P
from oracle import likelihood as L
from oracle.constants import TMAX, TMIN

pytestmark = pytest.mark.gpu

KNOBS = ('BNPC_ZERO_COPY', 'BNPC_MH_SCREEN', 'BNPC_MASK_COUNTS_MAX')
SPAN = L.TOTAL_SPAN             # elements one trip of the full grid covers

# (M, K): K * M =
SHAPES = [
    (1, 1),                     # 1: one thread
    (255, 1), (1, 255),         # 255: one ragged block
    (256, 1), (1, 256),         # 256: one full block
    (257, 1), (1, 257),         # 257: two blocks, one element in the second
    (255, 257), (257, 255),     # 65535: 256 blocks, the last one ragged
    (256, 256),                 # 65536: 256 full blocks, still one trip
    (1, 65537),                 # 65537: the first second trip, one element
    (1, 3 * SPAN + 77),         # 196685: four trips, a ragged tail
    (257, 766),                 # 196862 = 3 * 65536 + 254, dense rows
]
# distinct error pairs, two of them extreme
RATES = ((0.01, 0.2), (1e-6, 0.45), (0.3, 1e-6), (0.05, 0.1))

TotalCase = collections.namedtuple('TotalCase',
    'M K KM assign n1 n0 theta isolated empty_rows')


def _shape_id(s):
    return f'M{s[0]}-K{s[1]}'


# ---------------------------------------------------- inputs, NumPy only
def special_indices(KM):
    """first and last index of the array, last index of every trip"""
    out = {0, KM - 1}
    out.update(range(SPAN - 1, KM, SPAN))
    return sorted(out)


def _probe_columns(M):
    cols = set()
    for m_, K in SHAPES:
        if m_ == M:
            cols.update(i % M for i in special_indices(K * M))
    return sorted(cols)


_DATA = {}


def total_data(M):
    """(matrix, probes, spares) for the contexts of M mutations.  Ordinary
    cells (0 / 1, a fifth missing); probe cells that hold ONE observation
    (probes[m] = the cells whose only entry is in column m): alone in a
    cluster they make an isolated element; and two spare cells that hold
    nothing at all here - switched on (spare_data) they add one count at one
    element."""
    if M in _DATA:
        return _DATA[M]
    rng = np.random.RandomState(1000 + M)
    n = 3000 if M == 1 else 600
    x = (rng.random_sample((n, M)) < 0.35).astype(np.float64)
    x[rng.random_sample(x.shape) < 0.2] = np.nan
    probes = {}
    if M == 1:
        probes[0] = [int(i) for i in np.flatnonzero(~np.isnan(x[:, 0]))[:8]]
    else:
        extra = []
        for m in _probe_columns(M):
            probes[m] = []
            for value in (1.0, 0.0, 1.0, 0.0):
                row = np.full(M, np.nan)
                row[m] = value
                probes[m].append(n + len(extra))
                extra.append(row)
        x = np.vstack([x] + extra)
    x = np.vstack([x, np.full((2, M), np.nan)])
    spares = (x.shape[0] - 2, x.shape[0] - 1)
    _DATA[M] = (x, probes, spares)
    return _DATA[M]


def spare_data(M, which):
    """total_data's matrix with one spare cell switched on: 'A' observes a 1
    in column 0, 'B' a 0 in column M - 1.  -> (matrix, cell, column, value)"""
    x, _, spares = total_data(M)
    x = x.copy()
    cell = spares[0 if which == 'A' else 1]
    col, value = (0, 1.0) if which == 'A' else (M - 1, 0.0)
    x[cell, col] = value
    return x, cell, col, value


def counts_of(x, assign, K):
    n1 = np.zeros((K, x.shape[1]), dtype=np.int32)
    n0 = np.zeros_like(n1)
    np.add.at(n1, assign, (x == 1).astype(np.int32))
    np.add.at(n0, assign, (x == 0).astype(np.int32))
    return n1, n0


_CASES = {}


def total_case(M, K):
    """Assignment, counts and parameters of one shape.  Where K allows, the
    rows of the special indices hold one probe cell each (isolated non-zero
    elements), a run of ids holds no cell (rows that are all zero), the other
    cells spread over the rest."""
    if (M, K) in _CASES:
        return _CASES[(M, K)]
    x, probes, _ = total_data(M)
    N, KM = x.shape[0], K * M
    rng = np.random.RandomState(1009 * K + M)
    special = collections.OrderedDict()
    for i in special_indices(KM):
        special.setdefault(i // M, []).append(i % M)
    assign = np.full(N, -1, dtype=np.int64)
    isolated, empty = [], []
    rest = np.arange(K)
    if K >= 16:
        free = {m: list(cells) for m, cells in probes.items()}
        for k, cols in special.items():
            for m in cols:
                assign[free[m].pop()] = k
                isolated.append(k * M + m)
        empty = [k for k in range(K // 3, K // 3 + max(2, K // 8))
            if k not in special]
        rest = np.setdiff1d(rest, np.array(list(special) + empty))
    todo = assign < 0
    assign[todo] = rest[rng.randint(0, rest.size, int(todo.sum()))]
    n1, n0 = counts_of(x, assign, K)
    theta = np.clip(rng.uniform(size=(K, M)), TMIN, TMAX).astype(np.float32)
    edge = np.array([TMIN, TMAX, 0.5], dtype=np.float32)
    flat = theta.reshape(-1)
    live = np.flatnonzero((n1 | n0).ravel())
    # the bounds and 0.5: on the special elements and on a share of the
    # elements with counts, and on a few without
    pick = np.concatenate([np.array(special_indices(KM)),
        live[::7], rng.randint(0, KM, 5)])
    flat[pick] = edge[np.arange(pick.size) % 3]
    _CASES[(M, K)] = TotalCase(M, K, KM, assign, n1, n0, theta,
        np.array(isolated, dtype=np.int64), np.array(empty, dtype=np.int64))
    return _CASES[(M, K)]


_REFS = {}


def total_reference(case, j):
    """(total, sum |term|, sum counts) of case under RATES[j], made once"""
    key = (case.M, case.K, j)
    if key not in _REFS:
        _REFS[key] = L.total_ll_reference(case.theta, case.n1, case.n0,
            *RATES[j])
    return _REFS[key]


# ------------------------------------------------------------ the device
class _Contexts:
    def __init__(self):
        self.ctx = {}

    def get(self, M, which='off'):
        if (M, which) not in self.ctx:
            data = total_data(M)[0] if which == 'off' \
                else spare_data(M, which)[0]
            self.ctx[(M, which)] = _lib.Context(data=data)
        return self.ctx[(M, which)]

    def close(self):
        for ctx in self.ctx.values():
            ctx.close()


@pytest.fixture(scope='module')
def ctxs():
    if L.TOTAL_REFERENCE is None:
        pytest.skip('no arithmetic with a 64-bit significand on this host')
    c = _Contexts()
    yield c
    c.close()


def _set_knobs(monkeypatch, ctx, knobs):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    ctx.reload_options()


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def _resident(ctx, case, x):
    n1, n0 = ctx.colcounts_by_label(case.assign, np.arange(case.K))
    w1, w0 = counts_of(x, case.assign, case.K)
    assert np.array_equal(n1, w1) and np.array_equal(n0, w0)


def _assert_case_is_what_it_claims(case):
    live = (case.n1 | case.n0).ravel() != 0
    if case.K < 16:
        return
    assert set(special_indices(case.KM)) == set(case.isolated.tolist())
    rows = collections.Counter((case.isolated // case.M).tolist())
    for i in case.isolated:
        # nothing else in its row (row 765 of 257 x 766 holds two of them)
        k = int(i) // case.M
        assert live[i] and live[k * case.M:(k + 1) * case.M].sum() == rows[k]
    assert case.empty_rows.size >= 2
    assert not live.reshape(case.K, case.M)[case.empty_rows].any()
    if case.M >= 255:       # whole blocks of 256 elements without a count
        run = case.empty_rows.size * case.M
        assert run >= 3 * 256


@pytest.mark.parametrize('shape', SHAPES, ids=_shape_id)
def test_ll_total_at_every_launch_form(shape, ctxs, monkeypatch):
    """Every trial of E = 1 .. 4 within total_ll_bound of the reference; the
    same bits for a rate pair alone and in each slot 0 .. 3 beside others, on
    both result routes and on a second call; theta without counts is not
    read into the sum."""
    case = total_case(*shape)
    _assert_case_is_what_it_claims(case)
    ctx = ctxs.get(case.M)
    _set_knobs(monkeypatch, ctx, {})
    _resident(ctx, case, total_data(case.M)[0])
    fp = np.array([r[0] for r in RATES])
    fn = np.array([r[1] for r in RATES])

    alone = np.array([ctx.ll_total(case.theta, [fp[j]], [fn[j]])[0]
        for j in range(4)])
    for j in range(4):
        total, mag, mass = total_reference(case, j)
        bound = L.total_ll_bound(case.KM, mag, mass)
        dist = L.total_ll_distance(alone[j], total)
        print(f'\n[total] {_shape_id(shape)} rates {RATES[j]}: got '
            f'{alone[j]!r}, |got - ref| {dist:.3e}, bound {bound:.3e}, '
            f'ratio {dist / bound if bound else 0:.4f}')
        assert dist <= bound, (shape, RATES[j], alone[j], float(total),
            dist, bound)
        assert alone[j] < 0 or mass == 0
    # the four pairs really are four values
    if case.n1.sum() + case.n0.sum():
        assert np.unique(alone).size == 4

    def slots_and_repeat(route):
        for E in (2, 3, 4):
            for first in range(4):
                order = [(first + s) % 4 for s in range(E)]
                got = ctx.ll_total(case.theta, fp[order], fn[order])
                assert got.shape == (E,)
                assert np.array_equal(_bits(got), _bits(alone[order])), \
                    (shape, route, E, order, got, alone[order])
        again = ctx.ll_total(case.theta, fp, fn)
        assert np.array_equal(_bits(again), _bits(alone)), (shape, route)
        assert np.array_equal(_bits(ctx.ll_total(case.theta, fp, fn)),
            _bits(again))

    slots_and_repeat('default')
    for zero_copy in ('0', '1'):
        _set_knobs(monkeypatch, ctx, {'BNPC_ZERO_COPY': zero_copy})
        slots_and_repeat('BNPC_ZERO_COPY=' + zero_copy)
        for j in range(4):
            assert np.array_equal(_bits(
                ctx.ll_total(case.theta, [fp[j]], [fn[j]])), _bits(alone[[j]]))
        # issued, other work on the context, picked up later
        ctx.ll_total_issue(case.theta, fp[:3], fn[:3])
        ctx.view_set(1, np.arange(min(40, ctx.N)))
        assert np.array_equal(_bits(ctx.ll_total_wait()), _bits(alone[:3]))
    _set_knobs(monkeypatch, ctx, {})

    # theta where there is no count: first, last and around every trip's end
    dead = np.flatnonzero((case.n1 | case.n0).ravel() == 0)
    if dead.size:
        marks = np.array(special_indices(case.KM))
        near = dead[np.clip(np.searchsorted(dead, marks), 0, dead.size - 1)]
        touch = np.unique(np.concatenate([dead[[0, -1]], near, dead[::97]]))
        other = case.theta.copy()
        flat = other.reshape(-1)
        flat[touch] = np.where(flat[touch] == np.float32(0.123),
            np.float32(0.9), np.float32(0.123))
        assert not np.array_equal(other, case.theta)
        got = ctx.ll_total(other, fp, fn)
        assert np.array_equal(_bits(got), _bits(alone)), (shape, got, alone)


def _count_targets(case):
    """(spare, row, where): elements that take one more count, in the first
    block, in block 255 of the grid, in the last block of the last trip."""
    M, K, KM = case.M, case.K, case.KM
    out = [('A', 0, 'first block'), ('B', K - 1, 'last block, last trip')]
    if K > 2:
        out.append(('A', K // 2, 'a middle row'))
    k = SPAN // M - 1                       # its column M - 1 ends block 255
    if k < K - 1:
        assert SPAN - 256 <= k * M + M - 1 < SPAN
        out.append(('B', k, 'block 255 of the first trip'))
    trips = -(-KM // SPAN)
    first = (trips - 1) * SPAN              # first index of the last trip
    if trips > 1 and first % M == 0 and first // M not in (0, K // 2):
        out.append(('A', first // M, 'first index of the last trip'))
    return out


@pytest.mark.parametrize('shape', SHAPES, ids=_shape_id)
def test_ll_total_one_more_count_adds_that_elements_term(shape, ctxs,
        monkeypatch):
    """A cell that observes one mutation only, put into cluster k, adds one
    count at (k, m): the total moves by log P(x | theta[k, m]) to within the
    bounds of the two totals.  Elements of the first block, of block 255, of
    the last (ragged) block and of the last trip."""
    case = total_case(*shape)
    base_ctx = ctxs.get(case.M)
    _set_knobs(monkeypatch, base_ctx, {})
    _resident(base_ctx, case, total_data(case.M)[0])
    fp = np.array([r[0] for r in RATES])
    fn = np.array([r[1] for r in RATES])
    base = base_ctx.ll_total(case.theta, fp, fn)
    ld = np.longdouble
    for which, k, where in _count_targets(case):
        x, cell, m, value = spare_data(case.M, which)
        ctx = ctxs.get(case.M, which)
        _set_knobs(monkeypatch, ctx, {})
        moved = case._replace(assign=case.assign.copy())
        moved.assign[cell] = k
        n1, n0 = ctx.colcounts_by_label(moved.assign, np.arange(case.K))
        w1, w0 = case.n1.copy(), case.n0.copy()
        (w1 if value == 1 else w0)[k, m] += 1
        assert np.array_equal(n1, w1) and np.array_equal(n0, w0), where
        got = ctx.ll_total(case.theta, fp, fn)
        t = ld(float(case.theta[k, m]))
        o = ld(float(np.float32(1) - case.theta[k, m]))
        for j in range(4):
            f, n = ld(RATES[j][0]), ld(RATES[j][1])
            term = np.log(t * (1 - n) + o * f) if value == 1 \
                else np.log(t * n + o * (1 - f))
            total0, mag0, mass0 = total_reference(case, j)
            total1, mag1, mass1 = L.total_ll_reference(case.theta, w1, w0,
                *RATES[j])
            b0 = L.total_ll_bound(case.KM, mag0, mass0)
            b1 = L.total_ll_bound(case.KM, mag1, mass1)
            assert L.total_ll_distance(got[j], total1) <= b1, (shape, where)
            step = ld(got[j]) - ld(base[j])
            assert abs(step - term) <= b0 + b1, (shape, where, RATES[j],
                float(step), float(term), b0 + b1)
            assert step < 0


def test_ll_total_refusals(ctxs, monkeypatch):
    case = total_case(257, 255)
    ctx = ctxs.get(257)
    _set_knobs(monkeypatch, ctx, {})
    _resident(ctx, case, total_data(257)[0])
    th = case.theta
    for E in (0, 5):
        with pytest.raises(RuntimeError, match='E out of range'):
            ctx.ll_total(th, np.full(E, 0.01), np.full(E, 0.2))
        with pytest.raises(RuntimeError, match='E out of range'):
            ctx.ll_total_issue(th, np.full(E, 0.01), np.full(E, 0.2))
    for bad in (0.0, 1.0):
        for slot in (0, 3):
            rates = np.full(4, 0.1)
            rates[slot] = bad
            with pytest.raises(RuntimeError, match='error rates must lie'):
                ctx.ll_total(th, rates, np.full(4, 0.2))
            with pytest.raises(RuntimeError, match='error rates must lie'):
                ctx.ll_total(th, np.full(4, 0.2), rates)
    for K in (case.K - 1, case.K + 1):
        other = np.full((K, case.M), 0.5, dtype=np.float32)
        with pytest.raises(RuntimeError, match='resident counts'):
            ctx.ll_total(other, [0.01], [0.2])
    want = ctx.ll_total(th, [0.01, 0.02], [0.2, 0.3])
    ctx.ll_total_issue(th, [0.01, 0.02], [0.2, 0.3])
    with pytest.raises(RuntimeError, match='already pending'):
        ctx.ll_total_issue(th, [0.05], [0.1])
    with pytest.raises(RuntimeError, match='already pending'):
        ctx.ll_total(th, [0.05], [0.1])
    # the refused calls left the pending total alone
    assert np.array_equal(_bits(ctx.ll_total_wait()), _bits(want))
    with pytest.raises(RuntimeError, match='no deferred total is pending'):
        ctx.ll_total_wait()
    # and none of them left the context unusable
    assert np.array_equal(_bits(ctx.ll_total(th, [0.01, 0.02], [0.2, 0.3])),
        _bits(want))


# ------------------------------------------------ the screen, view counts
SD = np.array([0.1, 0.25, 0.5])


def _exact_decisions(old, sd, sd_idx, U, u, n1, n0, prior, FP, FN):
    """(new, A, decline) of the SciPy-level arithmetic on explicit counts"""
    probe = P.CRP.__new__(P.CRP)
    probe.param_proposal_sd = sd
    probe.p, probe.q = prior
    probe.beta_prior_uniform = bool(prior[0] == prior[1] == 1)
    probe.FP, probe.FN = FP, FN
    with np.errstate(all='ignore'):
        new, A, decline, _ = probe._mh_math(old, sd[sd_idx], U, u, n1, n0,
            False, None)
    return new, A, decline


def _knife(rng, A):
    """the uniform that sits ON the decision: exp(A) nudged both ways"""
    with np.errstate(all='ignore'):
        near = np.exp(np.clip(A, -700, -1e-300))
    eps = rng.choice([1e-15, 1e-12, 1e-9, 1e-6], A.shape) \
        * rng.choice([-1, 1], A.shape)
    return np.clip(near * (1 + eps), 1e-300, 1 - 1e-16)


def _screen_on_counts(rng, ctx, src, counts, theta_mode, prior, FP, FN,
        u_mode, same_rows=False):
    """One batch against explicit counts (G x M), screened on the device
    from counts source `src`.  same_rows: every row gets the LAST row's old
    parameters and draws (and, on the knife edge, the uniforms that sit on
    the last row's decisions), so that rows differ by their counts alone.
    Asserts what test_gpu_parity._screen_case and its caller assert; returns
    the flags with 3 folded into 2."""
    n1, n0 = counts
    G, M = n1.shape
    if theta_mode == 'uniform':
        old = rng.uniform(size=(G, M))
    else:                               # 'posterior'
        old = (n1 + .25) / (n1 + n0 + .5) + rng.normal(size=(G, M)) * 0.01
    sd_idx = rng.randint(0, 3, (G, M)).astype(np.int32)
    U = rng.uniform(size=(G, M))
    u = rng.uniform(size=(G, M))
    if same_rows:
        old, sd_idx, U, u = (np.repeat(a[-1:], G, axis=0)
            for a in (old, sd_idx, U, u))
    old = np.clip(old, P.TMIN, P.TMAX).astype(np.float32)
    args = (n1, n0, prior, FP, FN)
    new, A, decline = _exact_decisions(old, SD, sd_idx, U, u, *args)
    if u_mode == 'knife':
        u = _knife(rng, A)
        if same_rows:
            u = np.repeat(u[-1:], G, axis=0)
        new, A, decline = _exact_decisions(old, SD, sd_idx, U, u, *args)
    uniform = bool(prior[0] == prior[1] == 1)
    flags, new32 = ctx.mh_screen(src, old, SD, (sd_idx, U, u), P.TMIN,
        P.TMAX, FP, FN, prior[0], prior[1], uniform, with_theta=True)
    what = (src, G, theta_mode, prior, u_mode, same_rows)
    assert np.isin(flags, (0, 1, 2, 3)).all(), what
    given = flags == 3
    assert not (given & decline).any(), what
    assert np.array_equal(new32[given].view(np.int32),
        new[given].view(np.int32)), (what, np.argwhere(
            given & (new32.view(np.int32) != new.view(np.int32)))[:3])
    flags = np.where(given, 2, flags).astype(np.uint8)
    bad = ((flags == 0) & ~decline) | ((flags == 2) & decline)
    assert not bad.any(), (what, np.argwhere(bad)[:3], A[bad][:3])
    return flags


def test_mh_screen_on_the_view_counts_and_their_sum(ctxs, monkeypatch):
    """counts_src = 1: rows 0 and 1 of the batch are the two segments of the
    last view_counts, a third row their sum.  One cell against hundreds, so
    that a screen that took row 0 or row 1 for the sum decides otherwise:
    no flag 0 on a proposal the exact arithmetic accepts, no flag 2 / 3 on
    one it declines, flag-3 proposals bit for bit, more than 0.9 of the
    batch decided away from the knife edge - and, on uniforms that sit on
    the SUM's decisions with the same parameters and draws in every row, row
    2's flags differ from row 0's and from row 1's on more than a tenth of
    the elements (a kernel that read one of them for the sum: on none; the
    one cell observes 4 mutations in 5, and three knife offsets in four lie
    inside the screen's margin)."""
    M = 257
    x = total_data(M)[0]
    ctx = ctxs.get(M)
    _set_knobs(monkeypatch, ctx, {})
    rng = np.random.RandomState(41)
    cells = rng.randint(0, 600, 420)            # ordinary cells, repeats
    labels = np.ones(cells.size, dtype=np.int64)
    labels[rng.permutation(cells.size)[:50]] = -1
    labels[[0, 419]] = -1                       # first and last slot: none
    labels[77] = 0                              # ONE cell in segment 0
    ctx.view_set(1, cells)
    n1, n0 = ctx.view_counts(1, labels, 2)
    for g in range(2):
        sub = x[cells[labels == g]]
        assert np.array_equal(n1[g], (sub == 1).sum(axis=0))
        assert np.array_equal(n0[g], (sub == 0).sum(axis=0))
    assert (n1[0] + n0[0]).max() == 1 and (n1[1] + n0[1]).min() > 200
    assert (n1[0] + n0[0]).sum() > 0.7 * M
    three = (np.vstack([n1, n1[:1] + n1[1:]]), np.vstack([n0, n0[:1] + n0[1:]]))
    ruled = seen = 0
    differ = np.zeros(2)
    compared = 0
    for G, counts in ((2, (n1, n0)), (3, three)):
        for theta_mode in ('uniform', 'posterior'):
            for prior in ((.25, .25), (1, 1)):
                for FP, FN in ((.01, .2), (1e-4, .45)):
                    for u_mode in ('random', 'knife'):
                        flags = _screen_on_counts(rng, ctx, 1, counts,
                            theta_mode, prior, FP, FN, u_mode)
                        if u_mode == 'random':
                            ruled += int((flags != 1).sum())
                            seen += flags.size
                    if G == 3:
                        flags = _screen_on_counts(rng, ctx, 1, counts,
                            theta_mode, prior, FP, FN, 'knife',
                            same_rows=True)
                        differ += [(flags[2] != flags[0]).sum(),
                            (flags[2] != flags[1]).sum()]
                        compared += M
    print(f'\n[screen] decided {ruled} of {seen}; row 2 differs from row 0 '
        f'on {differ[0]:.0f}, from row 1 on {differ[1]:.0f} of {compared}')
    assert ruled > 0.9 * seen, (ruled, seen)
    assert differ[0] > 0.1 * compared and differ[1] > 0.1 * compared, \
        (differ, compared)


def _screen_args(rng, G, M):
    old = np.clip(rng.uniform(size=(G, M)), TMIN, TMAX).astype(np.float32)
    return old, (rng.randint(0, 3, (G, M)).astype(np.int32),
        rng.uniform(size=(G, M)), rng.uniform(size=(G, M)))


def test_mh_screen_refusals(ctxs, monkeypatch):
    M = 257
    ctx = ctxs.get(M)
    _set_knobs(monkeypatch, ctx, {})
    rng = np.random.RandomState(43)
    N = ctx.N

    def screen(src, G, cols=M):
        old, draws = _screen_args(rng, G, cols)
        return ctx.mh_screen(src, old, SD, draws, TMIN, TMAX, .01, .2, .25,
            .25, False)

    ctx.view_set(1, np.arange(300))
    ctx.view_counts(1, rng.randint(0, 2, 300), 2)
    assert screen(1, 2).shape == (2, M) and screen(1, 3).shape == (3, M)
    for G in (1, 4):
        with pytest.raises(RuntimeError, match='last view counts'):
            screen(1, G)
    ctx.view_counts(1, rng.randint(0, 3, 300), 3)
    for G in (2, 3):
        with pytest.raises(RuntimeError, match='last view counts'):
            screen(1, G)
    ctx.colcounts_by_label(rng.randint(0, 5, N), np.arange(5))
    assert screen(0, 5).shape == (5, M)
    for G in (4, 6):
        with pytest.raises(RuntimeError, match='resident per-cluster counts'):
            screen(0, G)
    for cols in (M - 1, M + 1):
        with pytest.raises(RuntimeError, match='batch shape does not match'):
            screen(0, 5, cols)
    # the refusals left the resident counts usable
    assert screen(0, 5).shape == (5, M)


def test_mh_screen_guards_leave_the_element_to_the_host(ctxs, monkeypatch):
    """What the screen does not model is flagged 1, nothing else changes:
    U or u exactly 0, exactly 1 or NaN; sd_idx -1 or 8; old one float32 step
    outside [TMIN, TMAX]; and U = 1 where the proposal interval's upper tail
    (37 to 38.6 deviations out) has a subnormal mass, so that the inverse
    normal of it no longer lands on the bound.  Under BNPC_MH_SCREEN=2 no
    proposal is vouched for: the same flags with 3 read as 2."""
    M, K = 257, 9
    ctx = ctxs.get(M)
    _set_knobs(monkeypatch, ctx, {})
    rng = np.random.RandomState(47)
    n1, n0 = ctx.colcounts_by_label(rng.randint(0, K, ctx.N), np.arange(K))
    old = (n1 + .25) / (n1 + n0 + .5) + rng.normal(size=(K, M)) * 0.01
    old = np.clip(old, TMIN, TMAX).astype(np.float32)
    sd = np.array([0.1, 0.25, 0.5, 0.02])
    sd_idx = rng.randint(0, 3, (K, M)).astype(np.int32)
    U = rng.uniform(size=(K, M))
    u = rng.uniform(size=(K, M))

    def run(old, sd_idx, U, u):
        return ctx.mh_screen(0, old, sd, (sd_idx, U, u), TMIN, TMAX, .01, .2,
            .25, .25, False, with_theta=True)

    base, base32 = run(old, sd_idx, U, u)
    assert (base == 3).sum() > 50 and (base == 0).sum() > 50
    tmin32, tmax32 = np.float32(TMIN), np.float32(TMAX)
    guards = [('U', 0.0), ('U', 1.0), ('U', np.nan), ('u', 0.0), ('u', 1.0),
        ('u', np.nan), ('sd_idx', -1), ('sd_idx', 8),
        ('old', np.nextafter(tmin32, np.float32(-1))),
        ('old', np.nextafter(tmax32, np.float32(2)))]
    tails = np.arange(37.0, 38.65, 0.1)
    GM = K * M
    # the first and last element, both sides of block edges, the middle
    fixed = [0, 255, 256, 257, 511, 512, GM - 257, GM - 2, GM - 1]
    more = [i for i in rng.permutation(GM).tolist() if i not in fixed]
    at = rng.permutation(np.array(fixed + more)[:len(guards) * 2
        + tails.size])
    assert at.size == len(guards) * 2 + tails.size \
        and {0, GM - 1} <= set(at.tolist())
    arrays = {'old': old.copy(), 'sd_idx': sd_idx.copy(), 'U': U.copy(),
        'u': u.copy()}
    for i, (name, value) in enumerate(guards * 2):
        arrays[name].reshape(-1)[at[i]] = value
    for i, hi in enumerate(tails):
        j = at[2 * len(guards) + i]
        arrays['U'].reshape(-1)[j] = 1.0
        arrays['sd_idx'].reshape(-1)[j] = 3
        arrays['old'].reshape(-1)[j] = np.float32(float(tmax32) - hi * sd[3])
    assert arrays['old'].dtype == np.float32
    flags, new32 = run(**arrays)
    hit = np.zeros(GM, dtype=bool)
    hit[at] = True
    hit = hit.reshape(K, M)
    assert np.all(flags[hit] == 1), (flags[hit], at)
    assert np.array_equal(flags[~hit], base[~hit])
    keep = ~hit & (base == 3)
    assert np.array_equal(new32[keep].view(np.int32),
        base32[keep].view(np.int32))

    _set_knobs(monkeypatch, ctx, {'BNPC_MH_SCREEN': '2'})
    plain, _ = run(**arrays)
    assert not (plain == 3).any()
    assert np.array_equal(plain, np.where(flags == 3, 2, flags))
    plain0, _ = run(old, sd_idx, U, u)
    assert np.array_equal(plain0, np.where(base == 3, 2, base))
    _set_knobs(monkeypatch, ctx, {})
    again, again32 = run(**arrays)
    assert np.array_equal(again, flags)
    assert np.array_equal(again32[again == 3].view(np.int32),
        new32[flags == 3].view(np.int32))
