"""The sweep's hint records at every tie, rank and launch edge.

bnpc_ll_theta_pinned_top2 and its two halves in visiting order make, per row
of the matrix, the record a Gibbs sweep decides most cells from: the four
largest entries of ll + prior, the columns and log-likelihoods of the first
three, the weights e2 / e3 and row_here.  Up to 64 columns k_row_top2 makes it
(one thread per row, 256 rows per workgroup), above that k_row_top4_wave (one
wave per row, 4 rows per workgroup, 64 per-lane lists merged by an xor
butterfly).  Context.last_launch() reports the sums kernel, not the hint
kernel: which hint form ran follows from K alone (K <= 64 against K > 64, the
one branch of hint_launch), and every case checks that the evaluation that ran
was the one of its K columns.

The expected record is built here, in NumPy, from the matrix the call returns
and the prior (`reference`): value descending, first column on ties, third and
fourth rounded up to float32 - the contract of the kernel comments and of
include/bnpc_hip.h.  The prior is a free float64 input: with one parameter row
in every column all entries of a row are the same log-likelihood, so the
ranking - and every tie in it - is exactly that of the prior, and one launch
puts a chosen pattern into every row.  Each case first asserts, on the
reference alone, that the pattern it is meant to hold is there.

The unmarked tests run the CPU stand-in of the device (_lib.hints_from_matrix)
over the same patterns, on matrices built in NumPy.
"""
import collections
import ctypes as C

import numpy as np
import pytest

from bnpc_amd import _lib
import test_host_logic as H

FP, FN = 0.01, 0.2
N, M, MISS = 257, 40, 0.2
FAR = 300.0                     # columns not named: at least this far below
SENTINEL = -1234.5
KNOBS = ('BNPC_KW', 'BNPC_MSPLIT', 'BNPC_ZERO_COPY')
K_THREAD = (1, 2, 3, 4, 5, 63, 64)                          # k_row_top2
K_WAVE = (65, 66, 127, 128, 129, 321, 1024, 1025)           # k_row_top4_wave
K_MISSING = (5, 64, 65, 129)
K_FUZZ = (5, 13, 64, 65, 130, 321)
FUZZ_SEEDS = range(6)
HINT_THROUGH_MAX = 1024         # bnpc_ctx.h: rows up to here are written through
EXACT = ('best', 'second', 'third', 'fourth', 'col', 'col2', 'col3')
RANKS = (('ll_best', 'col'), ('ll_second', 'col2'), ('ll_third', 'col3'))


def hint_form(K):
    return 'k_row_top2' if K <= 64 else 'k_row_top4_wave'


# ------------------------------------------------------------ the reference
def f32_above(x):
    """float32 not below the float64 values: cast, one step up where the
    cast fell below; -inf stays -inf."""
    x = np.asarray(x, dtype=np.float64)
    f = x.astype(np.float32)
    low = f.astype(np.float64) < x
    f[low] = np.nextafter(f[low], np.float32(np.inf))
    assert np.all(f.astype(np.float64) >= x)
    return f


def reference(ll, prior):
    """The records of the first K = len(prior) columns of `ll`, as a dict of
    arrays (plus 'vals': the five largest entries in float64, -inf where
    there are fewer columns - for the cases' preconditions)."""
    prior = np.asarray(prior, dtype=np.float64)
    K = prior.size
    ll = np.asarray(ll, dtype=np.float64)[:, :K]
    n = ll.shape[0]
    rows = np.arange(n)
    post = ll + prior[None, :]
    cols = np.broadcast_to(np.arange(K), post.shape)
    rank = np.lexsort((cols, -post), axis=1)    # value down, then column up
    vals = np.full((n, 5), -np.inf)
    for r in range(min(5, K)):
        vals[:, r] = post[rows, rank[:, r]]
    w = {'vals': vals, 'best': vals[:, 0].copy(), 'second': vals[:, 1].copy(),
        'third': f32_above(vals[:, 2]), 'fourth': f32_above(vals[:, 3])}
    for r, (lik, col) in enumerate(RANKS):
        if r < K:
            c = rank[:, r]
            w[lik] = ll[rows, c]
            w[col] = np.where((vals[:, r] > -np.inf) | (r == 0), c, -1) \
                .astype(np.int16)
        else:
            w[lik] = np.zeros(n)
            w[col] = np.full(n, -1, dtype=np.int16)
    for e, lik, col in (('e2', 'll_second', 'col2'), ('e3', 'll_third',
            'col3')):
        w[e] = np.where(w[col] >= 0, np.exp(w[lik] - w['ll_best']), 0.0) \
            .astype(np.float32)
    with np.errstate(invalid='ignore'):
        w['row_here'] = ((w['fourth'].astype(np.float64) > w['second'] - 72.0)
            & (w['second'] > w['best'] - 48.0)
            & (3 < K <= HINT_THROUGH_MAX)).astype(np.int16)
    return w


def pick_rows(want, idx):
    return {name: a[idx] for name, a in want.items()}


def _same(got, want, what, name):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, name, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert not bad.size, (f'{what}: {name} differs in {bad.size} of '
        f'{want.size} rows, first row {bad[0]}: {got[bad[0]]!r} vs '
        f'{want[bad[0]]!r}')


def check_records(hint, want, what, row_here=True, empty_rows=True):
    """Every field of the records against the reference.  empty_rows=False:
    ll_best is not compared in rows whose every entry is -inf (see
    test_placement_patterns)."""
    n = want['best'].size
    assert hint is not None and hint.size == n, (what, n)
    for name in EXACT + (('row_here',) if row_here else ()):
        _same(hint[name], want[name], what, name)
    for lik, col in RANKS:
        there = want[col] >= 0
        if lik == 'll_best' and not empty_rows:
            there = there & (want['best'] > -np.inf)
        _same(hint[lik][there], want[lik][there], what, lik)
    for e, col in (('e2', 'col2'), ('e3', 'col3')):
        there = want[col] >= 0
        assert np.all(hint[e][~there] == 0), (what, e)
        # (float32 of the device's exp(): the sweep loop allows 2.5e-7, a
        # quarter of its band of 1e-6; float32 denormals: absolute)
        np.testing.assert_allclose(hint[e][there], want[e][there],
            rtol=2.5e-7, atol=1e-37, err_msg=f'{what}: {e}')


# ----------------------------------------------------------- the patterns
Pattern = collections.namedtuple('Pattern', 'name prior cols eq gt')
# cols: the expected (col, col2, col3), None = not stated; eq / gt: pairs
# (i, j) of ranks whose float64 values must be equal / strictly descending


def far(K):
    """distinct priors far below everything a pattern names"""
    return -(FAR + 0.01 * np.arange(K))


def placed(K, cols, values, rest=None):
    p = far(K) if rest is None else np.full(K, rest, dtype=np.float64)
    assert len(set(cols)) == len(cols) and max(cols) < K and min(cols) >= 0
    p[list(cols)] = values
    return p


def _descending(k):
    return [(i, i + 1) for i in range(k - 1)]


def placement_patterns(K):
    """The patterns of one K, each where K has room for it."""
    out = []

    def add(name, prior, cols, eq=(), gt=()):
        cols = tuple(cols)[:3] + (None,) * (3 - len(tuple(cols)[:3]))
        out.append(Pattern(name, prior, cols, tuple(eq), tuple(gt)))

    t = min(4, K)
    down = -np.arange(t, dtype=np.float64)
    # the four largest by column, values falling / rising: no insert shifts
    # the list, or every insert does
    low, high = list(range(t)), list(range(K - t, K))
    # (the last named one lies above whatever follows it: -inf if nothing)
    add('order-falling-low', placed(K, low, down), low,
        gt=_descending(t + 1))
    add('order-rising-high', placed(K, high, down[::-1]), high[::-1],
        gt=_descending(t + 1))
    if K > 4:
        add('order-rising-low', placed(K, low, down[::-1]), low[::-1],
            gt=_descending(t + 1))
        add('order-falling-high', placed(K, high, down), high,
            gt=_descending(t + 1))
    # all K equal
    add('full-tie', np.zeros(K), range(min(3, K)),
        eq=_descending(min(5, K)), gt=[(min(5, K) - 1, min(5, K))][:K < 5])
    # two columns tie for first place: the lower one is col
    pairs = [(0, 1), (1, 2), (31, 32), (62, 63), (0, K - 1), (0, 32)]
    if K > 64:      # one lane's own list (k, k + 64); across the strides
        pairs += [(63, 64), (0, 64), (5, 69)]
    for a, b in sorted(set(pairs)):
        if a < b < K:
            add(f'tie-first-{a}-{b}', placed(K, (a, b), 0.0), (a, b),
                eq=[(0, 1)], gt=[(1, 2)] if K > 2 else [])
    triples = [(0, K // 2, K - 1), (3, 67, 131), (0, 16, 32)]
    for tr in sorted(set(triples)):
        if tr[0] < tr[1] < tr[2] < K:
            add('tie-first-three-%d-%d-%d' % tr, placed(K, tr, 0.0), tr,
                eq=[(0, 1), (1, 2)], gt=[(2, 3)] if K > 3 else [])
    if K >= 3:      # second and third
        for a, b in sorted({(0, max(1, K // 2)), (0, 64), (1, 33)}):
            if a < b < (K - 1 if K < 5 else K - 2):
                cols, vals = [K - 1, a, b], [0.0, -1.0, -1.0]
                if K >= 5:
                    cols, vals = cols + [K - 2], vals + [-2.0]
                add(f'tie-second-third-{a}-{b}', placed(K, cols, vals),
                    cols, eq=[(1, 2)], gt=[(0, 1)] + ([(2, 3)] if K > 3
                    else []))
    if K >= 4:      # third and fourth: the lower column is col3
        for a, b in sorted({(1, K - 2), (1, 65), (2, 34)}):
            if a < b < K - 1:
                add(f'tie-third-fourth-{a}-{b}', placed(K, [K - 1, 0, a, b],
                    [0.0, -1.0, -2.0, -2.0]), [K - 1, 0, a],
                    eq=[(2, 3)], gt=[(0, 1), (1, 2)] + ([(3, 4)] if K > 4
                    else []))
    if K >= 5:      # fourth and fifth: the fourth is a value only
        for a, b in sorted({(2, K - 2), (2, 66), (3, 35)}):
            if a < b < K - 1:
                add(f'tie-fourth-fifth-{a}-{b}', placed(K, [K - 1, 0, 1, a,
                    b], [0.0, -1.0, -2.0, -3.0, -3.0]), [K - 1, 0, 1],
                    eq=[(3, 4)], gt=[(0, 1), (1, 2), (2, 3)])
    if K == 321:    # five of one lane's five columns: its list overflows
        lane7 = [7, 71, 135, 199, 263]
        five = -np.arange(5, dtype=np.float64)
        add('lane-overflow-falling', placed(K, lane7, five), lane7,
            gt=_descending(5))
        add('lane-overflow-rising', placed(K, lane7, five[::-1]),
            lane7[::-1], gt=_descending(5))
    if K >= 49:     # one entry per quarter of the wave
        q = [0, 16, 32, 48]
        add('quarters-falling', placed(K, q, down), q, gt=_descending(4))
        add('quarters-rising', placed(K, q, down[::-1]), q[::-1],
            gt=_descending(4))
    if K in K_MISSING:
        for m in (1, 2, 3):
            fin = -np.arange(m, dtype=np.float64)
            gone = [(i, i + 1) for i in range(m, 4)]    # -inf == -inf
            none = [-1] * (3 - m)           # the ranks that are not there
            low, high = list(range(m)), list(range(K - m, K))
            add(f'finite-{m}-low', placed(K, low, fin, -np.inf), low + none,
                eq=gone, gt=_descending(m + 1))
            add(f'finite-{m}-high', placed(K, high, fin, -np.inf),
                high + none, eq=gone, gt=_descending(m + 1))
            add(f'finite-{m}-high-rising', placed(K, high, fin[::-1],
                -np.inf), high[::-1] + none, eq=gone, gt=_descending(m + 1))
        add('all-minus-inf', np.full(K, -np.inf), [0, -1, -1],
            eq=_descending(5))
    return out


def assert_pattern(want, pat, K, what):
    """The pattern is there, in every row, on the reference alone."""
    v = want['vals']
    for name, c in zip(('col', 'col2', 'col3'), pat.cols):
        assert c is None or np.all(want[name] == c), (what, name, c,
            want[name][:4])
    assert pat.eq or pat.gt, what
    for i, j in pat.eq:
        assert np.all(v[:, i] == v[:, j]), (what, 'eq', i, j)
    for i, j in pat.gt:
        assert np.all(v[:, i] > v[:, j]), (what, 'gt', i, j)
    if (2, 3) in pat.eq:
        _same(want['fourth'], want['third'], what, 'fourth == third')
    if pat.name == 'all-minus-inf':
        for name in ('best', 'second', 'third', 'fourth'):
            assert np.all(want[name] == -np.inf), (what, name)
        assert np.all(want['e2'] == 0) and np.all(want['e3'] == 0), what


THROUGH = [(g2, g4) for g2 in (47.5, 48.5) for g4 in (71.5, 72.5)]
THROUGH_CASES = [(K, g2, g4) for K in (13, 130) for g2, g4 in THROUGH] \
    + [(1024, 47.5, 71.5), (1025, 47.5, 71.5)]


def through_prior(K, g2, g4):
    """the runner-up g2 below the best, the fourth g4 below the runner-up:
    the two thresholds (48, 72) of a written-through row, one each side"""
    return placed(K, [K - 1, 0, K // 2, 1],
        [0.0, -g2, -g2 - 1.0, -g2 - g4])


def through_expected(K, g2, g4):
    return int(g2 < 48 and g4 < 72 and 3 < K <= HINT_THROUGH_MAX)


def assert_through(want, K, g2, g4, what):
    v = want['vals']
    assert np.all(v[:, 0] > v[:, 1]) and np.all(v[:, 1] > v[:, 2]) \
        and np.all(v[:, 2] > v[:, 3]) and np.all(v[:, 3] > v[:, 4] + 100), what
    for name, c in zip(('col', 'col2', 'col3'), (K - 1, 0, K // 2)):
        assert np.all(want[name] == c), (what, name)
    assert np.all(want['row_here'] == through_expected(K, g2, g4)), \
        (what, np.bincount(want['row_here']))


# -------------------------------------------- parameters and host matrices
_POOL = np.clip(np.random.RandomState(5).uniform(size=(3, M)), 1e-5,
    1 - 1e-5).astype(np.float32)


def uniform_theta(K, row=0):
    return np.ascontiguousarray(np.broadcast_to(_POOL[row], (K, M)))


def fuzz_case(K, seed):
    """(pool row of every column, prior): at most 9 distinct values a row.
    (13 columns over 3 x 3 values leave third == fourth in a sixth of the
    rows of some seeds: two parameter rows there, 6 values)"""
    rng = np.random.RandomState(1000 * K + seed)
    pool = 2 if K == 13 else 3
    return rng.randint(0, pool, K), -rng.randint(0, 3, K).astype(np.float64)


def fuzz_sparse_case(K, seed):
    """The same draw on 12 columns of K >= 64, the others far below: with
    ten columns and more per value the plain draw ties the four largest in
    nearly every row, all on one parameter row; here the ranks are taken by
    different parameter rows again."""
    rng = np.random.RandomState(2000 * K + seed)
    live = rng.permutation(K)[:12]
    pick, prior = rng.randint(0, 3, K), far(K)
    prior[live] = -rng.randint(0, 3, 12).astype(np.float64)
    return pick, prior


def fuzz_cases(K):
    for seed in FUZZ_SEEDS:
        yield f'K={K} seed={seed}', fuzz_case(K, seed), True
    if K >= 64:
        for seed in FUZZ_SEEDS:
            yield f'K={K} sparse seed={seed}', fuzz_sparse_case(K, seed), False


def assert_tie_dense(want, K, what, dense=True):
    v = want['vals']
    first = np.mean(v[:, 0] == v[:, 1])
    low = np.mean(want['third'] == want['fourth'])
    if dense and K >= 13:
        assert first >= 0.25 and low >= 0.25, (what, first, low)
    return first, low, np.mean((want['ll_best'] != want['ll_second'])
        | (want['ll_second'] != want['ll_third']))


def assert_fuzz_is_mixed(stats, K):
    """over the seeds of one K: rows that tie for first and rows that do
    not, and records whose three log-likelihoods are not all one value"""
    first, low, mixed = (np.array(x) for x in zip(*stats))
    assert first.max() > 0 and first.min() < 1, (K, first)
    assert low.max() > 0, (K, low)
    assert mixed.max() > 0, (K, mixed)


_data = {}


def data_matrix():
    if 'x' not in _data:
        _data['x'] = H.synth(N + M, N, M, 10, MISS)
    return _data['x']


def host_pool_ll(rows):
    """the pool's three columns for the first `rows` cells, in NumPy"""
    x = data_matrix()[:rows]
    t64 = _POOL.astype(np.float64)
    om64 = (1 - _POOL).astype(np.float64)
    L1 = np.log(t64 * (1 - FN) + om64 * FP)
    L0 = np.log(t64 * FN + om64 * (1 - FP))
    out = np.empty((rows, 3))
    for k in range(3):
        out[:, k] = np.where(x == 1, L1[k], np.where(x == 0, L0[k], 0.0)) \
            .sum(axis=1)
    return out


# ------------------------------------------------------- CPU (stand-in)
CPU_ROWS = 33


@pytest.mark.parametrize('K', K_THREAD + K_WAVE)
def test_stand_in_placement_patterns(K):
    """_lib.hints_from_matrix on every placement pattern equals the
    reference in every field; every pattern's precondition holds."""
    ll = np.repeat(host_pool_ll(CPU_ROWS)[:, :1], K, axis=1)
    pats = placement_patterns(K)
    assert pats
    for pat in pats:
        what = f'K={K} {pat.name}'
        want = reference(ll, pat.prior)
        assert_pattern(want, pat, K, what)
        check_records(_lib.hints_from_matrix(ll, pat.prior), want, what,
            row_here=False)


def test_placement_patterns_reach_what_they_name():
    """every family of patterns is present at the sizes that have room"""
    names = {K: {p.name for p in placement_patterns(K)}
        for K in K_THREAD + K_WAVE + K_MISSING}
    for K in K_THREAD + K_WAVE:
        assert 'full-tie' in names[K] and 'order-falling-low' in names[K]
        if K >= 2:
            assert 'tie-first-0-1' in names[K]
            assert f'tie-first-0-{K - 1}' in names[K]
        if K >= 4:
            assert any(s.startswith('tie-third-fourth') for s in names[K])
            assert any(s.startswith('tie-first-three') for s in names[K])
            assert any(s.startswith('tie-second-third') for s in names[K])
        if K >= 5:
            assert any(s.startswith('tie-fourth-fifth') for s in names[K])
        if K >= 63:
            assert {'tie-first-31-32', 'tie-first-0-32', 'quarters-rising',
                'quarters-falling'} <= names[K]
        if K >= 64:
            assert 'tie-first-62-63' in names[K]
        if K > 69:
            assert {'tie-first-63-64', 'tie-first-0-64', 'tie-first-5-69'} \
                <= names[K]
    assert {'lane-overflow-falling', 'lane-overflow-rising'} <= names[321]
    for K in K_MISSING:
        assert {'all-minus-inf', 'finite-1-low', 'finite-2-high',
            'finite-3-high-rising'} <= names[K]


@pytest.mark.parametrize('K', K_FUZZ)
def test_stand_in_tie_dense_fuzz(K):
    pool = host_pool_ll(N)
    stats = []
    for what, (pick, prior), dense in fuzz_cases(K):
        ll = pool[:, pick]
        want = reference(ll, prior)
        stats.append(assert_tie_dense(want, K, what, dense))
        check_records(_lib.hints_from_matrix(ll, prior), want, what,
            row_here=False)
    assert_fuzz_is_mixed(stats, K)


def test_stand_in_write_through_patterns():
    """the stand-in makes no row_here; the rest of the record on the
    write-through patterns, and both outcomes among the expected ones"""
    seen = set()
    for K, g2, g4 in THROUGH_CASES:
        ll = np.repeat(host_pool_ll(CPU_ROWS)[:, :1], K, axis=1)
        prior = through_prior(K, g2, g4)
        what = f'K={K} g2={g2} g4={g4}'
        want = reference(ll, prior)
        assert_through(want, K, g2, g4, what)
        seen.add(int(want['row_here'][0]))
        check_records(_lib.hints_from_matrix(ll, prior), want, what,
            row_here=False)
    assert seen == {0, 1}


def test_reference_rounds_third_and_fourth_up():
    x = np.array([-np.inf, -1.0, -0.1, -100.30000000000001, -1e-300, 3.3])
    f = f32_above(x)
    assert f[0] == -np.inf and f[1] == -1.0
    assert np.all(f.astype(np.float64) >= x)
    assert np.all(np.nextafter(f[1:], np.float32(-np.inf))
        .astype(np.float64) < x[1:])


# ------------------------------------------------------------- the device
class _Dev:
    def __init__(self):
        self.data = data_matrix()
        self.ctx = _lib.Context(data=self.data)
        self.lib = _lib.load()

    def knobs(self, monkeypatch):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        self.ctx.reload_options()

    def hinted(self, view, theta, ld, prior):
        """one hinted call: (matrix [:, :K], records), both copied"""
        K = theta.shape[0]
        ll, hint = self.ctx.ll_theta_pinned_top2(view, theta, FP, FN, ld,
            prior)
        assert self.ctx.last_launch()[1] == K
        assert hint is not None, 'no hint buffer: zero-copy memory missing'
        hint = hint.copy()
        self.ctx.matrix_wait()
        return ll[:, :K].copy(), hint

    def lazy_next(self, view, K, ld):
        """A hinted call of the shape of the one that follows, on other
        parameters, with no matrix_wait() after it: the next call is then
        not eager (ll_top2_impl: matrix_eager = lazy_fetched).  Its matrix -
        the pinned buffer the next call fills - is left full of a sentinel;
        returns that view."""
        ll, _ = self.ctx.ll_theta_pinned_top2(view, uniform_theta(K, 1), FP,
            FN, ld, np.zeros(K))
        self.ctx.sync()         # (a copy that call may have queued is over)
        ll[:] = SENTINEL
        return ll


@pytest.fixture(scope='module')
def dev():
    d = _Dev()
    yield d
    d.ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize('K', K_THREAD + K_WAVE)
def test_placement_patterns(K, dev, monkeypatch):
    """Section 1: one parameter row in every column, the ranking set by the
    prior; k_row_top2 for K <= 64, k_row_top4_wave above (by K alone).

    Known and left open: on a row whose every entry is -inf k_row_top2 takes
    no branch and leaves ll_best = 0.0 beside col = 0, where k_row_top4_wave
    and _lib.hints_from_matrix give column 0's log-likelihood.  A sweep's
    priors are finite, so no sweep meets such a row.  Up to 64 columns the
    all-minus-inf case therefore checks every field but ll_best; above, all
    of them."""
    dev.knobs(monkeypatch)
    theta = uniform_theta(K)
    pats = placement_patterns(K)
    print(f'\n[hint form] K={K}: {hint_form(K)}, {len(pats)} patterns')
    for i, pat in enumerate(pats):
        what = f'{hint_form(K)} K={K} {pat.name}'
        ll, hint = dev.hinted(0, theta, K + 3, pat.prior)
        if i == 0:
            assert np.array_equal(ll, dev.ctx.ll_theta(0, theta, FP, FN)), what
            assert np.all(ll == ll[:, :1]), what    # one value per row
        want = reference(ll, pat.prior)
        assert_pattern(want, pat, K, what)
        check_records(hint, want, what, empty_rows=K > 64)


@pytest.mark.gpu
def test_last_column_of_an_int16(dev, monkeypatch):
    """K = HINT_COLS_MAX = 32767 on a gathered view of 5 rows: column 32766
    wins alone, and loses an exact tie to column 100; one more column is
    refused."""
    dev.knobs(monkeypatch)
    K = _lib.HINT_COLS_MAX
    assert K == 32767
    ctx = dev.ctx
    cells = np.array([5, 200, 5, 256, 0])
    ctx.view_set(1, cells)
    theta = uniform_theta(K)
    for tie in (False, True):
        what = f'K={K} tie={tie}'
        prior = placed(K, [K - 1, 100] if tie else [K - 1], 0.0)
        ll, hint = dev.hinted(1, theta, K, prior)
        assert ll.shape == (5, K)
        if not tie:
            assert np.array_equal(ll, ctx.ll_theta(1, theta, FP, FN)), what
        want = reference(ll, prior)
        assert np.all(want['col'] == (100 if tie else K - 1)), what
        assert np.all(want['col2'] == (K - 1 if tie else 0)), what
        assert np.all((want['best'] == want['second']) == tie), what
        assert np.all(want['row_here'] == 0), what
        check_records(hint, want, what)
    # one more column
    theta = uniform_theta(K + 1)
    prior = np.zeros(K + 1)
    host_p, hint_p = C.POINTER(C.c_double)(), C.c_void_p()
    assert dev.lib.bnpc_ll_theta_pinned_top2(ctx._h, 1,
        _lib.ptr(theta, C.c_float), K + 1, FP, FN, K + 1, _lib.ptr(prior),
        C.byref(host_p), C.byref(hint_p)) == 2
    assert 'K out of range' in dev.lib.bnpc_last_error().decode()
    assert not hint_p.value
    ctx.sync()


@pytest.mark.gpu
@pytest.mark.parametrize('K', K_FUZZ)
def test_tie_dense_fuzz(K, dev, monkeypatch):
    """Section 2: columns drawn from three parameter rows, priors from
    {0, -1, -2}: ties at different ranks in different rows, and the
    log-likelihoods must follow their columns."""
    dev.knobs(monkeypatch)
    stats = []
    for what, (pick, prior), dense in fuzz_cases(K):
        theta = np.ascontiguousarray(_POOL[pick])
        what = f'{hint_form(K)} {what}'
        ll, hint = dev.hinted(0, theta, K + 3, prior)
        if not stats:
            assert np.array_equal(ll, dev.ctx.ll_theta(0, theta, FP, FN)), what
        want = reference(ll, prior)
        stats.append(assert_tie_dense(want, K, what, dense))
        check_records(hint, want, what)
    assert_fuzz_is_mixed(stats, K)


@pytest.mark.gpu
@pytest.mark.parametrize('K', (13, 130))
def test_row_count_edges_on_gathered_views(K, dev, monkeypatch):
    """Section 3: 256 rows per workgroup (thread form), 4 per workgroup (wave
    form): views of 1, 3, 4, 5, 255, 256 and 257 rows with repeated cells,
    rows of K and of K + 3 entries."""
    dev.knobs(monkeypatch)
    ctx = dev.ctx
    pick, prior = fuzz_case(K, 0)
    theta = np.ascontiguousarray(_POOL[pick])
    whole = ctx.ll_theta(0, theta, FP, FN)
    rng = np.random.RandomState(K)
    for n in (1, 3, 4, 5, 255, 256, 257):
        cells = rng.randint(0, N, n)
        if n > 1:
            cells[-1] = cells[0]            # a cell twice
        ctx.view_set(1, cells)
        for ld in (K, K + 3):
            what = f'{hint_form(K)} K={K} n={n} ld={ld}'
            ll, hint = dev.hinted(1, theta, ld, prior)
            assert ll.shape == (n, K) and hint.size == n, what
            if (n, ld) == (257, K):
                assert np.array_equal(ll, whole[cells]), what
            want = reference(ll, prior)
            check_records(hint, want, what)
            if n > 1:
                for name in hint.dtype.names:
                    assert hint[name][-1] == hint[name][0], (what, name)


@pytest.mark.gpu
@pytest.mark.parametrize('K,g2,g4', THROUGH_CASES)
def test_write_through_on_both_sides_of_its_thresholds(K, g2, g4, dev,
        monkeypatch):
    """Section 4: row_here = 1 in every row exactly where the runner-up is
    within 48 of the best, the fourth within 72 of the runner-up and
    3 < K <= 1024; those rows are in the host matrix when the call returns,
    on a call that does not copy the matrix by itself."""
    dev.knobs(monkeypatch)
    ctx = dev.ctx
    theta = uniform_theta(K)
    prior = through_prior(K, g2, g4)
    what = f'{hint_form(K)} K={K} g2={g2} g4={g4}'
    full = ctx.ll_theta(0, theta, FP, FN)
    stale = dev.lazy_next(0, K, K + 3)
    ll, hint = ctx.ll_theta_pinned_top2(0, theta, FP, FN, K + 3, prior)
    # (the same pinned buffer: ensure_pin has not reallocated it)
    assert ll.ctypes.data == stale.ctypes.data and ll.shape == stale.shape
    hint = hint.copy()
    here = hint['row_here'] == 1
    early = ll[here, :K].copy()
    ctx.matrix_wait()
    late = ll[:, :K].copy()
    want = reference(late, prior)
    assert_through(want, K, g2, g4, what)
    check_records(hint, want, what)
    assert here.all() == bool(through_expected(K, g2, g4)), what
    assert np.array_equal(early, full[here]), what
    assert np.array_equal(late, full), what


def _orders(n, rng):
    return (('identity', np.arange(n)), ('reversed', np.arange(n)[::-1]),
        ('random', rng.permutation(n)))


def in_order_case(K):
    """(pool row of every column, prior): the best on parameter row 0, the
    runner-up 48 below it on parameter row 1 - within reach or not by the
    sign of the row's difference between the two, so rows on both sides of
    the write-through threshold -, third and fourth tied."""
    pick = fuzz_case(K, 1)[0]
    cols = [K - 1, 1, 2, K // 2]
    pick[cols] = [0, 1, 0, 0]
    return pick, placed(K, cols, [0.0, -48.0, -60.0, -60.0])


@pytest.mark.gpu
@pytest.mark.parametrize('K', (13, 130))
def test_records_in_visiting_order(K, dev, monkeypatch):
    """Section 5 (bnpc_ll_theta_pinned_sums_issue + bnpc_hints_in_order_issue):
    record r is the reference's record of row order[r]; row_here and the
    written-through rows land at the rows' own places."""
    dev.knobs(monkeypatch)
    ctx = dev.ctx
    pick, prior = in_order_case(K)
    theta = np.ascontiguousarray(_POOL[pick])
    rng = np.random.RandomState(50 + K)
    small = np.array([9, 256, 9, 0, 131])
    ctx.view_set(1, small)
    outcomes = set()
    for view, n in ((0, N), (1, small.size)):
        full = ctx.ll_theta(view, theta, FP, FN)
        want = reference(full, prior)
        assert np.all(want['third'] == want['fourth'])
        outcomes |= set(want['row_here'].tolist())
        for kind, order in _orders(n, rng):
            what = f'{hint_form(K)} K={K} n={n} {kind}'
            stale = dev.lazy_next(view, K, K + 3)
            ll, hint = ctx.ll_theta_pinned_top2_in_order(view, theta, FP, FN,
                K + 3, prior, order)
            assert ll.ctypes.data == stale.ctypes.data, what
            assert ctx.last_launch()[1] == K
            hint = hint.copy()
            here = np.zeros(n, dtype=bool)
            here[order] = hint['row_here'] == 1
            early = ll[here, :K].copy()
            ctx.matrix_wait()
            assert np.array_equal(ll[:, :K], full), what
            check_records(hint, pick_rows(want, order), what)
            _same(here, want['row_here'] == 1, what, 'row_here by row')
            assert np.array_equal(early, full[here]), what
    assert outcomes == {0, 1}, outcomes
    # more rows than cells: the second half is refused
    ctx.view_set(1, np.r_[np.arange(N), 0])
    ctx.ll_theta_pinned_sums_issue(1, theta, FP, FN, K + 3, prior)
    with pytest.raises(RuntimeError, match='more rows than cells'):
        ctx.hints_in_order_issue(np.arange(N + 1))
    ctx.sync()
