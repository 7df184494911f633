"""Every launch form of the cells x clusters x mutations sum (-m gpu), each
reached on purpose and compared with the strict-order reference over its
WHOLE output.

`ll_common` (bnpc_kernels.hip) picks a table builder (k_tables_theta_flat,
k_tables_theta or k_tables_relayout) and a sums kernel (k_ll_seqp, k_ll<KW>,
k_ll8_asm<1|2, split?>, k_ll8_lds<2>, with or without k_ll_combine) from the
shape and the knobs.  Each case below names the form it is meant to reach and
first checks, through Context.last_launch(), that this form ran: when a
threshold is retuned, the case must be re-aimed (new shape or knobs), not
dropped.  Then:
  * caller-built tables (ll_tables): bit for bit the strict-order sums;
  * device-built tables, unsplit: 1e-12 against the strict-order sums over
    NumPy-built tables, and bit for bit the same evaluation under another
    forced cluster tile;
  * device-built tables, split over the mutations: 1e-12 on every entry, and
    the same bits on a second call;
  * every form: a gathered view of permuted and repeated cells gives the
    matching rows (the same bits, the same form running), and an output with
    ld > K keeps a sentinel in columns K..ld, on both the in-place host
    result and the device-buffer result.

The tile hint records of k_row_top2_wide are checked field by field against
the matrix they come with.
"""
import collections

import numpy as np
import pytest

from bnpc_amd import _lib
from oracle import seqsum as S
import test_host_logic as H

pytestmark = pytest.mark.gpu

FP, FN = 0.01, 0.2
SENTINEL = -1234.5
ZC_OUT_MAX = 512 << 10          # in-place host results up to this size

# name -> (cells, mutations, missing share)
MATS = {
    'm64x40': (64, 40, 0.2),
    'm130x130': (130, 130, 0.2),
    'm1000x333': (1000, 333, 0.2),
    'm2000x300': (2000, 300, 0.2),
    'm4100x1003': (4100, 1003, 0.2),
    'm5000x1000': (5000, 1000, 0.2),
    'm20000x3100': (20000, 3100, 0.2),
}

Case = collections.namedtuple('Case',
    'mat view K entry knobs form ms builder edge')
# view: None = the whole matrix (view 0), or (n, seed) = n cells drawn with
# repeats from the matrix (view 1).  builder: the table builder the shape
# implies (not reported by last_launch; kept for the reader).
CASES = [
    Case('m1000x333', None, 37, 'tables', {}, 'k_ll_seqp', 1, '-',
        'caller tables, strict order'),
    Case('m1000x333', None, 37, 'tables', {'BNPC_KW': '1'}, 'k_ll<1>', 1,
        'k_tables_relayout', 'forced narrow tile'),
    Case('m1000x333', None, 37, 'tables', {'BNPC_KW': '8'},
        'k_ll8_asm<1, false>', 1, 'k_tables_relayout', 'one block per wave'),
    Case('m1000x333', None, 1, 'theta', {}, 'k_ll<1> + k_ll_combine', 21,
        'k_tables_theta_flat', 'one cluster, split'),
    Case('m64x40', None, 9, 'theta', {}, 'k_ll8_asm<1, true>', 3,
        'k_tables_theta_flat', 'MS < 4: one partial plane, no combine'),
    Case('m130x130', None, 5, 'theta', {},
        'k_ll8_asm<1, true> + k_ll_combine', 9, 'k_tables_theta_flat',
        'MS % 4 != 0, K % 8 != 0'),
    Case('m5000x1000', None, 200, 'theta', {}, 'k_ll8_asm<2, true>', 4,
        'k_tables_theta_flat', 'one chunk quad: the sum lands in place'),
    Case('m5000x1000', None, 14, 'theta', {},
        'k_ll8_asm<2, true> + k_ll_combine', 42, 'k_tables_theta_flat',
        'ragged nblk (79) and K'),
    Case('m4100x1003', None, 61, 'theta', {},
        'k_ll8_asm<2, true> + k_ll_combine', 32, 'k_tables_theta_flat',
        'nblk % 8 = 1, K % 8 = 5, M % 8 = 3'),
    Case('m5000x1000', (20000, 7), 210, 'theta', {}, 'k_ll8_asm<2, false>',
        1, 'k_tables_theta_flat', 'no split from 8192 waves (8451)'),
    Case('m5000x1000', None, 3151, 'theta', {}, 'k_ll8_asm<2, false>', 1,
        'k_tables_theta', 'K % 8 = 7, non-flat builder'),
    Case('m5000x1000', None, 3151, 'tables', {'BNPC_KW': '8'},
        'k_ll8_asm<2, false>', 1, 'k_tables_relayout', 'K % 8 = 7'),
    Case('m20000x3100', None, 1203, 'tables', {'BNPC_KW': '8'},
        'k_ll8_lds<2>', 1, 'k_tables_relayout',
        'K % 8 = 3, nblk % 8 = 1 (idle waves)'),
    Case('m20000x3100', None, 1203, 'theta', {}, 'k_ll8_lds<2>', 1,
        'k_tables_theta', 'K % 8 = 3, nblk % 8 = 1 (idle waves)'),
    Case('m2000x300', None, 2, 'theta', {'BNPC_MSPLIT': '0'}, 'k_ll<2>', 1,
        'k_tables_theta_flat', 'narrow tile, unsplit'),
    Case('m2000x300', None, 4, 'theta', {'BNPC_MSPLIT': '0'}, 'k_ll<4>', 1,
        'k_tables_theta_flat', 'narrow tile, unsplit'),
]
KNOBS = ('BNPC_KW', 'BNPC_MSPLIT', 'BNPC_ZERO_COPY')


def _case_id(c):
    knobs = ','.join(f'{k[5:]}={v}' for k, v in c.knobs.items())
    view = f'-view{c.view[0]}' if c.view else ''
    return f'{c.mat}{view}-K{c.K}-{c.entry}' + (f'-{knobs}' if knobs else '')


class _Mats:
    """Matrices, contexts and references, each built once per module."""

    def __init__(self):
        self.data, self.ctx, self.ref = {}, {}, {}

    def matrix(self, name):
        if name not in self.data:
            N, M, miss = MATS[name]
            self.data[name] = H.synth(N + M, N, M, 10, miss)
            self.ctx[name] = _lib.Context(data=self.data[name])
        return self.data[name], self.ctx[name]

    @staticmethod
    def theta(M, K):
        rng = np.random.RandomState(7 * K + M)
        return np.clip(rng.uniform(size=(K, M)), 1e-5, 1 - 1e-5) \
            .astype(np.float32)

    def reference(self, name, K, view):
        """(cells, strict-order sums over NumPy-built tables for them)"""
        key = (name, K, view)
        if key not in self.ref:
            data, _ = self.matrix(name)
            N, M = data.shape
            cells = np.arange(N) if view is None \
                else np.random.RandomState(view[1]).randint(0, N, view[0])
            L1, L0 = host_tables(self.theta(M, K))
            self.ref[key] = (cells, S.table_sums(data[cells], L1, L0))
        return self.ref[key]

    def close(self):
        for ctx in self.ctx.values():
            ctx.close()


@pytest.fixture(scope='module')
def mats():
    assert S._LIB is not None, \
        'oracle/_build/liboracle_seqsum.so missing: run make -C oracle'
    m = _Mats()
    yield m
    m.close()


def host_tables(theta):
    t64 = theta.astype(np.float64)
    om64 = (1 - theta).astype(np.float64)
    return (np.log(t64 * (1 - FN) + om64 * FP),
        np.log(t64 * FN + om64 * (1 - FP)))


def _set_knobs(monkeypatch, ctx, knobs):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    ctx.reload_options()


def _evaluate(ctx, case, view, theta, tables, out=None):
    if case.entry == 'tables':
        return ctx.ll_tables(view, tables[0], tables[1], out=out)
    return ctx.ll_theta(view, theta, FP, FN, out=out)


def _assert_form(ctx, case, where):
    name, K, ms = ctx.last_launch()
    assert (name, K, ms) == (case.form, case.K, case.ms), (
        f'{_case_id(case)} ({where}) ran {name!r} with {ms} mutation '
        f'chunk(s), not {case.form!r} with {case.ms}: the dispatcher changed '
        f'- re-aim this case (shape or knobs) at the form it is meant to '
        f'cover ({case.edge}) instead of dropping it')
    return name, ms


def _first_difference(got, want):
    bad = np.argwhere(got != want)
    if not bad.size:
        return ''
    r, k = bad[0]
    return (f'{len(bad)} entries differ, first [{r}, {k}]: '
        f'{got[r, k]!r} vs {want[r, k]!r}')


@pytest.mark.parametrize('case', CASES, ids=_case_id)
def test_launch_form_whole_output(case, mats, monkeypatch):
    data, ctx = mats.matrix(case.mat)
    N, M = data.shape
    cells, want = mats.reference(case.mat, case.K, case.view)
    n = cells.size
    theta = mats.theta(M, case.K)
    tables = host_tables(theta)
    view = 0
    if case.view is not None:
        view = 1
        ctx.view_set(view, cells)
    _set_knobs(monkeypatch, ctx, case.knobs)

    got = _evaluate(ctx, case, view, theta, tables)
    form = _assert_form(ctx, case, 'first call')
    print(f'\n[form] {_case_id(case)}: last_launch {form[0]!r}, '
        f'{form[1]} chunk(s); builder {case.builder}; {case.edge}')
    assert got.shape == (n, case.K)
    if case.entry == 'tables':
        assert np.array_equal(got, want), _first_difference(got, want)
    else:
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)

    # the same call again, into rows of ld > K: columns K..ld keep the
    # sentinel; in-place host result and device buffer alike
    routes = [None]
    if n * (case.K + 5) * 8 <= ZC_OUT_MAX:
        routes.append('0')          # BNPC_ZERO_COPY=0: the device buffer
    for zc in routes:
        knobs = dict(case.knobs)
        if zc is not None:
            knobs['BNPC_ZERO_COPY'] = zc
        _set_knobs(monkeypatch, ctx, knobs)
        out = np.full((n, case.K + 5), SENTINEL)
        _evaluate(ctx, case, view, theta, tables, out=out)
        _assert_form(ctx, case, f'ld = K + 5, zero copy {zc or "default"}')
        assert np.array_equal(out[:, :case.K], got), \
            _first_difference(out[:, :case.K], got)
        assert np.all(out[:, case.K:] == SENTINEL)
    _set_knobs(monkeypatch, ctx, case.knobs)

    # a gathered view of the same size: the cells permuted, with repeats
    pick = np.random.RandomState(case.K + n).randint(0, n, n)
    ctx.view_set(2, cells[pick])
    sub = _evaluate(ctx, case, 2, theta, tables)
    _assert_form(ctx, case, 'gathered view')
    assert np.array_equal(sub, got[pick]), _first_difference(sub, got[pick])

    if case.entry == 'theta' and case.ms == 1:
        # unsplit sums keep the strict mutation order whatever the tiling
        other = '4' if case.form.startswith('k_ll8') else '8'
        _set_knobs(monkeypatch, ctx, {'BNPC_MSPLIT': '0', 'BNPC_KW': other})
        alt = _evaluate(ctx, case, view, theta, tables)
        name, _, ms = ctx.last_launch()
        assert ms == 1 and name != case.form, (name, ms)
        assert np.array_equal(alt, got), _first_difference(alt, got)


# ------------------------------------------------- hints of sweep tiles
def _wide_hint_expected(mat, prior):
    post = mat + prior[None, :]
    col = np.argmax(post, axis=1)           # the first maximum
    rows = np.arange(post.shape[0])
    rest = post.copy()
    rest[rows, col] = -np.inf
    return post[rows, col], col, rest.max(axis=1)


def _check_wide_hints(mat, hint, prior, what):
    n, K = mat.shape
    assert hint is not None and hint.size == n, what
    best, col, second = _wide_hint_expected(mat, prior)
    col32 = hint['col'].astype(np.uint16).astype(np.int64) \
        | (hint['col2'].astype(np.uint16).astype(np.int64) << 16)
    bad = np.flatnonzero(col32 != col)
    assert not bad.size, (what, f'row {bad[0]}: column {col32[bad[0]]} vs '
        f'{col[bad[0]]}')
    assert np.array_equal(hint['best'], best), what
    assert np.array_equal(hint['second'], second), what
    assert np.all(hint['col3'] == -1) and np.all(hint['row_here'] == 2), what
    assert np.all(hint['third'] == -np.inf), what
    assert np.all(hint['fourth'] == -np.inf), what
    for f in ('e2', 'e3', 'll_best', 'll_second', 'll_third'):
        assert np.all(hint[f] == 0), (what, f)
    return col


def test_tile_hint_records_are_the_rows_top_two(monkeypatch):
    """bnpc_ll_rows_issue_hint (k_row_top2_wide): per row of a tile the
    largest entry of ll + prior, its column (first one on ties, 32 bits in
    col | col2 << 16) and the largest entry of all other columns, bit for bit
    from the matrix that comes with it; K from 1 to thousands, views that are
    not a multiple of 64 slots, exact ties and near-duplicate columns."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    rng = np.random.RandomState(31)
    N, M = 900, 130
    data = H.synth(31, N, M, 6, 0.15)
    ctx = _lib.Context(data=data)
    KMAX = 3001
    store = np.clip(rng.uniform(size=(KMAX, M)), 1e-5, 1 - 1e-5) \
        .astype(np.float32)
    # near-duplicates of row 5 (rows torn between columns) and exact copies
    store[70:90] = store[5]
    store[70:90, :3] = np.clip(store[70:90, :3] + .01, 1e-5, 1 - 1e-5)
    store[2] = store[0]
    store[300] = store[257]
    ctx.theta_put(0, store)
    views = {0: np.arange(N), 1: rng.randint(0, N, 333),
        2: rng.permutation(N)[:577]}
    for v in (1, 2):
        ctx.view_set(v, views[v])
    slot = 0
    for K in (1, 2, 3, 63, 64, 65, 255, 256, 257, 1100, 3001):
        for v, cells in views.items():
            rows = np.arange(K) if v != 2 else rng.permutation(KMAX)[:K]
            if v == 2 and K > 3:
                rows[3] = rows[1]           # one parameter row, two columns
            prior = -rng.uniform(0, 9, size=K)
            if K > 2:
                prior[2] = prior[0]         # rows 0 and 2 are equal: a tie
            if v == 2 and K > 3:
                prior[3] = prior[1]
            if K > 257 and v == 0:
                prior[257] = prior[300] = prior[0]
                prior[200] = -np.inf        # a column that never wins
            ld = K + 3
            ctx.ll_rows_issue_hint(v, rows, FP, FN, ld, slot, prior)
            mat, hint = ctx.ll_rows_wait_hint(slot, cells.size, ld)
            mat, hint = mat[:, :K].copy(), hint.copy()
            slot ^= 1
            what = (K, v)
            # the matrix is the one ll_theta gives for these parameters
            assert np.array_equal(mat, ctx.ll_theta(v, store[rows], FP, FN)), \
                what
            _check_wide_hints(mat, hint, prior, what)
    ctx.close()


def test_tile_hint_records_past_65535_columns(monkeypatch):
    """A tile of 70000 columns on a narrow matrix: the best column lies above
    65535 in most rows, so the high half of the 32-bit column (col2) is
    needed; an exact tie across the 16-bit boundary takes the first."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    rng = np.random.RandomState(65)
    N, M, K = 301, 12, 70000
    data = H.synth(65, N, M, 4, 0.1)
    ctx = _lib.Context(data=data)
    theta = np.clip(rng.uniform(size=(K, M)), 1e-5, 1 - 1e-5) \
        .astype(np.float32)
    theta[66001] = theta[65500]             # a tie across the 16-bit edge
    theta[69999] = theta[66000]             # a tie above it
    ctx.theta_put(0, theta)
    prior = -rng.uniform(0, 9, size=K)
    prior[66000:] += 12.0                   # the best lies up there
    prior[65500] = prior[66001] = 12.0
    prior[69999] = prior[66000]
    cells = rng.randint(0, N, 259)
    ctx.view_set(1, cells)
    rows = np.arange(K)
    for v, n in ((0, N), (1, cells.size)):
        ctx.ll_rows_issue_hint(v, rows, FP, FN, K, 0, prior)
        mat, hint = ctx.ll_rows_wait_hint(0, n, K)
        mat, hint = mat.copy(), hint.copy()
        col = _check_wide_hints(mat, hint, prior, ('70000', v))
        assert np.mean(col > 65535) > 0.5, np.bincount(col > 65535)
        assert not np.any(col == 69999) and not np.any(col == 66001)
    ctx.close()
