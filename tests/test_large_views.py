"""Column counts of views larger than one LDS range of the mask-count kernel
(-m gpu).

k_counts_masks stages a view's membership words in LDS, 896 blocks of 64
slots (57,344 cells) at a time.  Views past that - the two clusters of a
split / merge move on a matrix of more than 57,344 cells, a whole-matrix view
by label - are counted range by range: the same integers as NumPy."""
import numpy as np
import pytest

from oracle import crp_numpy as O
from bnpc_amd import _lib, model as P
import test_host_logic as H

pytestmark = pytest.mark.gpu

RANGE_CELLS = 896 * 64


def _numpy_counts(data, cells, labels, G):
    n1 = np.zeros((G, data.shape[1]), dtype=np.int64)
    n0 = np.zeros_like(n1)
    for g in range(G):
        sub = data[cells[labels == g]]
        n1[g] = (sub == 1).sum(axis=0)
        n0[g] = (sub == 0).sum(axis=0)
    return n1, n0


@pytest.fixture(scope='module')
def narrow():
    data = H.synth(57, 60000, 40, 5, 0.15)
    ctx = _lib.Context(data=data)
    yield data, ctx
    ctx.close()


@pytest.mark.parametrize('zero_copy', ['1', '0'])
def test_view_counts_past_one_lds_range(narrow, zero_copy, monkeypatch):
    """bnpc_view_counts on gathered views (repeats, slots of no segment) of
    one range, one range + 1 cell, about two ranges and more; 2 and 9
    segments (9: two workgroup rows, the second one mostly empty)."""
    data, ctx = narrow
    N = data.shape[0]
    monkeypatch.setenv('BNPC_ZERO_COPY', zero_copy)
    ctx.reload_options()
    rng = np.random.RandomState(int(zero_copy) + 1)
    for n in (RANGE_CELLS - 1, RANGE_CELLS, RANGE_CELLS + 1, 120000, 180031):
        cells = rng.randint(0, N, n)
        ctx.view_set(1, cells)
        for G in (2, 9):
            labels = rng.randint(-1, G, n)
            n1, n0 = ctx.view_counts(1, labels, G)
            w1, w0 = _numpy_counts(data, cells, labels, G)
            assert np.array_equal(n1, w1), (n, G)
            assert np.array_equal(n0, w0), (n, G)
    # a whole-matrix view, every slot in one segment
    n1, n0 = ctx.view_counts(0, np.zeros(N, dtype=np.int64), 1)
    assert np.array_equal(n1[0], (data == 1).sum(axis=0))
    assert np.array_equal(n0[0], (data == 0).sum(axis=0))
    ctx.reload_options()


@pytest.mark.parametrize('N', [RANGE_CELLS, RANGE_CELLS + 1])
def test_colcounts_by_label_on_either_side_of_the_mask_guard(N, monkeypatch):
    """bnpc_colcounts_by_label takes the mask kernel for a matrix of at most
    one LDS range and few clusters, the cell-list kernel otherwise: with the
    cluster limit (BNPC_MASK_COUNTS_MAX) raised and lowered, both sides of
    the cell guard give NumPy's integers."""
    data = H.synth(N, N, 33, 4, 0.2)
    ctx = _lib.Context(data=data)
    rng = np.random.RandomState(N)
    for limit in ('4096', '64', '0'):
        monkeypatch.setenv('BNPC_MASK_COUNTS_MAX', limit)
        ctx.reload_options()
        for K in (1, 5, 70):
            assign = rng.randint(0, K, N) * 3
            ids = rng.permutation(np.unique(assign))
            n1, n0 = ctx.colcounts_by_label(assign, ids)
            for g, cid in enumerate(ids):
                sub = data[assign == cid]
                assert np.array_equal(n1[g], (sub == 1).sum(axis=0)), \
                    (limit, K, g)
                assert np.array_equal(n0[g], (sub == 0).sum(axis=0)), \
                    (limit, K, g)
    ctx.close()


SM_ROUNDS = 2


def _split_merge_trace(mod, data):
    """The state after each of SM_ROUNDS split / merge rounds from a start
    with every cell in one cluster (rounds of test_split_merge_moves_match_
    oracle: a seeded move, then a seeded parameter update)."""
    m = H.make(mod, 'fixed', data)
    np.random.seed(8)
    m.init(mode='together')
    m.update_parameters()
    trace = []
    for rnd in range(SM_ROUNDS):
        np.random.seed(1004 + rnd)
        res = m.update_assignments_split_merge([.6, .4], 2)
        ids = list(m.cells_per_cluster)
        trace.append((res, np.random.random(), m.assignment.copy(),
            [(int(k), int(v)) for k, v in m.cells_per_cluster.items()],
            m.parameters[ids].copy()))
        np.random.seed(rnd)
        m.update_parameters()
    return m, trace


_SM_ORACLE = {}


def _sm_oracle(data):
    if 'trace' not in _SM_ORACLE:
        _SM_ORACLE['trace'] = _split_merge_trace(O, data)[1]
    return _SM_ORACLE['trace']


@pytest.mark.parametrize('native', ['1', '0'])
def test_split_merge_on_more_cells_than_one_range_matches_oracle(native,
        monkeypatch):
    """A 60,000-cell matrix started with every cell in one cluster: the first
    split move counts a view of all 60,000 cells, and so does the merge of
    the two halves.  Native moves (the default) and moves walked by the
    binding (BNPC_NATIVE_MOVES=0) against the oracle, in the style of
    test_split_merge_moves_match_oracle: results, stream position,
    assignment, cluster table and parameters identical after every round."""
    monkeypatch.setenv('BNPC_NATIVE_MOVES', native)
    data = H.synth(60, 60000, 40, 3, 0.1)
    p, got = _split_merge_trace(P, data)
    moves = getattr(p, '_native_moves', 0)
    p.close()
    want = _sm_oracle(data)
    for rnd, (a, b) in enumerate(zip(got, want)):
        assert a[0] == b[0], rnd
        assert a[1] == b[1], rnd
        assert np.array_equal(a[2], b[2]), rnd
        assert a[3] == b[3], rnd
        assert np.array_equal(a[4], b[4]), rnd
    # a split of all 60,000 cells was accepted, a merge of them was tried
    assert want[0][0] == ([1, 0], 0) and want[1][0][1] == 1, \
        [w[0] for w in want]
    assert (moves > 0) == (native == '1'), moves
