"""Doublet scores (-pd): the host side.  postproc.host_doublets on cases
computed by hand, against an independent per-cell loop, and on data with
planted doublets; the routing of postproc.doublets, the two files
save_outputs writes, and the flag.  CPU only: the clustering handle is the
NumPy stand-in of tests/fake_device.py, which has no doublets method."""
import math
import os
import re

import numpy as np
import pytest

import run_BnpC
from bnpc_amd import _lib, postproc
from bnpc_amd import io as bio
from fake_device import FakePosterior
from test_outputs import load_case
from test_support import save

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FILES = ('doublets_posterior_mean.tsv',
    'doublet_summary_posterior_mean.txt')
COLUMNS = ['cluster', 'n_obs', 'll_cluster', 'best_cluster', 'll_best',
    'pair_a', 'pair_b', 'll_pair', 'delta', 'p_doublet']
WHOLE = ('cluster', 'n_obs', 'best_cluster', 'pair_a', 'pair_b')
REDUCED = ('own', 'll_single', 'lse_single', 'll_pair', 'lse_pair',
    'best_single', 'best_pair')
ULP = 2.0 ** -52


def test_one_cell_of_two_clusters_by_hand():
    """M = 2, theta = [[1, 0], [0.5, 0]], FN = 0.25, FP = 0.125, the cells
    (1, 0) in cluster 0 and (0, missing) in cluster 1"""
    FN, FP = 0.25, 0.125
    theta = np.array([[1.0, 0.0], [0.5, 0.0]])
    data = np.array([[1.0, 0.0], [0.0, np.nan]])
    labels = np.array([0, 1])
    # candidate 0: t = (1, 0), o = (0, 1); candidate 1: t = o = 0.5 at m = 0;
    # the pair: o = (0 * 0.5, 1 * 1) = (0, 1): the tables of cluster 0
    L1 = np.log(np.array([[0.75, 0.125], [0.5 * 0.75 + 0.5 * 0.125, 0.125],
        [0.75, 0.125]]))
    L0 = np.log(np.array([[0.25, 0.875], [0.5 * 0.25 + 0.5 * 0.875, 0.875],
        [0.25, 0.875]]))
    got1, got0 = postproc.doublet_tables(theta, FN, FP)
    assert np.array_equal(got1, L1) and np.array_equal(got0, L0)
    fit = postproc.host_doublets(data, labels, theta, FN, FP)
    assert sorted(fit) == sorted(REDUCED + ('scores', 'n_obs'))
    scores = np.array([(0.0 + L1[:, 0]) + L0[:, 1], 0.0 + L0[:, 0]])
    assert np.array_equal(fit['scores'], scores)
    assert fit['scores'].shape == (2, 3)
    assert fit['n_obs'].tolist() == [2, 1]
    assert np.array_equal(fit['own'], [scores[0, 0], scores[1, 1]])
    assert fit['best_single'].tolist() == [0, 1]
    assert np.array_equal(fit['ll_single'], [scores[0, 0], scores[1, 1]])
    assert fit['best_pair'].tolist() == [[0, 1], [0, 1]]
    assert np.array_equal(fit['ll_pair'], scores[:, 2])
    # one cell per cluster: log n_k = 0, lN = log 2, lT = log 1 = 0
    for i in range(2):
        y = scores[i, :2] + (0.0 - math.log(2.0))
        mx = max(y)
        want = mx + math.log(math.exp(y[0] - mx) + math.exp(y[1] - mx))
        assert fit['lse_single'][i] == want
        assert fit['lse_pair'][i] == scores[i, 2]       # one term: exp(0)
    # other log-weights move the lse and nothing else
    logw = np.array([-1.0, 0.5])
    other = postproc.host_doublets(data, labels, theta, FN, FP, logw=logw)
    for key in ('scores', 'own', 'll_single', 'll_pair', 'best_single',
            'best_pair'):
        assert np.array_equal(other[key], fit[key]), key
    assert np.array_equal(other['lse_pair'], scores[:, 2] + ((-1.0 + 0.5) - 0.0))
    assert not np.array_equal(other['lse_single'], fit['lse_single'])


def test_one_cluster_has_no_pair():
    rng = np.random.RandomState(0)
    data = (rng.random_sample((5, 7)) < 0.5).astype(np.float64)
    theta = rng.random_sample((1, 7))
    labels = np.zeros(5, dtype=np.int64)
    fit = postproc.host_doublets(data, labels, theta, 0.2, 0.01)
    assert fit['scores'].shape == (5, 1)
    assert (fit['best_pair'] == -1).all() and fit['best_pair'].shape == (5, 2)
    assert (fit['ll_pair'] == -np.inf).all()
    assert (fit['lse_pair'] == -np.inf).all()
    assert np.array_equal(fit['own'], fit['ll_single'])
    assert np.array_equal(fit['lse_single'], fit['ll_single'])  # log(5/5) = 0
    t = postproc.doublets(None, data, labels, theta, 0.2, 0.01, 0.05)
    assert not t['p_doublet'].any() and t['p_doublet'].dtype == np.float64
    assert (t['pair_a'] == -1).all() and (t['pair_b'] == -1).all()
    assert (t['delta'] == -np.inf).all()
    assert t['total']['called'] == 0 and t['total']['candidates'] == 1
    assert t['total']['expected_doublets'] == 0.0
    assert t['total']['pair_counts'] == {}


def test_all_missing_row_and_ties():
    rng = np.random.RandomState(1)
    K, M = 4, 9
    theta = rng.random_sample((K, M))
    theta[2] = theta[1]                     # two identical clusters
    data = (rng.random_sample((8, M)) < 0.5).astype(np.float64)
    data[3] = np.nan
    labels = np.arange(8) % K
    fit = postproc.host_doublets(data, labels, theta, 0.3, 0.02)
    # the all-missing row: 0.0 everywhere, the first candidate of each group
    assert not fit['scores'][3].any()
    assert not np.signbit(fit['scores'][3]).any()
    assert fit['best_single'][3] == 0 and fit['ll_single'][3] == 0.0
    assert fit['best_pair'][3].tolist() == [0, 1] and fit['ll_pair'][3] == 0.0
    assert fit['own'][3] == 0.0 and fit['n_obs'][3] == 0
    # equal sizes: the priors of each group sum to one
    assert abs(fit['lse_single'][3]) <= 8 * ULP
    assert abs(fit['lse_pair'][3]) <= 8 * ULP
    # identical clusters tie in every cell, bit for bit: the first wins
    assert np.array_equal(fit['scores'][:, 1], fit['scores'][:, 2])
    assert (fit['best_single'] != 2).all()
    a, b = postproc.doublet_pairs(K)
    col = {pair: K + c for c, pair in enumerate(zip(a.tolist(), b.tolist()))}
    assert np.array_equal(fit['scores'][:, col[(0, 1)]],
        fit['scores'][:, col[(0, 2)]])
    assert np.array_equal(fit['scores'][:, col[(1, 3)]],
        fit['scores'][:, col[(2, 3)]])
    assert not any(pair in ([0, 2], [2, 3])
        for pair in fit['best_pair'].tolist())
    assert 1 in fit['best_single']          # and the tie is reached
    # a pair of a cluster with its twin is not the cluster: the union of two
    # soft genotypes is another table
    assert not np.array_equal(fit['scores'][:, col[(1, 2)]],
        fit['scores'][:, 1])


@pytest.mark.parametrize('K', range(2, 10))
def test_pair_index(K):
    a, b = postproc.doublet_pairs(K)
    ia, ib = np.triu_indices(K, 1)
    assert np.array_equal(a, ia) and np.array_equal(b, ib)
    assert a.size == K * (K - 1) // 2
    index = K + a * (2 * K - a - 1) // 2 + (b - a - 1)
    assert np.array_equal(index, np.arange(K, K + a.size))
    # the tables and the reductions use this order
    rng = np.random.RandomState(K)
    theta = rng.random_sample((K, 3))
    L1, L0 = postproc.doublet_tables(theta, 0.2, 0.01)
    assert L1.shape == L0.shape == (K + a.size, 3)
    for c in (K, K + a.size - 1, K + a.size // 2):
        o = (1.0 - theta[a[c - K]]) * (1.0 - theta[b[c - K]])
        t = 1.0 - o
        assert np.array_equal(L1[c], np.log(t * (1 - 0.2) + o * 0.01))
        assert np.array_equal(L0[c], np.log(t * 0.2 + o * (1 - 0.01)))
    scores = rng.random_sample((4, K + a.size))
    best = K + np.array([0, a.size - 1, a.size // 2, 1 % a.size])
    scores[np.arange(4), best] = 2.0
    red = postproc.doublet_reduce(scores, np.zeros(4, dtype=int), K,
        np.zeros(K), 0.0, 0.0)
    assert red['best_pair'].tolist() \
        == [[a[c - K], b[c - K]] for c in best.tolist()]


def planted(N, K, M, FN, FP, missing, rng, doublets=30):
    """N cells dealt round to K clusters of random 0 / 1 genotypes, `doublets`
    of them replaced by the union of two different clusters; observed with
    the error rates FN and FP and `missing` of the entries lost
    -> data, labels, genotypes, {cell: (a, b)}"""
    geno = (rng.random_sample((K, M)) < 0.5).astype(np.float64)
    labels = np.arange(N) % K
    truth = geno[labels]
    pairs = {}
    for i in rng.choice(N, doublets, replace=False).tolist():
        a, b = sorted(rng.choice(K, 2, replace=False).tolist())
        truth[i] = np.maximum(geno[a], geno[b])
        pairs[i] = (a, b)
    u = rng.random_sample((N, M))
    data = np.where(truth == 1, u >= FN, u < FP).astype(np.float64)
    data[rng.random_sample((N, M)) < missing] = np.nan
    return data, labels, geno, pairs


def test_planted_doublets_are_found():
    rng = np.random.RandomState(3)
    for K, M, FN, FP, missing in ((4, 60, 0.2, 0.01, 0.2),
            (6, 200, 0.3, 0.001, 0.3)):
        data, labels, geno, pairs = planted(600, K, M, FN, FP, missing, rng)
        assert len(pairs) == 30
        t = postproc.doublets(None, data, labels, geno, FN, FP, 0.05)
        p = t['p_doublet']
        print(f'K = {K}, M = {M}: called {t["total"]["called"]}, sum of p '
            f'{t["total"]["expected_doublets"]:.6f}, smallest planted p '
            f'{min(p[i] for i in pairs):.6f}, largest other p '
            f'{max(p[i] for i in range(600) if i not in pairs):.6f}')
        for i, pair in pairs.items():
            assert p[i] > 0.5, i
            assert (t['pair_a'][i], t['pair_b'][i]) == pair, i
        assert sorted(np.flatnonzero(p > 0.5).tolist()) == sorted(pairs)
        total = t['total']
        assert total['called'] == 30
        assert abs(total['expected_doublets'] - 30) <= 0.5
        assert total['expected_doublets'] == p.sum()
        assert sum(total['pair_counts'].values()) == 30
        assert total['pair_counts'] == {pair: list(pairs.values()).count(pair)
            for pair in sorted(set(pairs.values()))}
        assert (total['cells'], total['clusters'], total['candidates'],
            total['rate']) == (600, K, K + K * (K - 1) // 2, 0.05)
        assert np.array_equal(t['delta'], t['ll_pair'] - t['ll_best'])
        assert np.array_equal(t['n_obs'], (~np.isnan(data)).sum(axis=1))
        # missing as NaN, as 3 and as uint8 codes: the same bits
        threes = np.where(np.isnan(data), 3.0, data)
        for other in (threes, threes.astype(np.uint8)):
            u = postproc.doublets(None, other, labels, geno, FN, FP, 0.05)
            assert u.keys() == t.keys()
            for key in t:
                assert np.array_equal(u[key], t[key]) if key != 'total' \
                    else u[key] == t[key], key


def test_scores_against_an_independent_loop():
    """per cell and candidate, Python floats and math.fsum: the sequential
    sum is within (M + 2) 2^-52 fsum|terms| of it (the bound of
    tests/test_sample_pass_edges.py)"""
    rng = np.random.RandomState(5)
    N, K, M = 23, 5, 41
    theta = rng.random_sample((K, M))
    theta[rng.randint(0, 6, (K, M)) == 0] = 0.0
    theta[rng.randint(0, 6, (K, M)) == 0] = 1.0
    data = (rng.random_sample((N, M)) < 0.4).astype(np.float64)
    data[rng.random_sample((N, M)) < 0.3] = np.nan
    labels = np.arange(N) % K
    FN, FP = 0.21, 0.003
    fit = postproc.host_doublets(data, labels, theta, FN, FP)
    cands = [(k, None) for k in range(K)] + [(a, b) for a in range(K)
        for b in range(a + 1, K)]
    assert fit['scores'].shape == (N, len(cands))
    worst = 0.0
    for i in range(N):
        for c, (a, b) in enumerate(cands):
            terms = []
            for m in range(M):
                if np.isnan(data[i, m]):
                    continue
                if b is None:
                    t = float(theta[a, m])
                    o = 1.0 - t
                else:
                    o = (1.0 - float(theta[a, m])) * (1.0 - float(theta[b, m]))
                    t = 1.0 - o
                terms.append(math.log(t * (1 - FN) + o * FP) if data[i, m]
                    else math.log(t * FN + o * (1 - FP)))
            want = math.fsum(terms)
            room = (M + 2) * ULP * math.fsum(abs(x) for x in terms)
            assert abs(fit['scores'][i, c] - want) <= room, (i, c)
            if room:
                worst = max(worst, abs(fit['scores'][i, c] - want) / room)
    print(f'largest share of the bound used: {worst:.3f}')
    # the reductions are those of the scores
    sizes = np.bincount(labels).astype(np.float64)
    both = (N * N - int((sizes ** 2).sum())) // 2
    red = postproc.doublet_reduce(fit['scores'], labels, K, np.log(sizes),
        np.log(np.float64(N)), np.log(np.float64(both)))
    for key in REDUCED:
        assert np.array_equal(red[key], fit[key]), key
    for i in range(N):
        row = fit['scores'][i].tolist()
        assert fit['own'][i] == row[labels[i]]
        assert fit['ll_single'][i] == max(row[:K])
        assert fit['best_single'][i] == row[:K].index(max(row[:K]))
        assert fit['ll_pair'][i] == max(row[K:])
        assert tuple(fit['best_pair'][i]) == cands[K + row[K:].index(
            max(row[K:]))]
        y = [row[k] + (math.log(sizes[k]) - math.log(N)) for k in range(K)]
        want = math.log(math.fsum(math.exp(v) for v in y))
        assert abs(fit['lse_single'][i] - want) <= 1e-12 * (1 + abs(want))
        y = [row[K + c] + ((math.log(sizes[a]) + math.log(sizes[b]))
            - math.log(both)) for c, (a, b) in enumerate(cands[K:])]
        want = math.log(math.fsum(math.exp(v) for v in y))
        assert abs(fit['lse_pair'][i] - want) <= 1e-12 * (1 + abs(want))


def test_bad_input_is_refused():
    data = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    theta = np.array([[0.9, 0.1], [0.2, 0.8]])
    labels = np.array([0, 1, 1])
    postproc.host_doublets(data, labels, theta, 0.2, 0.01)
    for bad in ([0, 0, 0], [0, 1, 2], [0, -1, 1]):
        with pytest.raises(ValueError, match='labels'):
            postproc.host_doublets(data, np.array(bad), theta, 0.2, 0.01)
    for bad in (1.5, -0.1, np.nan):
        wrong = theta.copy()
        wrong[1, 0] = bad
        with pytest.raises(ValueError, match='theta'):
            postproc.host_doublets(data, labels, wrong, 0.2, 0.01)
    for FN, FP in ((0.0, 0.01), (0.2, 1.0), (np.nan, 0.01)):
        with pytest.raises(ValueError, match='FN'):
            postproc.host_doublets(data, labels, theta, FN, FP)
    with pytest.raises(ValueError, match='logw'):
        postproc.host_doublets(data, labels, theta, 0.2, 0.01,
            logw=np.array([0.0, np.inf]))
    with pytest.raises(ValueError, match='missing'):
        postproc.host_doublets(data * 2, labels, theta, 0.2, 0.01)
    for rate in (0, 1, True, -0.05, np.nan):
        with pytest.raises(ValueError, match='rate'):
            postproc.doublets(None, data, labels, theta, 0.2, 0.01, rate)


def small():
    rng = np.random.RandomState(7)
    data, labels, geno, pairs = planted(40, 3, 25, 0.2, 0.01, 0.2, rng, 4)
    return data, labels, np.clip(geno, 0.02, 0.97)


def test_handle_without_the_method_takes_the_host_loop():
    data, labels, theta = small()
    post = FakePosterior(labels[None, :])
    assert not hasattr(post, 'doublets')
    want = postproc.host_doublets(data, labels, theta, 0.2, 0.01)
    for handle in (post, None):
        got = postproc.doublets(handle, data, labels, theta, 0.2, 0.01, 0.1)
        assert list(got) == COLUMNS + ['total']
        assert np.array_equal(got['ll_cluster'], want['own'])
        assert np.array_equal(got['best_cluster'], want['best_single'])
        assert np.array_equal(got['ll_best'], want['ll_single'])
        assert np.array_equal(got['pair_a'], want['best_pair'][:, 0])
        assert np.array_equal(got['pair_b'], want['best_pair'][:, 1])
        assert np.array_equal(got['ll_pair'], want['ll_pair'])
        assert np.array_equal(got['cluster'], labels)
        assert np.array_equal(got['p_doublet'], 1 / (1 + np.exp(
            (np.log(1 - 0.1) + want['lse_single'])
            - (np.log(0.1) + want['lse_pair']))))
        assert ((got['p_doublet'] > 0) & (got['p_doublet'] < 1)).all()


def test_handle_with_the_method_is_asked():
    data, labels, theta = small()
    want = postproc.host_doublets(data, labels, theta, 0.2, 0.01)

    class Handle(FakePosterior):
        calls = 0

        def doublets(self, d, lab, th, fn, fp):
            assert np.array_equal(d, postproc.data_codes(data))
            assert np.array_equal(lab, labels) and np.array_equal(th, theta)
            assert (fn, fp) == (0.2, 0.01)
            self.calls += 1
            # (marked, so that the host loop cannot have made them)
            return (want['own'] - 1, want['ll_single'], want['lse_single'],
                want['ll_pair'] + 2, want['lse_pair'], want['best_single'],
                want['best_pair'], None, None, None)
    post = Handle(labels[None, :])
    got = postproc.doublets(post, data, labels, theta, 0.2, 0.01, 0.05)
    assert post.calls == 1
    assert np.array_equal(got['ll_cluster'], want['own'] - 1)
    assert np.array_equal(got['delta'],
        (want['ll_pair'] + 2) - want['ll_single'])
    assert np.array_equal(got['p_doublet'], 1 / (1 + np.exp(
        (np.log(1 - 0.05) + want['lse_single'])
        - (np.log(0.05) + want['lse_pair']))))


@pytest.fixture
def host_posterior(monkeypatch):
    monkeypatch.setattr(_lib, 'Posterior', FakePosterior)


def same(got, want):
    assert got.keys() == want.keys()
    for key in want:
        if key != 'total':
            assert np.array_equal(got[key], want[key]), key
    assert got['total'] == want['total']


def test_posterior_estimate_doublets(golden_dir, tmp_path, host_posterior):
    d, case, results = load_case(golden_dir, 'fixture', tmp_path / 'ref')
    data = bio.load_data(os.path.join(d, 'input.tsv'))
    plain = postproc.posterior_estimate(results, data)
    assert plain.keys() == postproc.posterior_estimate(results, data,
        doublets=False).keys()
    inf = postproc.posterior_estimate(results, data, doublets=0.05)
    assert sorted(set(inf) - set(plain)) == ['doublets']
    for key in plain:
        assert np.array_equal(inf[key], plain[key]), key
    pooled = postproc.concat_chain_results(results)
    want = postproc.doublets(None, data, plain['cluster_of'],
        plain['cluster_genotypes'], np.mean(pooled['FN']),
        np.mean(pooled['FP']), 0.05)
    same(inf['doublets'], want)
    assert inf['doublets']['total']['rate'] == 0.05
    assert np.array_equal(inf['doublets']['cluster'], plain['assignment'])
    other = postproc.posterior_estimate(results, data, doublets=0.2)
    assert (other['doublets']['p_doublet']
        >= inf['doublets']['p_doublet']).all()
    every = postproc.posterior_estimate(results, data, support=True,
        cells=True, fit=True, mutations=True, doublets=0.05)
    assert sorted(set(every) - set(plain)) == ['cell_genotypes', 'doublets',
        'fit', 'mutation_fit', 'support']
    same(every['doublets'], want)


def test_mean_hierarchy_calls_back_after_the_genotypes(golden_dir, tmp_path,
        host_posterior):
    d, case, results = load_case(golden_dir, 'fixture', tmp_path / 'ref')
    pooled = postproc.concat_chain_results(results)
    seen = []

    def first(post, assign):
        seen.append(('open', post.closed if hasattr(post, 'closed') else None))

    def second(post, assign, params):
        seen.append(('genotypes', assign.copy(), params.copy()))
    assign, params = postproc._mean_hierarchy(pooled['assignments'],
        pooled['params'], while_open=first, with_genotypes=second)
    assert [s[0] for s in seen] == ['open', 'genotypes']
    assert np.array_equal(seen[1][1], assign)
    assert np.array_equal(seen[1][2], params)
    plain = postproc._mean_hierarchy(pooled['assignments'], pooled['params'])
    assert np.array_equal(plain[0], assign) and np.array_equal(plain[1], params)


def test_save_outputs_writes_the_two_files(golden_dir, tmp_path,
        host_posterior, capsys):
    d, case, results = load_case(golden_dir, 'fixture', tmp_path / 'ref')
    out = tmp_path / 'out'
    args, names = save(d, case, results, out, posterior_doublets=0.05)
    assert capsys.readouterr().out == ''            # verbosity 0
    data = bio.load_data(os.path.join(d, 'input.tsv'))
    want = postproc.posterior_estimate(results, data, doublets=0.05)
    assign, want = want['assignment'], want['doublets']
    N = data.shape[0]
    rows = [ln.split('\t') for ln in
        (out / NEW_FILES[0]).read_text().splitlines()]
    assert rows[0] == ['cell'] + COLUMNS
    assert len(rows) == N + 1 and all(len(r) == len(rows[0]) for r in rows)
    assert [r[0] for r in rows[1:]] == [str(x) for x in names[0].tolist()]
    for col, key in enumerate(COLUMNS, 1):
        got = [r[col] for r in rows[1:]]
        if key in WHOLE:
            assert got == [str(int(x)) for x in want[key].tolist()], key
            continue
        assert all(re.fullmatch(r'-?\d+\.\d{4}|-inf', x) for x in got), key
        assert got == [f'{x:.4f}' for x in want[key].tolist()], key
    # the cluster ids are the labels of assignment.txt
    assert [int(r[1]) for r in rows[1:]] == assign
    clusters = set(assign)
    assert {int(r[4]) for r in rows[1:]} <= clusters
    lines = (out / NEW_FILES[1]).read_text().splitlines()
    assert [ln.split(':')[0] for ln in lines] == ['cells', 'clusters',
        'candidates', 'rate', 'expected_doublets', 'called', 'pair_counts',
        'top_cells']
    model = dict(ln.split(':', 1) for ln in lines)
    model = {k: v.strip() for k, v in model.items()}
    total = want['total']
    K = len(clusters)
    assert int(model['cells']) == N == total['cells']
    assert int(model['clusters']) == K == total['clusters']
    assert int(model['candidates']) == K + K * (K - 1) // 2
    assert model['rate'] == '0.05'
    assert model['expected_doublets'] == f'{total["expected_doublets"]:.4f}'
    assert int(model['called']) == total['called'] \
        == int((want['p_doublet'] > 0.5).sum())
    assert model['pair_counts'].split() == [f'{a}-{b}:{n}'
        for (a, b), n in total['pair_counts'].items()]
    assert all(n > 0 for n in total['pair_counts'].values())
    p, delta = want['p_doublet'], want['delta']
    order = sorted(range(N), key=lambda i: (-p[i], -delta[i], i))[:10]
    top = [x.rsplit(':', 1) for x in model['top_cells'].split(' ')]
    assert [x[0] for x in top] == [str(names[0][i]) for i in order]
    assert [x[1] for x in top] == [f'{p[i]:.4f}' for i in order]
    assert 'posterior_doublets: 0.05\n' in (out / 'args.txt').read_text()
    # everything else is what a run without the flag writes, byte for byte
    plain, false = tmp_path / 'plain', tmp_path / 'false'
    save(d, case, results, plain)
    save(d, case, results, false, posterior_doublets=False)
    for other in (plain, false):
        assert sorted(os.listdir(other)) \
            == sorted(set(os.listdir(out)) - set(NEW_FILES))
        for name in os.listdir(other):
            if name != 'args.txt':
                assert (other / name).read_bytes() \
                    == (out / name).read_bytes(), name
        assert 'posterior_doublets' not in (other / 'args.txt').read_text()
    assert (plain / 'args.txt').read_bytes() \
        == (false / 'args.txt').read_bytes()


def test_top_cells_break_ties_by_delta_then_index(tmp_path):
    N = 12
    p = np.array([0.5, 0.9, 0.9, 0.9, 0.1, 0.9] + [0.0] * 6)
    delta = np.array([0.0, 1.0, 3.0, 1.0, 0.0, 2.0] + [-1.0] * 6)
    zeros = np.zeros(N, dtype=np.int64)
    tables = {'cluster': zeros, 'n_obs': zeros, 'll_cluster': delta,
        'best_cluster': zeros, 'll_best': delta, 'pair_a': zeros,
        'pair_b': zeros + 1, 'll_pair': delta, 'delta': delta, 'p_doublet': p,
        'total': {'cells': N, 'clusters': 2, 'candidates': 3, 'rate': 0.05,
            'expected_doublets': float(p.sum()), 'called': 4,
            'pair_counts': {(0, 1): 4}}}
    paths = bio.save_doublets(str(tmp_path), 'mean', 'posterior', tables)
    assert [os.path.basename(x) for x in paths] == list(NEW_FILES)
    with open(paths[1]) as f:
        model = dict(ln.rstrip('\n').split(': ', 1) for ln in f)
    top = [x.split(':')[0] for x in model['top_cells'].split(' ')]
    assert top == ['2', '5', '1', '3', '0', '4', '6', '7', '8', '9']
    assert model['pair_counts'] == '0-1:4'
    with open(paths[0]) as f:
        rows = [ln.split('\t') for ln in f.read().splitlines()]
    assert [r[0] for r in rows[1:]] == [str(i) for i in range(N)]


def test_verbose_run_prints_one_line(golden_dir, tmp_path, host_posterior,
        capsys):
    d, case, results = load_case(golden_dir, 'fixture', tmp_path / 'ref')
    data, names = bio.load_data(os.path.join(d, 'input.tsv'), get_names=True)
    out = tmp_path / 'out'
    out.mkdir()
    args = run_BnpC.parse_args(['d.csv', '-pd', '-v', '1', '-e', 'posterior'])
    run_BnpC.save_outputs(args, results, data, str(out), names)
    lines = [ln for ln in capsys.readouterr().out.splitlines()
        if ln.startswith('posterior doublets: ')]
    assert len(lines) == 1
    assert re.fullmatch(r'posterior doublets: \d+ called, \d+\.\d{4} expected '
        r'\(rate 0\.05\)', lines[0])
    model = dict(ln.split(': ', 1) for ln in
        (out / NEW_FILES[1]).read_text().splitlines())
    assert f': {model["called"]} called, {model["expected_doublets"]} ' \
        in lines[0]


def test_flag_and_its_check():
    """(the input path is a required argument: `d.csv` stands for it)"""
    args = run_BnpC.parse_args(['d.csv'])
    assert args.posterior_doublets is False
    assert 'posterior_doublets' not in vars(args)
    run_BnpC.check_args(args)
    for flag in ('-pd', '--posterior_doublets'):
        args = run_BnpC.parse_args(['d.csv', flag])
        assert vars(args)['posterior_doublets'] == 0.05
        run_BnpC.check_args(args)
        args = run_BnpC.parse_args(['d.csv', flag, '0.2'])
        assert vars(args)['posterior_doublets'] == 0.2
    assert vars(run_BnpC.parse_args(['-pd', '0.01', 'd.csv'])) \
        ['posterior_doublets'] == 0.01
    for bad in ('0', '1', '-0.5', '1.5'):
        with pytest.raises(SystemExit):
            run_BnpC.parse_args(['d.csv', '-pd', bad])
    run_BnpC.check_args(run_BnpC.parse_args('d.csv -pd -e ML posterior'
        .split()))
    for ests in ('ML', 'ML MAP'):
        args = run_BnpC.parse_args(['d.csv', '-pd', '-e'] + ests.split())
        with pytest.raises(SystemExit, match='posterior'):
            run_BnpC.check_args(args)
        # main() stops there: before the input is looked at
        with pytest.raises(SystemExit, match='--posterior_doublets'):
            run_BnpC.main(args)


def test_binding_and_header_list_the_entry_points():
    for name in ('bnpc_post_doublets', 'bnpc_post_doublets_times'):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    assert hasattr(_lib.Posterior, 'doublets')
    assert hasattr(_lib.Posterior, 'doublets_times')
    with open(os.path.join(ROOT, 'include', 'bnpc_hip.h')) as f:
        header = f.read()
    assert re.search(r'\bint bnpc_post_doublets\(bnpc_post \*post, '
        r'const uint8_t \*codes', header)
    assert re.search(r'\bint bnpc_post_doublets_times\(bnpc_post \*post',
        header)
    with open(os.path.join(ROOT, 'bnpc_amd', 'csrc', 'bnpc_post_passes.hip')) as f:
        source = f.read()
    assert f'#define DB_TILE {_lib.DOUBLET_TILE} ' in source
    assert f'#define DB_UNROLL {_lib.DOUBLET_UNROLL} ' in source
    assert _lib.ABI_VERSION == 12
