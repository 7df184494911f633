"""Placement of held-out cells: the host side.  postproc.host_place against
the Gibbs conditional of the model class, on closed forms and on data drawn
from known clones; the tables of postproc.place_cells and the two files
io.save_placement writes.  CPU only: without a clustering handle that has a
place method, place_cells takes the host loop."""
import os
import re

import numpy as np
import pytest

from bnpc_amd import _lib, postproc
from bnpc_amd import io as bio
from fake_device import attach

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FILES = ('placement_posterior_mean.tsv',
    'placement_summary_posterior_mean.txt')
COLUMNS = ['cell', 'cluster', 'prob', 'next_cluster', 'next_prob', 'p_new',
    'entropy', 'n_obs', 'lpd', 'lpd_per_obs']
SUMS = ('prob_sum', 'new_sum', 'ent_sum', 'lpd', 'lp')
ULP = 2.0 ** -52
PRIOR = (0.25, 0.25)


def samples(rng, S, N, W, M, clusters=None, in_range=False):
    """S samples of N cells: labels that are not compact (in_range: inside
    [0, N), as a clustering handle on the device takes them; else negative
    ones and ones past N too), each sample with a cluster count of its own
    (at most W); a float32 trace whose unused rows are NaN; FN, FP, alpha per
    sample"""
    a = np.empty((S, N), dtype=np.int64)
    par = np.full((S, W, M), np.nan, dtype=np.float32)
    for s in range(S):
        Ks = clusters[s] if clusters is not None else rng.randint(1, W + 1)
        assert 1 <= Ks <= min(W, N)
        ids = np.sort(rng.choice(N, Ks, replace=False)) if in_range \
            else np.sort(rng.choice(5 * N, Ks, replace=False)) - N
        a[s] = ids[rng.permutation(np.concatenate([np.arange(Ks),
            rng.randint(0, Ks, N - Ks)]))]
        par[s, :Ks] = np.clip(rng.random_sample((Ks, M)), 1e-3, 1 - 1e-3)
    return (a, par, rng.uniform(0.05, 0.3, S), rng.uniform(1e-4, 0.05, S),
        rng.uniform(0.3, 4.0, S))


def new_cells(rng, Q, M):
    """0 / 1 / NaN; where there is room, a row of each alone"""
    data = (rng.random_sample((Q, M)) < 0.4).astype(np.float64)
    data[rng.random_sample((Q, M)) < 0.3] = np.nan
    for row, val in zip(range(Q - 1, 1, -1), (np.nan, 1.0, 0.0)):
        data[row] = val
    return data


def clustering(rng, N, K):
    return rng.permutation(np.concatenate([np.arange(K),
        rng.randint(0, K, N - K)])).astype(np.int64)


def test_one_sample_is_the_models_gibbs_conditional():
    """y_c - log(N + alpha) of host_place against get_lpost_single and
    get_lpost_single_new_cluster of the model class (the reference's
    expressions, libs/CRP.py:223-234) with the query row as cell N of a model
    of N + 1 cells, taken out of cells_per_cluster: CRP_prior is then
    log(n) - log(N + alpha)."""
    from libs.CRP import CRP
    rng = np.random.RandomState(11)
    N, M, W, Q = 23, 19, 6, 5
    prior = (0.25, 0.75)
    a, par, FN, FP, alpha = samples(rng, 1, N, W, M, clusters=[4])
    new = new_cells(rng, Q, M)
    got = postproc.host_place(new, a, clustering(rng, N, 3), par, FN, FP,
        alpha, prior)
    assert sorted(got) == sorted(SUMS + ('n_obs', 'scores', 'y'))
    rank = np.unique(a[0], return_inverse=True)[1].ravel()
    sizes = np.bincount(rank)
    for j in range(Q):
        # (the training rows' entries are not read for cell N)
        model = attach(CRP(np.concatenate([np.zeros((N, M)), new[j:j + 1]]),
            DP_alpha=[1, 1], param_beta=list(prior), FN_error=FN[0],
            FP_error=FP[0]))
        model.DP_a = alpha[0]
        model.assignment = np.append(rank, 0)
        model.cells_per_cluster = {r: int(n) for r, n in enumerate(sizes)}
        model.parameters = np.zeros((N + 1, M), dtype=np.float32)
        model.parameters[:4] = par[0, :4]
        model.init_DP_prior()
        want = np.append(model.get_lpost_single(N, np.arange(4)),
            model.get_lpost_single_new_cluster()[N])
        y = got['y'][0, j]
        assert np.isnan(y[4:W]).all()
        have = np.append(y[:4], y[W]) - np.log(N + alpha[0])
        np.testing.assert_allclose(have, want, rtol=1e-12, atol=1e-12)
        assert np.array_equal(got['y'][0, j, :4],
            got['scores'][0, j, :4] + np.log(sizes.astype(np.float64)))


def test_all_missing_row_gives_the_crp_weights():
    """Score 0 everywhere: pr_r = n_r / (N + alpha), p_new = alpha /
    (N + alpha), and lp = log(sum of the weights) - log(N + alpha) = 0, each
    within the roundings of K_s + 1 exps, adds and divisions: (W + 5) ulps
    of a value of size 1 + log(N + alpha)."""
    rng = np.random.RandomState(3)
    S, N, M, W, K = 6, 31, 9, 7, 3
    a, par, FN, FP, alpha = samples(rng, S, N, W, M)
    labels = clustering(rng, N, K)
    new = new_cells(rng, 5, M)
    assert np.isnan(new[4]).all()
    got = postproc.host_place(new, a, labels, par, FN, FP, alpha, PRIOR)
    assert got['n_obs'][4] == 0
    tol = (W + 5) * ULP * (1 + np.log(N + alpha.max()))
    assert np.abs(got['lp'][:, 4]).max() <= tol
    assert abs(got['lpd'][4]) <= 2 * tol
    prob = np.zeros(K)
    for s in range(S):
        assert not got['scores'][s, 4][~np.isnan(got['scores'][s, 4])].any()
        prob += np.bincount(labels, minlength=K) / (N + alpha[s])
    np.testing.assert_allclose(got['prob_sum'][4], prob, rtol=0,
        atol=S * (W + 5) * ULP)
    np.testing.assert_allclose(got['new_sum'][4],
        (alpha / (N + alpha)).sum(), rtol=0, atol=S * (W + 5) * ULP)
    # the other rows are not at the prior
    assert (np.abs(got['lp'][:, :4]) > 0.1).all()


def test_probabilities_sum_to_one():
    """prob.sum(1) + p_new = 1: every term is in [0, 1] and goes through an
    exp, the sum of W + 1 of them, a division, the share's division, a
    product, the sums over at most W rows, S samples and K clusters and the
    division by S - 2 (W + 1) + K + S + 8 roundings of an ulp each at the
    most."""
    rng = np.random.RandomState(4)
    S, N, M, W, K, Q = 9, 40, 13, 8, 4, 17
    a, par, FN, FP, alpha = samples(rng, S, N, W, M)
    labels = clustering(rng, N, K)
    t = postproc.place_cells(None, new_cells(rng, Q, M), a, labels, par, FN,
        FP, alpha, PRIOR)
    assert t['prob'].shape == (Q, K) and (t['prob'] >= 0).all()
    off = np.abs(t['prob'].sum(axis=1) + t['p_new'] - 1)
    assert off.max() <= (2 * (W + 1) + K + S + 8) * ULP
    assert (t['entropy'] >= 0).all() \
        and (t['entropy'] <= np.log(W + 1) + 1e-12).all()


def test_one_cluster():
    rng = np.random.RandomState(5)
    S, N, M, Q = 4, 12, 6, 7
    a, par, FN, FP, alpha = samples(rng, S, N, 3, M, clusters=[1, 3, 2, 1])
    labels = np.zeros(N, dtype=np.int64)
    new = new_cells(rng, Q, M)
    red = postproc.host_place(new, a, labels, par, FN, FP, alpha, PRIOR)
    assert red['prob_sum'].shape == (Q, 1)
    t = postproc.place_cells(None, new, a, labels, par, FN, FP, alpha, PRIOR)
    assert (t['next_cluster'] == -1).all() and not t['next_prob'].any()
    assert set(t['cluster'].tolist()) <= {0, -1}
    assert np.array_equal(t['cluster'] == -1, t['p_new'] > t['prob'][:, 0])
    assert t['total']['clusters'] == 1
    assert t['total']['placed'] == [int((t['cluster'] == 0).sum())]
    assert t['total']['new'] == int((t['cluster'] == -1).sum())
    # every row's mass is in cluster 0: prob + p_new = 1 to the bound above
    assert np.abs(t['prob'][:, 0] + t['p_new'] - 1).max() \
        <= (2 * 4 + 1 + S + 8) * ULP


def test_sample_of_singletons():
    """N clusters of one cell: every log(n) is 0, every share 0 or 1"""
    rng = np.random.RandomState(6)
    N, M, Q, K = 9, 5, 4, 3
    a = (rng.permutation(N) * 7 - 20)[None, :]
    par = np.clip(rng.random_sample((1, N, M)), .01, .99).astype(np.float32)
    labels = clustering(rng, N, K)
    new = new_cells(rng, Q, M)
    got = postproc.host_place(new, a, labels, par, [0.2], [0.01], [1.5],
        PRIOR)
    assert np.array_equal(got['y'][0, :, :N], got['scores'][0, :, :N])
    rank = np.unique(a[0], return_inverse=True)[1].ravel()
    y = got['y'][0]
    e = np.exp(y - y.max(axis=1, keepdims=True))
    pr = e / e.sum(axis=1, keepdims=True)
    want = np.zeros((Q, K))
    for i in range(N):
        want[:, labels[i]] += pr[:, rank[i]]
    np.testing.assert_allclose(got['prob_sum'], want, rtol=0,
        atol=(2 * N + 8) * ULP)


def test_rows_past_the_cluster_count_are_not_read():
    rng = np.random.RandomState(7)
    S, N, M, W, Q = 5, 20, 8, 6, 6
    a, par, FN, FP, alpha = samples(rng, S, N, W, M,
        clusters=[2, 6, 1, 4, 3])
    assert np.isnan(par).any()
    labels = clustering(rng, N, 3)
    new = new_cells(rng, Q, M)
    got = postproc.host_place(new, a, labels, par, FN, FP, alpha, PRIOR)
    filled = np.where(np.isnan(par), np.float32(0.5), par)
    other = postproc.host_place(new, a, labels, filled, FN, FP, alpha, PRIOR)
    for key in SUMS:
        assert np.isfinite(got[key]).all(), key
        assert np.array_equal(got[key], other[key]), key
    assert np.array_equal(np.isnan(got['scores']), np.isnan(other['scores']))
    for s, Ks in enumerate([2, 6, 1, 4, 3]):
        assert np.isnan(got['scores'][s, :, Ks:W]).all()
        assert np.isfinite(got['scores'][s, :, :Ks]).all()
        assert np.isfinite(got['scores'][s, :, W]).all()
    # a wider trace moves nothing but the new cluster's slot
    wide = np.concatenate([par, np.full((S, 2, M), np.nan, np.float32)], 1)
    more = postproc.host_place(new, a, labels, wide, FN, FP, alpha, PRIOR)
    for key in SUMS:
        assert np.array_equal(got[key], more[key]), key
    assert np.array_equal(more['scores'][:, :, W + 2], got['scores'][:, :, W])


def clones_case():
    """S = 12 samples of N = 70 training cells from four clones over M = 33
    mutations and Q = 65 held-out cells of the same clones with FN 0.1, FP
    0.01 and a fifth of their entries missing; the last held-out row is
    empty.  The samples know the clones; every third splits clone 0 in two."""
    rng = np.random.RandomState(2024)
    S, N, M, Q, C = 12, 70, 33, 65, 4
    geno = (rng.random_sample((C, M)) < 0.5).astype(np.float64)
    clone = rng.permutation(np.arange(N) % C)
    a = np.tile(clone * 5 + 3, (S, 1))
    par = np.zeros((S, C + 1, M), dtype=np.float32)
    for s in range(S):
        soft = np.clip(geno + rng.normal(0, 0.02, geno.shape), 0.03, 0.97)
        par[s, :C] = soft
        if s % 3 == 0:
            half = np.flatnonzero(clone == 0)[::2]
            a[s, half] = 1                  # ranks: 1 -> 0, 3 -> 1, 8 -> 2 ...
            par[s] = np.concatenate([soft[:1], soft])
    truth = np.arange(Q) % C
    new = geno[truth].copy()
    flip = rng.random_sample(new.shape)
    new = np.where(new == 1, (flip >= 0.1).astype(float),
        (flip < 0.01).astype(float))
    new[rng.random_sample(new.shape) < 0.2] = np.nan
    new[Q - 1] = np.nan
    return (new, a, clone, par, np.full(S, 0.1), np.full(S, 0.01),
        np.full(S, 1.0), truth)


def test_held_out_cells_of_known_clones_are_recovered():
    new, a, clone, par, FN, FP, alpha, truth = clones_case()
    assert (a.shape, par.shape[2], new.shape[0]) == ((12, 70), 33, 65)
    t = postproc.place_cells(None, new, a, clone, par, FN, FP, alpha, PRIOR)
    seen = t['n_obs'] > 0
    assert seen.sum() == 64 and not seen[64]
    assert np.array_equal(t['cluster'][seen], truth[seen])
    assert (t['cluster_prob'][seen] > 0.5).all()
    # the empty row sits at the prior: the clones' sizes
    np.testing.assert_allclose(t['prob'][64], np.bincount(clone) / 71.0,
        rtol=0, atol=1e-12)
    assert t['lpd'][64] == pytest.approx(0, abs=1e-12)
    assert t['lpd_per_obs'][64] == 0
    assert (t['lpd'][seen] < 0).all()
    total = t['total']
    assert total['placed'] == np.bincount(t['cluster'][t['cluster'] >= 0],
        minlength=4).tolist()
    assert total['new'] == 0 and total['cells'] == 65
    assert total['samples'] == 12 and total['clusters'] == 4
    assert total['lpd'] == pytest.approx(t['lpd'].sum())
    assert total['mean_lpd_per_obs'] == pytest.approx(
        t['lpd'].sum() / t['n_obs'].sum())
    order = sorted(range(65), key=lambda i: (t['lpd_per_obs'][i], i))[:10]
    assert total['worst_cells'] == order


def test_a_cell_of_no_clone_opens_a_cluster():
    new, a, clone, par, FN, FP, alpha, truth = clones_case()
    geno = par[1, :4] > 0.5
    odd = (~geno[0]).astype(np.float64)         # the complement of clone 0
    far = [(odd != g).sum() for g in geno]
    assert min(far) >= 10
    t = postproc.place_cells(None, np.stack([odd, new[0]]), a, clone, par, FN,
        FP, np.full(12, 1.0), PRIOR)
    assert t['cluster'].tolist() == [-1, 0]
    assert t['cluster_prob'][0] == t['p_new'][0] > 0.5
    assert t['next_cluster'][0] == int(np.argmax(t['prob'][0]))
    assert t['next_cluster'][1] != 0
    assert t['total']['new'] == 1 and sum(t['total']['placed']) == 1


def test_ties_go_to_the_smaller_index():
    """two MPEAR clusters that split every sample cluster in halves"""
    rng = np.random.RandomState(8)
    N, M = 8, 5
    a = np.array([[0, 0, 0, 0, 1, 1, 1, 1]] * 3)
    labels = np.array([1, 0, 1, 0, 0, 1, 0, 1])
    par = np.clip(rng.random_sample((3, 2, M)), .1, .9).astype(np.float32)
    t = postproc.place_cells(None, new_cells(rng, 4, M), a, labels, par,
        [.1] * 3, [.01] * 3, [1e-6] * 3, PRIOR)
    assert np.array_equal(t['prob'][:, 0], t['prob'][:, 1])
    assert (t['cluster'] == 0).all() and (t['next_cluster'] == 1).all()
    assert np.array_equal(t['next_prob'], t['cluster_prob'])


def test_bad_arguments():
    rng = np.random.RandomState(9)
    a, par, FN, FP, alpha = samples(rng, 3, 10, 4, 6)
    labels = clustering(rng, 10, 2)
    new = new_cells(rng, 4, 6)
    with pytest.raises(ValueError, match='0, 1 or missing'):
        postproc.host_place(np.where(new == 1, 2.0, new), a, labels, par, FN,
            FP, alpha, PRIOR)
    with pytest.raises(ValueError, match='mutations'):
        postproc.host_place(new[:, :5], a, labels, par, FN, FP, alpha, PRIOR)
    with pytest.raises(ValueError, match='alpha'):
        postproc.host_place(new, a, labels, par, FN, FP, [1.0, 0.0, 1.0],
            PRIOR)
    with pytest.raises(ValueError, match='label'):
        postproc.host_place(new, a, labels[:-1], par, FN, FP, alpha, PRIOR)


# ---------------------------------------------------------------- the files
def test_save_placement_writes_the_two_files(tmp_path):
    new, a, clone, par, FN, FP, alpha, truth = clones_case()
    odd = (~(par[1, 0] > 0.5)).astype(np.float64)    # a cell of no clone
    new = np.concatenate([new[:6], odd[None, :], new[64:]])
    want = postproc.place_cells(None, new, a, clone, par, FN, FP, alpha,
        PRIOR)
    assert want['cluster'].tolist()[:7] == [0, 1, 2, 3, 0, 1, -1]
    # the labels of assignment.txt: cluster k of the tables is the k-th
    # smallest of them
    ids = [2, 5, 11, 40]
    assignment = np.array(ids)[clone]
    names = [f'held{i}' for i in range(8)]
    paths = bio.save_placement(str(tmp_path), 'mean', 'posterior', want,
        assignment, names)
    assert [os.path.basename(x) for x in paths] == list(NEW_FILES)
    Q, K = 8, 4
    with open(paths[0]) as f:
        rows = [ln.split('\t') for ln in f.read().splitlines()]
    assert rows[0] == COLUMNS + [str(i) for i in ids]
    assert len(rows) == Q + 1 and all(len(r) == 10 + K for r in rows)
    assert [r[0] for r in rows[1:]] == names
    for i, r in enumerate(rows[1:]):
        k = want['cluster'][i]
        assert r[1] == ('new' if k < 0 else str(ids[k]))
        nk = want['next_cluster'][i]
        assert r[3] == str(ids[nk] if nk >= 0 else -1)
        assert r[7] == str(want['n_obs'][i])
        for col, key in ((2, 'cluster_prob'), (4, 'next_prob'), (5, 'p_new'),
                (6, 'entropy'), (8, 'lpd'), (9, 'lpd_per_obs')):
            assert re.fullmatch(r'-?\d+\.\d{4}', r[col]), key
            assert r[col] == f'{want[key][i]:.4f}', key
        assert r[10:] == [f'{x:.4f}' for x in want['prob'][i]]
    assert rows[7][1] == 'new' and rows[8][7] == '0'
    with open(paths[1]) as f:
        lines = f.read().splitlines()
    assert [ln.split(':')[0] for ln in lines] == ['samples', 'cells',
        'clusters', 'placed', 'new', 'lpd', 'mean_lpd_per_obs', 'worst_cells']
    model = {k: v.strip() for k, v in (ln.split(':', 1) for ln in lines)}
    total = want['total']
    assert int(model['samples']) == 12
    assert int(model['cells']) == Q and int(model['clusters']) == K
    assert model['placed'].split() == [f'{ids[k]}:{n}'
        for k, n in enumerate(total['placed'])]
    assert int(model['new']) == total['new'] == 1
    assert model['lpd'] == f'{total["lpd"]:.4f}'
    assert model['mean_lpd_per_obs'] == f'{total["mean_lpd_per_obs"]:.4f}'
    assert [x.split(':')[0] for x in model['worst_cells'].split()] \
        == [names[i] for i in total['worst_cells']]
    # without names the cells are numbered
    other = tmp_path / 'bare'
    other.mkdir()
    paths = bio.save_placement(str(other), 'mean', 'posterior', want,
        assignment)
    with open(paths[0]) as f:
        assert [ln.split('\t')[0] for ln in f.read().splitlines()[1:]] \
            == [str(i) for i in range(Q)]


def test_binding_and_header_list_the_entry_points():
    for name in ('bnpc_post_place', 'bnpc_post_place_times'):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    assert hasattr(_lib.Posterior, 'place')
    assert hasattr(_lib.Posterior, 'place_times')
    with open(os.path.join(ROOT, 'include', 'bnpc_hip.h')) as f:
        header = f.read()
    assert re.search(r'\bint bnpc_post_place\(bnpc_post \*post, '
        r'const uint8_t \*codes', header)
    assert re.search(r'\bint bnpc_post_place_times\(bnpc_post \*post', header)
    assert 'libs/CRP.py:223-234' in header
    assert _lib.ABI_VERSION == 12
