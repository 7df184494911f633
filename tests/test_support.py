"""Per-cell cluster support and cluster similarity (-ps): the host side.
postproc.host_support against the definition taken straight from the samples,
postproc.cluster_support on constructed cases, the two tables save_outputs
writes, and the flag.  CPU only: the pair counts come from the NumPy stand-in
of tests/fake_device.py."""
import argparse
import os
import re

import numpy as np
import pytest

import run_BnpC
from bnpc_amd import _lib, postproc
from bnpc_amd import io as bio
from fake_device import FakePosterior
from test_outputs import golden_files, load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FILES = ('cell_support_posterior_mean.tsv',
    'cluster_similarity_posterior_mean.tsv')


def definition(a, labels, K):
    """differ_to[i][k] = sum over s of #{j : labels[j] == k,
    a[s][j] != a[s][i]}"""
    a, labels = np.asarray(a), np.asarray(labels)
    N = labels.size
    out = np.zeros((N, K), dtype=np.int64)
    for k in range(K):
        members = a[:, labels == k]                      # S x n_k
        for i in range(N):
            out[i, k] = np.count_nonzero(members != a[:, i:i + 1])
    return out


def random_case(rng, S, N, K, nlab=None):
    """S samples of N cells and a clustering compact in [0, K), in random
    cell order"""
    labels = rng.randint(0, K, N)
    labels[rng.permutation(N)[:K]] = np.arange(K)
    a = rng.randint(0, nlab or max(2, K // 2 + 1), (S, N))
    return a, labels


@pytest.mark.parametrize('S,N,K', [(1, 2, 1), (1, 2, 2), (7, 65, 4),
    (30, 130, 130), (12, 97, 1), (5, 40, 17)])
def test_host_support_is_the_definition(S, N, K):
    rng = np.random.RandomState(S * 1000 + N + K)
    a, labels = random_case(rng, S, N, K)
    got = postproc.host_support(FakePosterior(a).differ(), labels)
    assert got.dtype == np.int64 and got.shape == (N, K)
    assert np.array_equal(got, definition(a, labels, K))


def test_every_sample_equal_to_the_clustering():
    labels = np.array([2, 0, 0, 1, 2, 2, 1, 0, 2])
    a = np.tile(labels * 7 + 3, (5, 1))
    t = postproc.cluster_support(
        postproc.host_support(FakePosterior(a).differ(), labels), labels, 5)
    want = np.zeros((9, 3))
    want[np.arange(9), labels] = 1.0
    assert np.array_equal(t['support'], want)
    assert np.array_equal(t['own'], np.ones(9))
    assert np.array_equal(t['next_support'], np.zeros(9))
    # all other supports tie at 0: the smallest other index
    assert t['next_cluster'].tolist() == [0, 1, 1, 0, 0, 0, 0, 1, 0]
    assert np.array_equal(t['similarity'], np.eye(3))


def test_singleton_cluster_and_no_nan():
    labels = np.array([0, 1, 1, 1])
    a = np.array([[0, 0, 1, 1], [0, 1, 1, 2], [3, 3, 3, 3]])
    S = 3
    differ_to = postproc.host_support(FakePosterior(a).differ(), labels)
    assert np.array_equal(differ_to, definition(a, labels, 2))
    t = postproc.cluster_support(differ_to, labels, S)
    assert t['support'][0, 0] == 1.0 and t['own'][0] == 1.0
    assert t['similarity'][0, 0] == 1.0
    assert not np.isnan(t['support']).any()
    assert not np.isnan(t['similarity']).any()
    # cell 0 against the three members of cluster 1: differs 2 + 3 + 2 times
    # over 3 samples x 3 members
    assert t['support'][0, 1] == 1 - 5 / 9
    assert t['next_cluster'][0] == 1 and t['next_support'][0] == 1 - 5 / 9
    # block[0][1] = 5 over S * 1 * 3 pairs; block[1][1] over S * 3 * 2
    assert t['similarity'][0, 1] == t['similarity'][1, 0] == 1 - 5 / 9
    inside = differ_to[1:, 1].sum()
    assert t['similarity'][1, 1] == 1 - inside / (S * 6)


def test_one_cluster_has_no_next():
    rng = np.random.RandomState(1)
    a = rng.randint(0, 3, (6, 11))
    labels = np.zeros(11, dtype=int)
    t = postproc.cluster_support(
        postproc.host_support(FakePosterior(a).differ(), labels), labels, 6)
    assert t['support'].shape == (11, 1) and t['similarity'].shape == (1, 1)
    assert np.array_equal(t['next_cluster'], np.full(11, -1))
    assert np.array_equal(t['next_support'], np.zeros(11))
    assert np.array_equal(t['own'], t['support'][:, 0])


def test_a_tie_goes_to_the_smaller_index():
    # cell 0 (cluster 0) is as far from cluster 1 as from cluster 2; cell 3
    # (cluster 2) sits with cluster 1 and cluster 0 equally often
    labels = np.array([0, 1, 2, 2, 1, 0])
    a = np.array([[0, 0, 0, 1, 1, 0], [0, 1, 1, 0, 0, 0]])
    differ_to = definition(a, labels, 3)
    t = postproc.cluster_support(differ_to, labels, 2)
    assert t['support'][0, 1] == t['support'][0, 2]
    assert t['next_cluster'][0] == 1
    assert t['support'][3, 0] == t['support'][3, 1]
    assert t['next_cluster'][3] == 0
    assert t['next_support'][3] == t['support'][3, 0]


def test_similarity_is_symmetric_and_own_matches_the_table():
    rng = np.random.RandomState(2)
    a, labels = random_case(rng, 9, 70, 6, nlab=5)
    differ_to = postproc.host_support(FakePosterior(a).differ(), labels)
    t = postproc.cluster_support(differ_to, labels, 9)
    assert np.array_equal(t['similarity'], t['similarity'].T)
    assert np.array_equal(t['own'], t['support'][np.arange(70), labels])
    assert (t['next_cluster'] != labels).all()
    assert ((0 <= t['support']) & (t['support'] <= 1)).all()
    # straight from the definition, pair by pair
    same = (a[:, :, None] == a[:, None, :]).mean(axis=0)       # N x N
    n_k = np.bincount(labels)
    for k in range(6):
        for l in range(6):
            sub = same[np.ix_(labels == k, labels == l)]
            if k == l:
                want = (sub.sum() - n_k[k]) / (n_k[k] * (n_k[k] - 1))
            else:
                want = sub.mean()
            assert abs(t['similarity'][k, l] - want) < 1e-12


@pytest.fixture
def host_posterior(monkeypatch):
    monkeypatch.setattr(_lib, 'Posterior', FakePosterior)


def test_posterior_estimate_support(golden_dir, tmp_path, host_posterior):
    d, case, results = load_case(golden_dir, 'fixture', tmp_path / 'ref')
    data = bio.load_data(os.path.join(d, 'input.tsv'))
    plain = postproc.posterior_estimate(results, data)
    assert 'support' not in plain
    inf = postproc.posterior_estimate(results, data, support=True)
    assert sorted(set(inf) - set(plain)) == ['support']
    for key in ('assignment', 'cluster_genotypes', 'FN', 'FP', 'genotypes'):
        assert np.array_equal(inf[key], plain[key])
    pooled = postproc.concat_chain_results(results)['assignments']
    labels = np.asarray(inf['assignment'])
    want = postproc.cluster_support(postproc.host_support(
        FakePosterior(pooled).differ(), labels), labels, pooled.shape[0])
    assert sorted(inf['support']) == sorted(want)
    for key in want:
        assert np.array_equal(inf['support'][key], want[key]), key


def namespace(d, case, **more):
    return argparse.Namespace(estimator=case['estimator'],
        single_chains=case['single_chains'], verbosity=0, transpose=True,
        true_clusters=os.path.join(d, 'true_clusters.txt'),
        true_data=os.path.join(d, 'true_data.tsv'), **more)


def save(d, case, results, out, **more):
    out.mkdir()
    data, names = bio.load_data(os.path.join(d, 'input.tsv'), get_names=True)
    args = namespace(d, case, **more)
    run_BnpC.save_outputs(args, results, data, str(out), names)
    return args, names


def posterior_row(path):
    with open(path) as f:
        rows = [ln.rstrip('\n').split('\t') for ln in f]
    row, = [r for r in rows[1:] if r[:2] == ['mean', 'posterior']]
    return [int(x) for x in row[2].split()]


def test_save_outputs_writes_the_two_tables(golden_dir, tmp_path,
        host_posterior):
    d, case, results = load_case(golden_dir, 'fixture', tmp_path / 'ref')
    out = tmp_path / 'out'
    args, names = save(d, case, results, out, posterior_support=True)
    for name in NEW_FILES:
        assert (out / name).exists()
    assign = posterior_row(out / 'assignment.txt')
    N, ids = len(assign), sorted(set(assign))
    K = len(ids)
    pooled = postproc.concat_chain_results(results)['assignments']
    labels = np.searchsorted(ids, assign)
    want = postproc.cluster_support(postproc.host_support(
        FakePosterior(pooled).differ(), labels), labels, pooled.shape[0])

    rows = [ln.split('\t') for ln in
        (out / NEW_FILES[0]).read_text().splitlines()]
    assert rows[0] == ['cell', 'cluster', 'support', 'next_cluster',
        'next_support'] + [str(i) for i in ids]
    assert len(rows) == N + 1 and all(len(r) == 5 + K for r in rows)
    assert [r[0] for r in rows[1:]] == [str(x) for x in names[0].tolist()]
    assert [int(r[1]) for r in rows[1:]] == assign
    table = np.array([[float(x) for x in r[2:]] for r in rows[1:]])
    assert all(re.fullmatch(r'-?\d+\.\d{4}', x) for r in rows[1:]
        for x in [r[2]] + r[4:])
    assert np.abs(table[:, 0] - want['own']).max() <= 5e-5
    assert np.array_equal(table[:, 1],
        [ids[k] if k >= 0 else -1 for k in want['next_cluster']])
    assert np.abs(table[:, 2] - want['next_support']).max() <= 5e-5
    assert np.abs(table[:, 3:] - want['support']).max() <= 5e-5

    rows = [ln.split('\t') for ln in
        (out / NEW_FILES[1]).read_text().splitlines()]
    assert rows[0] == [''] + [str(i) for i in ids]
    assert [r[0] for r in rows[1:]] == [str(i) for i in ids]
    sim = np.array([[float(x) for x in r[1:]] for r in rows[1:]])
    assert sim.shape == (K, K)
    assert np.abs(sim - want['similarity']).max() <= 5e-5
    assert 'posterior_support: True\n' in (out / 'args.txt').read_text()
    # everything else is what a run without the flag writes
    plain = tmp_path / 'plain'
    save(d, case, results, plain)
    assert sorted(os.listdir(plain)) \
        == sorted(set(os.listdir(out)) - set(NEW_FILES))
    for name in os.listdir(plain):
        if name != 'args.txt':
            assert (plain / name).read_bytes() == (out / name).read_bytes()


def test_without_the_flag_nothing_changes(golden_dir, tmp_path,
        host_posterior):
    """Flag absent (the bare Namespace of the existing tests) or False: the
    files of a run that knows no such flag - the reference's genotype and
    metric tables of the golden case, the three run files, and an args.txt
    that lists the arguments it was given and nothing else."""
    d, case, results = load_case(golden_dir, 'fixture', tmp_path / 'ref')
    absent, false = tmp_path / 'absent', tmp_path / 'false'
    args, _ = save(d, case, results, absent)
    save(d, case, results, false, posterior_support=False)
    want = sorted(golden_files(d) + ['args.txt', 'assignment.txt',
        'errors.txt'])
    assert sorted(os.listdir(absent)) == want
    assert sorted(os.listdir(false)) == want
    for name in want:
        assert (absent / name).read_bytes() == (false / name).read_bytes()
        if name.startswith('genotypes_'):
            with open(os.path.join(d, name), 'rb') as f:
                assert (absent / name).read_bytes() == f.read()
    assert (absent / 'args.txt').read_text() == ''.join(
        f'{key}: {val}\n' for key, val in vars(args).items())
    assert 'posterior_support' not in (absent / 'args.txt').read_text()


def test_flag_and_its_check():
    args = run_BnpC.parse_args(['d.csv'])
    assert args.posterior_support is False
    assert 'posterior_support' not in vars(args)
    run_BnpC.check_args(args)
    for flag in ('-ps', '--posterior_support'):
        args = run_BnpC.parse_args(['d.csv', flag])
        assert args.posterior_support is True
        assert vars(args)['posterior_support'] is True
        run_BnpC.check_args(args)
    run_BnpC.check_args(run_BnpC.parse_args('d.csv -ps -e ML posterior'
        .split()))
    run_BnpC.check_args(run_BnpC.parse_args('d.csv -e ML'.split()))
    for ests in ('ML', 'ML MAP'):
        args = run_BnpC.parse_args(['d.csv', '-ps', '-e'] + ests.split())
        with pytest.raises(SystemExit, match='posterior'):
            run_BnpC.check_args(args)
        # main() stops there: before the input is looked at
        with pytest.raises(SystemExit, match='--posterior_support'):
            run_BnpC.main(args)


def test_pass_width_of_binding_and_header():
    with open(os.path.join(ROOT, 'include', 'bnpc_hip.h')) as f:
        kc, = re.findall(r'#define\s+BNPC_SUPPORT_KC\s+(\d+)', f.read())
    assert int(kc) == _lib.SUPPORT_KC
    assert 'bnpc_post_support' in _lib.SIGNATURES
    assert not hasattr(FakePosterior, 'support')    # the host path above
