"""The support pass on the device (bnpc_post_support, through
_lib.Posterior.support) against the host loop it restates
(postproc.host_support) and against the kernels that already read the same
pair counts: array_equal on int64, no tolerance."""
import contextlib
import io
import os

import numpy as np
import pytest

from bnpc_amd import _lib, postproc
from bnpc_amd import io as bio

KC = _lib.SUPPORT_KC        # clusters per pass of the kernel


def samples(rng, S, N, nlab):
    return rng.randint(0, nlab, (S, N)).astype(np.int64)


def clustering(rng, N, K):
    """compact in [0, K), in random cell order"""
    labels = rng.randint(0, K, N)
    labels[rng.permutation(N)[:K]] = np.arange(K)
    return labels


def check(post, differ, labels):
    got = post.support(labels)
    want = postproc.host_support(differ, labels)
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    return got


@pytest.mark.gpu
@pytest.mark.parametrize('S', [1, 33])
@pytest.mark.parametrize('N', [2, 63, 64, 65, 129, 200])
def test_edges_of_the_tiling(N, S):
    rng = np.random.RandomState(100 * N + S)
    a = samples(rng, S, N, 5)
    post = _lib.Posterior(a)
    try:
        differ = post.differ()
        check(post, differ, np.zeros(N, dtype=int))             # K = 1
        check(post, differ, rng.permutation(N))                 # K = N
        for K in sorted({min(2, N), min(7, N)}):
            check(post, differ, clustering(rng, N, K))
        # the first and the last 64-cell block hold a single cluster each
        last = 64 * ((N - 1) // 64)
        if last > 0:
            labels = np.zeros(N, dtype=int)
            labels[last:] = 1
            if last > 64:
                labels[64:last] = 2 + clustering(rng, last - 64,
                    min(3, last - 64))
            check(post, differ, labels)
    finally:
        post.close()


@pytest.fixture(scope='module')
def post600():
    rng = np.random.RandomState(600)
    a = samples(rng, 5, 600, 9)
    post = _lib.Posterior(a)
    yield post, post.differ(), rng
    post.close()


@pytest.mark.gpu
@pytest.mark.parametrize('K', [KC - 1, KC, KC + 1, 2 * KC + 3])
def test_pass_boundary(post600, K):
    post, differ, rng = post600
    check(post, differ, clustering(rng, 600, K))


@pytest.mark.gpu
def test_two_thousand_singletons():
    rng = np.random.RandomState(2000)
    a = samples(rng, 3, 2000, 11)
    post = _lib.Posterior(a)
    try:
        got = check(post, post.differ(), rng.permutation(2000))
        assert got.sum() == 2 * post.differ_sum
    finally:
        post.close()


@pytest.mark.gpu
def test_invariants_against_the_existing_kernels():
    """N = 6000: 94 x 94 tiles, more workgroups than one round of the chip's
    compute units takes at K = 40."""
    rng = np.random.RandomState(6000)
    N, S, K = 6000, 4, 40
    a = samples(rng, S, N, 30)
    labels = clustering(rng, N, K)
    post = _lib.Posterior(a)
    try:
        got = post.support(labels)
        assert got.shape == (N, K) and got.dtype == np.int64
        assert got.sum() == 2 * post.differ_sum
        assert got[np.arange(N), labels].sum() \
            == 2 * post.mpear_sums(labels[None])[0]
    finally:
        post.close()
    for i in rng.choice(N, 16, replace=False):
        counts = (a != a[:, i:i + 1]).sum(axis=0)
        want = np.bincount(labels, weights=counts, minlength=K) \
            .astype(np.int64)
        assert np.array_equal(got[i], want), i


@pytest.mark.gpu
def test_bad_input_is_an_error():
    """Rejected on the host, before anything is launched; the Posterior is
    usable afterwards."""
    rng = np.random.RandomState(7)
    a = samples(rng, 4, 70, 3)
    post = _lib.Posterior(a)
    try:
        differ = post.differ()
        good = clustering(rng, 70, 3)
        bad = good.copy()
        bad[5] = 3
        with pytest.raises(RuntimeError, match='code 2'):   # a label == K
            post.support(bad, K=3)
        check(post, differ, good)
        bad = good.copy()
        bad[69] = -1
        with pytest.raises(RuntimeError, match='code 2'):   # negative
            post.support(bad)
        check(post, differ, good)
        with pytest.raises(RuntimeError, match='code 2'):   # cluster 3 empty
            post.support(np.where(good == 2, 4, good))
        check(post, differ, good)
        with pytest.raises(RuntimeError, match='code 2'):
            post.support(good, K=65534)
        check(post, differ, good)
    finally:
        post.close()


@pytest.fixture(scope='module')
def cli_runs(tmp_path_factory):
    """run_BnpC.py in process on example_data.csv, 120 steps, with and
    without -ps: (data, the chain's results, both output directories)"""
    import run_BnpC
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)),
        'golden')
    src = os.path.join(golden, 'example_data.csv')
    tmp = tmp_path_factory.mktemp('support_cli')
    base = [src, '-n', '1', '-s', '120', '--seed', '42', '-np', '-e',
        'posterior', 'ML', '-v', '0', '--debug']
    with_ps, without = tmp / 'with', tmp / 'without'
    with contextlib.redirect_stdout(io.StringIO()):
        results = run_BnpC.main(run_BnpC.parse_args(base + ['-ps', '-o',
            str(with_ps)]))
        run_BnpC.main(run_BnpC.parse_args(base + ['-o', str(without)]))
    return bio.load_data(src), results, with_ps, without


@pytest.mark.gpu
def test_posterior_estimate_with_support(cli_runs):
    data, results, _, _ = cli_runs
    plain = postproc.posterior_estimate(results, data)
    inf = postproc.posterior_estimate(results, data, support=True)
    assert 'support' not in plain
    for key in ('assignment', 'cluster_genotypes', 'FN', 'FP'):
        assert np.array_equal(inf[key], plain[key]), key
    pooled = postproc.concat_chain_results(results)['assignments']
    labels = np.asarray(inf['assignment'])
    want = postproc.cluster_support(postproc.host_support(
        _lib.codist(pooled), labels), labels, pooled.shape[0])
    assert sorted(inf['support']) == sorted(want)
    for key in want:
        assert np.array_equal(inf['support'][key], want[key]), key


@pytest.mark.gpu
def test_cli_writes_the_support_tables(cli_runs):
    _, _, with_ps, without = cli_runs
    new = {'cell_support_posterior_mean.tsv',
        'cluster_similarity_posterior_mean.tsv'}
    assert new <= set(os.listdir(with_ps))
    assert set(os.listdir(without)) == set(os.listdir(with_ps)) - new
    for name in os.listdir(without):
        if name in ('assignment.txt', 'errors.txt') \
                or name.startswith('genotypes_'):
            assert (without / name).read_bytes() \
                == (with_ps / name).read_bytes(), name
    assign = bio.load_txt(str(with_ps / 'assignment.txt'))   # posterior row
    ids = sorted(set(assign))
    rows = [ln.split('\t') for ln in
        (with_ps / 'cell_support_posterior_mean.tsv').read_text()
        .splitlines()]
    assert rows[0][5:] == [str(i) for i in ids]
    assert [int(r[1]) for r in rows[1:]] == assign
    for r in rows[1:]:
        own = ids.index(int(r[1]))
        assert r[2] == r[5 + own]
        assert int(r[3]) != int(r[1])
        if len(ids) > 1:
            assert r[4] == r[5 + ids.index(int(r[3]))]
            assert float(r[4]) == max(float(x) for k, x in enumerate(r[5:])
                if k != own)
    sim = [ln.split('\t') for ln in
        (with_ps / 'cluster_similarity_posterior_mean.tsv').read_text()
        .splitlines()]
    assert sim[0] == [''] + [str(i) for i in ids]
    assert [r[0] for r in sim[1:]] == [str(i) for i in ids]
    table = np.array([[float(x) for x in r[1:]] for r in sim[1:]])
    assert table.shape == (len(ids), len(ids))
    assert np.array_equal(table, table.T)
    assert 'posterior_support: True' in (with_ps / 'args.txt').read_text()
    assert 'posterior_support' not in (without / 'args.txt').read_text()
