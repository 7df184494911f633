"""The posterior genotype pass on the device (bnpc_post_genotypes, through
_lib.Posterior.genotypes) against the host loop it restates
(postproc.host_genotypes, utils.py:148-192): array_equal, no tolerance."""
import numpy as np
import pytest

from bnpc_amd import _lib, postproc


def make_case(rng, S, N, M, K, nlab, p_together=0.5, p_shared=0.0,
        never=(), spread=False, wide=None):
    """S samples of N cells with labels < nlab; K compact clusters; each
    cluster outside `never` is put together in a sample with probability
    p_together, on a label another cell carries with probability p_shared
    (together, not alone).  spread: the labels mapped onto a sorted random
    subset of [0, N) that includes N - 1."""
    cl = rng.randint(0, K, size=N)
    cl[rng.permutation(N)[:K]] = np.arange(K)
    a = rng.randint(0, nlab, size=(S, N))
    for k in range(K):
        cells = np.flatnonzero(cl == k)
        if k in never:
            # at least two labels in every sample
            if cells.size > 1:
                for s in range(S):
                    if np.unique(a[s, cells]).size == 1:
                        a[s, cells[0]] = (a[s, cells[1]] + 1) % nlab
            continue
        for s in range(S):
            if rng.random_sample() < p_together:
                if rng.random_sample() < p_shared and cells.size < N:
                    other = rng.choice(np.flatnonzero(cl != k))
                    a[s, cells] = a[s, other]
                else:
                    a[s, cells] = rng.randint(0, nlab)
    if spread:
        pool = rng.choice(N - 1, size=nlab - 1, replace=False)
        perm = np.sort(np.append(pool, N - 1))
        a = perm[a]
    width = max(np.unique(row).size for row in a) + (wide or 0)
    params = rng.random_sample((S, width, M)).astype(np.float32)
    return a.astype(np.int64), cl, params


def check(a, cl, params, chunk=0):
    want = postproc.host_genotypes(a, cl, params)
    post = _lib.Posterior(a)
    try:
        got = post.genotypes(cl, params, chunk=chunk)
    finally:
        post.close()
    assert got.shape == want.shape
    assert np.array_equal(got, want), np.abs(got - want).max()
    return want


def kinds(a, cl):
    """(clusters never together, clusters together but never alone)"""
    never, shared = 0, 0
    for k in np.unique(cl):
        sub = a[:, cl == k]
        oth = a[:, cl != k]
        tog = (sub == sub[:, :1]).all(axis=1)
        if not tog.any():
            never += 1
            continue
        alone = np.array([not (oth[s] == sub[s, 0]).any() for s in range(len(a))])
        if not (tog & alone).any():
            shared += 1
    return never, shared


@pytest.mark.gpu
def test_one_sample_two_cells():
    a = np.array([[0, 1]])
    params = np.array([[[0.25, 0.5, 0.125], [0.75, 1.0, 0.0]]],
        dtype=np.float32)
    check(a, np.array([0, 0]), params)          # one cluster, never together
    check(a, np.array([0, 1]), params)          # two singletons
    check(a, np.array([1, 0]), params)
    check(np.array([[1, 1]]), np.array([0, 0]), params)


@pytest.mark.gpu
@pytest.mark.parametrize('S,N,M,K,nlab', [(3, 7, 5, 3, 4), (37, 101, 67, 6, 9),
    (64, 129, 130, 11, 30), (50, 300, 1, 20, 60)])
def test_ragged_sizes(S, N, M, K, nlab):
    rng = np.random.RandomState(S + N + M)
    check(*make_case(rng, S, N, M, K, nlab, never=(1,)))


@pytest.mark.gpu
def test_together_but_never_alone():
    rng = np.random.RandomState(5)
    a, cl, params = make_case(rng, 40, 90, 33, 8, 20, p_together=0.6,
        p_shared=1.0)
    never, shared = kinds(a, cl)
    assert shared >= 4
    check(a, cl, params)


@pytest.mark.gpu
def test_never_together_dot_branch():
    """Clusters that are never together, one spanning more than 4 labels in
    every sample (the host's np.dot sums more than 4 rows)."""
    rng = np.random.RandomState(6)
    a, cl, params = make_case(rng, 30, 200, 45, 5, 25, never=(0, 2, 4))
    big = np.flatnonzero(cl == 0)
    assert big.size > 20
    assert all(np.unique(a[s, big]).size > 4 for s in range(a.shape[0]))
    never, _ = kinds(a, cl)
    assert never == 3
    check(a, cl, params)


@pytest.mark.gpu
def test_singletons_and_labels_up_to_n_minus_1():
    rng = np.random.RandomState(7)
    N = 150
    a, cl, params = make_case(rng, 25, N, 40, N, 60, spread=True, wide=3)
    assert a.max() == N - 1
    check(a, cl, params)
    a, cl, params = make_case(rng, 25, N, 40, 12, 80, spread=True,
        never=(3,))
    check(a, cl, params)


@pytest.mark.gpu
def test_hundreds_of_clusters():
    rng = np.random.RandomState(8)
    a, cl, params = make_case(rng, 60, 2000, 70, 300, 400, p_together=0.3,
        p_shared=0.3, never=(0, 150))
    check(a, cl, params)


@pytest.mark.gpu
def test_past_the_lds_threshold():
    """N = 80 000: the flags pass's working set (2.25 N bytes) leaves LDS for
    global memory; N = 340 000: the histogram pass's (N / 2 bytes) too."""
    rng = np.random.RandomState(9)
    check(*make_case(rng, 3, 80000, 9, 25, 40, never=(2,)))
    check(*make_case(rng, 2, 340000, 3, 6, 12, never=(1,)))


@pytest.mark.gpu
def test_streamed_in_chunks():
    rng = np.random.RandomState(10)
    a, cl, params = make_case(rng, 45, 120, 50, 9, 15, p_shared=0.3,
        never=(4,))
    want = check(a, cl, params)
    for chunk in (1, 7, 44, 45, 100):
        assert np.array_equal(check(a, cl, params, chunk=chunk), want)


@pytest.mark.gpu
def test_float64_trace_with_padding():
    """A pooled trace padded with float64 zeros converts losslessly."""
    rng = np.random.RandomState(11)
    a, cl, params = make_case(rng, 20, 64, 16, 4, 6)
    params = np.pad(params.astype(np.float64), [(0, 0), (0, 2), (0, 0)])
    check(a, cl, params)


@pytest.mark.gpu
def test_bad_input_is_an_error():
    a = np.array([[0, 1, 2], [0, 0, 3]])        # label 3 >= N
    params = np.zeros((2, 4, 2), dtype=np.float32)
    post = _lib.Posterior(a)
    try:
        with pytest.raises(RuntimeError, match='code 2'):
            post.genotypes(np.array([0, 0, 1]), params)
    finally:
        post.close()
    a = np.array([[0, 1, 2], [0, 0, 2]])
    post = _lib.Posterior(a)
    try:
        with pytest.raises(RuntimeError, match='code 2'):   # cluster 1 empty
            post.genotypes(np.array([0, 0, 2]), params)
        with pytest.raises(RuntimeError, match='code 2'):   # row 2 of 2
            post.genotypes(np.array([0, 1, 2]), params[:, :2])
    finally:
        post.close()


@pytest.mark.gpu
def test_cli_writes_genotypes_and_metrics(golden_dir, tmp_path):
    """run_BnpC.py on example_data.csv with -tc / -td: the genotype tables and
    the three metric files; the posterior table is the one written from
    posterior_estimate's own result; -tc / -td leave args (but for the two
    paths), assignment.txt and errors.txt as they are without them."""
    import contextlib
    import io
    import os
    import run_BnpC
    from bnpc_amd import io as bio
    src = os.path.join(golden_dir, 'example_data.csv')
    data = bio.load_data(src)
    rng = np.random.RandomState(3)
    tc, td = tmp_path / 'true_clusters.txt', tmp_path / 'true_data.csv'
    tc.write_text(' '.join(str(x) for x in rng.randint(0, 5, data.shape[0])))
    truth = np.where(np.isnan(data), 3, data).astype(int).T
    truth[0, :3] = 3
    td.write_text('\n'.join(' '.join(str(x) for x in row) for row in truth))
    base = [src, '-n', '1', '-s', '120', '--seed', '42', '-np', '-e',
        'posterior', 'ML', 'MAP', '-v', '0', '--debug']
    with_truth, without = tmp_path / 'with', tmp_path / 'without'
    with contextlib.redirect_stdout(io.StringIO()):
        results = run_BnpC.main(run_BnpC.parse_args(base + ['-o',
            str(with_truth), '-tc', str(tc), '-td', str(td)]))
        run_BnpC.main(run_BnpC.parse_args(base + ['-o', str(without)]))
    files = set(os.listdir(with_truth))
    for est in ('posterior', 'ML', 'MAP'):
        assert f'genotypes_{est}_mean.tsv' in files
    assert {'V_measure.txt', 'ARI.txt', 'hammingDist.txt'} <= files
    for name in ('V_measure.txt', 'ARI.txt', 'hammingDist.txt'):
        rows = (with_truth / name).read_text().splitlines()
        assert [r.split('\t')[:2] for r in rows[1:]] == [['mean', 'posterior'],
            ['mean', 'ML'], ['mean', 'MAP']]
        low = -1 if name == 'ARI.txt' else 0        # ARI below chance < 0
        assert all(low <= float(r.split('\t')[2]) <= 1 for r in rows[1:])
    for name in ('assignment.txt', 'errors.txt'):
        assert (with_truth / name).read_bytes() == (without / name).read_bytes()
    strip = lambda p: [ln for ln in p.read_text().splitlines()     # noqa: E731
        if not ln.startswith(('output:', 'true_clusters:', 'true_data:',
            'time:'))]
    assert strip(with_truth / 'args.txt') == strip(without / 'args.txt')
    inf = postproc.posterior_estimate(results, data)
    again = tmp_path / 'again'
    again.mkdir()
    written = bio.save_geno(str(again), 'mean', 'posterior',
        inf['cluster_genotypes'], inf['cluster_of'], inf['assignment'])
    for path in written:
        name = os.path.basename(path)
        assert (with_truth / name).read_bytes() == (again / name).read_bytes()
    assert np.array_equal(
        inf['cluster_genotypes'][inf['cluster_of']], inf['genotypes'])
