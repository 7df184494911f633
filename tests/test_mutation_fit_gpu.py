"""The per-mutation fit pass on the device (bnpc_post_mutation_fit, through
_lib.Posterior.mutation_fit) against the host loop it is pinned to
(postproc.host_mutation_fit).

call1_obs1, call1_obs0: array_equal (exact integers).
efn, efp, eg1: array_equal - multiplies, adds and correctly rounded divides in
a pinned order.
ll: rtol = atol = 1e-12, the project's figure for one likelihood evaluation
(tests/test_gpu_parity.py) - the device's log is its own.
sum_ll, sum_ll2: array_equal with the host reduction of the device's own ll.

The kernels' tiles: the cells go 64 to a lane mask, a wave of the counting
kernel takes 64 mutations of one sample and holds _lib.MUT_FIT_ROWS = 32
cluster rows of counts in LDS - a sample with more takes its rows in passes.
The cases are those of tests/test_cell_fit_gpu.py: a trace with entries
exactly 0, 1, 0.5 and a float32 denormal, 30 % missing data with rows of one
kind, error rates that differ per sample."""
import numpy as np
import pytest

from bnpc_amd import _lib, postproc
from test_cell_fit_gpu import case, matrix, rates, samples, trace, width

NAMES = ('sum_ll', 'sum_ll2', 'efn', 'efp', 'eg1', 'call1_obs1',
    'call1_obs0', 'll')


def compare(got, host):
    S, M = host['ll'].shape
    for name, g in zip(NAMES, got):
        assert g.shape == ((S, M) if name == 'll' else (M,)), name
        assert g.dtype == (np.int64 if name.startswith('call')
            else np.float64), name
    out = dict(zip(NAMES, got))
    for key in ('call1_obs1', 'call1_obs0', 'efn', 'efp', 'eg1'):
        assert np.array_equal(out[key], host[key]), \
            (key, np.flatnonzero(out[key] != host[key])[:5])
    ll = out['ll']
    err = np.abs(ll - host['ll']) / (1 + np.abs(host['ll']))
    print(f'll: max |dev - host| / (1 + |host|) = {err.max():.3e}')
    np.testing.assert_allclose(ll, host['ll'], rtol=1e-12, atol=1e-12)
    assert np.isfinite(ll).all()
    sums = postproc.mutation_fit_sums(ll)
    for key in ('sum_ll', 'sum_ll2'):
        assert np.array_equal(out[key], sums[key]), \
            (key, np.flatnonzero(out[key] != sums[key])[:5])


def equal(got, want):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5])


def check(data, a, params, FN, FP, **how):
    host = postproc.host_mutation_fit(data, a, params, FN, FP)
    post = _lib.Posterior(a)
    try:
        got = post.mutation_fit(data, params, FN, FP, matrix=True, **how)
    finally:
        post.close()
    compare(got, host)
    return got, host


@pytest.mark.gpu
@pytest.mark.parametrize('M', [1, 63, 64, 65, 129])
@pytest.mark.parametrize('N', [2, 63, 64, 65, 129])
def test_edges_of_the_tiling(N, M):
    data, a, params, FN, FP = case(1000 * N + M, 5, N, M, 5)
    got, host = check(data, a, params, FN, FP)
    assert (host['n1'] + host['n0']).any()
    # FN and FP swapped are another model: it does not pass
    swapped = postproc.host_mutation_fit(data, a, params, FP, FN)
    assert not np.allclose(got[7], swapped['ll'], rtol=1e-12, atol=1e-12)
    assert not np.array_equal(got[4], swapped['eg1'])


@pytest.mark.gpu
def test_columns_of_one_kind_and_the_special_parameters():
    data, a, params, FN, FP = case(2, 6, 40, 70, 4)
    data[:, 3], data[:, 4], data[:, 5] = np.nan, 1.0, 0.0
    for x in (0.0, 1.0, 0.5, 1e-42):
        assert (params == np.float32(x)).sum() > 50
    got, host = check(data, a, params, FN, FP)
    # the missing-only column: exactly nothing
    for name, g in zip(NAMES, got):
        assert not g[..., 3].any(), name
    assert (got[7][:, 4:6] < 0).all()
    assert not got[6][4] and not got[5][5]      # no 0 in column 4, no 1 in 5


@pytest.mark.gpu
@pytest.mark.parametrize('N', [64, 65, 300])
def test_every_cell_its_own_cluster(N):
    """64 distinct ranks in one block; a block of one cell; ranks past one
    byte"""
    rng = np.random.RandomState(N)
    S, M = 3, 70
    a = np.stack([rng.permutation(N) for _ in range(S)])
    a[1] = np.arange(N)[::-1]
    assert width(a) == N > _lib.MUT_FIT_ROWS
    FN, FP = rates(rng, S)
    check(matrix(rng, N, M), a, trace(rng, S, N, M), FN, FP)


@pytest.mark.gpu
def test_one_cluster_and_one_sample():
    rng = np.random.RandomState(4)
    S, N, M = 4, 77, 70
    FN, FP = rates(rng, S)
    one = np.full((S, N), 5)
    check(matrix(rng, N, M), one, trace(rng, S, 1, M), FN, FP)
    data, a, params, FN, FP = case(3, 1, 30, 45, 4)
    got, host = check(data, a, params, FN, FP)
    assert np.array_equal(got[0], got[7][0])


@pytest.mark.gpu
@pytest.mark.parametrize('D', [_lib.MUT_FIT_ROWS - 1, _lib.MUT_FIT_ROWS,
    _lib.MUT_FIT_ROWS + 1, 2 * _lib.MUT_FIT_ROWS + 1])
def test_rows_around_the_lds_tile(D):
    """exactly D clusters in every sample: one pass that is nearly full, one
    that is full, a second pass of one row, a third"""
    rng = np.random.RandomState(D)
    S, N, M = 3, 150, 66
    a = np.empty((S, N), dtype=np.int64)
    for s in range(S):
        labels = np.sort(rng.choice(N, D, replace=False))
        a[s] = labels[rng.permutation(np.arange(N) % D)]
    assert all(np.unique(row).size == D for row in a)
    FN, FP = rates(rng, S)
    check(matrix(rng, N, M), a, trace(rng, S, D, M), FN, FP)


@pytest.mark.gpu
def test_chunks_hints_and_calls_give_the_same_bits():
    S, N, M = 7, 131, 75
    data, a, params, FN, FP = case(5, S, N, M, 7)
    want, host = check(data, a, params, FN, FP)
    rng = np.random.RandomState(8)
    post = _lib.Posterior(a)
    try:
        equal(post.mutation_fit(data, params, FN, FP, matrix=True), want)
        for chunk in (1, 2, S, S + 27):
            equal(post.mutation_fit(data, params, FN, FP, chunk=chunk,
                matrix=True), want)
        hints = (np.sort(a[0]), np.sort(a[0])[::-1], a[3], np.arange(N),
            rng.randint(-5, 5, N), np.zeros(N, dtype=int))
        for hint in hints:
            for chunk in (0, 2):
                equal(post.mutation_fit(data, params, FN, FP, order=hint,
                    chunk=chunk, matrix=True), want)
        short = post.mutation_fit(data, params, FN, FP, chunk=2)
        assert short[7] is None
        equal(short[:7], want[:7])
        # the codes themselves, and missing as 3
        codes = np.where(np.isnan(data), 3, data).astype(np.uint8)
        equal(post.mutation_fit(codes, params, FN, FP, matrix=True), want)
        with pytest.raises(ValueError, match='labels'):
            post.mutation_fit(data, params, FN, FP, order=np.arange(N - 1))
        times = post.mutation_fit_times(data, params, FN, FP, chunk=2)
        assert len(times) == 5 and all(t >= 0 for t in times)
        assert times[2] > 0 and times[3] == 0
    finally:
        post.close()


def raw_call(post, codes, params, FN, FP, out):
    return _lib.load().bnpc_post_mutation_fit(post._h, _lib.ptr(codes),
        _lib.ptr(params), params.shape[1], params.shape[2], _lib.ptr(FN),
        _lib.ptr(FP), None, 0, *[_lib.ptr(o) for o in out])


@pytest.mark.gpu
def test_bad_input_is_code_2_and_the_handle_lives():
    S, N, M = 4, 70, 37
    data, a, params, FN, FP = case(6, S, N, M, 3)
    a[3, :4] = [0, 1, 2, 3]                 # sample 3 has >= 4 clusters
    W = width(a)
    params = trace(np.random.RandomState(7), S, W, M)
    codes = np.where(np.isnan(data), 3, data).astype(np.uint8)
    host = postproc.host_mutation_fit(data, a, params, FN, FP)

    def untouched(post, codes, params, FN, FP):
        out = [np.full(M, 7.25) for _ in range(5)] \
            + [np.full(M, 725, dtype=np.int64) for _ in range(2)] \
            + [np.full((S, M), 7.25)]
        assert raw_call(post, codes, params, FN, FP, out) == 2
        assert all((o == 7.25).all() for o in out[:5] + out[7:])
        assert all((o == 725).all() for o in out[5:7])

    post = _lib.Posterior(a)
    try:
        compare(post.mutation_fit(codes, params, FN, FP, matrix=True), host)
        # a row too few for sample 3
        untouched(post, codes, np.ascontiguousarray(params[:, :W - 1]), FN,
            FP)
        with pytest.raises(RuntimeError, match='code 2'):
            post.mutation_fit(data, params[:, :W - 1], FN, FP)
        for which, s, val in ((0, 2, 0.0), (1, 1, 1.0), (0, 0, np.nan),
                (1, 3, -0.1)):
            bad = [FN.copy(), FP.copy()]
            bad[which][s] = val
            untouched(post, codes, params, *bad)
        for at in ((N - 1, M - 1), (0, 0), (65, 5)):
            bad = codes.copy()
            bad[at] = 2
            untouched(post, bad, params, FN, FP)
        with pytest.raises(RuntimeError, match='code 2'):
            post.mutation_fit(np.where(bad == 3, np.nan, bad), params, FN, FP)
        with pytest.raises(ValueError, match='samples'):
            post.mutation_fit(data, params[:3], FN[:3], FP[:3])
        with pytest.raises(ValueError, match='cells'):
            post.mutation_fit(data[:, :M - 1], params, FN, FP)
        compare(post.mutation_fit(codes, params, FN, FP, matrix=True), host)
    finally:
        post.close()
    wrong = a.copy()
    wrong[1, 5] = N                         # a label >= N
    post = _lib.Posterior(wrong)
    try:
        untouched(post, codes, params, FN, FP)
        untouched(post, codes, params, FN, FP)
        assert post.differ().shape == (N * (N - 1) // 2,)
    finally:
        post.close()


@pytest.mark.gpu
def test_tables_through_the_device():
    """postproc.mutation_fit through the handle: the integers and the rates
    made of efn, efp, eg1 alone are those of the host loop, bit for bit"""
    S, N, M = 6, 90, 50
    data, a, params, FN, FP = case(9, S, N, M, 5)
    want = postproc.mutation_fit(None, data, a, params, FN, FP)
    post = _lib.Posterior(a)
    try:
        got = postproc.mutation_fit(post, data, a, params, FN, FP,
            order=a[2])
    finally:
        post.close()
    assert got.keys() == want.keys()
    for key in ('n_obs', 'n_ones', 'n_zeros', 'prevalence', 'FN_model',
            'FP_model', 'FN_call', 'FP_call', 'eg1'):
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    np.testing.assert_allclose(got['mean_ll'], want['mean_ll'], rtol=1e-12,
        atol=1e-12)
    for key in ('samples', 'mutations', 'observations', 'FN_model',
            'FP_model', 'FN_call', 'FP_call', 'FN', 'FP'):
        assert got['total'][key] == want['total'][key], key
