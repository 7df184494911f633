"""The per-cell fit pass on the device (bnpc_post_cell_fit, through
_lib.Posterior.cell_fit) against the host loop it is pinned to
(postproc.host_cell_fit).

ll: rtol = atol = 1e-12, the project's figure for one likelihood evaluation
(tests/test_gpu_parity.py) - the device adds the mutations in another order.
mean, m2: array_equal with the host reduction of the device's own ll.
lme: within (S + 4) * 2**-52 + 2**-52 * |lme| of the host reduction of the
device's ll (exp and log within one ulp, S sequential adds of terms in (0, 1]
of which one is exactly 1), and inside [min, max] of its column.

The kernels' tiles: a workgroup of the sums kernel takes _lib.CELL_TILE = 8
cells of one sample and strides the mutations by 256, the data are packed 32
mutations to a word; the reduction takes 256 cells per workgroup.  A handle
needs two cells at least, so the cell count 1 is a slab of one cell of two."""
import os

import numpy as np
import pytest

from bnpc_amd import _lib, postproc
from bnpc_amd import io as bio

NAMES = ('mean', 'm2', 'lme', 'll')
ULP = 2.0 ** -52


def trace(rng, S, W, M):
    """float32 draws in (0, 1); some entries exactly 0, 1, 0.5 and a float32
    denormal"""
    p = rng.random_sample((S, W, M)).astype(np.float32)
    p[p == 0] = 0.25
    kind = rng.randint(0, 12, p.shape)
    p[kind == 0] = 0.0
    p[kind == 1] = 1.0
    p[kind == 2] = 0.5
    p[kind == 3] = 1e-42
    return p


def samples(rng, S, N, nlab):
    """a few labels per sample, on a random subset of [0, N)"""
    a = rng.randint(0, nlab, (S, N))
    if N > nlab:
        a = np.sort(rng.choice(N, nlab, replace=False))[a]
    return a.astype(np.int64)


def matrix(rng, N, M):
    """0 / 1 / NaN; where there is room, a row of each alone"""
    data = (rng.random_sample((N, M)) < 0.4).astype(np.float64)
    data[rng.random_sample((N, M)) < 0.3] = np.nan
    for row, val in zip(range(N - 1, 1, -1), (np.nan, 1.0, 0.0)):
        data[row] = val
    return data


def rates(rng, S):
    """different in every sample and far apart: FN near 0.3, FP near 1e-6"""
    return rng.uniform(0.25, 0.35, S), rng.uniform(0.5e-6, 2e-6, S)


def width(a):
    return max(np.unique(row).size for row in a)


def case(seed, S, N, M, nlab):
    rng = np.random.RandomState(seed)
    a = samples(rng, S, N, min(nlab, N))
    return (matrix(rng, N, M), a, trace(rng, S, width(a), M)) + rates(rng, S)


def reduction(ll):
    """the host loop's reductions of a given matrix, in its order"""
    S, N = ll.shape
    acc = np.zeros(N)
    for s in range(S):
        acc += ll[s]
    mean = acc / S
    m2, es, mx = np.zeros(N), np.zeros(N), ll.max(axis=0)
    for s in range(S):
        m2 += (ll[s] - mean) ** 2
        es += np.exp(ll[s] - mx)
    return mean, m2, mx + np.log(es) - np.log(S)


def compare(got, host):
    mean, m2, lme, ll = got
    S, N = host['ll'].shape
    assert ll.shape == (S, N) and ll.dtype == np.float64
    assert mean.shape == m2.shape == lme.shape == (N,)
    err = np.abs(ll - host['ll']) / (1 + np.abs(host['ll']))
    print(f'll: max |dev - host| / (1 + |host|) = {err.max():.3e}')
    np.testing.assert_allclose(ll, host['ll'], rtol=1e-12, atol=1e-12)
    r_mean, r_m2, r_lme = reduction(ll)
    assert np.array_equal(mean, r_mean), np.flatnonzero(mean != r_mean)[:5]
    assert np.array_equal(m2, r_m2), np.flatnonzero(m2 != r_m2)[:5]
    off = np.abs(lme - r_lme)
    print(f'lme: max |dev - host reduction| = {off.max():.3e}')
    assert (off <= (S + 4) * ULP + ULP * np.abs(lme)).all()
    assert (lme >= ll.min(axis=0)).all() and (lme <= ll.max(axis=0)).all()
    assert np.isfinite(ll).all()


def equal(got, want):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5])


def check(data, a, params, FN, FP, **how):
    host = postproc.host_cell_fit(data, a, params, FN, FP)
    post = _lib.Posterior(a)
    try:
        got = post.cell_fit(data, params, FN, FP, matrix=True, **how)
    finally:
        post.close()
    compare(got, host)
    return got, host


@pytest.mark.gpu
@pytest.mark.parametrize('M', [1, 31, 32, 33, 255, 256, 257, 513])
@pytest.mark.parametrize('N', [1, 7, 8, 9, 63, 64, 65, 129])
def test_edges_of_the_tiling(N, M):
    if N == 1:
        data, a, params, FN, FP = case(M, 5, 2, M, 2)
        got, host = check(data, a, params, FN, FP, slab=1)
    else:
        data, a, params, FN, FP = case(1000 * N + M, 5, N, M, 5)
        got, host = check(data, a, params, FN, FP)
    # FN and FP swapped are another model: it does not pass
    swapped = postproc.host_cell_fit(data, a, params, FP, FN)['ll']
    assert host['n_obs'].any()
    assert not np.allclose(got[3], swapped, rtol=1e-12, atol=1e-12)


@pytest.mark.gpu
def test_rows_of_one_kind_and_the_special_parameters():
    data, a, params, FN, FP = case(2, 6, 40, 70, 4)
    assert np.isnan(data[39]).all() and (data[38] == 1).all() \
        and (data[37] == 0).all()
    for x in (0.0, 1.0, 0.5, 1e-42):
        assert (params == np.float32(x)).sum() > 50
    assert np.float32(1e-42) > 0
    (mean, m2, lme, ll), host = check(data, a, params, FN, FP)
    # the missing-only cell: exactly nothing
    assert not ll[:, 39].any() and mean[39] == 0 and m2[39] == 0 \
        and lme[39] == 0
    assert host['n_obs'][39] == 0 and host['n_obs'][38] == 70
    assert (ll[:, 37:39] < 0).all()


@pytest.mark.gpu
def test_one_sample():
    data, a, params, FN, FP = case(3, 1, 30, 45, 4)
    (mean, m2, lme, ll), host = check(data, a, params, FN, FP)
    assert np.array_equal(mean, ll[0]) and not m2.any()
    assert np.array_equal(lme, ll[0])
    t = postproc.cell_fit(None, data, a, params, FN, FP)
    assert not t['p_waic'].any() and not t['sd_ll'].any()


@pytest.mark.gpu
def test_singletons_labels_up_to_n_minus_1_and_one_cluster():
    rng = np.random.RandomState(4)
    S, N, M = 9, 77, 70
    a = samples(rng, S, N, 6)
    a[2] = rng.permutation(N)               # W = N: every cell alone
    a[5] = np.arange(N)[::-1]
    a[6] = N - 1                            # one cluster, the largest label
    a[7] = 0
    assert a.max() == N - 1 and width(a) == N
    FN, FP = rates(rng, S)
    check(matrix(rng, N, M), a, trace(rng, S, N, M), FN, FP)
    # one cluster in every sample
    one = np.full((S, N), 5)
    check(matrix(rng, N, M), one, trace(rng, S, 1, M), FN, FP)


@pytest.mark.gpu
def test_chunks_and_slabs_give_the_same_bits():
    S, N, M = 23, 29, 75
    data, a, params, FN, FP = case(5, S, N, M, 7)
    want, host = check(data, a, params, FN, FP)
    post = _lib.Posterior(a)
    try:
        equal(post.cell_fit(data, params, FN, FP, matrix=True), want)
        for chunk in (1, 5, S, S + 27):
            for slab in (1, 8, 13, N):
                equal(post.cell_fit(data, params, FN, FP, chunk=chunk,
                    slab=slab, matrix=True), want)
        short = post.cell_fit(data, params, FN, FP, chunk=5, slab=13)
        assert short[3] is None
        equal(short[:3], want[:3])
        # the codes themselves, and missing as 3
        codes = np.where(np.isnan(data), 3, data).astype(np.uint8)
        equal(post.cell_fit(codes, params, FN, FP, matrix=True), want)
        equal(post.cell_fit(codes.astype(np.float64), params, FN, FP,
            matrix=True), want)
    finally:
        post.close()


def raw_call(post, codes, params, FN, FP, out):
    return _lib.load().bnpc_post_cell_fit(post._h, _lib.ptr(codes),
        _lib.ptr(params), params.shape[1], params.shape[2], _lib.ptr(FN),
        _lib.ptr(FP), 0, 0, *[_lib.ptr(o) for o in out])


@pytest.mark.gpu
def test_bad_input_is_code_2_and_the_handle_lives():
    S, N, M = 4, 12, 37
    data, a, params, FN, FP = case(6, S, N, M, 3)
    a[3, :4] = [0, 1, 2, 3]                 # sample 3 has >= 4 clusters
    W = width(a)
    params = trace(np.random.RandomState(7), S, W, M)
    codes = np.where(np.isnan(data), 3, data).astype(np.uint8)
    host = postproc.host_cell_fit(data, a, params, FN, FP)

    def untouched(post, codes, params, FN, FP):
        out = [np.full(N, 7.25), np.full(N, 7.25), np.full(N, 7.25),
            np.full((S, N), 7.25)]
        assert raw_call(post, codes, params, FN, FP, out) == 2
        assert all((o == 7.25).all() for o in out)

    post = _lib.Posterior(a)
    try:
        compare(post.cell_fit(codes, params, FN, FP, matrix=True), host)
        # a row too few for sample 3
        untouched(post, codes, np.ascontiguousarray(params[:, :W - 1]), FN,
            FP)
        with pytest.raises(RuntimeError, match='code 2'):
            post.cell_fit(data, params[:, :W - 1], FN, FP)
        for which, s, val in ((0, 2, 0.0), (1, 1, 1.0), (0, 0, np.nan),
                (1, 3, -0.1)):
            bad = [FN.copy(), FP.copy()]
            bad[which][s] = val
            untouched(post, codes, params, *bad)
        bad = codes.copy()
        bad[N - 1, M - 1] = 2
        untouched(post, bad, params, FN, FP)
        with pytest.raises(RuntimeError, match='code 2'):
            post.cell_fit(np.where(bad == 3, np.nan, bad), params, FN, FP)
        with pytest.raises(ValueError, match='samples'):
            post.cell_fit(data, params[:3], FN[:3], FP[:3])
        with pytest.raises(ValueError, match='cells'):
            post.cell_fit(data[:, :M - 1], params, FN, FP)
        compare(post.cell_fit(codes, params, FN, FP, matrix=True), host)
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
def test_posterior_estimate_with_fit(golden_dir, tmp_path):
    """The tables through the device against the same call through the host
    loop.  With E = 1e-12 (1 + max |ll|) the bound on a cell's ll: its mean
    moves by E at most, lme by E (it is 1-Lipschitz in the largest change)
    plus the reduction's own bound, and m2 = sum of d**2 with every deviation
    d moved by 2 E at most: |change| <= 4 E sum |d| + 4 S E**2
    <= 4 E sqrt(S m2) + 4 S E**2."""
    from test_outputs import load_case
    d, case_, results = load_case(golden_dir, 'fixture', tmp_path / 'ref')
    data = bio.load_data(os.path.join(d, 'input.tsv'))
    plain = postproc.posterior_estimate(results, data, fit=False)
    assert 'fit' not in plain
    inf = postproc.posterior_estimate(results, data, fit=True)
    assert sorted(set(inf) - set(plain)) == ['fit']
    for key in plain:
        assert np.array_equal(inf[key], plain[key]), key
    pooled = postproc.concat_chain_results(results)
    args = (data, pooled['assignments'], pooled['params'], pooled['FN'],
        pooled['FP'])
    want = postproc.cell_fit(None, *args)
    ll = postproc.host_cell_fit(*args)['ll']
    S, N = ll.shape
    got = inf['fit']
    assert got.keys() == want.keys()
    E = 1e-12 * (1 + np.abs(ll).max(axis=0))
    assert (np.abs(got['mean_ll'] - want['mean_ll']) <= E).all()
    assert (np.abs(got['lppd'] - want['lppd']) <= E + (S + 4) * ULP
        + ULP * np.abs(want['lppd'])).all()
    m2 = want['p_waic'] * (S - 1)
    room = (4 * E * np.sqrt(S * m2) + 4 * S * E ** 2) * (1 + 1e-9)
    assert (np.abs(got['p_waic'] - want['p_waic']) * (S - 1) <= room).all()
    assert np.array_equal(got['sd_ll'], np.sqrt(got['p_waic']))
    assert np.array_equal(got['n_obs'], want['n_obs'])
    assert np.array_equal(got['mean_ll_per_obs'],
        got['mean_ll'] / got['n_obs'])
    total = got['total']
    assert total['lppd'] == got['lppd'].sum()
    assert total['p_waic'] == got['p_waic'].sum()
    assert total['waic'] == -2 * (total['lppd'] - total['p_waic'])
    assert {k: total[k] for k in ('samples', 'cells', 'observations')} \
        == {k: want['total'][k] for k in ('samples', 'cells', 'observations')}
