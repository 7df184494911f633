"""The placement pass on the device (bnpc_post_place, through
_lib.Posterior.place) against the host loop it is pinned to
(postproc.host_place).

scores: rtol = atol = 1e-12 of the host's (postproc.place_scores), the
project's figure for one likelihood evaluation (tests/test_gpu_parity.py): the
device's log in the tables; the NaN pattern is exactly the host's.

The reductions are compared with the host reduction (postproc.place_reduce) of
the device's own scores.  Both sides run the same +, x, / on the same scores;
they differ in exp and log, each taken to be within one ulp u = 2**-52 of the
true value on either side, and in what follows from that.  Per sample and new
cell, with C = K_s + 1 candidates, A the largest |y_c|, Lw the largest
|log n_c| or |log alpha| and Lna = log(N + alpha):
  y_c = score_c + log-weight differs by Ey = u (2 Lw + A): two ulps of the
      log-weight, and the sum rounded again; so does mx
  d = y_c - mx by 2 Ey + u |d|, and e_c = exp(d) by e (2 Ey + 2 u) + u e |d|,
      with e |d| <= 0.37
  es >= 1, the sum of C of them, by es Res with Res = 2 Ey + (1.4 C + 2) u
  pr_c = e_c / es by pr (4 Ey + (1.4 C + 5) u) + 0.37 u, and a sample's term of
      prob_sum or new_sum - at most C products with shares in [0, 1], the pr
      summing to 1 - by Et = 4 Ey + (3 C + 6) u
  lp = (mx + log(es)) - Lna by
      Elp = 3 Ey + (1.4 C + 4 + 3 log C) u + u (A + 3 Lna + |lp|)
  h = the sum of e_c d by C (3 Ey + 2 u) + 0.37 C^2 u, |h / es| <= log C, and
      the entropy term log(es) - h / es by
      Eh = (1 + log C) Res + C (3 Ey + 2 u) + 0.37 C^2 u + 4 u log C.
The S-term sums add the samples' bounds and S roundings of their partial sums:
  prob_sum, new_sum: sum of Et + S u;  ent_sum: sum of Eh + S u (1 + |ent_sum|)
and lpd, a log-mean-exp of the column of lp (1-Lipschitz in its largest
change), moves by the largest Elp plus its own (S + 4) u + u |lpd|, the bound
of lme in tests/test_cell_fit_gpu.py.

The kernels' tiles: a wave of the sums kernel takes 64 new cells and
T = _lib.DOUBLET_TILE candidates of the chunk's flat list and walks the
mutations _lib.DOUBLET_UNROLL at a time; the table kernel takes 256 mutations
per workgroup, the reductions 256 new cells."""
import numpy as np
import pytest

from bnpc_amd import _lib, postproc
from test_place import PRIOR, clustering, new_cells, samples

T = _lib.DOUBLET_TILE
NAMES = ('prob_sum', 'new_sum', 'ent_sum', 'lpd', 'lp', 'scores')
ULP = 2.0 ** -52


def bounds(red, a, alpha):
    """the docstring's bounds from the host reduction (keep=True) of the
    device's scores: {'prob_sum' (Q, 1), 'new_sum', 'ent_sum', 'lpd' (Q,),
    'lp' (S, Q)}"""
    S, N = a.shape
    y = red['y']
    Q = y.shape[1]
    u = ULP
    Et, Eh, Elp = np.zeros(Q), np.zeros(Q), np.zeros((S, Q))
    for s in range(S):
        sizes = np.unique(a[s], return_counts=True)[1]
        C = sizes.size + 1
        Lw = max(np.log(sizes.max()), abs(np.log(alpha[s])))
        Lna = np.log(N + alpha[s])
        A = np.nanmax(np.abs(y[s]), axis=1)
        Ey = u * (2 * Lw + A)
        Res = 2 * Ey + (1.4 * C + 2) * u
        Et += 4 * Ey + (3 * C + 6) * u
        Elp[s] = 3 * Ey + (1.4 * C + 4 + 3 * np.log(C)) * u \
            + u * (A + 3 * Lna + np.abs(red['lp'][s]))
        Eh += (1 + np.log(C)) * Res + C * (3 * Ey + 2 * u) \
            + 0.37 * C * C * u + 4 * u * np.log(C)
    Esum = Et + S * u
    return {'prob_sum': Esum[:, None], 'new_sum': Esum,
        'ent_sum': Eh + S * u * (1 + np.abs(red['ent_sum'])), 'lp': Elp,
        'lpd': Elp.max(axis=0) + (S + 4) * u + u * np.abs(red['lpd'])}


def compare(got, new, a, labels, par, FN, FP, alpha, prior=PRIOR):
    got = dict(zip(NAMES, got))
    S, N = a.shape
    Q, W, K = new.shape[0], par.shape[1], int(labels.max()) + 1
    assert got['prob_sum'].shape == (Q, K)
    for name in ('new_sum', 'ent_sum', 'lpd'):
        assert got[name].shape == (Q,) and got[name].dtype == np.float64, name
    assert got['lp'].shape == (S, Q)
    assert got['scores'].shape == (S, Q, W + 1)
    # the scores: the host's within the tables' tolerance, its NaN pattern
    host = postproc.place_scores(new, a, par, FN, FP, prior)
    assert np.array_equal(np.isnan(got['scores']), np.isnan(host))
    there = ~np.isnan(host)
    for s in range(S):
        Ks = np.unique(a[s]).size
        assert there[s, :, :Ks].all() and there[s, :, W].all()
        assert not there[s, :, Ks:W].any()
    err = np.abs(got['scores'][there] - host[there]) / (1 + np.abs(host[there]))
    print(f'scores: max |dev - host| / (1 + |host|) = {err.max():.3e}')
    np.testing.assert_allclose(got['scores'][there], host[there], rtol=1e-12,
        atol=1e-12)
    assert not np.signbit(got['scores'][got['scores'] == 0]).any()
    # the reductions of the device's scores
    red = postproc.place_reduce(got['scores'], a, labels, K, alpha, keep=True)
    tol = bounds(red, a, alpha)
    for name in NAMES[:5]:
        assert np.isfinite(got[name]).all(), name
        off = np.abs(got[name] - red[name])
        print(f'{name}: max |dev - host reduction| = {off.max():.3e}, '
            f'smallest bound {tol[name].min():.3e}')
        assert (off <= tol[name]).all(), (name, np.argwhere(off > tol[name])[:5])
    assert (got['prob_sum'] >= 0).all() and (got['new_sum'] > 0).all()
    return got


def equal(got, want):
    for name, g, w in zip(NAMES, got, want):
        assert (g is None) == (w is None), name
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape, name
            assert np.array_equal(g, w, equal_nan=True), \
                (name, np.argwhere(g != w)[:5])


def check(new, a, labels, par, FN, FP, alpha, prior=PRIOR, **how):
    post = _lib.Posterior(a)
    try:
        got = post.place(new, labels, par, FN, FP, alpha, prior, matrix=True,
            **how)
    finally:
        post.close()
    return compare(got, new, a, labels, par, FN, FP, alpha, prior)


def case(seed, S, N, M, W, K, Q, clusters=None):
    rng = np.random.RandomState(seed)
    a, par, FN, FP, alpha = samples(rng, S, N, W, M, clusters=clusters,
        in_range=True)
    return new_cells(rng, Q, M), a, clustering(rng, N, K), par, FN, FP, alpha


@pytest.mark.gpu
@pytest.mark.parametrize('Q', [1, 63, 64, 65, 129])
def test_edges_of_the_new_cell_blocks(Q):
    new, a, labels, par, FN, FP, alpha = case(100 + Q, 3, 20, 37, 5, 3, Q)
    got = check(new, a, labels, par, FN, FP, alpha)
    if Q > 4:
        # the empty row: nothing added up, the prior's probabilities
        assert np.isnan(new[Q - 1]).all()
        assert not np.nan_to_num(got['scores'][:, Q - 1]).any()
        assert np.abs(got['lp'][:, Q - 1]).max() < 1e-13
    # FN and FP swapped are another model: it does not pass
    other = postproc.place_scores(new, a, par, FP, FN, PRIOR)
    there = ~np.isnan(other)
    assert not np.allclose(got['scores'][there], other[there], rtol=1e-12,
        atol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize('M', [1, 2, 3, 257])
def test_edges_of_the_mutation_loop(M):
    assert _lib.DOUBLET_UNROLL == 2
    check(*case(200 + M, 3, 20, M, 5, 3, 70))


TILE_CASES = ([1, 7, 8, 9, 17, 3], [8, 17, 1, 9, 7, 2], [7, 9, 1, 1, 17, 8])


@pytest.mark.gpu
@pytest.mark.parametrize('clusters', TILE_CASES)
def test_cluster_counts_of_one_chunk_across_the_tiles(clusters):
    """the candidates of a chunk are one flat list, each sample's rows and
    then its new cluster: tiles of T cross the samples' boundaries, and over
    the cases the new cluster's slot is the first and the last of a tile"""
    assert T == 8
    places = set()
    for counts in TILE_CASES:
        assert {1, 7, 8, 9, 17} <= set(counts)
        places |= set(((np.cumsum(np.array(counts) + 1) - 1) % T).tolist())
    assert {0, T - 1} <= places
    new, a, labels, par, FN, FP, alpha = case(sum(clusters), len(clusters),
        40, 11, 17, 4, 66, clusters=clusters)
    assert [np.unique(row).size for row in a] == clusters
    slot = np.cumsum(np.array(clusters) + 1) - 1       # of the new clusters
    first = slot - np.array(clusters)
    assert (first % T != 0).any()           # a sample begins inside a tile
    assert (slot // T != first // T).any()  # and one spans two tiles
    check(new, a, labels, par, FN, FP, alpha, chunk=len(clusters))


@pytest.mark.gpu
def test_a_sample_of_singletons_and_a_wide_trace():
    """one sample has N clusters of one cell; the trace is wider than every
    other sample's cluster count, its unused rows NaN"""
    N = 20
    new, a, labels, par, FN, FP, alpha = case(7, 3, N, 9, N, 5, 40,
        clusters=[3, N, 1])
    assert np.unique(a[1]).size == N and np.isnan(par[0, 3:]).all()
    assert np.isnan(par[2, 1:]).all() and not np.isnan(par[1]).any()
    got = check(new, a, labels, par, FN, FP, alpha)
    # labels that are not compact: relabelled compactly, the same bits
    compact = np.stack([np.unique(row, return_inverse=True)[1].ravel()
        for row in a])
    assert not np.array_equal(compact, a)
    post = _lib.Posterior(compact)
    try:
        equal(post.place(new, labels, par, FN, FP, alpha, matrix=True),
            tuple(got[k] for k in NAMES))
    finally:
        post.close()


@pytest.mark.gpu
def test_a_trace_wider_than_every_sample():
    """W = 12 rows, at most 5 clusters a sample: the rows past a sample's
    count are NaN and never read; the new cluster's score sits at [W]"""
    clusters = [5, 2, 1, 4]
    new, a, labels, par, FN, FP, alpha = case(12, 4, 30, 10, 12, 3, 66,
        clusters=clusters)
    assert all(np.isnan(par[s, Ks:]).all() for s, Ks in enumerate(clusters))
    got = check(new, a, labels, par, FN, FP, alpha, chunk=3)
    assert np.isnan(got['scores'][:, :, 5:12]).all()
    assert np.isfinite(got['scores'][:, :, 12]).all()
    # the unused rows filled: the same bits
    post = _lib.Posterior(a)
    try:
        equal(post.place(new, labels, np.nan_to_num(par, nan=0.25), FN, FP,
            alpha, matrix=True), tuple(got[k] for k in NAMES))
    finally:
        post.close()


@pytest.mark.gpu
@pytest.mark.parametrize('K', [1, 5])
def test_one_and_five_clusters(K):
    new, a, labels, par, FN, FP, alpha = case(30 + K, 4, 25, 13, 6, K, 33)
    got = check(new, a, labels, par, FN, FP, alpha)
    assert got['prob_sum'].shape[1] == K
    # the clusters' labels permuted: the columns move with them
    perm = np.random.RandomState(K).permutation(K)
    post = _lib.Posterior(a)
    try:
        other = post.place(new, perm[labels], par, FN, FP, alpha)
    finally:
        post.close()
    assert np.array_equal(other[0][:, perm], got['prob_sum'])
    assert np.array_equal(other[1], got['new_sum'])


@pytest.mark.gpu
@pytest.mark.parametrize('value', [1e-6, 1e6])
def test_small_and_large_alpha(value):
    new, a, labels, par, FN, FP, alpha = case(41, 4, 25, 13, 6, 3, 33)
    alpha = np.array([value, 1.0, value, value * 1.5])
    got = check(new, a, labels, par, FN, FP, alpha)
    # a new cluster's probability rises with alpha, in every sample
    post = _lib.Posterior(a)
    try:
        ones = post.place(new, labels, par, FN, FP, np.ones(4))[1]
    finally:
        post.close()
    if value < 1:
        assert (got['new_sum'] <= ones).all() and (got['new_sum'] < ones).any()
    else:
        assert (got['new_sum'] >= ones).all() and (got['new_sum'] > ones).any()


@pytest.mark.gpu
def test_chunks_and_slabs_give_the_same_bits():
    S, Q = 5, 131
    new, a, labels, par, FN, FP, alpha = case(5, S, 30, 11, 9, 4, Q)
    post = _lib.Posterior(a)
    try:
        want = post.place(new, labels, par, FN, FP, alpha, matrix=True)
        compare(want, new, a, labels, par, FN, FP, alpha)
        # two calls
        equal(post.place(new, labels, par, FN, FP, alpha, matrix=True), want)
        for chunk in (1, 2, S - 1, 0):
            for slab in (64, 128, 0):
                equal(post.place(new, labels, par, FN, FP, alpha, chunk=chunk,
                    slab=slab, matrix=True), want)
        # slabs that do not end on a block of 64 cells, chunks past S
        for chunk, slab in ((3, 1), (2, 65), (S + 3, Q + 9), (1, 100)):
            equal(post.place(new, labels, par, FN, FP, alpha, chunk=chunk,
                slab=slab, matrix=True), want)
        short = post.place(new, labels, par, FN, FP, alpha, chunk=2, slab=65)
        equal(short, want[:4] + (None, None))
        # the codes themselves, and missing as 3
        codes = np.where(np.isnan(new), 3, new).astype(np.uint8)
        equal(post.place(codes, labels, par, FN, FP, alpha, matrix=True), want)
        equal(post.place(codes.astype(np.float64), labels, par, FN, FP, alpha,
            matrix=True), want)
        # two new cells swapped: their results swap, nobody else's moves
        i, j = 3, 70
        assert not np.array_equal(new[i], new[j], equal_nan=True)
        swapped = new.copy()
        swapped[[i, j]] = new[[j, i]]
        other = post.place(swapped, labels, par, FN, FP, alpha, matrix=True)
        order = np.arange(Q)
        order[[i, j]] = [j, i]
        assert not np.array_equal(other[0], want[0])
        assert not np.array_equal(other[3], want[3])
        equal((other[0][order], other[1][order], other[2][order],
            other[3][order], other[4][:, order], other[5][:, order]), want)
        t = post.place_times(new, labels, par, FN, FP, alpha)
        assert len(t) == 6 and all(x >= 0 for x in t) and t[4] > 0
    finally:
        post.close()


def raw_call(post, codes, labels, par, FN, FP, alpha, mix1, mix0, out):
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    return _lib.load().bnpc_post_place(post._h, _lib.ptr(codes),
        codes.shape[0], codes.shape[1], _lib.ptr(labels),
        int(labels.max()) + 1, _lib.ptr(par), par.shape[1], _lib.ptr(FN),
        _lib.ptr(FP), _lib.ptr(alpha), mix1, mix0, 0, 64,
        *[_lib.ptr(o) for o in out])


@pytest.mark.gpu
def test_bad_input_is_code_2_and_nothing_is_written():
    S, N, M, W, K, Q = 3, 12, 9, 4, 3, 131
    new, a, labels, par, FN, FP, alpha = case(6, S, N, M, W, K, Q)
    codes = np.where(np.isnan(new), 3, new).astype(np.uint8)

    def untouched(post, codes=codes, labels=labels, par=par, FN=FN, FP=FP,
            alpha=alpha, mix1=0.5, mix0=0.5):
        out = [np.full((Q, K), 7.25)] + [np.full(Q, 7.25) for _ in range(3)]
        out += [np.full((S, Q), 7.25), np.full((S, Q, W + 1), 7.25)]
        assert raw_call(post, codes, labels, par, FN, FP, alpha, mix1, mix0,
            out) == 2
        assert all((o == 7.25).all() for o in out)
        return _lib.load().bnpc_last_error().decode()

    post = _lib.Posterior(a)
    try:
        want = post.place(codes, labels, par, FN, FP, alpha, matrix=True)
        compare(want, new, a, labels, par, FN, FP, alpha)
        # a code other than 0 / 1 / 3 in a later slab of 64 new cells: named
        # in the file's own numbering
        bad = codes.copy()
        bad[100, 3] = 2
        assert 'cell 100 at mutation 3' in untouched(post, codes=bad)
        with pytest.raises(ValueError, match='cell 100 at mutation 3'):
            post.place(np.where(bad == 3, np.nan, bad), labels, par, FN, FP,
                alpha, slab=64)
        with pytest.raises(ValueError, match='cell 100 at mutation 3'):
            post.place_times(bad, labels, par, FN, FP, alpha, slab=64)
        # alpha
        for val in (0.0, -1.0, np.nan, np.inf):
            worse = alpha.copy()
            worse[S - 1] = val
            assert 'alpha' in untouched(post, alpha=worse)
        with pytest.raises(RuntimeError, match='code 2'):
            post.place(codes, labels, par, FN, FP, np.zeros(S))
        # a rate outside (0, 1)
        for fn, fp in ((0.0, FP[1]), (FN[1], 1.0), (np.nan, FP[1]),
                (FN[1], -0.1)):
            fns, fps = FN.copy(), FP.copy()
            fns[1], fps[1] = fn, fp
            assert 'sample 1' in untouched(post, FN=fns, FP=fps)
        # the mixing constants
        for m1, m0 in ((0.0, 1.0), (1.0, 0.0), (np.nan, 0.5), (0.5, 1.5)):
            untouched(post, mix1=m1, mix0=m0)
        with pytest.raises(RuntimeError, match='code 2'):
            post.place(codes, labels, par, FN, FP, alpha, prior=(0.0, 1.0))
        # a label of the clustering out of range
        worse = labels.copy()
        worse[0] = -1
        assert 'label' in untouched(post, labels=worse)
        # a sample with more clusters than the trace has rows
        assert max(np.unique(row).size for row in a) > 1
        assert 'clusters' in untouched(post, par=np.ascontiguousarray(
            par[:, :1]))
        # shapes the binding refuses before the call
        with pytest.raises(ValueError, match='mutations'):
            post.place(new[:, :M - 1], labels, par, FN, FP, alpha)
        with pytest.raises(ValueError, match='labels'):
            post.place(new, labels[:-1], par, FN, FP, alpha)
        with pytest.raises(ValueError, match='samples'):
            post.place(new, labels, par, FN, FP, alpha[:-1])
        # the handle lives
        equal(post.place(codes, labels, par, FN, FP, alpha, matrix=True),
            want)
    finally:
        post.close()


@pytest.mark.gpu
def test_tables_through_the_device_and_the_host():
    """postproc.place_cells on a handle with the method against the host
    loop.  A score of the device is within E = 1e-12 (1 + |score|) of the
    host's (the tolerance above), so every y_c moves by E at the most: pr_c
    by 2 E pr_c, prob and p_new by 2 E, lp and lpd (1-Lipschitz in the largest
    change) by E, and a sample's entropy - sum of pr_c log pr_c by
    2 E (1 + log(W + 1)); to each the reduction's own bound (the module's
    docstring) is added."""
    from test_place import clones_case
    new, a, clone, par, FN, FP, alpha, truth = clones_case()
    assert a.min() >= 0 and a.max() < a.shape[1]
    host = postproc.place_cells(None, new, a, clone, par, FN, FP, alpha,
        PRIOR)
    post = _lib.Posterior(a)
    try:
        dev = postproc.place_cells(post, new, a, clone, par, FN, FP, alpha,
            PRIOR)
    finally:
        post.close()
    assert dev.keys() == host.keys()
    for key in ('cluster', 'next_cluster', 'n_obs'):
        assert np.array_equal(dev[key], host[key]), key
    seen = dev['n_obs'] > 0
    assert np.array_equal(dev['cluster'][seen], truth[seen])
    red = postproc.host_place(new, a, clone, par, FN, FP, alpha, PRIOR)
    S, W = a.shape[0], par.shape[1]
    tol = bounds(red, a, alpha)
    E = 1e-12 * (1 + np.nanmax(np.abs(red['scores']), axis=(0, 2)))
    for key, bound in (('prob', 2 * E[:, None] + tol['prob_sum'] / S),
            ('p_new', 2 * E + tol['new_sum'] / S),
            ('cluster_prob', 2 * E + tol['new_sum'] / S),
            ('next_prob', 2 * E + tol['new_sum'] / S),
            ('entropy', 2 * E * (1 + np.log(W + 1)) + tol['ent_sum'] / S),
            ('lpd', E + tol['lpd'])):
        off = np.abs(dev[key] - host[key])
        print(f'{key}: max |dev - host| = {off.max():.3e}, smallest bound '
            f'{bound.min():.3e}')
        assert (off <= bound).all(), key
    assert dev['total']['placed'] == host['total']['placed']
    assert dev['total']['new'] == host['total']['new'] == 0
