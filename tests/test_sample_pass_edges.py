"""The posterior sample passes of bnpc_post_passes.hip (bnpc_post_genotypes, -pg
and -pf with the rank pass they share) at the edges their feature tests do
not enter, against the host loops they are pinned to (postproc.host_genotypes,
host_cell_genotypes, host_cell_fit).  array_equal wherever the sibling files
assert array_equal; cell_fit through test_cell_fit_gpu.compare, its bounds
unchanged.  Every test asserts on its own inputs, from the host side alone,
that it reaches the edge it names (the *_inputs functions need no device).

A  the sample loops wrap their grid: k_gt_flags, k_gt_hist and k_cg_rank walk
   `s = blockIdx.x; s < S; s += gridDim.x` on a grid of min(S, 65535),
   k_cf_tables and k_cf_sums `q = blockIdx.y; ...; q += gridDim.y`.
   S = 65538 = 65535 + 3: three workgroups take a second sample and reuse
   their LDS area and the `part` array.
B  ranks that need the upper byte of the uint16 that k_cg_accum and k_cf_sums
   unpack from a 16-byte load: samples of 255, 256, 257 and 300 clusters.
C  gt_scan with more than one bitmap word per thread while the working set
   is still in LDS: N = 8193, 8224 (257 words, the last one with one bit and
   full) and 16385 (513 words, three per thread).
D  the second workgroup of k_cf_reduce (256 cells each) and of k_gt_accum
   (256 mutations each).
E  k_cf_reduce where exp(ll - max) flushes to zero, with the maximum at the
   first, the last and an inner sample, and on a constant column.
F  ll against an exactly rounded sum, within a bound derived from M (B, D, E
   and the wrapped rows of A).

The bound of F.  postproc.host_cell_fit makes the argument of every log the
same bits on host and device (each operation rounded on its own, no FMA
contraction in the build), so the two differ only in the log routine and in
the order of the sum over the M mutations.  With t the host's float64 terms
(its `el`) of one (sample, cell):
  each device log is within 2 ulp of the host's term (both routines are
  within 1 ulp of the true logarithm): at most 2 * 2**-52 * sum |t| in all;
  any order of adding M terms errs by at most (M - 1) * 2**-53 * sum |t| to
  first order;
together (2 + (M - 1) / 2) * 2**-52 * sum |t|, which
  |ll_dev - fsum(t)| <= (M + 2) * 2**-52 * fsum(|t|)
covers with the second-order terms to spare.  At M = 33 and |ll| around 100
that is 8e-13 absolute, against the 1e-12 * (1 + |ll|) = 1e-10 of the sibling
file.  The host's own ll (NumPy's pairwise sum of the same terms) is held to
the same bound first.

Not covered, for the record: the wrap of k_gt_flags, k_gt_hist and k_cg_rank
on the global-slice path (a grid of 512) needs more than 512 samples of more
than 70 000 resp. 257 984 cells, and the handle's pair counts of that many
cells take tens to hundreds of GB; the 64-bit sums of k_post_support past
2**32 need N x S above 4.3e9."""
import math

import numpy as np
import pytest

from bnpc_amd import _lib, postproc
import test_cell_fit_gpu as CF
import test_cell_genotypes_gpu as CG
import test_genotypes_gpu as G

ULP = 2.0 ** -52
GRID_MAX = 65535        # bnpc_post.h: the most workgroups of a sample loop
CG_LDS_MAX = 65536      # bnpc_post_passes.hip: the rank pass's LDS limit, bytes
GT_LDS_MAX = 163840     # bnpc_post_passes.hip: the genotype passes' LDS limit
S_WRAP = GRID_MAX + 3


# ---------------------------------------------------------------------------
# F: the exactly rounded sum
# ---------------------------------------------------------------------------
def terms(data, a, params, FN, FP, only=None):
    """host_cell_fit's float64 terms `el` of the samples `only` (default:
    all), (samples, cells, mutations), and the row sums as it takes them"""
    codes = postproc.data_codes(data)
    a = np.asarray(a)
    FN = np.asarray(FN, dtype=np.float64)
    FP = np.asarray(FP, dtype=np.float64)
    out, sums = [], []
    for s in (range(a.shape[0]) if only is None else only):
        rank = np.unique(a[s], return_inverse=True)[1].ravel()
        th = np.asarray(params[s], dtype=np.float32)[:rank.max() + 1]
        t = th.astype(np.float64)
        o = (np.float32(1) - th).astype(np.float64)
        L1 = np.log(t * (1 - FN[s]) + o * FP[s])
        L0 = np.log(t * FN[s] + o * (1 - FP[s]))
        el = np.where(codes == 1, L1[rank], np.where(codes == 0, L0[rank], 0))
        out.append(el)
        sums.append(el.sum(axis=1))
    return np.array(out), np.array(sums)


def exact_and_room(el):
    """fsum of every (sample, cell)'s terms and the bound on its ll"""
    S, N, M = el.shape
    exact, room = np.empty((S, N)), np.empty((S, N))
    for s in range(S):
        for i, row in enumerate(el[s].tolist()):
            exact[s, i] = math.fsum(row)
            room[s, i] = (M + 2) * ULP * math.fsum(abs(x) for x in row)
    return exact, room


def check_ll_bound(ll, host_ll, el, sums, what):
    """ll: the device's rows of the samples `el` was made for"""
    assert np.array_equal(sums, host_ll)    # these are the host's terms
    exact, room = exact_and_room(el)
    assert (np.abs(host_ll - exact) <= room).all()      # the reference alone
    off = np.abs(ll - exact)
    ratio = np.divide(off, room, out=np.zeros_like(off), where=room > 0)
    print(f'{what}: max |ll_dev - exact| / bound = {ratio.max():.4f}')
    assert (off <= room).all(), (what, np.argwhere(off > room)[:5],
        ratio.max())
    # never past the sibling file's figure
    assert (room <= 1e-12 * (1 + np.abs(exact))).all()


# ---------------------------------------------------------------------------
# A: grid wrap
# ---------------------------------------------------------------------------
def wrap_samples(rng, S, N):
    """one to three labels per sample, each sample on labels of its own out
    of [0, N): the bitmap of a sample is rarely that of the sample before"""
    pool = np.argsort(rng.random_sample((S, N)), axis=1)[:, :3]
    k = rng.randint(1, 4, S)
    pick = rng.randint(0, 6, (S, N)) % k[:, None]
    pick[:, :3] = np.arange(3) % k[:, None]     # exactly k labels
    return np.take_along_axis(pool, pick, axis=1).astype(np.int64)


def wrapped_differ(a):
    """the sample that a workgroup takes on its second trip is not the one
    of its first trip, which also left a label behind that the second lacks
    (a bit in an area that was not cleared)"""
    assert a.shape[0] == S_WRAP > GRID_MAX
    for s in range(GRID_MAX, S_WRAP):
        first = a[s - GRID_MAX]
        assert not np.array_equal(a[s], first)
        assert np.setdiff1d(first, a[s]).size


def wrap_cell_inputs():
    rng = np.random.RandomState(65538)
    N, M = 9, 33        # two cell tiles, the second of one cell; two words
    a = wrap_samples(rng, S_WRAP, N)
    wrapped_differ(a)
    assert CG.width(a) == 3 and a.max() == N - 1
    assert N > _lib.CELL_TILE and N % _lib.CELL_TILE == 1 and 32 < M <= 64
    return rng, a, N, M


@pytest.mark.gpu
def test_wrapped_rank_launch_of_the_cell_genotypes():
    """chunk=0: one chunk of 65538 samples, k_cg_rank on 65535 workgroups;
    chunk=65536: a wrap by exactly one sample, then a chunk of two;
    chunk=65535: no wrap, then three.  k_cg_accum walks the chunk in one
    thread, so only the ranks depend on the wrap."""
    rng, a, N, M = wrap_cell_inputs()
    params = CG.trace(rng, S_WRAP, 3, M)
    want = postproc.host_cell_genotypes(a, params)
    post = _lib.Posterior(a)
    try:
        for chunk in (0, GRID_MAX + 1, GRID_MAX):
            CG.equal(post.cell_genotypes(params, chunk=chunk), want)
    finally:
        post.close()


@pytest.mark.gpu
def test_wrapped_table_and_sum_launches_of_the_cell_fit():
    """As above for -pf: k_cf_tables and k_cf_sums wrap along blockIdx.y.
    The three wrapped rows of ll are held to the bound F as well."""
    rng, a, N, M = wrap_cell_inputs()
    params = CF.trace(rng, S_WRAP, 3, M)
    data = CF.matrix(rng, N, M)
    FN, FP = CF.rates(rng, S_WRAP)
    host = postproc.host_cell_fit(data, a, params, FN, FP)
    tail = range(GRID_MAX, S_WRAP)
    el, sums = terms(data, a, params, FN, FP, only=tail)
    post = _lib.Posterior(a)
    try:
        got = post.cell_fit(data, params, FN, FP, matrix=True)
        CF.compare(got, host)
        for chunk in (GRID_MAX + 1, GRID_MAX):
            CF.equal(post.cell_fit(data, params, FN, FP, chunk=chunk,
                matrix=True), got)
    finally:
        post.close()
    ll = got[3]
    np.testing.assert_allclose(ll[GRID_MAX:], host['ll'][GRID_MAX:],
        rtol=1e-12, atol=1e-12)
    assert host['ll'][GRID_MAX:].any(axis=1).all()
    # a row taken from the workgroup's first trip would be another row
    assert not np.allclose(host['ll'][GRID_MAX:], host['ll'][:3],
        rtol=1e-9, atol=1e-9)
    check_ll_bound(ll[GRID_MAX:], host['ll'][GRID_MAX:], el, sums,
        'wrapped rows')


def wrap_genotype_inputs():
    rng = np.random.RandomState(19)
    N, M, K = 4, 5, 2
    a, cl, params = G.make_case(rng, S_WRAP, N, M, K, 3, never=(0,))
    mine, rest = np.flatnonzero(cl == 1), np.flatnonzero(cl == 0)
    assert mine.size == 2 and rest.size == 2
    # the three labels of a sample on three of [0, N) of its own
    onto = np.argsort(rng.random_sample((S_WRAP, N)), axis=1)[:, :3]
    a = np.take_along_axis(onto, a, axis=1)
    # cluster 1 together and alone in the wrapped samples: on the smallest
    # label that cluster 0's two cells leave free
    for s in range(GRID_MAX, S_WRAP):
        a[s, mine] = np.setdiff1d(np.arange(N), a[s, rest])[0]
    assert CG.width(a) == 3 == params.shape[1] and a.max() == N - 1
    return a, cl, params


@pytest.mark.gpu
def test_wrapped_flag_and_histogram_launches_of_the_genotypes():
    """Cluster 0 is never together (k_gt_hist, its per-cluster inner loop and
    the reuse of `part`), cluster 1 is chosen in samples past 65535."""
    a, cl, params = wrap_genotype_inputs()
    wrapped_differ(a)
    assert G.kinds(a, cl) == (1, 0)
    sub, oth = a[:, cl == 1], a[:, cl == 0]
    pick = (sub == sub[:, :1]).all(axis=1) \
        & ~(oth == sub[:, :1]).any(axis=1)
    assert pick[GRID_MAX:].all() and pick[:GRID_MAX].any() \
        and not pick[:GRID_MAX].all()
    G.check(a, cl, params)


# ---------------------------------------------------------------------------
# B: ranks past one byte
# ---------------------------------------------------------------------------
def wide_samples():
    rng = np.random.RandomState(300)
    N, counts = 300, (255, 256, 257, 300)
    a = np.empty((len(counts), N), dtype=np.int64)
    for s, d in enumerate(counts):
        # d labels of [0, N) with 0 and N - 1 among them, every one carried
        labels = np.sort(np.append(rng.choice(np.arange(1, N - 1), d - 2,
            replace=False), (0, N - 1)))
        cells = rng.permutation(N)
        a[s, cells[:d]] = labels
        a[s, cells[d:]] = labels[rng.randint(0, d, N - d)]
    # a cell of the last tile (296 .. 299) with a rank >= 256 in two samples
    for s in (2, 3):
        at = np.flatnonzero(a[s] == N - 1)[0]
        a[s, [at, 297]] = a[s, [297, at]]
    assert [np.unique(r).size for r in a] == list(counts)
    assert a.min() == 0 and a.max() == N - 1
    rank = np.array([np.unique(r, return_inverse=True)[1].ravel() for r in a])
    assert rank[:2].max() == 255 and (rank[:, 297] >= 256).sum() == 2
    assert 297 // _lib.CELL_TILE == (N - 1) // _lib.CELL_TILE
    high = np.flatnonzero((rank >= 256).any(axis=0))
    assert (high % 2 == 0).any() and (high % 2 == 1).any()
    assert {256, 257, 299} <= set(rank[3].tolist())
    return rng, a, N


@pytest.mark.gpu
def test_ranks_past_one_byte_in_the_cell_genotypes():
    rng, a, N = wide_samples()
    params = CG.trace(rng, 4, N, 5)
    want = postproc.host_cell_genotypes(a, params)
    post = _lib.Posterior(a)
    try:
        CG.equal(post.cell_genotypes(params), want)
        CG.equal(post.cell_genotypes(params, chunk=1, slab=299), want)
    finally:
        post.close()
    # the rank's upper byte dropped is another table
    low = np.array([np.unique(r, return_inverse=True)[1].ravel() & 0xff
        for r in a])
    assert not np.array_equal(sum(params[s][low[s]].astype(np.float64)
        for s in range(4)), want[0])


@pytest.mark.gpu
def test_ranks_past_one_byte_in_the_cell_fit():
    rng, a, N = wide_samples()
    M = 33
    params = CF.trace(rng, 4, N, M)
    data = CF.matrix(rng, N, M)
    FN, FP = CF.rates(rng, 4)
    got, host = CF.check(data, a, params, FN, FP)
    check_ll_bound(got[3], host['ll'], *terms(data, a, params, FN, FP),
        'wide ranks')


# ---------------------------------------------------------------------------
# C: several bitmap words per thread, in LDS
# ---------------------------------------------------------------------------
def words(N):
    return (N + 31) // 32


def scan_edges(a, N, s=1):
    """sample s carries the last bit of word 255, the first of word 256 and
    the last bit of the bitmap; every sample has labels on both sides"""
    assert words(N) > 256 and (words(N) + 255) // 256 >= 2
    assert np.isin((8191, 8192, N - 1), a[s]).all()
    assert all((r < 8192).any() and (r >= 8192).any() for r in a)


@pytest.mark.gpu
@pytest.mark.parametrize('N', [8193, 8224, 16385])
def test_cell_passes_with_several_bitmap_words_per_thread(N):
    S, M = 3, 3
    assert 8 * words(N) + 1040 <= CG_LDS_MAX    # k_cg_rank works in LDS
    assert N <= _lib.CELL_RANK_LDS_CELLS
    rng = np.random.RandomState(N)
    a = np.array([np.sort(rng.choice(N, 40, replace=False))[
        rng.randint(0, 40, N)] for _ in range(S)]).astype(np.int64)
    a[1, [5, N - 2, 4000, 8192]] = 8191
    a[1, [6, N - 1, 4001, 8191]] = 8192
    a[1, [7, N - 3]] = N - 1
    a[(0, 2), N - 1] = 8192
    scan_edges(a, N)
    W = CG.width(a)
    assert 40 <= W <= 43
    params = CG.trace(rng, S, W, M)
    data = CF.matrix(rng, N, M)
    FN, FP = CF.rates(rng, S)
    want = postproc.host_cell_genotypes(a, params)
    host = postproc.host_cell_fit(data, a, params, FN, FP)
    post = _lib.Posterior(a)
    try:
        CG.equal(post.cell_genotypes(params), want)
        CF.compare(post.cell_fit(data, params, FN, FP, matrix=True), host)
    finally:
        post.close()


@pytest.mark.gpu
@pytest.mark.parametrize('N', [8193, 8224, 16385])
def test_genotypes_with_several_bitmap_words_per_thread(N):
    S, M, K = 3, 3, 6
    # k_gt_flags and k_gt_hist work in LDS
    assert 4 * (260 + 2 * words(N) + (N + 1) // 2 + 2 * K) <= GT_LDS_MAX
    assert 4 * (260 + 4 * words(N)) <= GT_LDS_MAX
    rng = np.random.RandomState(N + 1)
    a, cl, _ = G.make_case(rng, S, N, M, K, 40, never=(1,), spread=True)
    cells = np.flatnonzero(cl == 1)     # the cluster that is never together
    a[1, cells[:3]] = 8191
    a[1, cells[3:6]] = 8192
    a[1, cells[6]] = N - 1
    scan_edges(a, N)
    never, _ = G.kinds(a, cl)
    assert never >= 1 and not (a[:, cells] == a[:, cells[:1]]).all(axis=1).any()
    assert never < K                    # and some cluster takes pass 2's rows
    params = rng.random_sample((S, CG.width(a), M)).astype(np.float32)
    G.check(a, cl, params)


# ---------------------------------------------------------------------------
# D: second workgroups
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('N', [255, 256, 257])
def test_cell_fit_reduction_beside_its_workgroup_of_256_cells(N):
    S, M = 5, 33
    assert (N + 255) // 256 == (2 if N > 256 else 1)
    data, a, params, FN, FP = CF.case(7000 + N, S, N, M, 5)
    got, host = CF.check(data, a, params, FN, FP)
    check_ll_bound(got[3], host['ll'], *terms(data, a, params, FN, FP),
        f'N = {N}')
    if N == 257:
        # a last slab of one cell, its reduction a workgroup of its own
        post = _lib.Posterior(a)
        try:
            CF.equal(post.cell_fit(data, params, FN, FP, slab=256,
                matrix=True), got)
        finally:
            post.close()


def many_mutations(M):
    rng = np.random.RandomState(9000)    # the same samples at every M
    S, N, K = 12, 40, 5
    a, cl, params = G.make_case(rng, S, N, M, K, N, p_together=0.6,
        never=(1,))
    # cluster 3, wherever it is together, on a label of the never-together
    # cluster 1: together, never alone
    mine = np.flatnonzero(cl == 3)
    tog = (a[:, mine] == a[:, mine[:1]]).all(axis=1)
    assert tog.sum() >= 3
    a[np.ix_(tog, mine)] = a[tog, np.flatnonzero(cl == 1)[0]][:, None]
    assert G.kinds(a, cl) == (1, 1) and 0 <= a.min() and a.max() < N
    assert CG.width(a) <= params.shape[1] and params.shape[2] == M
    return a, cl, params


@pytest.mark.gpu
@pytest.mark.parametrize('M', [255, 256, 257, 513])
def test_genotype_sums_beside_their_workgroup_of_256_mutations(M):
    assert (M + 255) // 256 == {255: 1, 256: 1, 257: 2, 513: 3}[M]
    a, cl, params = many_mutations(M)
    want = G.check(a, cl, params)
    assert np.array_equal(G.check(a, cl, params, chunk=5), want)


# ---------------------------------------------------------------------------
# E: the reduction's extremes
# ---------------------------------------------------------------------------
def extreme_inputs():
    """One cluster per sample: row 0 of the trace is the sample.  FN = 0.3
    and FP = 1e-6 in every sample.  Mutations 0 .. 63: sample 0 has the
    parameters 1, sample 5 has 0, sample 2 has 1 at the even and 0 at the
    odd mutations, the other samples random draws; mutations 64 .. 69: the
    same parameters in every sample.  A parameter 0 where the cell shows a 1
    costs log(FP) = -13.8, a parameter 1 there log(1 - FN) = -0.36; a
    parameter 1 where it shows a 0 costs log(FN) = -1.2, a parameter 0 there
    nothing.  So
      cell 0, all ones: -23 in sample 0 (the maximum, first), -884 in sample
              5 - apart by more than the 745 past which exp gives 0;
      cell 1, all zeros: -77 in sample 0, about 0 in sample 5 (the maximum,
              last);
      cell 2, 1 at the even and 0 at the odd mutations: -11 in sample 2 (the
              maximum, inside), -50 in sample 0, -442 in sample 5;
      cell 3, only mutations 64 .. 69 observed: the same ll in every sample.
    """
    rng = np.random.RandomState(745)
    S, N, M = 6, 16, 70
    a = np.repeat(np.array([0, N - 1, 5, 5, 3, N - 1])[:, None], N, axis=1)
    params = CF.trace(rng, S, 1, M)
    even = (np.arange(64) % 2 == 0)
    params[0, 0, :64] = 1.0
    params[5, 0, :64] = 0.0
    params[2, 0, :64] = even
    params[:, 0, 64:] = np.float32([0.75, 0.0, 1.0, 0.5, 0.125, 0.9])
    data = CF.matrix(rng, N, M)
    data[0] = 1.0
    data[1] = 0.0
    data[2] = np.arange(M) % 2 == 0
    data[3, :64] = np.nan
    data[3, 64:] = [1, 0, 1, 0, 1, 0]
    FN, FP = np.full(S, 0.3), np.full(S, 1e-6)
    host = postproc.host_cell_fit(data, a, params, FN, FP)
    ll = host['ll']
    spread = ll.max(axis=0) - ll.min(axis=0)
    assert spread[0] > 745 and np.exp(-spread[0]) == 0.0
    for cell, where in ((0, 0), (1, S - 1), (2, 2)):
        col = ll[:, cell]
        assert col.argmax() == where and (col == col.max()).sum() == 1
    assert (ll[:, 3] == ll[0, 3]).all() and ll[0, 3] < 0
    assert host['m2'][3] == 0
    return data, a, params, FN, FP, host


@pytest.mark.gpu
def test_reduction_where_exp_underflows_and_at_every_place_of_the_maximum():
    data, a, params, FN, FP, host = extreme_inputs()
    S, N = a.shape
    post = _lib.Posterior(a)
    try:
        got = post.cell_fit(data, params, FN, FP, matrix=True)
    finally:
        post.close()
    CF.compare(got, host)
    mean, m2, lme, ll = got
    room = (S + 4) * ULP + ULP * np.abs(lme)
    # the constant column
    assert (ll[:, 3] == ll[0, 3]).all() and m2[3] == 0
    assert mean[3] == ll[0, 3] and abs(lme[3] - ll[0, 3]) <= room[3]
    # the device's columns have the shape of the host's
    assert ll[:, 0].max() - ll[:, 0].min() > 745
    assert [ll[:, c].argmax() for c in (0, 1, 2)] == [0, S - 1, 2]
    # an exactly rounded log-mean-exp of the device's own ll
    for i in range(N):
        col = ll[:, i].tolist()
        mx = max(col)
        ref = mx + math.log(math.fsum(math.exp(v - mx) for v in col)) \
            - math.log(S)
        assert abs(lme[i] - ref) <= room[i], (i, lme[i], ref)
    # the cell whose other samples vanish: the log of one sample's share
    assert abs(lme[0] - (ll[0, 0] - math.log(S))) <= room[0]
    check_ll_bound(ll, host['ll'], *terms(data, a, params, FN, FP),
        'extremes')
