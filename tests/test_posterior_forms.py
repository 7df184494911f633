"""The posterior estimator's device kernels (bnpc_amd/csrc/bnpc_codist.hip and,
for the Ward linkage, bnpc_amd/csrc/bnpc_post_ward.hip) at the forms and edges a real workload takes and tests/test_posterior.py does
not: k_codist's 32-sample rounds and 64 x 64 tiles, the 64 Mi-element slabs of
bnpc_post_fetch, a sum of pair counts past 2^32, k_mpear_sums with several
tiles per workgroup and every candidate chunking, and the Ward linkage at its
grid thresholds and on matrices that are nothing but ties.

Everything is exact: integer counts against oracle.posterior_numpy's
differ_rows / same_label_sums (plain NumPy, no pdist - checked on the CPU in
tests/test_oracle_golden.py), float64 against NumPy's division and SciPy's
linkage bit for bit.  No tolerances."""
import numpy as np
import pytest

from oracle import posterior_numpy as Q
from bnpc_amd import _lib

pytestmark = pytest.mark.gpu

INT32 = np.iinfo(np.int32)


def pair_index(i, j, N):
    """position of the pair i < j in the condensed vector"""
    assert 0 <= i < j < N
    return i * (2 * N - i - 1) // 2 + (j - i - 1)


def both_counts(a):
    """the pair counts of bnpc_codist and of a bnpc_post object"""
    a = np.asarray(a)
    one = _lib.codist(a)
    post = _lib.Posterior(a)
    try:
        two = post.differ()
        total = post.differ_sum
    finally:
        post.close()
    assert one.dtype == np.int32 and two.dtype == np.int32
    return one, two, total


def assert_counts(a, want):
    one, two, total = both_counts(a)
    assert np.array_equal(one, want)
    assert np.array_equal(two, want)
    assert total == int(want.sum(dtype=np.int64))


# --------------------------------------------------------------- pair counts
# every N edge of the 64 x 64 tiles (one tile, its last row, two and three
# tiles, four with a ragged last one) with every S edge of the 32-sample
# rounds (a short, a full and an overfull first round; two full; two and one)
COUNT_SHAPES = [(2, 1), (2, 33), (63, 31), (63, 64), (64, 32), (64, 65),
    (65, 1), (65, 33), (127, 32), (127, 65), (128, 31), (128, 64), (129, 32),
    (129, 33), (193, 31), (193, 65)]
assert {n for n, _ in COUNT_SHAPES} == {2, 63, 64, 65, 127, 128, 129, 193}
assert {s for _, s in COUNT_SHAPES} == {1, 31, 32, 33, 64, 65}


@pytest.mark.parametrize('N,S', COUNT_SHAPES)
def test_pair_counts_at_tile_and_round_edges(N, S):
    rng = np.random.RandomState(N * 100 + S)
    a = rng.randint(0, 3, size=(S, N))
    assert_counts(a, Q.differ_rows(a))


@pytest.mark.parametrize('N,S', [(2, 1), (64, 31), (65, 33), (129, 32),
    (193, 65)])
def test_pair_counts_all_equal_and_all_distinct(N, S):
    pairs = N * (N - 1) // 2
    assert_counts(np.full((S, N), 7), np.zeros(pairs, dtype=np.int32))
    rng = np.random.RandomState(N + S)
    distinct = np.stack([rng.permutation(N) for _ in range(S)])
    assert_counts(distinct, np.full(pairs, S, dtype=np.int32))


@pytest.mark.parametrize('N,S', [(63, 33), (65, 31), (129, 32), (193, 65)])
def test_pair_counts_with_negative_and_extreme_labels(N, S):
    """k_codist pads with the labels -1 - column: real labels from [-64, -1],
    INT32_MIN, INT32_MAX and 0 count like any others."""
    pool = np.concatenate([np.arange(-64, 0), [INT32.min, INT32.max, 0]]) \
        .astype(np.int32)
    rng = np.random.RandomState(N * 7 + S)
    a = pool[rng.randint(0, pool.size, size=(S, N))]
    a[0, :3] = (INT32.min, INT32.max, 0)
    # a sample that is the padding itself, column by column
    a[-1] = -1 - (np.arange(N) % 64)
    assert_counts(a, Q.differ_rows(a))


@pytest.mark.parametrize('N', [65, 129, 193])
def test_one_cell_apart_marks_exactly_its_pairs(N):
    for c in (0, 63, 64, N - 1):
        a = np.zeros((1, N), dtype=np.int32)
        a[0, c] = 1
        want = np.zeros(N * (N - 1) // 2, dtype=np.int32)
        for other in range(N):
            if other != c:
                want[pair_index(min(c, other), max(c, other), N)] = 1
        assert want.sum() == N - 1
        assert_counts(a, want)


def test_one_cell_or_no_sample_is_refused():
    for shape in ((3, 1), (0, 5)):
        a = np.zeros(shape, dtype=np.int32)
        with pytest.raises(RuntimeError):
            _lib.codist(a)
        post = None
        try:
            with pytest.raises(RuntimeError):
                post = _lib.Posterior(a)
        finally:
            if post is not None:
                post.close()


# ------------------------------------------- slabs, the 64-bit sum, 16 653 tiles
BIG_N = 11586           # the smallest N with more than 2^26 pairs
SLAB = 1 << 26


@pytest.fixture(scope='module')
def big():
    """14 samples label = bit s of the cell, 64 samples of singletons (+64 on
    every pair, added to the reference analytically)."""
    N = BIG_N
    assert (N - 1) * (N - 2) // 2 <= SLAB < N * (N - 1) // 2
    cell = np.arange(N, dtype=np.int32)
    bits = np.stack([(cell >> s) & 1 for s in range(14)])
    a = np.concatenate([bits, np.tile(cell, (64, 1))])
    ref = Q.differ_rows(bits)
    ref += 64
    post = _lib.Posterior(a)
    try:
        yield post, ref
    finally:
        post.close()


def test_second_slab_and_a_sum_past_32_bits(big):
    post, ref = big
    assert post.S == 78 and post.pairs == 67111905
    total = int(ref.sum(dtype=np.int64))
    assert total > 2 ** 32
    assert np.array_equal(post.differ(), ref)
    assert post.differ_sum == total
    want = ref / np.float64(78)
    got = post.dist()
    if not np.array_equal(got, want):
        for at in (SLAB - 1, SLAB):
            print(f'[slab] element {at}: count {ref[at]}, dist {got[at]!r}, '
                f'expected {want[at]!r}')
    assert np.array_equal(got, want)


def test_mpear_sums_sixteen_tiles_per_workgroup(big):
    post, ref = big
    nt = -(-BIG_N // 64)
    assert nt * (nt + 1) // 2 == 16653
    rng = np.random.RandomState(5)
    lab = np.stack([rng.randint(0, 3, BIG_N), np.zeros(BIG_N, dtype=int)])
    want = Q.same_label_sums(ref, lab)
    assert want[1] == post.differ_sum
    assert np.array_equal(post.mpear_sums(lab), want)


def test_mpear_sums_two_tiles_per_workgroup():
    """N = 2881: 46 tile rows, 1081 tiles on a grid of 1024 - workgroups 0 to
    56 take a second tile with the accumulator of the first."""
    S, N = 9, 2881
    nt = -(-N // 64)
    assert nt == 46 and nt * (nt + 1) // 2 == 1081
    rng = np.random.RandomState(6)
    a = rng.randint(0, 4, size=(S, N))
    ref = Q.differ_rows(a)
    lab = np.stack([rng.randint(0, 2, N), rng.randint(0, 7, N),
        rng.randint(0, 40, N), np.full(N, 9), np.arange(N)])
    want = Q.same_label_sums(ref, lab)
    post = _lib.Posterior(a)
    try:
        assert np.array_equal(post.differ(), ref)
        assert want[3] == post.differ_sum and want[4] == 0
        assert np.array_equal(post.mpear_sums(lab), want)
    finally:
        post.close()


# ----------------------------------------------------------- candidate forms
FORM_N, FORM_S = 130, 7
FORM_C = [1, 31, 32, 33, 64, 65, 127, 128, 129, 256, 257, 385, 1024, 1025]


def form_candidate(c):
    """Cells 0 .. m-1 in one cluster (label 65533), the last q cells in one
    (label 0), singletons between; m = 2 + c % 64 and q in (0, 2 .. 16) from
    (c // 64) % 16.  With every pair count positive both clusters' sums grow
    strictly with their sizes, so candidates 32, 64 and 128 apart differ."""
    N = FORM_N
    m = 2 + c % 64
    step = (c // 64) % 16
    q = step + 1 if step else 0
    lab = 1 + np.arange(N)
    lab[:m] = 65533
    if q:
        lab[N - q:] = 0
    return lab


@pytest.fixture(scope='module')
def forms():
    rng = np.random.RandomState(7)
    a = rng.randint(0, 4, size=(FORM_S, FORM_N))
    a[0] = np.arange(FORM_N)                # every pair differs at least once
    differ = Q.differ_rows(a)
    assert differ.min() >= 1
    lab = np.stack([form_candidate(c) for c in range(max(FORM_C))])
    assert lab.min() == 0 and lab.max() == 65533
    ref = Q.same_label_sums(differ, lab)
    for k in (32, 64, 128):                 # a chunk mix-up cannot pass
        assert np.all(ref[:-k] != ref[k:]), k
    return a, differ, lab, ref


@pytest.mark.parametrize('C', FORM_C)
def test_mpear_sums_candidate_chunks(forms, C):
    a, differ, lab, ref = forms
    lab, ref = lab[:C].copy(), ref[:C].copy()
    post = _lib.Posterior(a)
    try:
        assert np.array_equal(post.differ(), differ)
        assert np.array_equal(post.mpear_sums(lab), ref)
        # the last slot holds a sum in one call and must hold 0 in the next
        lab[-1] = 65533
        ref[-1] = post.differ_sum
        assert np.array_equal(post.mpear_sums(lab), ref)
        lab[-1] = np.arange(FORM_N)
        ref[-1] = 0
        assert np.array_equal(post.mpear_sums(lab), ref)
    finally:
        post.close()


def test_mpear_sums_label_range_and_no_candidates(forms):
    a, differ, lab, ref = forms
    post = _lib.Posterior(a)
    try:
        for bad in (65534, -1):
            one = lab[:3].copy()
            one[1, 5] = bad
            with pytest.raises(ValueError):
                post.mpear_sums(one)
        got = post.mpear_sums(lab[:0])
        assert got.shape == (0,) and got.dtype == np.int64
        assert np.array_equal(post.mpear_sums(lab[:3]), ref[:3])
    finally:
        post.close()


# ---------------------------------------------------------------------- Ward
def tie_rich(S, N, K, seed):
    """the samples of test_ward_linkage_on_device_is_scipys: distances k / S
    with many exact ties, a block of cells at distance 0"""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, K, size=(S, N))
    noise = rng.random_sample((S, N)) < 0.3
    base = rng.randint(0, K, N)
    a = np.where(noise, a, base[None, :])
    a[:, : N // 3] = a[:, :1]
    return a


def assert_ward_is_scipys(a):
    from scipy.cluster.hierarchy import linkage
    post = _lib.Posterior(a)
    try:
        want = linkage(post.dist(), method='ward')
        got = post.ward()
        assert got.shape == want.shape == (a.shape[1] - 1, 4)
        assert np.array_equal(got, want)
    finally:
        post.close()


@pytest.mark.parametrize('N', [256, 257, 1536, 1537])
def test_ward_at_the_grid_thresholds(N):
    """one / two workgroups of the Lance-Williams pass at 256 / 257 cells,
    one / two slices of a row scan at 1536 / 1537"""
    assert_ward_is_scipys(tie_rich(24, N, 5, N))


def test_ward_past_the_init_grid():
    """4097 rows on k_ward_init's 4096 workgroups (row 4096 is workgroup 0's
    second), 2049 double2 per row: a third scan pass of one, three slices"""
    assert_ward_is_scipys(tie_rich(40, 4097, 6, 4097))


def degenerate(kind, S, N):
    if kind == 'zeros':                     # every sample one cluster
        return np.full((S, N), 3)
    if kind == 'ones':                      # every sample all singletons
        return np.tile(np.arange(N), (S, 1))
    a = np.zeros((S, N), dtype=np.int32)    # two fixed blocks
    a[:, N // 2:] = 1
    return a


@pytest.mark.parametrize('N', [2, 3, 64, 257])
@pytest.mark.parametrize('kind', ['zeros', 'ones', 'blocks'])
def test_ward_on_nothing_but_ties(kind, N):
    """every minimum is shared by all live columns: `first index of the
    minimum, the previous element wins ties` decides every merge"""
    a = degenerate(kind, 5, N)
    want = {'zeros': {0}, 'ones': {5}, 'blocks': {0, 5} - ({0} if N == 2
        else set())}[kind]
    assert set(np.unique(Q.differ_rows(a))) == want
    assert_ward_is_scipys(a)


def raw_ward(post):
    raw = np.empty((post.N - 1, 4), dtype=np.float64)
    _lib.check(_lib.load().bnpc_post_ward(post._h, _lib.ptr(raw)),
        'post_ward')
    return raw


def test_ward_plain_launches_make_the_same_merges(monkeypatch):
    """the replayed graph and plain launches: the same raw linkage (merges in
    chain order, before the sort), and the chain's step count in its bounds"""
    n = 300
    a = tie_rich(30, n, 5, 300)
    post = _lib.Posterior(a)
    try:
        monkeypatch.delenv('BNPC_WARD_DEVICE', raising=False)
        graph = raw_ward(post)
        steps = post.ward_stats()[1]
        assert n - 1 <= steps <= 8 * n + 64
        monkeypatch.setenv('BNPC_WARD_DEVICE', 'plain')
        plain = raw_ward(post)
        assert np.array_equal(graph, plain)
        assert post.ward_stats()[1] == steps
        assert np.all(graph[:, 0] < graph[:, 1])
        assert np.array_equal(_lib.ward_finish(plain, n), post.ward())
    finally:
        post.close()


def test_ward_twice_leaves_the_counts_alone():
    a = tie_rich(12, 257, 4, 1)
    post = _lib.Posterior(a)
    try:
        before = post.differ()
        first = post.ward()
        second = post.ward()
        assert np.array_equal(first, second)
        assert np.array_equal(post.differ(), before)
        assert np.array_equal(before, Q.differ_rows(a))
        steps = post.ward_stats()[1]
        assert 256 <= steps <= 8 * 257 + 64
    finally:
        post.close()
