"""Between-chain agreement of the clustering (-pc) on the device:
bnpc_post_chain_agreement against postproc.host_chain_agreement, the
definition (itself checked against a restatement in
tests/test_chain_agreement.py).  Integers on both sides: array_equal, no
tolerance.  Shapes: N at, below and above one and two 64-cell tiles; chain
lengths inside, at and past the 32-sample staging round, one-sample chains."""
import numpy as np
import pytest

from bnpc_amd import _lib, postproc
from test_chain_agreement import (brute_tables, chains_that_differ,
    exact_half, identical_chains, opposite_chains)

pytestmark = pytest.mark.gpu

LENGTHS = {2: [33, 1], 3: [31, 32, 65], 8: [1, 31, 32, 33, 65, 1, 33, 32]}


def device(a, bounds):
    post = _lib.Posterior(a)
    try:
        return post.chain_agreement(bounds)
    finally:
        post.close()


def same(got, want):
    assert len(got) == len(want) == 3
    for name, g, w in zip(('abs_sum', 'max_abs', 'flips'), got, want):
        assert g.dtype == np.int64 and g.shape == w.shape, name
        assert np.array_equal(g, w), name


@pytest.mark.parametrize('C', sorted(LENGTHS))
@pytest.mark.parametrize('N', [2, 63, 64, 65, 129, 200])
def test_tiling_edges(N, C):
    rng = np.random.RandomState(1000 * C + N)
    a, bounds = chains_that_differ(rng, LENGTHS[C], N)
    want = postproc.host_chain_agreement(a, bounds)
    assert want[0].any() or N == 2
    same(device(a, bounds), want)


def test_a_boundary_at_every_place_of_a_staging_round():
    """two chains whose boundary is inside, at and just past the first and
    the second round of 32 samples"""
    rng = np.random.RandomState(5)
    for first, second in ((31, 32), (32, 31), (33, 64), (64, 33), (65, 1)):
        a, bounds = chains_that_differ(rng, [first, second], 70)
        same(device(a, bounds), postproc.host_chain_agreement(a, bounds))


def test_wide_products():
    """S_c R_c = 4.9e9 > 2**32: a 32-bit product anywhere shows"""
    a = np.zeros((140000, 3), dtype=np.int32)
    a[:70000:3, 2] = 1          # chain 0: cells 0, 1 together, 2 mostly too
    a[70000:] = np.arange(3)    # chain 1: all apart, but
    a[70000::7, 2] = 1          # cells 1, 2 together in every seventh sample
    bounds = [0, 70000, 140000]
    want = postproc.host_chain_agreement(a, bounds)
    assert want[1].max() == 70000 * 70000 > 2 ** 32
    assert want[0].max() > want[1].max()
    same(device(a, bounds), want)


def test_identical_chains_agree_everywhere():
    a, bounds = identical_chains(np.random.RandomState(2), 33, 3, 70)
    got = device(a, bounds)
    for table in got:
        assert table.shape == (3, 70) and not table.any()


def test_opposite_chains_flip_every_pair():
    a, bounds = opposite_chains(33, 40, 70)
    abs_sum, max_abs, flips = device(a, bounds)
    assert (max_abs == 33 * 40).all()
    assert (abs_sum == 33 * 40 * 69).all()
    assert (flips == 69).all()


def test_exact_half_is_not_a_majority():
    a, bounds = exact_half(64, 33, 66)
    got = device(a, bounds)
    same(got, postproc.host_chain_agreement(a, bounds))
    # cells 0 and 1 share a label in exactly half of chain 0 and always in
    # chain 1: apart on one side, together on the other
    assert got[2][0, 0] >= 1 and got[2][1, 1] >= 1


@pytest.fixture(scope='module')
def handle():
    rng = np.random.RandomState(11)
    a, bounds = chains_that_differ(rng, [40, 33, 70], 130)
    post = _lib.Posterior(a)
    yield post, a, bounds
    post.close()


def test_pooled_counts_are_the_handles(handle):
    """the tables made from the per-chain counts of a restatement and the
    POOLED counts of post.differ() are the kernel's"""
    from scipy.spatial.distance import squareform
    post, a, bounds = handle
    pooled = squareform(post.differ()).astype(np.int64)
    same(post.chain_agreement(bounds), brute_tables(a, bounds, pooled=pooled))


def test_second_call_gives_the_same_tables(handle):
    post, a, bounds = handle
    first = post.chain_agreement(bounds)
    same(post.chain_agreement(bounds), first)
    other = [0, 100, 143]
    want = postproc.host_chain_agreement(a, other)
    same(post.chain_agreement(other), want)
    same(post.chain_agreement(bounds), first)


def test_other_passes_are_unchanged(handle):
    post, a, bounds = handle
    labels = np.arange(130) % 4
    support = post.support(labels)
    sums = post.mpear_sums(np.stack([labels, labels // 2]))
    differ = post.differ()
    post.chain_agreement(bounds)
    assert np.array_equal(post.support(labels), support)
    assert np.array_equal(post.mpear_sums(np.stack([labels, labels // 2])),
        sums)
    assert np.array_equal(post.differ(), differ)
    assert np.array_equal(support, postproc.host_support(differ, labels))


@pytest.mark.parametrize('bounds', [[0, 143], [0, 40, 40, 143],
    [0, 73, 40, 143], [1, 40, 143], [0, 40, 142], [0, 40, 144],
    [0, 40, 150, 143]])
def test_bad_bounds_are_code_2_and_write_nothing(handle, bounds):
    post, a, good = handle
    b = np.array(bounds, dtype=np.int64)
    out = [np.full((b.size - 1, 130), -7, dtype=np.int64) for _ in range(3)]
    rc = _lib.load().bnpc_post_chain_agreement(post._h, _lib.ptr(b),
        b.size - 1, *[_lib.ptr(x) for x in out])
    assert rc == 2
    assert all((x == -7).all() for x in out)
    with pytest.raises(ValueError):
        postproc.host_chain_agreement(a, bounds)
    same(post.chain_agreement(good), postproc.host_chain_agreement(a, good))


def test_times_returns_two_positive_times(handle):
    post, a, bounds = handle
    differ = post.differ()
    t_pass, t_codist = post.chain_agreement_times(bounds, reps=2)
    assert t_pass > 0 and t_codist > 0
    assert np.array_equal(post.differ(), differ)
