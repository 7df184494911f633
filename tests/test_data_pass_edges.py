"""The two posterior passes over the data of bnpc_post_passes.hip (-pm,
bnpc_post_mutation_fit, and -pd, bnpc_post_doublets, with the mask builder
they share) at the edges their feature tests do not enter, against the host
loops they are pinned to (postproc.host_mutation_fit, postproc.host_doublets).
Every comparison goes through test_mutation_fit_gpu.compare / equal and
test_doublets_gpu.compare / equal, their bounds unchanged: array_equal
wherever they assert array_equal, 1e-12 for the device's log and
(C + 4) * 2**-52 for a log-sum-exp of C terms.  Every test asserts on its own
inputs, from the host side alone, that it reaches the edge it names (the
*_inputs functions need no device; the unmarked tests run them on the CPU).

A  several mask slabs: post_build_masks uploads the codes in slabs of
   post_mask_slab_cells(N, M) cells - about 64 MiB of codes, 64 cells at the
   least - and k_mf_masks writes slab j0 at d_masks + (j0 / 64) * Mp.  At
   M = 2**19 + 1 a slab is one block of 64 cells, so N = 130 is slabs of 64,
   64 and 2 cells: the slab loop, the offset, the staging of a slab's sorted
   cells through the permutation (-pm), a partial last slab, and a bad code's
   slab index turned back into (cell, mutation) of the caller.
B  the second workgroup over the mutations of k_mf_masks, k_mf_reduce and
   k_db_tables (256 each): M = 255, 256, 257, 513.
C  k_db_sums past its first workgroup (block b = blockIdx.y * 4 + wave): four
   blocks (wave 3), five and six (blockIdx.y = 1), for all N and for resident
   slabs that start inside a block; k_db_reduce's second workgroup of 256
   cells.
D  k_mf_count wraps its grid: `q = blockIdx.y; q < sc; q += gridDim.y` on
   min(n, 65535) rows.  S = 65538: three waves take a second sample and reuse
   their LDS tile and their register subtotals, going from two passes of
   MF_ROWS rows to one, from one to two and from two to one.
E  k_db_tables wraps its grid over min(slots, 65535) candidate slots: K = 362
   clusters are P = 65703 candidates in 65704 slots, 169 workgroups take a
   second slot.  The same call is six blocks of k_db_sums and two workgroups
   of k_db_reduce with a long walk over the pairs.

The sequential sums of A.  test_doublets_gpu.compare forms the scores'
reference in a Python loop over the mutations; at M = 2**19 + 1 the same sum
is taken here as np.cumsum(terms, axis=1)[:, -1], one candidate at a time
(compare_long, otherwise compare's own checks line for line).  A CPU test
shows on M = 65 that a result made of those sums passes compare's loop
unchanged, array_equal.

Not covered, for the record: the wrap of k_db_sums over the cell blocks (a
grid of 65535 x 4 blocks) needs N > 16.7 million cells; a chunk at the bound
chunk_max = 2**24 candidates needs K >= 5793 clusters, whose resident scores
take 8.6 GB per block of 64 cells beside 268 MB of tables per mutation, and
a host reduction of as much - minutes, not seconds; post_mask_slab_cells' cap
of 65535 blocks needs N > 4.19 million cells."""
import functools
import os
import re
import time

import numpy as np
import pytest

from bnpc_amd import _lib, postproc
import test_doublets_gpu as DB
import test_mutation_fit_gpu as MF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'bnpc_amd', 'csrc')
GRID_MAX = 65535        # the most workgroups of a launch's second dimension
T = _lib.DOUBLET_TILE
M_SLABS = 2 ** 19 + 1   # the smallest M whose slabs are one block of cells
S_WRAP = GRID_MAX + 3
ERROR = re.compile(r'^(mutation fit|doublets): code (\d+) of cell (\d+) at '
    r'mutation (\d+) is not 0, 1 or 3$')


# ---------------------------------------------------------------------------
# the drivers' arithmetic, restated
# ---------------------------------------------------------------------------
def slab_cells(N, M):
    """bnpc_post.h: post_mask_slab_cells"""
    nb = (N + 63) // 64
    return 64 * min(min(nb, 65535), max(1, (64 << 20) // (M * 64)))


def default_chunk(chunk, per_sample, S):
    """bnpc_post.h: post_default_chunk"""
    sc = chunk if chunk else max(1, (512 << 20) // per_sample)
    return min(sc, S, 2 ** 31 - 1)


def fit_chunk(chunk, S, N, M, W):
    """mf_run: the samples of a chunk of the trace"""
    return default_chunk(chunk, W * M * 4 + M * 48 + N * 2, S)


def doublet_chunk(chunk, P, M):
    """db_run: the candidates of a chunk of tables"""
    chunk_max = min(P, 1 << 24)
    if chunk:
        return min(chunk, chunk_max)
    return min(chunk_max, max(T, (512 << 20) // (M * 16)))


def resident_slabs(N, nc):
    """db_run: (i0, cells, b0, off, nblk) of every resident slab of nc cells"""
    out = []
    for i0 in range(0, N, nc):
        cells = min(nc, N - i0)
        b0 = i0 // 64
        out.append((i0, cells, b0, i0 - b0 * 64,
            (i0 + cells - 1) // 64 - b0 + 1))
    return out


def flat(text):
    return ' '.join(text.split())


def test_the_restated_arithmetic_is_the_source_s():
    with open(os.path.join(CSRC, 'bnpc_post.h')) as f:
        header = f.read()
    body = flat(re.search(r'inline int64_t post_mask_slab_cells\(int64_t N, '
        r'int64_t M\)\s*\{(.*?)\n\}', header, re.S).group(1))
    assert body == ('const int64_t nb = (N + 63) / 64; '
        'return 64 * std::min<int64_t>(std::min<int64_t>(nb, 65535), '
        'std::max<int64_t>(1, (int64_t)(((size_t)64 << 20) / '
        '((size_t)M * 64))));')
    body = flat(re.search(r'inline int64_t post_default_chunk\(.*?\{(.*?)\n\}',
        header, re.S).group(1))
    assert body == ('int64_t sc = chunk; if (sc == 0) '
        'sc = std::max<int64_t>(1, (int64_t)(((size_t)512 << 20) / '
        'bytes_per_sample)); '
        'return std::min<int64_t>(std::min(sc, S), INT_MAX);')
    with open(os.path.join(CSRC, 'bnpc_post_passes.hip')) as f:
        source = flat(f.read())
    for line in (
            # mf_run
            'const size_t sample_floats = (size_t)W * M;',
            'const size_t per_sample = sample_floats * 4 + (size_t)M * 48 '
            '+ (size_t)N * 2;',
            'const int64_t sc = post_default_chunk(chunk, per_sample, S);',
            'dim3(mtiles, (unsigned)std::min<int64_t>(n, 65535))',
            'for (int q = blockIdx.y; q < sc; q += gridDim.y) {',
            'dim3((unsigned)((M + 255) / 256)), dim3(256), 0, 0, d_sub,',
            # post_build_masks
            'for (int64_t j0 = 0; j0 < N; j0 += slab_cells) {',
            'd_masks + (size_t)(j0 / 64) * Mp, d_bad);',
            'dim3((unsigned)((Mp + 255) / 256), (unsigned)((cells + 63) / 64))',
            # db_run
            'const int64_t chunk_max = std::min<int64_t>(P, (int64_t)1 << 24);',
            'int64_t sc = chunk ? std::min(chunk, chunk_max) : '
            'std::min<int64_t>(chunk_max, std::max<int64_t>(DB_TILE, '
            '(int64_t)(((size_t)512 << 20) / ((size_t)M * 16))));',
            'const int64_t b0 = i0 / 64, off = i0 - b0 * 64;',
            'const int64_t nblk = (i0 + cells - 1) / 64 - b0 + 1;',
            'dim3((unsigned)((M + 255) / 256), (unsigned)std::min<int64_t>( '
            'tiles * DB_TILE, 65535))',
            'for (int q = blockIdx.y; q < slots; q += gridDim.y) {',
            'dim3((unsigned)tiles, (unsigned)std::min<int64_t>((nblk + 3) / 4, '
            '65535))',
            'for (long long b = (long long)blockIdx.y * 4 + wave; b < nblk;',
            'dim3((unsigned)((cells + 255) / 256))'):
        assert line in source, line
    assert f'#define MF_ROWS {_lib.MUT_FIT_ROWS} ' in source
    assert f'#define DB_TILE {T} ' in source
    # the figures of the docstring
    assert slab_cells(130, M_SLABS) == 64 and slab_cells(130, M_SLABS - 1) == 128
    assert slab_cells(65535 * 64 + 1, 1) == 65535 * 64 > 4.19e6
    assert 65535 * 4 * 64 > 16.7e6
    assert 5792 * 5793 // 2 < 2 ** 24 <= 5793 * 5794 // 2


def last_error():
    return _lib.load().bnpc_last_error().decode()


def reported():
    """(pass, code, cell, mutation) of the last error"""
    hit = ERROR.match(last_error())
    assert hit, last_error()
    return (hit.group(1),) + tuple(int(x) for x in hit.groups()[1:])


def timed(what, call, *args, **kwargs):
    t = time.perf_counter()
    out = call(*args, **kwargs)
    print(f'{what}: {time.perf_counter() - t:.2f} s')
    return out


# ---------------------------------------------------------------------------
# A: several mask slabs
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def slab_codes():
    """(130, 2**19 + 1) codes, 40 % zeros, 30 % ones, 30 % missing; read-only,
    shared"""
    N, M = 130, M_SLABS
    assert slab_cells(N, M) == 64 and slab_cells(N, M - 1) == 128
    assert [min(64, N - j0) for j0 in range(0, N, 64)] == [64, 64, 2]
    rng = np.random.RandomState(M)
    kinds = np.array([0, 0, 0, 0, 1, 1, 1, 3, 3, 3], dtype=np.uint8)
    codes = kinds[rng.randint(0, 10, (N, M), dtype=np.uint8)]
    codes.setflags(write=False)
    return codes


@pytest.fixture(scope='module', autouse=True)
def shared_codes_are_dropped_after_the_module():
    yield
    slab_codes.cache_clear()


def order_of(hint):
    """mf_run's permutation: the cells in the stable order of their labels"""
    return np.argsort(np.asarray(hint), kind='stable')


def slab_fit_inputs():
    codes = slab_codes()
    N, M = codes.shape
    S, W = 2, 3
    rng = np.random.RandomState(130)
    a = MF.samples(rng, S, N, W)
    assert MF.width(a) == W and a.max() < N
    params = MF.trace(rng, S, W, M)
    FN, FP = MF.rates(rng, S)
    hints = {'default': None, 'reversed': N - 1 - np.arange(N),
        'identity': np.arange(N), 'first sample': a[0]}
    block = np.arange(N) // 64
    for name, hint in hints.items():
        perm = order_of(a[S - 1] if hint is None else hint)
        moved = (perm // 64 != block).sum()     # cells that change their slab
        assert (moved == 0) == (name == 'identity'), name
        if name == 'reversed':
            # (all but the cells 64 and 65)
            assert (perm == np.arange(N)[::-1]).all() and moved == N - 2
    assert fit_chunk(0, S, N, M, W) == S
    return codes, a, params, FN, FP, hints


@pytest.fixture(scope='module')
def slab_fit():
    codes, a, params, FN, FP, hints = slab_fit_inputs()
    host = timed('A, -pm: host_mutation_fit', postproc.host_mutation_fit,
        codes, a, params, FN, FP)
    return codes, a, params, FN, FP, hints, host


def slab_doublet_inputs():
    codes = slab_codes()
    N, M = codes.shape
    K = 2
    rng = np.random.RandomState(131)
    labels = rng.permutation(np.arange(N) % K).astype(np.int64)
    labels[N - 2:] = (0, 1)
    # both clusters in every slab
    assert all(np.unique(labels[j0:j0 + 64]).size == K
        for j0 in range(0, N, 64))
    theta = DB.genotypes(rng, K, M)
    P = K + K * (K - 1) // 2
    assert P == 3 and doublet_chunk(0, P, M) == P
    return codes, labels, theta, rng.uniform(0.25, 0.35), \
        rng.uniform(0.5e-6, 2e-6)


def mask_layout(codes, perm, per_slab, shift=0):
    """What the counting kernels see of the cells where post_build_masks lays
    slab j0 at block j0 / 64 (+ shift for the slabs after the first): the
    codes by cell, 3 where no slab was laid"""
    N, M = codes.shape
    nb = (N + 63) // 64
    laid = np.full(((nb + shift) * 64, M), 3, dtype=np.uint8)
    for j0 in range(0, N, per_slab):
        cells = min(per_slab, N - j0)
        at = (j0 // 64 + (shift if j0 else 0)) * 64
        laid[at:at + cells] = codes[perm[j0:j0 + cells]]
    seen = np.empty_like(codes)
    seen[perm] = laid[:N]       # block b, lane l is the sorted cell 64 b + l
    return seen


def test_slab_inputs_tell_a_misplaced_slab():
    """the preconditions of A, and on the first 200 mutations: the tables
    expected from a mask layout whose later slabs lie one block too far are
    not the correct ones, under every hint and for both passes"""
    codes, a, params, FN, FP, hints = slab_fit_inputs()
    N, M = codes.shape
    cols = slice(0, 200)
    sub, par = np.ascontiguousarray(codes[:, cols]), params[:, :, cols]
    right = postproc.host_mutation_fit(sub, a, par, FN, FP)
    for name, hint in hints.items():
        perm = order_of(a[-1] if hint is None else hint)
        assert np.array_equal(mask_layout(sub, perm, slab_cells(N, M)), sub)
        wrong = postproc.host_mutation_fit(mask_layout(sub, perm,
            slab_cells(N, M), shift=1), a, par, FN, FP)
        for key in ('call1_obs1', 'call1_obs0', 'efn', 'efp', 'eg1'):
            assert (wrong[key] != right[key]).mean() > 0.9, (name, key)
        assert not np.isclose(wrong['ll'], right['ll'], rtol=1e-9,
            atol=1e-9).any(), name
    codes, labels, theta, fn, fp = slab_doublet_inputs()
    sub, th = np.ascontiguousarray(codes[:, cols]), theta[:, cols]
    right = postproc.host_doublets(sub, labels, th, fn, fp)
    wrong = postproc.host_doublets(mask_layout(sub, np.arange(N),
        slab_cells(N, M), shift=1), labels, th, fn, fp)
    moved = np.arange(N) >= 64
    assert np.array_equal(wrong['scores'][~moved], right['scores'][~moved])
    assert not np.isclose(wrong['scores'][moved], right['scores'][moved],
        rtol=1e-9, atol=1e-9).any()


@pytest.mark.gpu
def test_mutation_fit_over_three_mask_slabs(slab_fit):
    codes, a, params, FN, FP, hints, host = slab_fit
    S = a.shape[0]
    post = _lib.Posterior(a)
    try:
        t = time.perf_counter()
        want = post.mutation_fit(codes, params, FN, FP, matrix=True)
        print(f'A, -pm: the device call: {time.perf_counter() - t:.2f} s')
        MF.compare(want, host)
        for name, hint in hints.items():
            MF.equal(post.mutation_fit(codes, params, FN, FP, order=hint,
                matrix=True), want)
        assert fit_chunk(1, S, *codes.shape, params.shape[1]) == 1 < S
        MF.equal(post.mutation_fit(codes, params, FN, FP, chunk=1,
            order=hints['reversed'], matrix=True), want)
    finally:
        post.close()


def fit_raw_call(post, codes, params, FN, FP, order, out):
    order = None if order is None \
        else np.ascontiguousarray(order, dtype=np.int32)
    return _lib.load().bnpc_post_mutation_fit(post._h, _lib.ptr(codes),
        _lib.ptr(params), params.shape[1], params.shape[2], _lib.ptr(FN),
        _lib.ptr(FP), None if order is None else _lib.ptr(order), 0,
        *[_lib.ptr(o) for o in out])


def first_bad(spots, perm, M):
    """the bad code post_build_masks reports: the smallest slab index of the
    first slab that holds one - the first in the sorted order of the cells"""
    place = np.empty(perm.size, dtype=np.int64)
    place[perm] = np.arange(perm.size)
    return min(spots, key=lambda at: place[at[0]] * M + at[1])


@pytest.mark.gpu
def test_bad_code_in_a_later_slab_of_the_mutation_fit(slab_fit):
    """The slab index of a bad code goes back to the caller's cell through
    the permutation of the hint.  Places are given in the sorted order."""
    codes, a, params, FN, FP, hints, host = slab_fit
    (S, N), M = a.shape, codes.shape[1]
    bad = codes.copy()
    out = [np.full(M, 7.25) for _ in range(5)] \
        + [np.full(M, 725, dtype=np.int64) for _ in range(2)] \
        + [np.full((S, M), 7.25)]
    # sorted places: in the second slab, in the third, the last cell of the
    # last slab at the last mutation; the caller's last cell; two at once,
    # the later place at the smaller mutation
    cases = ([(64 + 5, 7)], [(128, 3)], [(N - 1, M - 1)], None,
        [(N - 1, 0), (70, M - 1)], [(128, 0), (127, M - 1)])
    post = _lib.Posterior(a)
    try:
        for name in ('reversed', 'default', 'identity'):
            hint = hints[name]
            perm = order_of(a[S - 1] if hint is None else hint)
            for places in cases:
                spots = [(N - 1, M - 1)] if places is None \
                    else [(int(perm[j]), m) for j, m in places]
                if places is not None and len(places) == 2:
                    assert places[0][0] // 64 != places[1][0] // 64
                for at in spots:
                    bad[at] = 2
                try:
                    assert fit_raw_call(post, bad, params, FN, FP, hint,
                        out) == 2
                    assert reported() == ('mutation fit', 2) \
                        + first_bad(spots, perm, M), (name, places)
                finally:
                    for at in spots:
                        bad[at] = codes[at]
                assert all((o == 7.25).all() for o in out[:5] + out[7:])
                assert all((o == 725).all() for o in out[5:7])
        assert np.array_equal(bad, codes)
        MF.compare(post.mutation_fit(bad, params, FN, FP, matrix=True,
            order=hints['reversed']), host)
    finally:
        post.close()


def sequential_scores(codes, L1, L0):
    """test_doublets_gpu.compare's sequential sums over the mutations, one
    candidate at a time"""
    is1, is0 = codes == 1, codes == 0
    seq = np.empty((codes.shape[0], L1.shape[0]))
    for c in range(L1.shape[0]):
        terms = np.where(is1, L1[c], np.where(is0, L0[c], 0.0))
        seq[:, c] = np.cumsum(terms, axis=1)[:, -1]
    return seq


def compare_long(got, data, labels, theta, FN, FP):
    """test_doublets_gpu.compare with the scores' reference from
    sequential_scores; every other line is compare's"""
    got = dict(zip(DB.NAMES, got))
    N, (K, M) = labels.size, theta.shape
    P = K + K * (K - 1) // 2
    for name in DB.NAMES[:5]:
        assert got[name].shape == (N,) and got[name].dtype == np.float64, name
    assert got['best_single'].shape == (N,) \
        and got['best_single'].dtype == np.int32
    assert got['best_pair'].shape == (N, 2) \
        and got['best_pair'].dtype == np.int32
    assert got['scores'].shape == (N, P)
    assert got['L1'].shape == got['L0'].shape == (P, M)
    h1, h0 = postproc.doublet_tables(theta, FN, FP)
    for name, dev, host in (('L1', got['L1'], h1), ('L0', got['L0'], h0)):
        err = np.abs(dev - host) / (1 + np.abs(host))
        print(f'{name}: max |dev - host| / (1 + |host|) = {err.max():.3e}')
        np.testing.assert_allclose(dev, host, rtol=1e-12, atol=1e-12)
    assert np.isfinite(got['L1']).all() and np.isfinite(got['L0']).all()
    seq = sequential_scores(postproc.data_codes(data), got['L1'], got['L0'])
    assert np.array_equal(got['scores'], seq), \
        np.argwhere(got['scores'] != seq)[:5]
    assert not np.signbit(got['scores'][got['scores'] == 0]).any()
    default = DB.weights(labels, K)
    red = postproc.doublet_reduce(got['scores'], labels, K, *default)
    for name in ('own', 'best_single', 'best_pair', 'll_single', 'll_pair'):
        assert np.array_equal(got[name], red[name]), \
            (name, np.argwhere(got[name] != red[name])[:5])
    for name, C in (('lse_single', K), ('lse_pair', P - K)):
        if not C:
            assert (got[name] == -np.inf).all(), name
            continue
        off = np.abs(got[name] - red[name])
        print(f'{name}: max |dev - host reduction| = {off.max():.3e}')
        assert (off <= (C + 4) * DB.ULP + DB.ULP * np.abs(got[name])).all(), \
            name
    return got


def test_cumsum_is_the_sequential_sum_of_the_doublet_tests():
    """A result whose scores are sequential_scores of its tables passes
    test_doublets_gpu.compare, whose loop over the mutations asserts
    array_equal; one whose scores are NumPy's pairwise sums does not."""
    N, M, K = 70, 65, 4
    data, labels, theta, FN, FP = DB.case(65, N, M, K)
    codes = postproc.data_codes(data)
    L1, L0 = postproc.doublet_tables(theta, FN, FP)

    def result(scores):
        red = postproc.doublet_reduce(scores, labels, K, *DB.weights(labels, K))
        return tuple(red[name] for name in DB.NAMES[:7]) + (scores, L1, L0)

    seq = sequential_scores(codes, L1, L0)
    DB.compare(result(seq), data, labels, theta, FN, FP)
    compare_long(result(seq), data, labels, theta, FN, FP)
    assert np.array_equal(seq, postproc.host_doublets(data, labels, theta,
        FN, FP)['scores'])
    pairwise = np.stack([np.where(codes == 1, L1[c], np.where(codes == 0,
        L0[c], 0.0)).sum(axis=1) for c in range(L1.shape[0])], axis=1)
    assert not np.array_equal(pairwise, seq)
    for check in (DB.compare, compare_long):
        with pytest.raises(AssertionError):
            check(result(pairwise), data, labels, theta, FN, FP)


@pytest.mark.gpu
def test_doublets_over_three_mask_slabs_and_their_bad_codes():
    """No permutation here: a slab holds the caller's cells j0 .. j0 + 63, and
    of two bad codes the one in the earlier slab is reported."""
    codes, labels, theta, FN, FP = slab_doublet_inputs()
    (N, M), K, P = codes.shape, 2, 3
    logw, lN, lT = DB.weights(labels, K)
    bad = codes.copy()
    out = [np.full(N, 7.25) for _ in range(5)] + [
        np.full(N, 77, dtype=np.int32), np.full((N, 2), 77, dtype=np.int32),
        np.full((N, P), 7.25), np.full((P, M), 7.25), np.full((P, M), 7.25)]
    cases = ([(64 + 5, 7)], [(128, 3)], [(N - 1, M - 1)],
        [(N - 1, 0), (70, M - 1)], [(128, 0), (127, M - 1)])
    post = _lib.Posterior(labels[None, :])
    try:
        t = time.perf_counter()
        want = post.doublets(codes, labels, theta, FN, FP, matrix=True,
            tables=True)
        print(f'A, -pd: the device call: {time.perf_counter() - t:.2f} s')
        timed('A, -pd: the host reference', compare_long, want, codes, labels,
            theta, FN, FP)
        for spots in cases:
            for at in spots:
                bad[at] = 2
            try:
                assert DB.raw_call(post, bad, labels, theta, FN, FP, logw, lN,
                    lT, out) == 2
                assert reported() == ('doublets', 2) \
                    + first_bad(spots, np.arange(N), M), spots
                assert reported()[2:] == min(spots)
            finally:
                for at in spots:
                    bad[at] = codes[at]
            assert all((o == 7.25).all() for o in out[:5] + out[7:])
            assert (out[5] == 77).all() and (out[6] == 77).all()
        assert np.array_equal(bad, codes)
        DB.equal(post.doublets(bad, labels, theta, FN, FP, matrix=True,
            tables=True), want)
    finally:
        post.close()


# ---------------------------------------------------------------------------
# B: second workgroups over the mutations
# ---------------------------------------------------------------------------
GROUPS = {255: 1, 256: 1, 257: 2, 513: 3}


@pytest.mark.gpu
@pytest.mark.parametrize('M', sorted(GROUPS))
def test_mutation_fit_beside_its_workgroup_of_256_mutations(M):
    assert (M + 255) // 256 == GROUPS[M]
    S, N = 3, 70
    data, a, params, FN, FP = MF.case(3000 + M, S, N, M, 5)
    assert MF.width(a) == 5
    got, host = MF.check(data, a, params, FN, FP)
    # the last mutation is somebody's
    assert host['n1'][M - 1] + host['n0'][M - 1] > 0 and got[7][:, M - 1].all()
    post = _lib.Posterior(a)
    try:
        MF.equal(post.mutation_fit(data, params, FN, FP, chunk=2,
            matrix=True), got)
    finally:
        post.close()


@pytest.mark.gpu
@pytest.mark.parametrize('M', sorted(GROUPS))
def test_doublet_tables_beside_their_workgroup_of_256_mutations(M):
    assert (M + 255) // 256 == GROUPS[M]
    data, labels, theta, FN, FP = DB.case(4000 + M, 70, M, 4)
    DB.check(data, labels, theta, FN, FP)


# ---------------------------------------------------------------------------
# C: cells past one workgroup and past four blocks, -pd
# ---------------------------------------------------------------------------
BLOCKS = {193: (4, 1, 1), 256: (4, 1, 1), 257: (5, 2, 2), 321: (6, 2, 2)}


def past_four_blocks_inputs(N):
    nb = (N + 63) // 64
    assert (nb, (nb + 3) // 4, (N + 255) // 256) == BLOCKS[N]
    data, labels, theta, FN, FP = DB.case(5000 + N, N, 5, 3)
    # every cell of the last block shows something (test_doublets_gpu.matrix
    # leaves the last cell without an entry)
    last = slice((nb - 1) * 64, N)
    data[last, 0] = np.arange(N - (nb - 1) * 64) % 2
    assert not np.isnan(data[last]).all(axis=1).any()
    return data, labels, theta, FN, FP


@pytest.mark.gpu
@pytest.mark.parametrize('N', sorted(BLOCKS))
def test_doublet_sums_past_four_blocks_of_cells(N):
    """(blocks of 64 cells, workgroups of k_db_sums along y, workgroups of
    k_db_reduce): wave 3 has a block at four blocks, the second workgroup's
    wave 0 at five, its wave 1 at six"""
    nb = (N + 63) // 64
    assert (nb, (nb + 3) // 4, (N + 255) // 256) == BLOCKS[N]
    data, labels, theta, FN, FP = past_four_blocks_inputs(N)
    got = DB.check(data, labels, theta, FN, FP)
    assert got['scores'][(nb - 1) * 64:].all()


def resident_inputs():
    N, M, K = 700, 7, 5
    P = K + K * (K - 1) // 2
    assert P == 15 and doublet_chunk(T + 1, P, M) == T + 1 < P
    assert doublet_chunk(0, P, M) == P
    slabs = {nc: resident_slabs(N, nc) for nc in (257, 300, 320)}
    # a slab that starts inside a block and is more than a workgroup's four
    i0, cells, b0, off, nblk = slabs[300][1]
    assert (i0, cells, b0, off, nblk) == (300, 300, 4, 44, 6)
    assert [s[3:] for s in slabs[257]] == [(0, 5), (1, 5), (2, 3)]
    assert [s[3:] for s in slabs[320]] == [(0, 5), (0, 5), (0, 1)]
    # and a reduction of two workgroups in every first slab
    assert all((s[0][1] + 255) // 256 == 2 for s in slabs.values())
    return DB.case(700, N, M, K), sorted(slabs)


@pytest.mark.gpu
def test_resident_slabs_past_four_blocks_of_cells():
    (data, labels, theta, FN, FP), slabs = resident_inputs()
    post = _lib.Posterior(labels[None, :])
    try:
        want = post.doublets(data, labels, theta, FN, FP, matrix=True,
            tables=True)
        DB.compare(want, data, labels, theta, FN, FP)
        for slab in slabs:
            for chunk in (0, T + 1):
                DB.equal(post.doublets(data, labels, theta, FN, FP,
                    chunk=chunk, slab=slab, matrix=True, tables=True), want)
    finally:
        post.close()


# ---------------------------------------------------------------------------
# D: k_mf_count wraps
# ---------------------------------------------------------------------------
WRAP_COUNTS = {0: 33, 1: 1, 2: 40, GRID_MAX: 1, GRID_MAX + 1: 34,
    GRID_MAX + 2: 2}


def distinct(a):
    return (np.diff(np.sort(a, axis=1), axis=1) != 0).sum(axis=1) + 1


def wrap_fit_inputs():
    S, N, M, W = S_WRAP, 40, 3, 40
    rng = np.random.RandomState(S)
    counts = rng.randint(1, 4, S)
    for s, d in WRAP_COUNTS.items():
        counts[s] = d
    # the labels of a sample: `counts` of [0, N) of its own, the first of
    # its cells one each, so that every one is carried
    pool = np.argsort(rng.random_sample((S, N)), axis=1)
    cell = np.arange(N)[None, :]
    pick = np.where(cell < counts[:, None], cell,
        rng.randint(0, 2 ** 30, (S, N)) % counts[:, None])
    a = np.take_along_axis(pool, pick, axis=1).astype(np.int64)
    assert S > GRID_MAX and a.shape == (S, N) and 0 <= a.min() \
        and a.max() == N - 1
    assert np.array_equal(distinct(a), counts)
    assert all(np.unique(a[s]).size == d for s, d in WRAP_COUNTS.items())
    rest = np.delete(counts, list(WRAP_COUNTS))
    assert rest.min() == 1 and rest.max() == 3
    # the passes of MF_ROWS rows a wave takes on its first and second trip
    passes = (counts + _lib.MUT_FIT_ROWS - 1) // _lib.MUT_FIT_ROWS
    assert [(int(passes[s]), int(passes[s + GRID_MAX])) for s in range(3)] \
        == [(2, 1), (1, 2), (2, 1)]
    assert W == counts.max() and fit_chunk(0, S, N, M, W) == S
    assert fit_chunk(GRID_MAX + 1, S, N, M, W) == GRID_MAX + 1
    params = MF.trace(rng, S, W, M)
    data = MF.matrix(rng, N, M)
    # the rows of its tile that a wave's second sample uses hold, after its
    # first sample, counts at every mutation: the few cells of the first
    # rows of the samples 0 and 2 show an entry everywhere
    for first in (0, 2):
        rank = np.unique(a[first], return_inverse=True)[1].ravel()
        cells = np.flatnonzero(rank < counts[first + GRID_MAX])
        assert cells.size <= 4
        data[cells] = np.where(np.isnan(data[cells]), 1.0, data[cells])
    FN, FP = MF.rates(rng, S)
    assert np.unique(FN).size == S and np.unique(FP).size == S
    return data, a, params, FN, FP


@pytest.fixture(scope='module')
def wrap_fit():
    data, a, params, FN, FP = wrap_fit_inputs()
    host = timed(f'D: host_mutation_fit over {S_WRAP} samples',
        postproc.host_mutation_fit, data, a, params, FN, FP)
    return data, a, params, FN, FP, host


def row_from_counts(c1, c0, P, fn, fp):
    """host_mutation_fit's ll of one sample from its rows' counts"""
    ll = np.zeros(c1.shape[1])
    for r in range(c1.shape[0]):
        th = np.asarray(P[r], dtype=np.float32)
        t = th.astype(np.float64)
        o = (np.float32(1) - th).astype(np.float64)
        ll += c1[r] * np.log(t * (1 - fn) + o * fp) \
            + c0[r] * np.log(t * fn + o * (1 - fp))
    return ll


def row_counts(codes, labels):
    rank = np.unique(labels, return_inverse=True)[1].ravel()
    return tuple(np.array([(codes[rank == r] == v).sum(axis=0)
        for r in range(rank.max() + 1)], dtype=np.float64) for v in (1, 0))


def test_wrap_inputs_tell_a_wave_that_keeps_its_first_sample():
    """the preconditions of D, and: with the counts of a wave's first sample
    left in its tile, or its subtotals left in its registers, the rows
    expected of the wrapped samples are not the correct ones"""
    data, a, params, FN, FP = wrap_fit_inputs()
    codes = postproc.data_codes(data)
    for first in range(3):
        s = first + GRID_MAX
        both = [first, s]
        right = postproc.host_mutation_fit(data, a[both], params[both],
            FN[both], FP[both])['ll']
        (f1, f0), (c1, c0) = row_counts(codes, a[first]), \
            row_counts(codes, a[s])
        assert np.array_equal(row_from_counts(f1, f0, params[first],
            FN[first], FP[first]), right[0])
        assert np.array_equal(row_from_counts(c1, c0, params[s], FN[s],
            FP[s]), right[1])
        rows = min(f1.shape[0], c1.shape[0])
        k1, k0 = c1.copy(), c0.copy()
        k1[:rows] += f1[:rows]
        k0[:rows] += f0[:rows]
        for wrong in (row_from_counts(k1, k0, params[s], FN[s], FP[s]),
                right[1] + right[0], right[0]):
            assert not np.isclose(wrong, right[1], rtol=1e-9, atol=1e-9).any()


@pytest.mark.gpu
def test_wrapped_counting_launch_of_the_mutation_fit(wrap_fit):
    """chunk=0: one chunk of 65538 samples, k_mf_count on 65535 rows of
    workgroups; chunk=65536: a wrap by exactly one sample, then a chunk of
    two; chunk=65535: no wrap, then three."""
    data, a, params, FN, FP, host = wrap_fit
    tail = host['ll'][GRID_MAX:]
    assert tail.all() and not np.isclose(tail, host['ll'][:3], rtol=1e-9,
        atol=1e-9).any()
    post = _lib.Posterior(a)
    try:
        t = time.perf_counter()
        got = post.mutation_fit(data, params, FN, FP, matrix=True)
        print(f'D: the device call: {time.perf_counter() - t:.2f} s')
        MF.compare(got, host)
        for chunk in (GRID_MAX + 1, GRID_MAX):
            MF.equal(post.mutation_fit(data, params, FN, FP, chunk=chunk,
                matrix=True), got)
    finally:
        post.close()


# ---------------------------------------------------------------------------
# E: k_db_tables wraps
# ---------------------------------------------------------------------------
def wrap_doublet_inputs():
    K = N = 362
    M = 2
    P = K + K * (K - 1) // 2
    slots = (P + T - 1) // T * T
    assert P == 65703 and slots == 65704 and slots - GRID_MAX == 169
    assert doublet_chunk(0, P, M) == P
    nb = (N + 63) // 64
    assert nb == 6 and (nb + 3) // 4 == 2 and (N + 255) // 256 == 2
    data, labels, theta, FN, FP = DB.case(K, N, M, K)
    assert np.array_equal(np.sort(labels), np.arange(K))
    # the wrapped slots are pairs of their own: not the tables of the slots
    # the same workgroups took first
    L1, L0 = postproc.doublet_tables(theta, FN, FP)
    assert not np.array_equal(L1[GRID_MAX:], L1[:P - GRID_MAX])
    assert not np.array_equal(L0[GRID_MAX:], L0[:P - GRID_MAX])
    return data, labels, theta, FN, FP


def test_the_inputs_of_the_other_cases_reach_their_edges():
    """B, C and E on the CPU (A and D have tests of their own above)"""
    for M, groups in GROUPS.items():
        assert (M + 255) // 256 == groups
    for N in BLOCKS:
        past_four_blocks_inputs(N)
    resident_inputs()
    wrap_doublet_inputs()


@pytest.mark.gpu
def test_wrapped_table_launch_of_the_doublets():
    data, labels, theta, FN, FP = wrap_doublet_inputs()
    post = _lib.Posterior(labels[None, :])
    try:
        t = time.perf_counter()
        got = post.doublets(data, labels, theta, FN, FP, matrix=True,
            tables=True)
        print(f'E: the device call: {time.perf_counter() - t:.2f} s')
    finally:
        post.close()
    timed('E: the host reference', DB.compare, got, data, labels, theta, FN,
        FP)
