"""The placement pass (-pn: bnpc_post_place - pn_run with k_pn_tables,
k_pn_counts, k_pn_soft, k_pn_accum, k_pn_lpd, and k_cg_rank and k_db_sums as it
launches them - in bnpc_post_passes.hip) at the edges its feature tests
(tests/test_place_gpu.py) do not enter.  Every comparison goes through that
file's compare, check and equal, unchanged: the scores within 1e-12 of the
host's, the reductions within the bounds derived in its docstring, "the same
bits for any chunk and slab" as array_equal.  Every group has a *_inputs
function that needs no device, and an unmarked test that asserts on those
inputs, with pn_run's own arithmetic restated (plan), that they reach the edge
the group names.

A  more than 256 training cells, rows and clusters.  k_pn_counts walks the
   cells `for (long long i = tid; i < N; i += 256) atomicAdd(&cnt[...` and
   the sample's rows `for (int r = tid; r < D; r += 256)`, and reads ranks as
   unsigned short; k_cg_rank writes them with pitch N; k_pn_soft and
   k_pn_accum walk `c <= D` resp. `r < D` candidates; k_pn_accum's
   accumulator row is `j = blockIdx.y` on a grid of K + 2.  N = 257, 300, 513
   with samples of 1 to 513 clusters, W = N, K = 2 and 257; N = 300 once more
   with chunk=2, where `first[q] = (int)cn` restarts inside the samples.
B  new cells past the first workgroup and the first block group:
   `i = blockIdx.x * 256 + threadIdx.x` of k_pn_soft, k_pn_accum and k_pn_lpd
   at blockIdx.x >= 1 (Q = 255, 256, 257, 513, 700); k_db_sums'
   `b = blockIdx.y * 4 + wave` at blockIdx.y >= 1 with the placement's own
   pitch and c0 = 0; resident slabs of Q = 700 that start inside a block
   (`off` = 44, 24, ...) and are longer than a workgroup, a last workgroup of
   one cell, and `pitch = nblk_max * 64` of a slab that is not the whole call.
C  the wrapped grids: S = 65538 samples in one chunk.  k_pn_tables
   `for (int c = blockIdx.y; c < slots; c += gridDim.y)` over about 178 000
   slots, k_pn_counts `q += gridDim.x`, k_pn_soft `q += gridDim.y` and
   k_cg_rank `q += gridDim.x` (pitch N) each on 65535 workgroups.  The samples
   are seven templates in turn and 65535 % 7 = 1, so a workgroup's second
   sample is not its first.  The same call in chunks of 16384 wraps nowhere and
   has to give the same bits.
D  the cap `sc = min(sc, max(1, 2^24 / (W + 1)))` binds: W = 65533, S = 257,
   chunks of 256 and 1 samples where post_default_chunk alone gives 257.
E  exponentials that flush to zero.  k_pn_soft: `e = exp(d)` is exactly 0
   for candidates more than 745 below the maximum, `h += e * d` adds 0 * d,
   k_pn_accum multiplies a share with a probability of 0; the maximum at the
   first row, an inner row, the last row and the new cluster.  k_pn_lpd:
   `exp(col[s * pp] - mx)` is 0 for samples more than 745 below the column's
   maximum, which sits at the first, an inner and the last sample.

Not covered, for the record: the free-memory slab fit (`nc = fit`, rounded
to whole blocks) needs a full device; the global-slice rank path starts past
N = 257 984 training cells, and the handle's pair counts at that size take
tens of GB; K near 65533 needs as many training cells; the blockIdx.y wrap
of k_db_sums needs more than 16.7 million new cells."""
import os

import numpy as np
import pytest

from bnpc_amd import _lib, postproc
from test_data_pass_edges import default_chunk, flat, resident_slabs
from test_place import PRIOR, clustering, new_cells, samples
from test_place_gpu import NAMES, case, check, compare, equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = _lib.DOUBLET_TILE
GRID_MAX = 65535        # the most workgroups of a launch's dimension
S_WRAP = GRID_MAX + 3
FLUSH = 745.2           # exp(-x) is 0.0 past x = 745.14


# ---------------------------------------------------------------------------
# pn_run's arithmetic, restated
# ---------------------------------------------------------------------------
def plan(a, M, W, Q, chunk=0, slab=0):
    """-> (chunks, slabs, pitch).  chunks: (s0, n, first, cn, tiles) of every
    chunk of samples, first[q] the chunk's first candidate of its sample q, cn
    its candidates, tiles * T its slots; slabs: (i0, cells, b0, off, nblk) of
    every resident slab of new cells (the free-memory fit left aside: a slab
    is `slab` cells, or all of them)"""
    S = a.shape[0]
    distinct = np.array([np.unique(row).size for row in a])
    sc = default_chunk(chunk, W * M * 4 + (W + 1) * M * 16, S)
    sc = min(sc, max(1, (1 << 24) // (W + 1)))
    chunks = []
    for s0 in range(0, S, sc):
        n = min(sc, S - s0)
        ends = np.cumsum(distinct[s0:s0 + n] + 1)
        cn = int(ends[-1])
        chunks.append((s0, n, ends - distinct[s0:s0 + n] - 1, cn,
            (cn + T - 1) // T))
    nb = (Q + 63) // 64
    nc = min(slab, Q) if slab else Q
    nblk_max = nb if nc >= Q else (nc + 62) // 64 + 1
    return chunks, resident_slabs(Q, nc), nblk_max * 64


def test_the_restated_arithmetic_is_the_source_s():
    with open(os.path.join(ROOT, 'bnpc_amd', 'csrc',
            'bnpc_post_passes.hip')) as f:
        source = flat(f.read())
    for line in (
            # pn_run
            'int64_t sc = post_default_chunk(chunk, sample_floats * '
            'sizeof(float) + (size_t)(W + 1) * M * 16, S);',
            'sc = std::min<int64_t>(sc, std::max<int64_t>(1, ((int64_t)1 << 24) '
            '/ (W + 1)));',
            'nc = std::min(slab, Q);',
            'const int64_t nblk_max = nc >= Q ? nb : (nc + 62) / 64 + 1;',
            'const int64_t pitch = nblk_max * 64;',
            'for (int64_t i0 = 0; i0 < Q; i0 += nc) {',
            'first[q] = (int)cn;',
            'const int64_t tiles = (cn + DB_TILE - 1) / DB_TILE;',
            'post_launch_rank(p, area, s0, n, 0, N, N, d_rank);',
            'hipLaunchKernelGGL(k_pn_tables, dim3((unsigned)((M + 255) / 256), '
            '(unsigned)std::min<int64_t>( tiles * DB_TILE, 65535)),',
            'hipLaunchKernelGGL(k_pn_counts, '
            'dim3((unsigned)std::min<int64_t>(n, 65535)),',
            'hipLaunchKernelGGL(k_pn_soft, dim3((unsigned)((cells + 255) / '
            '256), (unsigned)std::min<int64_t>(n, 65535)),',
            'hipLaunchKernelGGL(k_pn_accum, dim3((unsigned)((cells + 255) / '
            '256), (unsigned)(K + 2)),',
            '(long long)nblk, (long long)pitch, 0LL, d_SC);',
            # the kernels' loops
            'for (int c = blockIdx.y; c < slots; c += gridDim.y) {',
            'for (int q = blockIdx.x; q < sc; q += gridDim.x) { const int base '
            '= first[q], D = distinct[q];',
            'for (long long i = tid; i < N; i += 256) atomicAdd(&cnt[',
            'for (int r = tid; r < D; r += 256) { int *row = cnt',
            'for (int q = blockIdx.y; q < sc; q += gridDim.y) { const int base '
            '= first[q], D = distinct[q]; double *col = SCO',
            'const int j = (int)blockIdx.y; double sum = acc[',
            # post_launch_rank, post_rank_area's grid through it
            'dim3((unsigned)std::min<int64_t>(n, area.grid))'):
        assert line in source, line
    with open(os.path.join(ROOT, 'bnpc_amd', 'csrc', 'bnpc_post.h')) as f:
        assert 'a.grid = (unsigned)std::min<int64_t>(S, 65535);' in f.read()
    assert f'#define DB_TILE {T} ' in source
    # the figures of the docstring
    assert np.exp(-FLUSH) == 0.0 and np.exp(-745.0) > 0
    assert GRID_MAX * 4 * 64 > 16.7e6 and GRID_MAX % 7 == 1
    assert 8 * ((_lib.CELL_RANK_LDS_CELLS + 31) // 32) + 1040 == 65536


def ranks(a):
    return np.array([np.unique(row, return_inverse=True)[1].ravel()
        for row in a])


# ---------------------------------------------------------------------------
# A: more than 256 training cells, rows and clusters
# ---------------------------------------------------------------------------
WIDE = {257: (1, 257, 128), 300: (255, 300, 256, 257), 513: (513, 2, 300)}
WIDE_CASES = [(N, K) for N in WIDE for K in (2, 257)]


def wide_inputs(N, K):
    rng = np.random.RandomState(1000 * N + K)
    M, Q = 5, 6
    a, par, FN, FP, alpha = samples(rng, len(WIDE[N]), N, N, M,
        clusters=WIDE[N], in_range=True)
    return new_cells(rng, Q, M), a, clustering(rng, N, K), par, FN, FP, alpha


def test_wide_inputs_pass_256_cells_rows_and_ranks():
    crowded = 0
    for N, K in WIDE_CASES:
        new, a, labels, par, FN, FP, alpha = wide_inputs(N, K)
        assert a.shape == (len(WIDE[N]), N) and N > 256
        assert par.shape[1] == N and new.shape == (6, 5)
        rank = ranks(a)
        assert (rank.max(axis=1) + 1).tolist() == list(WIDE[N])
        assert max(WIDE[N]) > 256 and rank.max() >= 256
        assert rank.max() < 2 ** 16
        sizes = [np.bincount(r) for r in rank]
        crowded += any((n[256:] > 1).any() for n in sizes)
        # a row with cells on either side of cell 256 somewhere: a count that
        # two trips of the cell loop add to
        assert any(((np.bincount(r[:256], minlength=N) > 0)
            & (np.bincount(r[256:], minlength=N) > 0)).any() for r in rank)
        assert labels.max() + 1 == K and labels.size == N
        if K == 257:
            assert K + 2 > 256          # k_pn_accum at blockIdx.y >= 256
            assert (labels >= 256).any()
        chunks, slabs, pitch = plan(a, 5, N, 6)
        assert len(chunks) == 1 and len(slabs) == 1 and pitch == 64
        assert chunks[0][3] == sum(WIDE[N]) + len(WIDE[N])
    assert crowded >= 1     # a row past 255 with more than one cell
    # chunk=2 at N = 300: the second chunk's list starts again at 0
    a = wide_inputs(300, 2)[1]
    chunks, _, _ = plan(a, 5, 300, 6, chunk=2)
    assert [(s0, n) for s0, n, _, _, _ in chunks] == [(0, 2), (2, 2)]
    assert chunks[0][2].tolist() == [0, 256] and chunks[1][2].tolist() == [0, 257]
    assert chunks[0][3] == 255 + 300 + 2 and chunks[1][3] == 256 + 257 + 2


@pytest.mark.gpu
@pytest.mark.parametrize('N,K', WIDE_CASES)
def test_more_than_256_training_cells_rows_and_clusters(N, K):
    new, a, labels, par, FN, FP, alpha = wide_inputs(N, K)
    got = check(new, a, labels, par, FN, FP, alpha)
    if N == 300:
        post = _lib.Posterior(a)
        try:
            equal(post.place(new, labels, par, FN, FP, alpha, chunk=2,
                matrix=True), tuple(got[k] for k in NAMES))
        finally:
            post.close()


# ---------------------------------------------------------------------------
# B: new cells past the first workgroup and block group
# ---------------------------------------------------------------------------
MANY = (255, 256, 257, 513)
Q_SLABS = 700
# (280 for a slab at off = 24 that is longer than a workgroup: at slab = 300
# the slab at off = 24 is the last one, of 100 cells)
SLABS = (300, 257, 320, 64, 280)


def many_inputs(Q):
    """(new, a, labels, par, FN, FP, alpha): S = 3, N = 20, M = 7, W = 5,
    K = 3"""
    return case(7000 + Q, 3, 20, 7, 5, 3, Q)


def test_many_inputs_pass_the_first_workgroup_and_block_group():
    for Q in MANY + (Q_SLABS,):
        new, a = many_inputs(Q)[:2]
        assert new.shape == (Q, 7) and a.shape == (3, 20)
        chunks, slabs, pitch = plan(a, 7, 5, Q)
        assert len(chunks) == 1 and slabs == [(0, Q, 0, 0, (Q + 63) // 64)]
        assert pitch == (Q + 63) // 64 * 64
        assert (Q + 255) // 256 == {255: 1, 256: 1, 257: 2, 513: 3, 700: 3}[Q]
    assert 257 % 256 == 1 and 513 % 256 == 1    # a last workgroup of one cell
    assert ((Q_SLABS + 63) // 64 + 3) // 4 == 3     # k_db_sums' blockIdx.y
    a = many_inputs(Q_SLABS)[1]
    seen = {}
    for slab in SLABS:
        for chunk in (0, 2):
            chunks, slabs, pitch = plan(a, 7, 5, Q_SLABS, chunk, slab)
            assert [n for _, n, _, _, _ in chunks] == ([2, 1] if chunk
                else [3])
            assert sum(cells for _, cells, _, _, _ in slabs) == Q_SLABS
            assert pitch == ((slab + 62) // 64 + 1) * 64
            # every slab inside the pitch
            assert all(off + cells <= pitch and nblk * 64 <= pitch
                for _, cells, _, off, nblk in slabs)
        seen[slab] = slabs
    # 300: slabs inside a block, one of them longer than a workgroup, on more
    # than four blocks
    assert [(off, cells) for _, cells, _, off, _ in seen[300]] \
        == [(0, 300), (44, 300), (24, 100)]
    assert (300 + 62) // 64 + 1 >= 5
    i0, cells, b0, off, nblk = seen[300][1]
    assert off and cells > 256 and nblk == 6 and (nblk + 3) // 4 == 2
    assert [(off, cells) for _, cells, _, off, _ in seen[280]] \
        == [(0, 280), (24, 280), (48, 140)]
    assert seen[280][1][4] == 5 and (5 + 3) // 4 == 2
    # 257: a last workgroup of one cell, in slabs at off = 1 and 2
    assert [(off, cells) for _, cells, _, off, _ in seen[257]] \
        == [(0, 257), (1, 257), (2, 186)]
    assert (257 + 255) // 256 == 2 and 257 - 256 == 1
    # 320: whole blocks, five of them; 64: one block a slab
    assert all(off == 0 and nblk == 5 for _, cells, _, off, nblk
        in seen[320][:2])
    assert len(seen[64]) == 11 and seen[64][-1][1] == 700 - 640


@pytest.mark.gpu
@pytest.mark.parametrize('Q', MANY)
def test_new_cells_beside_a_workgroup_of_256(Q):
    check(*many_inputs(Q))


@pytest.mark.gpu
def test_slabs_inside_a_block_and_longer_than_a_workgroup():
    new, a, labels, par, FN, FP, alpha = many_inputs(Q_SLABS)
    post = _lib.Posterior(a)
    try:
        want = post.place(new, labels, par, FN, FP, alpha, matrix=True)
        compare(want, new, a, labels, par, FN, FP, alpha)
        for slab in SLABS:
            for chunk in (0, 2):
                equal(post.place(new, labels, par, FN, FP, alpha, chunk=chunk,
                    slab=slab, matrix=True), want)
    finally:
        post.close()


# ---------------------------------------------------------------------------
# C: the wrapped grids
# ---------------------------------------------------------------------------
TEMPLATES = (2, 1, 3, 1, 2, 2, 1)       # clusters of the seven templates
WRAP_CHUNK = 16384


def wrap_inputs():
    """S = 65538 samples, sample s the template s % 7: N = 6, W = 3, M = 2,
    Q = 3, K = 2"""
    rng = np.random.RandomState(S_WRAP)
    N, W, M, Q, K = 6, 3, 2, 3, 2
    a, par, FN, FP, alpha = samples(rng, len(TEMPLATES), N, W, M,
        clusters=TEMPLATES, in_range=True)
    which = np.arange(S_WRAP) % len(TEMPLATES)
    return (new_cells(rng, Q, M), a[which], clustering(rng, N, K), par[which],
        FN[which], FP[which], alpha[which])


def test_wrap_inputs_are_one_chunk_past_every_grid():
    new, a, labels, par, FN, FP, alpha = wrap_inputs()
    S, N = a.shape
    W, M, Q = par.shape[1], par.shape[2], new.shape[0]
    assert (S, N, W, M, Q) == (S_WRAP, 6, 3, 2, 3) and labels.max() == 1
    # one chunk: what 512 MiB hold, and the cap, are both past S
    per_sample = W * M * 4 + (W + 1) * M * 16
    assert per_sample == 152 and (512 << 20) // per_sample > S
    assert default_chunk(0, per_sample, S) == S and (1 << 24) // (W + 1) > S
    chunks, slabs, pitch = plan(a, M, W, Q)
    assert len(chunks) == 1 and len(slabs) == 1
    s0, n, first, cn, tiles = chunks[0]
    assert n == S > GRID_MAX              # k_pn_counts, k_pn_soft, k_cg_rank
    assert tiles * T >= cn > GRID_MAX     # k_pn_tables
    assert 177000 < cn < 179000
    assert cn == sum(TEMPLATES) * (S // 7) + sum(TEMPLATES[:S % 7]) + S
    # a workgroup's second sample is another template than its first: another
    # cluster count, other labels, another trace and other rates
    distinct = np.array([np.unique(row).size for row in a])
    for s in range(GRID_MAX, S):
        t = s - GRID_MAX
        assert distinct[s] != distinct[t]
        assert not np.array_equal(a[s], a[t])
        assert FN[s] != FN[t] and FP[s] != FP[t] and alpha[s] != alpha[t]
    # a slot's second trip of k_pn_tables is another (sample, row)
    owner = np.repeat(np.arange(S), distinct + 1)
    row = np.arange(cn) - first[owner]
    back = np.arange(GRID_MAX, cn) - GRID_MAX
    assert (owner[GRID_MAX:] % 7 != owner[back] % 7).any()
    assert (row[GRID_MAX:] != row[back]).any()
    # in chunks of 16384 nothing wraps
    chunks, _, _ = plan(a, M, W, Q, chunk=WRAP_CHUNK)
    assert [c[1] for c in chunks] == [WRAP_CHUNK] * 4 + [2]
    assert all(n < GRID_MAX and tiles * T < GRID_MAX
        for _, n, _, _, tiles in chunks)


@pytest.mark.gpu
def test_wrapped_launches_of_one_chunk_of_65538_samples():
    new, a, labels, par, FN, FP, alpha = wrap_inputs()
    got = check(new, a, labels, par, FN, FP, alpha)
    post = _lib.Posterior(a)
    try:
        equal(post.place(new, labels, par, FN, FP, alpha, chunk=WRAP_CHUNK,
            matrix=True), tuple(got[k] for k in NAMES))
    finally:
        post.close()


# ---------------------------------------------------------------------------
# D: the chunk cap binds
# ---------------------------------------------------------------------------
def cap_inputs():
    """S = 257, W = 65533, M = 1, N = 10, Q = 2, K = 3, sample s with
    1 + s % 3 clusters"""
    rng = np.random.RandomState(65533)
    S, N, W, M, Q, K = 257, 10, 65533, 1, 2, 3
    a, par, FN, FP, alpha = samples(rng, S, N, W, M,
        clusters=[1 + s % 3 for s in range(S)], in_range=True)
    return new_cells(rng, Q, M), a, clustering(rng, N, K), par, FN, FP, alpha


def test_cap_inputs_are_cut_by_the_cap_alone():
    new, a, labels, par, FN, FP, alpha = cap_inputs()
    S, W, M = a.shape[0], par.shape[1], par.shape[2]
    assert (S, W, M) == (257, 65533, 1) and new.shape == (2, 1)
    assert [np.unique(row).size for row in a] == [1 + s % 3 for s in range(S)]
    per_sample = W * M * 4 + (W + 1) * M * 16
    assert default_chunk(0, per_sample, S) == S == 257
    assert (512 << 20) // per_sample > S
    assert max(1, (1 << 24) // (W + 1)) == 256
    chunks, slabs, pitch = plan(a, M, W, 2)
    assert [(s0, n) for s0, n, _, _, _ in chunks] == [(0, 256), (256, 1)]
    assert len(slabs) == 1
    chunks, _, _ = plan(a, M, W, 2, chunk=64)
    assert [n for _, n, _, _, _ in chunks] == [64, 64, 64, 64, 1]


@pytest.mark.gpu
def test_chunks_cut_by_the_candidate_cap():
    new, a, labels, par, FN, FP, alpha = cap_inputs()
    got = check(new, a, labels, par, FN, FP, alpha)
    post = _lib.Posterior(a)
    try:
        equal(post.place(new, labels, par, FN, FP, alpha, chunk=64,
            matrix=True), tuple(got[k] for k in NAMES))
    finally:
        post.close()


# ---------------------------------------------------------------------------
# E: flushing exponentials
# ---------------------------------------------------------------------------
# the samples' rows by pattern (sample 1: sample 0's trace reversed), their
# cells and alpha
FLUSH_ROWS = ((0, 3, 1), None, (4, 1, 3, 2), (3,), (4, 2))
FLUSH_SIZES = ((5, 5, 2), (5, 5, 2), (2, 6, 2, 2), (12,), (2, 10))
FLUSH_ALPHA = (1.5, 1e-250, 0.7, 1e-250, 2.0)


def flush_inputs():
    """M = 400 mutations, FN = FP = 1e-3, parameters 1e-6 or 1 - 1e-6 after
    five random patterns A, B, C, F, G (0 .. 4): an observed entry costs 0.001
    where it agrees with a row and 6.9 where it does not, 0.69 under a new
    cluster.  Two patterns differ in about 200 mutations, 1380 apart, so a
    cell that follows a pattern flushes every other row of a sample.  Sample
    1 has sample 0's trace reversed (1 - theta); there and in sample 3 alpha is
    1e-250, log alpha = -576, so a cell that no row of these samples fits has
    lp = -850, more than 745 below its lp in a sample that has its row.
    New cells: 0, 1, 2 follow A, B, C; 3 follows F with 30% missing; 4 follows
    no pattern; 5 is empty; 6 is A with 50 entries flipped (its row 345 below a
    perfect fit, the new cluster 277: neither flushes); 7 follows G; 8 is A's complement, row 0
    of the reversed sample."""
    rng = np.random.RandomState(745)
    M, N, K = 400, 12, 3
    pat = rng.random_sample((5, M)) < 0.5
    S, W = len(FLUSH_ROWS), 4
    par = np.full((S, W, M), np.nan, dtype=np.float32)
    a = np.empty((S, N), dtype=np.int64)
    for s, sizes in enumerate(FLUSH_SIZES):
        if FLUSH_ROWS[s] is not None:
            par[s, :len(sizes)] = np.where(pat[list(FLUSH_ROWS[s])],
                1 - 1e-6, 1e-6)
        ids = np.sort(rng.choice(N, len(sizes), replace=False))
        a[s] = rng.permutation(np.repeat(ids, sizes))
    par[1, :3] = np.float32(1) - par[0, :3]
    new = np.stack([pat[0], pat[1], pat[2], pat[3], rng.random_sample(M) < 0.5,
        pat[0], pat[0], pat[4], ~pat[0]]).astype(np.float64)
    new[3, rng.random_sample(M) < 0.3] = np.nan
    new[5] = np.nan
    flip = rng.choice(M, 50, replace=False)
    new[6, flip] = 1 - new[6, flip]
    return (new, a, clustering(rng, N, K), par, np.full(S, 1e-3),
        np.full(S, 1e-3), np.array(FLUSH_ALPHA))


def candidates(red, s, j, D):
    """y_c of new cell j in sample s, in candidate order"""
    y = red['y'][s, j]
    return np.append(y[:D], y[-1])


def flush_facts(y_of, lp):
    """the facts the group is about, of the y (a function (s, j) -> the
    candidates' y_c) and lp (S, Q) of either side"""
    D = [len(sizes) for sizes in FLUSH_SIZES]
    # the maximum at the first row, an inner row, the last row and the new
    # cluster, every other row more than 745 below: e_c = 0 exactly
    for (s, j), where in (((0, 0), 0), ((2, 1), 1), ((0, 1), 2), ((2, 2), 3),
            ((2, 3), 2), ((3, 3), 0), ((1, 8), 0), ((0, 2), D[0]),
            ((2, 0), D[2]), ((4, 0), D[4]), ((4, 4), D[4])):
        y = y_of(s, j)
        assert y.size == D[s] + 1 and y.argmax() == where, (s, j)
        d = y - y.max()
        rest = np.delete(d[:D[s]], where) if where < D[s] else d[:D[s]]
        assert (rest < -FLUSH).all() and not np.exp(rest).any(), (s, j)
        # (the new cluster beside a fitting row: small, not flushed)
        if where < D[s] and FLUSH_ALPHA[s] > 1e-200:
            assert -FLUSH + 300 < d[-1] < -100 and np.exp(d[-1]) > 0
    assert 0 < 1 < D[2] - 1             # ((2, 1), 1) is an inner row
    # no flush where the rows are close: cell 6 in sample 0
    d = y_of(0, 6) - y_of(0, 6).max()
    assert d.argmax() == D[0] and -100 < d[0] < -40 and np.exp(d[0]) > 0
    # lp: the column's maximum at the first, an inner and the last sample,
    # samples more than 745 below it
    S = lp.shape[0]
    for j, where in ((0, 0), (1, 2), (2, S - 1), (8, 1)):
        col = lp[:, j]
        assert col.argmax() == where and (col == col.max()).sum() == 1
        low = col - col.max() < -FLUSH
        assert low.any() and not np.exp(col[low] - col.max()).any()
        assert (np.exp(col[~low] - col.max()) > 0).all()
    assert lp[1, 0] - lp[0, 0] < -FLUSH and lp[3, 0] - lp[0, 0] < -FLUSH
    assert lp[1, 2] - lp[4, 2] < -FLUSH and lp[0, 8] - lp[1, 8] > -FLUSH
    # the empty row is at the prior
    assert np.abs(lp[:, 5]).max() < 1e-13


def test_flush_inputs_flush_and_keep_a_new_cluster_alive():
    new, a, labels, par, FN, FP, alpha = flush_inputs()
    assert new.shape == (9, 400) and np.isnan(new[5]).all()
    assert (np.isnan(new).sum(axis=1)[[0, 1, 2, 4, 6, 7, 8]] == 0).all()
    assert [np.bincount(r).tolist() for r in ranks(a)] \
        == [list(sizes) for sizes in FLUSH_SIZES]
    assert np.array_equal(par[1, :3], np.float32(1) - par[0, :3])
    assert set(np.unique(par[~np.isnan(par)]).tolist()) \
        == {float(np.float32(x)) for x in (1e-6, 1 - 1e-6,
            np.float32(1) - np.float32(1e-6), np.float32(1)
            - np.float32(1 - 1e-6))}
    red = postproc.host_place(new, a, labels, par, FN, FP, alpha, PRIOR)
    D = [len(sizes) for sizes in FLUSH_SIZES]
    flush_facts(lambda s, j: candidates(red, s, j, D[s]), red['lp'])
    # every cell keeps a new cluster that is not flushed in some sample, and
    # in the host's sums
    alive = np.zeros(new.shape[0], dtype=bool)
    for s in range(a.shape[0]):
        for j in range(new.shape[0]):
            y = candidates(red, s, j, D[s])
            alive[j] |= np.exp(y[-1] - y.max()) > 0
    assert alive.all() and (red['new_sum'] > 0).all()
    # a share times a probability of 0: flushed rows with cells of more than
    # one cluster of the clustering
    rank = ranks(a)[0]
    assert all(np.unique(labels[rank == r]).size > 1 for r in (0, 1))
    for name in ('prob_sum', 'new_sum', 'ent_sum', 'lpd', 'lp'):
        assert np.isfinite(red[name]).all(), name


@pytest.mark.gpu
def test_exponentials_that_flush_to_zero():
    new, a, labels, par, FN, FP, alpha = flush_inputs()
    got = check(new, a, labels, par, FN, FP, alpha)
    # the device's own scores and lp have the shape the inputs were made for
    dev = postproc.place_reduce(got['scores'], a, labels, 3, alpha, keep=True)
    D = [len(sizes) for sizes in FLUSH_SIZES]
    flush_facts(lambda s, j: candidates(dev, s, j, D[s]), got['lp'])
    post = _lib.Posterior(a)
    try:
        equal(post.place(new, labels, par, FN, FP, alpha, chunk=2, slab=4,
            matrix=True), tuple(got[k] for k in NAMES))
    finally:
        post.close()
