"""The per-cell genotype pass on the device (bnpc_post_cell_genotypes, through
_lib.Posterior.cell_genotypes) against the host loop it is pinned to
(postproc.host_cell_genotypes): array_equal on all three tables, no
tolerance.

The kernel's tiles: a workgroup takes _lib.CELL_TILE = 8 cells and 256
mutations, so the cell counts 63 / 64 / 65 / 129 sit on and beside multiples
of 8 (7 / 8 / 9 are added) and the mutation counts 255 / 256 / 257 beside the
one edge along the mutations."""
import contextlib
import io
import os

import numpy as np
import pytest

from bnpc_amd import _lib, postproc
from bnpc_amd import io as bio

TABLES = ('sum1', 'sum2', 'ones')


def trace(rng, S, W, M):
    """float32 draws in (0, 1); some entries exactly 0.5, 0, denormal-small
    and just beside 0.5"""
    p = rng.random_sample((S, W, M)).astype(np.float32)
    p[p == 0] = 0.25
    kind = rng.randint(0, 12, p.shape)
    p[kind == 0] = 0.5
    p[kind == 1] = 0.0
    p[kind == 2] = 1e-42                    # a float32 denormal
    p[kind == 3] = np.nextafter(np.float32(0.5), np.float32(1))
    p[kind == 4] = np.nextafter(np.float32(0.5), np.float32(0))
    p[kind == 5] = 1e-30                    # its square is a float32 denormal
    return p


def samples(rng, S, N, nlab, spread=True):
    """a few labels per sample, on a random subset of [0, N)"""
    a = rng.randint(0, nlab, (S, N))
    if spread and N > nlab:
        a = np.sort(rng.choice(N, nlab, replace=False))[a]
    return a.astype(np.int64)


def width(a):
    return max(np.unique(row).size for row in a)


def equal(got, want):
    for name, g, w in zip(TABLES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5])


def check(a, params, **how):
    want = postproc.host_cell_genotypes(a, params)
    post = _lib.Posterior(a)
    try:
        got = post.cell_genotypes(params, **how)
    finally:
        post.close()
    equal(got, want)
    return want


@pytest.mark.gpu
def test_one_sample_two_cells_one_mutation():
    for a in ([[0, 1]], [[1, 0]], [[1, 1]], [[0, 0]]):
        a = np.array(a)
        for x in (0.5, 0.75, 0.0, 1e-42):
            params = np.array([[[x], [0.625]]], dtype=np.float32)
            want = check(a, params)
            assert want[2].max() <= 1


@pytest.mark.gpu
@pytest.mark.parametrize('M', [1, 255, 256, 257])
@pytest.mark.parametrize('N', [7, 8, 9, 63, 64, 65, 129])
def test_edges_of_the_tiling(N, M):
    rng = np.random.RandomState(1000 * N + M)
    a = samples(rng, 7, N, min(5, N))
    check(a, trace(rng, 7, width(a), M))


@pytest.mark.gpu
def test_singletons_labels_up_to_n_minus_1_and_one_cluster():
    rng = np.random.RandomState(3)
    S, N, M = 9, 77, 70
    a = samples(rng, S, N, 6)
    a[2] = rng.permutation(N)               # W = N: every cell alone
    a[5] = np.arange(N)[::-1]
    a[6] = N - 1                            # one cluster, the largest label
    a[7] = 0
    assert a.max() == N - 1 and width(a) == N
    check(a, trace(rng, S, N, M))


@pytest.mark.gpu
def test_chunks_give_the_same_bits():
    rng = np.random.RandomState(4)
    S, N, M = 37, 50, 40
    a = samples(rng, S, N, 7)
    params = trace(rng, S, width(a), M)
    want = check(a, params)
    post = _lib.Posterior(a)
    try:
        for chunk in (1, 5, 37, 64):
            equal(post.cell_genotypes(params, chunk=chunk), want)
    finally:
        post.close()


@pytest.mark.gpu
def test_slabs_give_the_same_bits():
    rng = np.random.RandomState(5)
    S, N, M = 11, 101, 33
    a = samples(rng, S, N, 9)
    params = trace(rng, S, width(a), M)
    want = postproc.host_cell_genotypes(a, params)
    post = _lib.Posterior(a)
    try:
        for slab in (1, 64, 100, 101, 0):
            equal(post.cell_genotypes(params, slab=slab), want)
        equal(post.cell_genotypes(params, chunk=4, slab=30), want)
    finally:
        post.close()


@pytest.mark.gpu
def test_past_the_lds_threshold_of_the_rank_pass():
    """One cell more than the rank pass keeps in LDS: its bitmap and prefix
    counts go to a slice of global memory per workgroup."""
    rng = np.random.RandomState(6)
    S, N, M = 2, _lib.CELL_RANK_LDS_CELLS + 1, 3
    a = samples(rng, S, N, 40)
    a[1, -1] = N - 1                        # the last bit of the bitmap
    check(a, trace(rng, S, width(a), M))


@pytest.mark.gpu
def test_float64_trace_with_padding_rows():
    rng = np.random.RandomState(7)
    S, N, M = 20, 64, 16
    a = samples(rng, S, N, 6)
    params = trace(rng, S, width(a), M)
    want = check(a, params)
    wide = np.pad(params.astype(np.float64), [(0, 0), (0, 3), (0, 0)])
    assert wide.dtype == np.float64 and wide.shape[1] == width(a) + 3
    assert np.array_equal(check(a, wide)[0], want[0])


@pytest.mark.gpu
def test_one_table_at_a_time():
    rng = np.random.RandomState(8)
    S, N, M = 6, 30, 20
    a = samples(rng, S, N, 4)
    params = trace(rng, S, width(a), M)
    post = _lib.Posterior(a)
    try:
        full = post.cell_genotypes(params)
        for k in range(3):
            want = tuple(j == k for j in range(3))
            got = post.cell_genotypes(params, want=want)
            assert [g is None for g in got] == [not w for w in want]
            assert got[k].dtype == full[k].dtype
            assert np.array_equal(got[k], full[k]), TABLES[k]
    finally:
        post.close()
    equal(full, postproc.host_cell_genotypes(a, params))


@pytest.mark.gpu
def test_bad_input_is_an_error_and_the_handle_lives():
    rng = np.random.RandomState(9)
    S, N, M = 4, 12, 5
    a = samples(rng, S, N, 3)
    a[3, :4] = [0, 1, 2, 3]                 # sample 3 has >= 4 clusters
    W = width(a)
    params = trace(rng, S, W, M)
    want = postproc.host_cell_genotypes(a, params)
    post = _lib.Posterior(a)
    try:
        with pytest.raises(ValueError, match='samples'):    # the wrong S
            post.cell_genotypes(params[:3])
        equal(post.cell_genotypes(params), want)
        with pytest.raises(RuntimeError, match='code 2'):   # row W - 1 of W - 1
            post.cell_genotypes(params[:, :W - 1])
        equal(post.cell_genotypes(params), want)
        with pytest.raises(RuntimeError, match='code 2'):
            post.cell_genotypes(params, chunk=-1)
        equal(post.cell_genotypes(params), want)
    finally:
        post.close()
    bad = a.copy()
    bad[1, 5] = N                           # a label >= N
    post = _lib.Posterior(bad)
    try:
        with pytest.raises(RuntimeError, match='code 2'):
            post.cell_genotypes(params)
        with pytest.raises(RuntimeError, match='code 2'):
            post.cell_genotypes(params)
        assert post.differ().shape == (N * (N - 1) // 2,)
    finally:
        post.close()


@pytest.mark.gpu
def test_posterior_estimate_with_cells(golden_dir, tmp_path):
    from test_outputs import load_case
    d, case, results = load_case(golden_dir, 'fixture', tmp_path / 'ref')
    assert len(results) == 2
    data = bio.load_data(os.path.join(d, 'input.tsv'))
    plain = postproc.posterior_estimate(results, data, cells=False)
    assert 'cell_genotypes' not in plain
    inf = postproc.posterior_estimate(results, data, cells=True)
    assert sorted(set(inf) - set(plain)) == ['cell_genotypes']
    for key in plain:
        assert np.array_equal(inf[key], plain[key]), key
    pooled = postproc.concat_chain_results(results)
    sum1, sum2, ones = postproc.host_cell_genotypes(pooled['assignments'],
        pooled['params'])
    S = pooled['assignments'].shape[0]
    mean = sum1 / S
    got = inf['cell_genotypes']
    assert sorted(got) == ['mean', 'prob', 'sd']
    assert np.array_equal(got['mean'], mean)
    assert np.array_equal(got['sd'],
        np.sqrt(np.maximum(sum2 / S - mean * mean, 0)))
    assert np.array_equal(got['prob'], ones / S)


@pytest.mark.gpu
def test_cli_writes_the_cell_tables(golden_dir, tmp_path):
    import run_BnpC
    src = os.path.join(golden_dir, 'example_data.csv')
    data = bio.load_data(src)
    N, M = data.shape
    # (--debug: the chain runs in this process, as in the other CLI tests)
    base = [src, '-n', '1', '-s', '200', '--seed', '42', '-np', '-v', '0',
        '--debug']
    with_pg, without = tmp_path / 'with', tmp_path / 'without'
    with contextlib.redirect_stdout(io.StringIO()):
        results = run_BnpC.main(run_BnpC.parse_args(base + ['-pg', '-o',
            str(with_pg)]))
        run_BnpC.main(run_BnpC.parse_args(base + ['-o', str(without)]))
    new = {f'genotypes_cell_{kind}_posterior_mean.tsv'
        for kind in ('prob', 'cont', 'sd')}
    assert new <= set(os.listdir(with_pg))
    assert set(os.listdir(without)) == set(os.listdir(with_pg)) - new
    for name in os.listdir(without):
        if name != 'args.txt':
            assert (without / name).read_bytes() \
                == (with_pg / name).read_bytes(), name
    pooled = postproc.concat_chain_results(results)
    S = pooled['assignments'].shape[0]
    ones = postproc.host_cell_genotypes(pooled['assignments'],
        pooled['params'])[2]
    tables = {}
    for name in new:
        rows = [ln.split('\t') for ln in
            (with_pg / name).read_text().splitlines()]
        assert len(rows) == M + 1 and all(len(r) == N + 1 for r in rows), name
        tables[name.split('_')[2]] = [r[1:] for r in rows[1:]]
    want = [[f'{x:.4f}' for x in row] for row in (ones / S).T.tolist()]
    assert tables['prob'] == want
    assert 'posterior_genotypes: True\n' in (with_pg / 'args.txt').read_text()
    assert 'posterior_genotypes' not in (without / 'args.txt').read_text()
