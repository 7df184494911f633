"""The device pass behind -po (bnpc_post_mutation_order) against the host loop
it is pinned to, postproc.host_mutation_order: exact integers, so every
comparison is np.array_equal.  Which route of the driver a case takes is
worked out on the CPU by plan(), the driver's arithmetic restated from
bnpc_post_passes.hip (po_run) with the constants _lib exports, and asserted
before the case runs.  Every counter of the pass is 32 bits wide (the packed
any-bits of a multi-word sample are flags, not counters), so no case has a
narrower width to cross."""
import contextlib
import io
import os

import numpy as np
import pytest

from bnpc_amd import _lib, postproc
from bnpc_amd import io as bio

pytestmark = pytest.mark.gpu

TABLES = ('anc', 'same', 'excl', 'conf')
TILE, STAGE = _lib.ORDER_TILE, _lib.ORDER_STAGE
LDS_ROWS, WG = _lib.ORDER_LDS_ROWS, _lib.ORDER_WG


def plan(S, N, W, M, chunk=0, slab=0):
    """po_run's decisions (with device memory to spare)"""
    ww = -(-W // 64)
    per_sample = W * M * 4 + ww * M * 8 + N * 2 + ww * 8
    sc = chunk or max(1, (512 << 20) // per_sample)
    sc = min(sc, S, max(1, (1 << 30) // ww))
    na = min(slab, M) if slab else M
    units = sc * ww
    return {'ww': ww, 'one_word': ww == 1, 'chunks': -(-S // sc),
        'slabs': -(-M // na), 'sym': na >= M, 'sizes_in_lds': W <= LDS_ROWS,
        'live_wraps': sc > WG, 'mask_rows_wrap': units > WG,
        'stages': -(-units // STAGE), 'stage_tail': units % STAGE,
        'tiles': -(-M // TILE), 'slab_cuts_a_tile': na < M and na % TILE != 0}


def clustered(rng, S, N, D):
    """S samples of N >= D + 3 cells with exactly D clusters each (any integer
    labels below N): where D > 3 the sizes 1, 2, 3 are among them, the other
    clusters share the remaining cells"""
    out = np.empty((S, N), dtype=np.int64)
    for s in range(S):
        names = rng.choice(N, D, replace=False)
        lab = list(range(D)) + [1] * (D > 1) + [2, 2] * (D > 2)
        rest = N - len(lab)
        assert rest >= 0
        lab += rng.randint(3, D, rest).tolist() if D > 3 else [D - 1] * rest
        out[s] = names[rng.permutation(lab)]
        assert np.unique(out[s]).size == D
    return out


def trace(rng, S, W, M, D=None, pad=0.9):
    """A float32 trace whose columns are carried at very different rates (so
    that every relation occurs), column 1 a copy of column 0; rows >= D hold
    `pad`"""
    rate = rng.choice([0.0, 0.03, 0.1, 0.3, 0.6, 1.0], M)
    p = np.where(rng.rand(S, W, M) < rate, 0.5 + rng.rand(S, W, M) / 2,
        rng.rand(S, W, M) / 2).astype(np.float32)
    if M > 1:
        p[:, :, 1] = p[:, :, 0]
    if D is not None:
        p[:, D:] = pad
    return p


def same_tables(got, want):
    for key, g, w in zip(TABLES, got, want):
        assert g.dtype == np.uint32 and g.shape == w.shape, key
        assert np.array_equal(g, w), key


@contextlib.contextmanager
def handle(a):
    post = _lib.Posterior(a)
    try:
        yield post
    finally:
        post.close()


@pytest.mark.parametrize('D', [1, 2, 63, 64, 65, 129])
def test_mask_word_edges(D):
    rng = np.random.RandomState(100 + D)
    S, N = 6, max(2 * D + 3, 8)
    assert N <= 300
    a = clustered(rng, S, N, D)
    seen = np.zeros(4, dtype=np.int64)
    with handle(a) as post:
        for M in (1, 2, 63, 64, 65, 129):
            for W in (D, D + 1, D + 64):
                p = plan(S, N, W, M)
                assert p['one_word'] == (W <= 64) and p['sym']
                assert p['tiles'] == -(-M // 64)
                params = trace(rng, S, W, M, D)
                want = postproc.host_mutation_order(a, params, 2)
                same_tables(post.mutation_order(params), want)
                seen += [int(t.astype(np.int64).sum()) for t in want]
                # NaN in the padding is not read either
                if W > D:
                    params[:, D:] = np.nan
                    same_tables(post.mutation_order(params), want)
    if D > 2:       # (two live clusters at the least)
        assert seen.all()               # every table counted something


def test_min_cells():
    rng = np.random.RandomState(2)
    S, N, D, M = 9, 30, 7, 20
    a = clustered(rng, S, N, D)
    a[0] = 4                            # one cluster of all N cells
    sizes = set(np.unique(a[1], return_counts=True)[1].tolist())
    assert {1, 2, 3} <= sizes
    params = trace(rng, S, D, M)
    with handle(a) as post:
        last = None
        for min_cells in (1, 2, 3, N, N + 1):
            want = postproc.host_mutation_order(a, params, min_cells)
            same_tables(post.mutation_order(params, min_cells), want)
            if last is not None:
                assert any(not np.array_equal(x, y)
                    for x, y in zip(want, last))
            last = want
        assert not any(t.any() for t in last)       # N + 1: nothing is live
        want = postproc.host_mutation_order(a, params, N)
        assert want[1].max() == 1       # the one sample of one cluster


def test_special_parameter_values():
    rng = np.random.RandomState(3)
    half = np.float32(0.5)
    special = np.array([half, np.nextafter(half, np.float32(1)),
        np.nextafter(half, np.float32(-1)), np.nan, -0.0, 0.0, 1.0, np.inf,
        -np.inf, 1e-45, -np.nan, 0.9, 0.1], dtype=np.float32)
    S, N, D, M = 8, 24, 5, 40
    a = clustered(rng, S, N, D)
    params = special[rng.randint(0, special.size, (S, D + 2, M))]
    params[:, D:] = 0.9
    want = postproc.host_mutation_order(a, params, 1)
    assert all(t.any() for t in want)
    with handle(a) as post:
        same_tables(post.mutation_order(params, 1), want)
        same_tables(post.mutation_order(params, 2),
            postproc.host_mutation_order(a, params, 2))


@pytest.mark.parametrize('W', [5, 70])
def test_any_chunk_and_slab_the_same_bits(W):
    rng = np.random.RandomState(4 + W)
    S, N, M = 7, 40, 130
    D = min(W, 18)
    a = clustered(rng, S, N, D)
    params = trace(rng, S, W, M, D)
    want = postproc.host_mutation_order(a, params, 2)
    assert all(t.any() for t in want)
    routes = set()
    with handle(a) as post:
        for chunk in (1, 2, S - 1, S, 0):
            for slab in (1, 63, 64, 65, M, 0):
                p = plan(S, N, W, M, chunk, slab)
                assert p['tiles'] == 3 and p['one_word'] == (W == 5)
                assert p['sym'] == (slab in (M, 0))
                assert p['slab_cuts_a_tile'] == (slab in (1, 63, 65))
                assert p['chunks'] == {1: 7, 2: 4, S - 1: 2, S: 1, 0: 1}[chunk]
                routes.add((p['sym'], p['chunks'] > 1, p['slabs'] > 1))
                same_tables(post.mutation_order(params, 2, chunk, slab), want)
        # and again: the same bits on every call
        same_tables(post.mutation_order(params, 2, 2, 65), want)
        same_tables(post.mutation_order(params), want)
    assert routes == {(True, False, False), (True, True, False),
        (False, False, True), (False, True, True)}


@pytest.mark.parametrize('W, M', [(2, 3), (65, 3), (LDS_ROWS + 1, 2)])
def test_samples_past_the_first_workgroups(W, M):
    """More samples than k_po_live has workgroups and k_po_masks launch rows,
    with the sizes in LDS (one word, two words) and in global slices."""
    rng = np.random.RandomState(5)
    S, N, D = WG + 7, 6, 2
    p = plan(S, N, W, M)
    assert p['chunks'] == 1 and p['live_wraps'] and p['mask_rows_wrap']
    assert p['sizes_in_lds'] == (W <= LDS_ROWS)
    assert p['one_word'] == (W == 2)
    assert p['stages'] > 1 and p['stage_tail'] != 0
    a = clustered(rng, S, N, D)
    params = np.full((S, W, M), 0.9, dtype=np.float32)
    params[:, :D] = trace(rng, S, D, M)
    # the late samples alone decide some entries
    params[WG:, :D, 0] = 0.9
    params[:WG, :D, 0] = 0.1
    want = postproc.host_mutation_order(a, params, 1)
    assert want[1][0, 0] == 7
    with handle(a) as post:
        same_tables(post.mutation_order(params, 1), want)
        if W == 2:
            # a chunk that ends inside a stage, and a last chunk of one
            assert plan(S, N, W, M, 515)['chunks'] == 3
            same_tables(post.mutation_order(params, 1, 515, 2), want)


def test_clusters_in_global_slices():
    """The sizes in global slices with live rows in every word of a few"""
    rng = np.random.RandomState(6)
    S, N, D, M, W = 5, 300, 290, 9, LDS_ROWS + 70
    assert not plan(S, N, W, M)['sizes_in_lds']
    a = clustered(rng, S, N, D)
    params = trace(rng, S, W, M, D)
    with handle(a) as post:
        for min_cells in (1, 2):
            want = postproc.host_mutation_order(a, params, min_cells)
            assert want[1].any()
            same_tables(post.mutation_order(params, min_cells), want)


def test_null_outputs_and_times():
    rng = np.random.RandomState(7)
    S, N, D, M = 6, 20, 4, 70
    a = clustered(rng, S, N, D)
    params = trace(rng, S, D, M)
    want = postproc.host_mutation_order(a, params, 2)
    with handle(a) as post:
        for pick in ((True, False, False, False), (False, True, False, True),
                (False, False, False, False), (False, False, True, False)):
            for slab in (0, 33):
                got = post.mutation_order(params, 2, 0, slab, want=pick)
                for p, g, w in zip(pick, got, want):
                    assert (g is None) == (not p)
                    assert g is None or np.array_equal(g, w)
        times = post.mutation_order_times(params, 2)
        assert len(times) == 4 and all(t >= 0 for t in times)
        assert times[3] > 0
        lib = _lib.load()
        assert lib.bnpc_post_mutation_order_times(post._h, _lib.ptr(params),
            D, M, 2, 0, 0, None) == 2


def test_bad_arguments_leave_the_handle_working():
    rng = np.random.RandomState(8)
    S, N, D, M = 5, 16, 4, 6
    a = clustered(rng, S, N, D)
    params = trace(rng, S, D, M)
    want = postproc.host_mutation_order(a, params, 2)
    lib = _lib.load()
    with handle(a) as post:
        for kw, shape in (({'min_cells': 0}, None), ({'min_cells': -1}, None),
                ({'chunk': -1}, None), ({'slab': -1}, None),
                ({}, (S, D - 1, M)),        # a sample has more clusters
                ({}, (S, 65534, 1)), ({}, (S, D, 0))):
            par = params if shape is None else np.zeros(shape, np.float32)
            with pytest.raises(RuntimeError, match=r'\(code 2\)'):
                post.mutation_order(par, **kw)
        # nothing is written
        out = [np.full((M, M), 77, dtype=np.uint32) for _ in range(4)]
        assert lib.bnpc_post_mutation_order(post._h, _lib.ptr(params), D, M, 0,
            0, 0, *[_lib.ptr(o) for o in out]) == 2
        assert lib.bnpc_post_mutation_order(post._h, _lib.ptr(params), D - 1,
            M, 2, 0, 0, *[_lib.ptr(o) for o in out]) == 2
        assert all((o == 77).all() for o in out)
        same_tables(post.mutation_order(params), want)
    # labels that index no cell
    with handle(a + N) as post:
        with pytest.raises(RuntimeError, match=r'\(code 2\)'):
            post.mutation_order(params)


def fake_results(rng, n, burn, N, M=6):
    return [{'assignments': rng.randint(0, 3, (n, N)), 'burn_in': burn,
        'params': rng.rand(n - burn, 3, M).astype(np.float32),
        'DP_alpha': rng.rand(n), 'ML': rng.rand(n), 'MAP': rng.rand(n),
        'FN': rng.rand(n) * 0.2 + 0.05, 'FP': rng.rand(n) * 0.01 + 0.001}]


def test_posterior_estimate_on_a_real_handle():
    rng = np.random.RandomState(9)
    results = fake_results(rng, 30, 10, 12)
    data = rng.randint(0, 2, (12, 6)).astype(float)
    plain = postproc.posterior_estimate(results, data)
    inf = postproc.posterior_estimate(results, data, ordering=2)
    assert sorted(set(inf) - set(plain)) == ['mutation_order']
    for key in plain:
        assert np.array_equal(inf[key], plain[key]), key
    pooled = postproc.concat_chain_results(results)
    want = postproc.mutation_order(None, pooled['assignments'],
        pooled['params'], 2)
    for key in want:
        if key != 'total':
            assert np.array_equal(inf['mutation_order'][key], want[key]), key
    assert inf['mutation_order']['total'] == want['total']


def test_cli_writes_the_three_files(tmp_path):
    import run_BnpC
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
        'example_data.csv')
    out = tmp_path / 'with'
    with contextlib.redirect_stdout(io.StringIO()):
        results = run_BnpC.main(run_BnpC.parse_args([src, '-n', '1', '-s',
            '120', '--seed', '42', '-np', '-v', '0', '--debug', '-po', '-o',
            str(out)]))
    names = bio.load_data(src, get_names=True)[1]
    pooled = postproc.concat_chain_results(results)
    want = postproc.mutation_order(None, pooled['assignments'],
        pooled['params'], 2)
    ref = tmp_path / 'ref'
    ref.mkdir()
    paths = bio.save_mutation_order(str(ref), 'mean', 'posterior', want,
        names[1])
    assert len(paths) == 3
    for path in paths:
        name = os.path.basename(path)
        assert (out / name).read_bytes() == (ref / name).read_bytes(), name
    assert 'posterior_order: 2\n' in (out / 'args.txt').read_text()
