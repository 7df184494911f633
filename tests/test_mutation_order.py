"""The posterior ordering of every pair of mutations (-po) on the CPU: the host
loop the device pass is pinned to against an independent per-cell form and
against hand-made traces, the derived tables (forest, ties, a majority cycle),
the writer and the flag.  The device pass itself: test_mutation_order_gpu.py.
The command line runs on the NumPy stand-ins of tests/fake_device.py."""
import os
import re

import numpy as np
import pytest

import run_BnpC
from bnpc_amd import _lib, postproc
from bnpc_amd import io as bio
from fake_device import FakeContext, FakePosterior

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, 'tests', 'golden', 'example_data.csv')
NEW_FILES = ('mutation_order_posterior_mean.tsv',
    'mutation_order_summary_posterior_mean.txt',
    'mutation_pairs_posterior_mean.tsv')
TABLES = ('anc', 'same', 'excl', 'conf')


def per_cell_tables(a, params, min_cells):
    """The definition restated per cell: drop the cells of clusters below
    min_cells, G = the called genotype of every remaining cell, relations
    from the cell counts n11 = G'G, n10 = G'(1 - G) being above 0."""
    S, N = a.shape
    M = params.shape[2]
    out = {k: np.zeros((M, M), dtype=np.uint32) for k in TABLES}
    seen = set()
    for s in range(S):
        labels, rank, sizes = np.unique(a[s], return_inverse=True,
            return_counts=True)
        keep = sizes[rank.ravel()] >= min_cells
        G = np.zeros((int(keep.sum()), M), dtype=np.int64)
        for row, i in enumerate(np.flatnonzero(keep)):
            for m in range(M):
                G[row, m] = params[s, rank.ravel()[i], m] > np.float32(0.5)
        n11 = G.T @ G
        n10 = G.T @ (1 - G)
        for x in range(M):
            for y in range(M):
                bits = (n11[x, y] > 0, n10[x, y] > 0, n10[y, x] > 0)
                kind = {(True, False, False): 'same',
                    (True, True, False): 'anc', (True, False, True): 'desc',
                    (False, True, True): 'excl',
                    (True, True, True): 'conf'}.get(bits, 'absent')
                seen.add(kind)
                if kind == 'desc':
                    continue            # counted at (y, x) as anc
                if kind != 'absent':
                    out[kind][x, y] += 1
    return out, seen


@pytest.mark.parametrize('min_cells', [1, 2, 3])
def test_host_loop_against_the_per_cell_form(min_cells):
    rng = np.random.RandomState(11)
    S, N, M, W = 30, 40, 13, 12
    a = np.stack([rng.randint(0, rng.randint(1, W + 1), N) * 3 + 1
        for _ in range(S)])
    params = rng.rand(S, W, M).astype(np.float32)
    params[:, :, 0] = 0.1           # never carried: absent
    params[:, :, 1] = params[:, :, 2]           # the same branch
    want, seen = per_cell_tables(a, params, min_cells)
    assert seen == {'same', 'anc', 'desc', 'excl', 'conf', 'absent'}
    got = postproc.host_mutation_order(a, params, min_cells)
    for key, table in zip(TABLES, got):
        assert table.dtype == np.uint32 and table.shape == (M, M)
        assert np.array_equal(table, want[key]), key
    anc, same, excl, conf = got
    for t in (same, excl, conf):
        assert np.array_equal(t, t.T)
    assert not np.diag(anc).any() and not np.diag(excl).any() \
        and not np.diag(conf).any()
    assert same[0, 0] == 0 and np.array_equal(same[1], same[2])


def one_sample(rows, sizes, W=None, pad=0.9):
    """A one-sample posterior: cluster r has sizes[r] cells and the parameter
    row rows[r]; the trace is padded to W rows with `pad`."""
    rows = np.asarray(rows, dtype=np.float32)
    a = np.repeat(np.arange(len(sizes)) * 2 + 5, sizes)[None, :]
    W = W or rows.shape[0]
    params = np.full((1, W, rows.shape[1]), pad, dtype=np.float32)
    params[0, :rows.shape[0]] = rows
    return a, params


def relation(a, params, min_cells, x, y):
    got = postproc.host_mutation_order(a, params, min_cells)
    hit = [k for k, t in zip(TABLES, got) if t[x, y]]
    hit += ['desc'] if got[0][y, x] else []
    assert len(hit) <= 1
    return hit[0] if hit else 'absent'


def test_hand_made_relations():
    hi, lo = 0.8, 0.2
    # a chain a > b > c, then d on a branch of its own, e the same as b
    #        a   b   c   d   e
    rows = [[hi, hi, hi, lo, hi],
            [hi, hi, lo, lo, hi],
            [hi, lo, lo, hi, lo],
            [hi, lo, lo, lo, lo]]
    a, params = one_sample(rows, [2, 2, 2, 2], W=7)
    for x, y, want in ((0, 1, 'anc'), (1, 2, 'anc'), (0, 2, 'anc'),
            (1, 0, 'desc'), (0, 3, 'anc'), (1, 3, 'excl'), (2, 3, 'excl'),
            (1, 4, 'same'), (4, 2, 'anc'), (3, 3, 'same')):
        assert relation(a, params, 2, x, y) == want, (x, y)
    # the padding rows (0.9 everywhere) are never read: no conflict anywhere
    assert not postproc.host_mutation_order(a, params, 2)[3].any()
    # a planted conflict: 11, 10 and 01 all occur
    a, params = one_sample([[hi, hi], [hi, lo], [lo, hi]], [2, 2, 2])
    assert relation(a, params, 2, 0, 1) == 'conf'
    # ... unless the 01 cluster is below min_cells: it would change the answer
    a, params = one_sample([[hi, hi], [hi, lo], [lo, hi]], [3, 3, 2])
    assert relation(a, params, 3, 0, 1) == 'anc'
    assert relation(a, params, 2, 0, 1) == 'conf'
    a, params = one_sample([[hi, hi], [hi, lo], [lo, hi]], [1, 1, 1])
    assert relation(a, params, 1, 0, 1) == 'conf'
    assert relation(a, params, 2, 0, 1) == 'absent'
    with pytest.raises(ValueError):
        postproc.host_mutation_order(a, params, 0)


def test_the_calling_rule_at_its_edge():
    half = np.float32(0.5)
    above = np.nextafter(half, np.float32(1))
    below = np.nextafter(half, np.float32(-1))
    assert below < half < above
    #        0.5  above below NaN  carried
    rows = [[half, above, below, np.nan, 0.9],
            [0.1, 0.1, 0.1, 0.1, 0.9]]
    a, params = one_sample(rows, [2, 2])
    assert params.dtype == np.float32
    anc, same, excl, conf = postproc.host_mutation_order(a, params, 2)
    assert np.diag(same).tolist() == [0, 1, 0, 0, 1]
    assert anc[4].tolist() == [0, 1, 0, 0, 0] and not anc[:4].any()
    assert not excl.any() and not conf.any()
    # float64 padding converts losslessly; float64 draws round to float32
    assert np.array_equal(postproc.host_mutation_order(a,
        params.astype(np.float64), 2)[1], same)


def tables_from(counts, S, M):
    """A fake handle that answers with given count tables"""
    class Handle:
        def mutation_order(self, params, min_cells):
            return tuple(np.asarray(counts.get(k, np.zeros((M, M))),
                dtype=np.uint32) for k in TABLES)
    return Handle(), np.zeros((S, 3), dtype=np.int64), None


def test_a_handle_with_the_method_is_asked():
    rng = np.random.RandomState(3)
    S, N, M, W = 9, 12, 5, 4
    a = rng.randint(0, W, (S, N))
    params = rng.rand(S, W, M).astype(np.float32)
    host = postproc.host_mutation_order(a, params, 1)
    asked = []

    class Handle:
        def mutation_order(self, p, min_cells):
            asked.append((p is params, min_cells))
            return host
    got = postproc.mutation_order(Handle(), a, params, 1)
    want = postproc.mutation_order(None, a, params, 1)
    assert asked == [(True, 1)]
    for key in want:
        if key != 'total':
            assert np.array_equal(got[key], want[key]), key
    assert got['total'] == want['total']
    assert got['total']['samples'] == S and got['total']['pairs'] == 10
    assert got['total']['min_cells'] == 1
    assert np.array_equal(got['carried'], np.diag(host[1]) / S)
    shares = [got['total'][k] for k in ('ancestral', 'same', 'exclusive',
        'conflict', 'absent', 'undecided')]
    assert abs(sum(shares) - 1) < 1e-12 and min(shares) >= -1e-12


def test_a_chain_and_a_branch_make_a_forest():
    hi, lo = 0.8, 0.2
    rows = [[hi, hi, hi, lo, hi],
            [hi, hi, lo, lo, hi],
            [hi, lo, lo, hi, lo],
            [hi, lo, lo, lo, lo]]
    a, params = one_sample(rows, [2, 2, 2, 2])
    a, params = np.repeat(a, 3, axis=0), np.repeat(params, 3, axis=0)
    t = postproc.mutation_order(None, a, params, 2)
    assert t['depth'].tolist() == [0, 1, 3, 1, 1]
    # c's ancestors a, b, e: b and e tie in depth and count - the smaller
    assert t['parent'].tolist() == [-1, 0, 1, 0, 0]
    assert t['p_parent'].tolist() == [0, 1, 1, 1, 1]
    assert t['same_as'].tolist() == [-1, -1, -1, -1, 1]
    assert t['n_same'].tolist() == [0, 1, 0, 0, 1]
    assert t['n_descendants'].tolist() == [4, 1, 0, 0, 1]
    assert t['n_exclusive'].tolist() == [0, 1, 1, 3, 1]
    assert t['skipped_ancestors'].tolist() == [0] * 5
    assert t['worst_conflict'].tolist() == [-1] * 5
    assert not t['conflict'].any() and not t['p_worst_conflict'].any()
    total = t['total']
    assert (total['roots'], total['max_depth']) == (1, 3)
    assert total['ancestral'] == 0.6 and total['same'] == 0.1
    assert total['exclusive'] == 0.3 and total['undecided'] == 0
    assert total['most_conflicting'] == [0, 1, 2, 3, 4]


def test_a_majority_cycle_still_gives_a_forest():
    """Three kinds of samples: a > b > c, b > c > a, c > a > b.  Two thirds
    say a > b, two thirds b > c, two thirds c > a: every mutation has one
    majority ancestor and the same depth, so none may be a parent."""
    hi, lo = 0.8, 0.2
    chain = lambda order: [[hi if order.index(m) <= r else lo
        for m in range(3)] for r in range(3)]
    parts = [one_sample(chain(order), [2, 2, 2])
        for order in ([0, 1, 2], [1, 2, 0], [2, 0, 1])]
    a = np.concatenate([p[0] for p in parts])
    params = np.concatenate([p[1] for p in parts])
    t = postproc.mutation_order(None, a, params, 2)
    assert t['anc'].tolist() == [[0, 2, 1], [1, 0, 2], [2, 1, 0]]
    assert t['depth'].tolist() == [1, 1, 1]
    assert t['parent'].tolist() == [-1, -1, -1]
    assert t['skipped_ancestors'].tolist() == [1, 1, 1]
    assert t['total']['skipped_ancestors'] == 3
    assert t['total']['roots'] == 3 and t['total']['ancestral'] == 1.0
    # following `parent` never comes back: a forest
    for m in range(3):
        at, steps = m, 0
        while at >= 0 and steps < 4:
            at, steps = t['parent'][at], steps + 1
        assert at < 0


def test_ties_of_parent_and_worst_conflict():
    S, M = 10, 4
    anc = np.zeros((M, M))
    # 3 has the ancestors 0, 1, 2; 2 has the ancestor 0: depths 0, 0, 1, 3
    anc[0, 3], anc[1, 3], anc[2, 3], anc[0, 2] = 9, 9, 6, 9
    conf = np.zeros((M, M))
    conf[0, 1] = conf[1, 0] = 2
    conf[0, 2] = conf[2, 0] = 2
    post, a, params = tables_from({'anc': anc, 'conf': conf}, S, M)
    t = postproc.mutation_order(post, a, params, 2)
    assert t['depth'].tolist() == [0, 0, 1, 3]
    assert t['parent'].tolist() == [-1, -1, 0, 2]     # the deepest first
    assert t['p_parent'].tolist() == [0, 0, 0.9, 0.6]
    assert t['worst_conflict'].tolist() == [1, 0, 0, -1]
    assert t['p_worst_conflict'].tolist() == [0.2, 0.2, 0.2, 0]
    assert np.allclose(t['conflict'], [4 / 30, 2 / 30, 2 / 30, 0])
    assert t['total']['most_conflicting'] == [0, 1, 2, 3]
    # equal depth: the larger count, then the smaller index
    anc = np.zeros((M, M))
    anc[0, 3], anc[1, 3], anc[2, 3] = 7, 8, 8
    post, a, params = tables_from({'anc': anc}, S, M)
    assert postproc.mutation_order(post, a, params, 2)['parent'][3] == 1
    # exactly half is no majority
    anc[:] = 0
    anc[0, 1] = 5
    post, a, params = tables_from({'anc': anc}, S, M)
    assert postproc.mutation_order(post, a, params, 2)['parent'][1] == -1


def test_one_mutation():
    a, params = one_sample([[0.8], [0.2]], [2, 2])
    t = postproc.mutation_order(None, a, params, 2)
    assert t['same'].tolist() == [[1]] and t['carried'].tolist() == [1.0]
    assert t['conflict'].tolist() == [0.0]
    assert t['parent'].tolist() == [-1] and t['worst_conflict'].tolist() == [-1]
    total = t['total']
    assert total['pairs'] == 0 and total['undecided'] == 0
    assert total['mean_conflict'] == 0 and total['roots'] == 1


def test_writer(tmp_path, monkeypatch):
    rng = np.random.RandomState(5)
    S, N, M, W = 12, 20, 6, 5
    a = rng.randint(0, W, (S, N))
    params = rng.rand(S, W, M).astype(np.float32)
    t = postproc.mutation_order(None, a, params, 1)
    names = np.array([f'chr{m}:100' for m in range(M)])
    paths = bio.save_mutation_order(str(tmp_path), 'mean', 'posterior', t,
        names)
    assert [os.path.basename(p) for p in paths] == list(NEW_FILES)
    rows = [ln.split('\t') for ln in open(paths[0]).read().splitlines()]
    assert rows[0] == ['mutation', 'carried', 'depth', 'parent', 'p_parent',
        'same_as', 'n_same', 'n_descendants', 'n_exclusive', 'conflict',
        'worst_conflict', 'p_worst_conflict']
    assert [r[0] for r in rows[1:]] == names.tolist()
    name_of = lambda i, none: names[i] if i >= 0 else none
    for m, r in enumerate(rows[1:]):
        assert r[1] == f'{t["carried"][m]:.4f}'
        assert r[2] == str(t['depth'][m])
        assert r[3] == name_of(t['parent'][m], 'root')
        assert r[4] == f'{t["p_parent"][m]:.4f}'
        assert r[5] == name_of(t['same_as'][m], '-')
        assert r[6:9] == [str(t[k][m]) for k in ('n_same', 'n_descendants',
            'n_exclusive')]
        assert r[9] == f'{t["conflict"][m]:.4f}'
        assert r[10] == name_of(t['worst_conflict'][m], '-')
        assert r[11] == f'{t["p_worst_conflict"][m]:.4f}'
    lines = open(paths[1]).read().splitlines()
    assert [ln.split(': ')[0] for ln in lines] == ['samples', 'mutations',
        'pairs', 'min_cells', 'ancestral', 'same', 'exclusive', 'conflict',
        'absent', 'undecided', 'mean_conflict', 'roots', 'max_depth',
        'skipped_ancestors', 'most_conflicting', 'pairs_table']
    model = dict(ln.split(': ', 1) for ln in lines)
    assert model['samples'] == '12' and model['pairs'] == '15'
    assert model['conflict'] == f'{t["total"]["conflict"]:.4f}'
    assert model['pairs_table'] == 'written'
    top = model['most_conflicting'].split(' ')
    assert [x.rsplit(':', 1)[0] for x in top] \
        == [names[m] for m in t['total']['most_conflicting']]
    assert re.fullmatch(r'\d\.\d{4}', top[0].rsplit(':', 1)[1])
    rows = [ln.split('\t') for ln in open(paths[2]).read().splitlines()]
    assert rows[0] == ['a', 'b', 'p_anc', 'p_desc', 'p_same', 'p_excl',
        'p_conflict']
    assert [(r[0], r[1]) for r in rows[1:]] == [(names[x], names[y])
        for x in range(M) for y in range(x + 1, M)]
    r = rows[1 + 5 + 3]                 # the pair (1, 5)
    assert r[2:] == [f'{v / S:.4f}' for v in (t['anc'][1, 5], t['anc'][5, 1],
        t['same'][1, 5], t['excl'][1, 5], t['conf'][1, 5])]
    # without names: 0..M-1; above the limit no pairs file
    assert bio.MUTATION_PAIRS_MAX == 1000
    monkeypatch.setattr(bio, 'MUTATION_PAIRS_MAX', M - 1)
    out = tmp_path / 'big'
    out.mkdir()
    paths = bio.save_mutation_order(str(out), 'mean', 'posterior', t)
    assert [os.path.basename(p) for p in paths] == list(NEW_FILES[:2])
    assert sorted(os.listdir(out)) == sorted(NEW_FILES[:2])
    assert open(paths[1]).read().endswith('pairs_table: skipped\n')
    assert open(paths[0]).read().splitlines()[1].split('\t')[0] == '0'


def fake_results(rng, n, burn, N, M=6):
    return [{'assignments': rng.randint(0, 3, (n, N)), 'burn_in': burn,
        'params': rng.rand(n - burn, 3, M).astype(np.float32),
        'DP_alpha': rng.rand(n), 'ML': rng.rand(n), 'MAP': rng.rand(n),
        'FN': rng.rand(n) * 0.2 + 0.05, 'FP': rng.rand(n) * 0.01 + 0.001}]


def test_posterior_estimate_ordering(monkeypatch):
    monkeypatch.setattr(_lib, 'Posterior', FakePosterior)
    assert not hasattr(FakePosterior, 'mutation_order')    # the host loop
    rng = np.random.RandomState(7)
    results = fake_results(rng, 30, 10, 12)
    data = rng.randint(0, 2, (12, 6)).astype(float)
    plain = postproc.posterior_estimate(results, data)
    assert plain.keys() == postproc.posterior_estimate(results, data,
        ordering=False).keys()
    inf = postproc.posterior_estimate(results, data, ordering=2)
    assert sorted(set(inf) - set(plain)) == ['mutation_order']
    for key in plain:
        assert np.array_equal(inf[key], plain[key]), key
    pooled = postproc.concat_chain_results(results)
    want = postproc.mutation_order(None, pooled['assignments'],
        pooled['params'], 2)
    for key, table in zip(TABLES, postproc.host_mutation_order(
            pooled['assignments'], pooled['params'], 2)):
        assert np.array_equal(inf['mutation_order'][key], table)
    for key in want:
        if key != 'total':
            assert np.array_equal(inf['mutation_order'][key], want[key]), key
    assert inf['mutation_order']['total'] == want['total']
    strict = postproc.posterior_estimate(results, data, ordering=1)
    assert strict['mutation_order']['total']['min_cells'] == 1


def run_cli(tmp_path, monkeypatch, name, *flags):
    """run_BnpC.main on the golden example, one chain of 12 steps, with the
    NumPy stand-ins for the device"""
    monkeypatch.setattr(_lib, 'Context', FakeContext)
    monkeypatch.setattr(_lib, 'Posterior', FakePosterior)
    monkeypatch.delenv('BNPC_DEVICE', raising=False)
    out = tmp_path / name
    args = run_BnpC.parse_args([EXAMPLE, '--debug', '-s', '12', '--seed', '5',
        '-FP', '.001', '-FN', '.1', '-o', str(out), *flags])
    return out, run_BnpC.main(args)


def test_cli_writes_the_three_files(tmp_path, monkeypatch, capsys):
    out, results = run_cli(tmp_path, monkeypatch, 'with', '-po', '-v', '1')
    lines = [ln for ln in capsys.readouterr().out.splitlines()
        if ln.startswith('posterior order: ')]
    assert len(lines) == 1
    assert re.fullmatch(r'posterior order: \d+ roots, depth \d+, conflict '
        r'share \d\.\d{4}', lines[0])
    data, names = bio.load_data(EXAMPLE, get_names=True)
    want = postproc.posterior_estimate(results, data,
        ordering=2)['mutation_order']
    assert lines[0] == (f'posterior order: {want["total"]["roots"]} roots, '
        f'depth {want["total"]["max_depth"]}, conflict share '
        f'{want["total"]["conflict"]:.4f}')
    ref = tmp_path / 'ref'
    ref.mkdir()
    bio.save_mutation_order(str(ref), 'mean', 'posterior', want, names[1])
    for name in NEW_FILES:
        assert (out / name).read_bytes() == (ref / name).read_bytes(), name
    assert 'posterior_order: 2\n' in (out / 'args.txt').read_text()

    strict, _ = run_cli(tmp_path, monkeypatch, 'strict', '-po', '1', '-v', '0')
    assert 'posterior_order: 1\n' in (strict / 'args.txt').read_text()
    assert 'min_cells: 1\n' in (strict / NEW_FILES[1]).read_text()

    # a run without the flag: the same files but the three, the same bytes
    plain, _ = run_cli(tmp_path, monkeypatch, 'without', '-v', '0')
    assert sorted(os.listdir(plain)) \
        == sorted(set(os.listdir(out)) - set(NEW_FILES))
    for name in os.listdir(plain):
        if name != 'args.txt':
            assert (plain / name).read_bytes() == (out / name).read_bytes(), \
                name
    assert 'posterior_order' not in (plain / 'args.txt').read_text()


def test_flag_and_its_checks(monkeypatch, capsys):
    """(the input path is a required argument: `d.csv` stands for it)"""
    args = run_BnpC.parse_args(['d.csv'])
    assert args.posterior_order is False
    assert 'posterior_order' not in vars(args)
    run_BnpC.check_args(args)
    for argv, want in ((['-po'], 2), (['--posterior_order'], 2),
            (['-po', '1'], 1), (['-po', '7', '-s', '3'], 7)):
        args = run_BnpC.parse_args(['d.csv'] + argv)
        assert vars(args)['posterior_order'] == want
        assert isinstance(args.posterior_order, int)
        run_BnpC.check_args(args)
    for bad in ('0', '-3', 'x'):
        with pytest.raises(SystemExit):
            run_BnpC.parse_args(['d.csv', '-po', bad])
    capsys.readouterr()
    run_BnpC.check_args(run_BnpC.parse_args('d.csv -po -e ML posterior'
        .split()))
    started = []
    monkeypatch.setattr(bio, 'load_data',
        lambda *a, **k: started.append(a) or 1 / 0)
    for argv in (['-po', '-e', 'ML'], ['-po', '3', '-e', 'ML', 'MAP']):
        args = run_BnpC.parse_args(['d.csv'] + argv)
        with pytest.raises(SystemExit, match='posterior'):
            run_BnpC.check_args(args)
        # main() stops there: before the input is looked at
        with pytest.raises(SystemExit, match='--posterior_order'):
            run_BnpC.main(args)
    assert not started


def test_binding_and_header_list_the_entry_points():
    for name in ('bnpc_post_mutation_order', 'bnpc_post_mutation_order_times'):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    assert len(_lib.SIGNATURES['bnpc_post_mutation_order'][1]) == 11
    assert len(_lib.SIGNATURES['bnpc_post_mutation_order_times'][1]) == 8
    assert hasattr(_lib.Posterior, 'mutation_order')
    assert hasattr(_lib.Posterior, 'mutation_order_times')
    with open(os.path.join(ROOT, 'include', 'bnpc_hip.h')) as f:
        header = f.read()
    assert re.search(r'\bint bnpc_post_mutation_order\(bnpc_post \*post, '
        r'const float \*params, int64_t W,\s+int64_t M, int64_t min_cells, '
        r'int64_t chunk,\s+int64_t slab, uint32_t \*anc, uint32_t \*same,\s+'
        r'uint32_t \*excl, uint32_t \*conf', header)
    assert re.search(r'\bint bnpc_post_mutation_order_times\(bnpc_post \*post, '
        r'const float \*params,\s+int64_t W, int64_t M, int64_t min_cells,\s+'
        r'int64_t chunk, int64_t slab, float \*ms\)', header)
    assert 'host_mutation_order' in header and 'three-gamete' in header
    with open(os.path.join(ROOT, 'bnpc_amd', 'csrc',
            'bnpc_post_passes.hip')) as f:
        source = f.read()
    for name, value in (('PO_TILE', _lib.ORDER_TILE),
            ('PO_STAGE', _lib.ORDER_STAGE),
            ('PO_LDS_ROWS', _lib.ORDER_LDS_ROWS), ('PO_WG', _lib.ORDER_WG)):
        assert re.search(rf'#define {name} {value}\b', source), name
    assert _lib.ABI_VERSION == 12
