"""Between-chain agreement of the clustering (-pc): the host side.
postproc.host_chain_agreement against a restatement that builds the N x N
per-chain matrices, constructed patterns, the derived floats and their tie
rules, the argument errors, the bounds posterior_estimate computes, the two
files and the flag.  CPU only: the clustering handle is the NumPy stand-in of
tests/fake_device.py, the chains run on its context."""
import os
import re

import numpy as np
import pytest

import run_BnpC
from bnpc_amd import _lib, postproc
from bnpc_amd import io as bio
from fake_device import FakeContext, FakePosterior

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FILES = ('chain_agreement_posterior_mean.tsv',
    'chain_summary_posterior_mean.txt')


def bounds_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def brute_tables(a, bounds, pooled=None):
    """The three tables from the N x N matrices of pair counts, one per chain
    (N <= 200 or so); pooled: the pooled matrix, if not the chains' sum."""
    a = np.asarray(a)
    S, N = a.shape
    b = [int(x) for x in bounds]
    C = len(b) - 1
    d = [(a[b[c]:b[c + 1], :, None] != a[b[c]:b[c + 1], None, :])
        .sum(axis=0).astype(np.int64) for c in range(C)]
    if pooled is None:
        pooled = sum(d)
    off = ~np.eye(N, dtype=bool)
    out = np.zeros((3, C, N), dtype=np.int64)
    for c in range(C):
        Sc = b[c + 1] - b[c]
        Rc = S - Sc
        same_c = Sc - d[c]
        same_r = (S - pooled) - same_c
        x = np.abs(same_c * Rc - same_r * Sc)
        flip = (2 * same_c > Sc) != (2 * same_r > Rc)
        out[0, c] = np.where(off, x, 0).sum(axis=1)
        out[1, c] = np.where(off, x, 0).max(axis=1)
        out[2, c] = np.where(off, flip, False).sum(axis=1)
    return tuple(out)


def chains_that_differ(rng, lengths, N):
    """Pooled samples of len(lengths) chains, each scattered around a
    clustering of its own: (S x N int32, bounds)."""
    rows = []
    for n in lengths:
        K = rng.randint(1, 6)
        base = rng.randint(0, K, N)
        for _ in range(n):
            row = base.copy()
            move = rng.rand(N) < 0.3
            row[move] = rng.randint(0, K + 1, int(move.sum()))
            rows.append(row)
    return np.array(rows, dtype=np.int32), bounds_of(lengths)


def identical_chains(rng, n, C, N):
    block = rng.randint(0, 4, (n, N))
    return np.tile(block, (C, 1)).astype(np.int32), bounds_of([n] * C)


def opposite_chains(n0, n1, N):
    """chain 0: all cells together; chain 1: every cell alone"""
    a = np.concatenate([np.zeros((n0, N), dtype=np.int32),
        np.tile(np.arange(N, dtype=np.int32), (n1, 1))])
    return a, bounds_of([n0, n1])


def exact_half(n0, n1, N):
    """chain 0 (n0 even): cells 0 and 1 share a label in exactly n0 / 2
    samples, every other cell is alone; chain 1: cells 0 and 1 together"""
    assert n0 % 2 == 0
    a = np.tile(np.arange(N, dtype=np.int32), (n0 + n1, 1))
    a[:n0:2, 1] = 0
    a[n0:, 1] = 0
    return a, bounds_of([n0, n1])


def same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and np.array_equal(g, w)


@pytest.mark.parametrize('lengths,N', [([5, 7], 2), ([1, 1], 9),
    ([3, 1, 8], 17), ([4, 9, 2, 6, 1, 3, 5, 2], 40), ([33, 31], 33)])
def test_host_loop_against_the_matrices(lengths, N):
    rng = np.random.RandomState(N + len(lengths))
    a, bounds = chains_that_differ(rng, lengths, N)
    got = postproc.host_chain_agreement(a, bounds)
    assert all(t.shape == (len(lengths), N) for t in got)
    same(got, brute_tables(a, bounds))
    assert got[0].any() or N == 2


def test_two_pairs_by_hand():
    # chain 0 (4 samples): cells 0, 1 together 3 times; chain 1 (2): never
    a = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 1, 2],
        [0, 1, 2], [0, 1, 1]])
    abs_sum, max_abs, flips = postproc.host_chain_agreement(a, [0, 4, 6])
    # pair (0, 1): same_c = 3, same_r = 0: x = 3 * 2 - 0 * 4 = 6, a flip
    # pair (0, 2): never together: x = 0
    # pair (1, 2): same_c = 0, same_r = 1: x = 0 * 2 - 1 * 4 = -4, no flip
    #              (1 of 2 is exactly half: apart)
    assert abs_sum.tolist() == [[6, 10, 4], [6, 10, 4]]
    assert max_abs.tolist() == [[6, 6, 4], [6, 6, 4]]
    assert flips.tolist() == [[1, 1, 0], [1, 1, 0]]


def test_identical_chains_agree_everywhere():
    a, bounds = identical_chains(np.random.RandomState(2), 7, 3, 21)
    for table in postproc.host_chain_agreement(a, bounds):
        assert table.shape == (3, 21) and not table.any()


def test_opposite_chains_flip_every_pair():
    a, bounds = opposite_chains(6, 9, 12)
    abs_sum, max_abs, flips = postproc.host_chain_agreement(a, bounds)
    assert (max_abs == 6 * 9).all() and (abs_sum == 6 * 9 * 11).all()
    assert (flips == 11).all()
    t = postproc.chain_agreement(None, a, bounds, np.zeros(12, dtype=int))
    assert (t['diff'] == 1.0).all() and (t['max_diff'] == 1.0).all()
    assert (t['flip_share'] == 1.0).all()
    assert t['total']['mean_diff'] == 1.0 and t['total']['flip_share'] == 1.0


def test_exact_half_is_not_a_majority():
    a, bounds = exact_half(6, 5, 4)
    abs_sum, max_abs, flips = postproc.host_chain_agreement(a, bounds)
    same((abs_sum, max_abs, flips), brute_tables(a, bounds))
    # 3 of 6 in chain 0 is "apart", 5 of 5 in chain 1 "together": a flip
    assert flips.tolist() == [[1, 1, 0, 0], [1, 1, 0, 0]]
    assert max_abs[0, 0] == 3 * 5 - 5 * 6 + 30     # |3 * 5 - 5 * 6| = 15
    # one sample more together in chain 0: a majority on both sides
    a[1, 1] = 0
    assert not postproc.host_chain_agreement(a, bounds)[2].any()


def test_derived_floats():
    rng = np.random.RandomState(3)
    lengths = [5, 9, 4]
    a, bounds = chains_that_differ(rng, lengths, 23)
    labels = rng.randint(0, 3, 23) * 2              # labels 0, 2, 4
    abs_sum, max_abs, flips = postproc.host_chain_agreement(a, bounds)
    t = postproc.chain_agreement(None, a, bounds, labels)
    S, N, C = 18, 23, 3
    for c, Sc in enumerate(lengths):
        span = Sc * (S - Sc)
        assert np.array_equal(t['diff'][:, c], abs_sum[c] / (span * (N - 1)))
        assert np.array_equal(t['max_diff'][:, c], max_abs[c] / span)
        assert np.array_equal(t['flip_share'][:, c], flips[c] / (N - 1))
        assert t['mean_diff_c'][c] == int(abs_sum[c].sum()) \
            / (span * N * (N - 1))
        assert t['max_diff_c'][c] == (max_abs[c] / span).max()
        assert t['flip_share_c'][c] == int(flips[c].sum()) / (N * (N - 1))
    assert np.array_equal(t['flips'], flips.T)
    assert t['samples'].tolist() == lengths
    assert ((t['diff'] >= 0) & (t['diff'] <= t['max_diff'])).all()
    assert (t['max_diff'] <= 1).all()
    assert np.array_equal(t['worst_diff'], t['diff'].max(axis=1))
    assert np.array_equal(t['worst_chain'], t['diff'].argmax(axis=1))
    assert t['clusters'].tolist() == [0, 2, 4]
    for row, k in enumerate((0, 2, 4)):
        assert np.array_equal(t['cluster_diff'][row],
            t['diff'][labels == k].mean(axis=0))
    total = t['total']
    assert total['chains'] == C and total['cells'] == N
    assert total['pairs'] == N * (N - 1) // 2 and total['samples'] == S
    assert total['mean_diff'] == t['mean_diff_c'].mean()
    assert total['worst_chain'] == int(t['mean_diff_c'].argmax())
    assert total['worst_mean_diff'] == t['mean_diff_c'].max()
    assert total['flip_share'] == int(flips.sum()) / (C * N * (N - 1))


def test_worst_chain_ties_go_to_the_smallest_index():
    # two chains of equal length: x of chain 1 is minus x of chain 0
    a, bounds = opposite_chains(4, 4, 5)
    t = postproc.chain_agreement(None, a, bounds, np.zeros(5, dtype=int))
    assert np.array_equal(t['diff'][:, 0], t['diff'][:, 1])
    assert t['worst_chain'].tolist() == [0] * 5
    assert t['total']['worst_chain'] == 0


def test_a_handle_with_the_method_is_asked():
    rng = np.random.RandomState(4)
    a, bounds = chains_that_differ(rng, [3, 4], 9)
    want = postproc.host_chain_agreement(a, bounds)

    class Handle(FakePosterior):
        calls = 0

        def chain_agreement(self, b):
            assert b.dtype == np.int64 and b.tolist() == bounds.tolist()
            self.calls += 1
            # (marked, so that the host loop cannot have made them)
            return want[0] * 2, want[1], want[2]
    post = Handle(a)
    labels = np.zeros(9, dtype=int)
    got = postproc.chain_agreement(post, a, bounds, labels)
    plain = postproc.chain_agreement(FakePosterior(a), a, bounds, labels)
    assert post.calls == 1
    assert np.array_equal(got['diff'], 2 * plain['diff'])
    assert np.array_equal(got['max_diff'], plain['max_diff'])
    with pytest.raises(ValueError):     # checked before the handle is asked
        postproc.chain_agreement(post, a, [0, 7], labels)
    assert post.calls == 1


@pytest.mark.parametrize('bounds,why', [([0, 7], 'C >= 2'), ([0], 'C >= 2'),
    ([0, 3, 3, 7], 'empty'), ([0, 5, 3, 7], 'empty'), ([1, 3, 7], 'from 0'),
    ([0, 3, 6], 'from 0'), ([0, 3, 8], 'from 0'), ([0, 3, 9, 7], 'empty'),
    ([0.0, 3.0, 7.0], 'integers')])
def test_bounds_that_cannot_run(bounds, why):
    a = np.zeros((7, 4), dtype=np.int32)
    with pytest.raises(ValueError, match=why):
        postproc.host_chain_agreement(a, bounds)
    with pytest.raises(ValueError, match=why):
        postproc.chain_agreement(None, a, bounds, np.zeros(4, dtype=int))


def test_sums_past_63_bits_are_refused():
    S, N = 2 ** 21, 2 ** 22
    with pytest.raises(ValueError, match='63 bits'):
        postproc.chain_bounds([0, 2 ** 20, S], S, N)
    # the largest product that fits, and the first that does not
    assert postproc.chain_bounds([0, 1, 2], 2, 3037000500)[-1] == 2
    with pytest.raises(ValueError, match='63 bits'):
        postproc.chain_bounds([0, 1, 2], 2, 3037000501)


def fake_results(rng, lengths, burn_ins, N, M=6):
    results = []
    for n, burn in zip(lengths, burn_ins):
        a = rng.randint(0, 3, (n, N))
        results.append({'assignments': a, 'burn_in': burn,
            'params': rng.rand(n - burn, 3, M).astype(np.float32),
            'DP_alpha': rng.rand(n), 'ML': rng.rand(n), 'MAP': rng.rand(n),
            'FN': rng.rand(n) * 0.2 + 0.05, 'FP': rng.rand(n) * 0.01 + 0.001})
    return results


def test_bounds_follow_every_chains_own_burn_in():
    rng = np.random.RandomState(6)
    results = fake_results(rng, [30, 22, 41], [10, 0, 33], 12)
    assert postproc.results_bounds(results).tolist() == [0, 20, 42, 50]
    pooled = postproc.concat_chain_results(results)
    assert pooled['assignments'].shape[0] == 50
    assert np.array_equal(pooled['assignments'][20:42],
        results[1]['assignments'])


@pytest.fixture
def host_posterior(monkeypatch):
    monkeypatch.setattr(_lib, 'Posterior', FakePosterior)


def test_posterior_estimate_chains(host_posterior):
    rng = np.random.RandomState(7)
    results = fake_results(rng, [30, 22, 41], [10, 0, 33], 12)
    # chain 1 holds one clustering throughout
    results[1]['assignments'][:] = np.arange(12) % 2
    data = rng.randint(0, 2, (12, 6)).astype(float)
    plain = postproc.posterior_estimate(results, data)
    assert plain.keys() == postproc.posterior_estimate(results, data,
        chains=False).keys()
    inf = postproc.posterior_estimate(results, data, chains=True)
    assert sorted(set(inf) - set(plain)) == ['chains']
    for key in plain:
        assert np.array_equal(inf[key], plain[key]), key
    pooled = postproc.concat_chain_results(results)
    want = postproc.chain_agreement(None, pooled['assignments'],
        [0, 20, 42, 50], plain['cluster_of'])
    assert inf['chains'].keys() == want.keys()
    for key in want:
        if key != 'total':
            assert np.array_equal(inf['chains'][key], want[key]), key
    assert inf['chains']['total'] == want['total']
    assert inf['chains']['total']['worst_chain'] == 1
    with pytest.raises(ValueError, match='C >= 2'):
        postproc.posterior_estimate(results[:1], data, chains=True)


def test_unstable_cells_break_ties_by_index(tmp_path):
    N, C = 12, 2
    worst = np.array([0.5, 0.9, 0.9, 0.2, 0.9] + [0.0] * 7)
    diff = np.stack([worst, worst / 2], axis=1)
    zeros = np.zeros((N, C), dtype=np.int64)
    tables = {'cluster': np.arange(N) % 2, 'worst_chain': zeros[:, 0],
        'worst_diff': worst, 'diff': diff, 'max_diff': diff, 'flips': zeros,
        'flip_share': diff, 'samples': np.array([3, 4]),
        'mean_diff_c': np.array([0.3, 0.15]),
        'max_diff_c': np.array([0.9, 0.45]),
        'flip_share_c': np.zeros(2), 'clusters': np.array([0, 1]),
        'cluster_diff': np.array([[0.1, 0.2], [0.3, 0.4]]),
        'total': {'chains': C, 'cells': N, 'pairs': 66, 'samples': 7,
            'mean_diff': 0.225, 'worst_chain': 0, 'worst_mean_diff': 0.3,
            'flip_share': 0.0}}
    paths = bio.save_chain_agreement(str(tmp_path), 'mean', 'posterior',
        tables)
    assert [os.path.basename(x) for x in paths] == list(NEW_FILES)
    with open(paths[1]) as f:
        model = dict(ln.rstrip('\n').split(': ', 1) for ln in f)
    top = [x.split(':')[0] for x in model['unstable_cells'].split(' ')]
    assert top == ['1', '2', '4', '0', '3', '5', '6', '7', '8', '9']
    assert model['cluster_diff'] == '0 0.1000 0.2000; 1 0.3000 0.4000'
    assert model['worst_chain'] == '0:0.3000'
    assert model['samples'] == '3 4'


def run_cli(tmp_path, monkeypatch, name, *flags):
    """run_BnpC.main on the golden example, two chains of 12 steps, with the
    NumPy stand-ins for the device"""
    monkeypatch.setattr(_lib, 'Context', FakeContext)   # inherited by fork
    monkeypatch.setattr(_lib, 'Posterior', FakePosterior)
    monkeypatch.delenv('BNPC_DEVICE', raising=False)
    monkeypatch.setenv('BNPC_NUM_DEVICES', '2')
    out = tmp_path / name
    args = run_BnpC.parse_args([os.path.join(ROOT, 'tests', 'golden',
        'example_data.csv'), '-n', '2', '-s', '12', '--seed', '5', '-FP',
        '.001', '-FN', '.1', '-o', str(out), *flags])
    return out, run_BnpC.main(args)


def test_cli_writes_the_two_files(tmp_path, monkeypatch, capsys):
    out, results = run_cli(tmp_path, monkeypatch, 'with', '-pc', '-v', '1')
    lines = [ln for ln in capsys.readouterr().out.splitlines()
        if ln.startswith('posterior chains: ')]
    assert len(lines) == 1
    assert re.fullmatch(r'posterior chains: mean difference \d\.\d{4}, worst '
        r'chain [01] \(\d\.\d{4}\), flip share \d\.\d{4}', lines[0])
    assert len(results) == 2
    data, names = bio.load_data(os.path.join(ROOT, 'tests', 'golden',
        'example_data.csv'), get_names=True)
    want = postproc.posterior_estimate(results, data, chains=True)
    assign, want = want['assignment'], want['chains']
    N, C = 100, 2
    rows = [ln.split('\t') for ln in
        (out / NEW_FILES[0]).read_text().splitlines()]
    assert rows[0] == ['cell', 'cluster', 'worst_chain', 'worst_diff',
        'diff_0', 'max_0', 'flips_0', 'diff_1', 'max_1', 'flips_1']
    assert len(rows) == N + 1 and all(len(r) == 4 + 3 * C for r in rows)
    assert [r[0] for r in rows[1:]] == [str(x) for x in names[0].tolist()]
    assert [int(r[1]) for r in rows[1:]] == assign
    assert [r[2] for r in rows[1:]] == [str(x) for x in want['worst_chain']]
    assert [r[3] for r in rows[1:]] == [f'{x:.4f}' for x in want['worst_diff']]
    for c in range(C):
        assert [r[4 + 3 * c] for r in rows[1:]] \
            == [f'{x:.4f}' for x in want['diff'][:, c]]
        assert [r[5 + 3 * c] for r in rows[1:]] \
            == [f'{x:.4f}' for x in want['max_diff'][:, c]]
        assert [r[6 + 3 * c] for r in rows[1:]] \
            == [str(x) for x in want['flips'][:, c].tolist()]
    lines = (out / NEW_FILES[1]).read_text().splitlines()
    assert [ln.split(':')[0] for ln in lines] == ['chains', 'samples',
        'cells', 'pairs', 'mean_diff', 'max_diff', 'flip_share',
        'worst_chain', 'cluster_diff', 'unstable_cells']
    model = {k: v.strip() for k, v in (ln.split(':', 1) for ln in lines)}
    bounds = postproc.results_bounds(results)
    assert model['chains'] == '2' and model['cells'] == '100'
    assert model['pairs'] == '4950'
    assert model['samples'].split() == [str(x) for x in np.diff(bounds)]
    for key in ('mean_diff', 'max_diff', 'flip_share'):
        assert model[key].split() == [f'{x:.4f}' for x in want[key + '_c']]
    assert len(model['cluster_diff'].split(';')) == len(set(assign))
    order = np.argsort(-want['worst_diff'], kind='stable')[:10]
    assert [x.rsplit(':', 1)[0] for x in model['unstable_cells'].split(' ')] \
        == [str(names[0][i]) for i in order]
    assert 'posterior_chains: True\n' in (out / 'args.txt').read_text()

    # a run without the flag: the same files but the two, the same bytes
    plain, _ = run_cli(tmp_path, monkeypatch, 'without', '-v', '0')
    assert sorted(os.listdir(plain)) \
        == sorted(set(os.listdir(out)) - set(NEW_FILES))
    for name in os.listdir(plain):
        if name != 'args.txt':
            assert (plain / name).read_bytes() == (out / name).read_bytes(), \
                name
    assert 'posterior_chains' not in (plain / 'args.txt').read_text()


def test_flag_and_its_checks(monkeypatch):
    """(the input path is a required argument: `d.csv` stands for it)"""
    args = run_BnpC.parse_args(['d.csv'])
    assert args.posterior_chains is False
    assert 'posterior_chains' not in vars(args)
    run_BnpC.check_args(args)
    for flag in ('-pc', '--posterior_chains'):
        args = run_BnpC.parse_args(['d.csv', flag, '-n', '2'])
        assert vars(args)['posterior_chains'] is True
        run_BnpC.check_args(args)
    run_BnpC.check_args(run_BnpC.parse_args('d.csv -pc -n 3 -e ML posterior'
        .split()))
    started = []
    monkeypatch.setattr(bio, 'load_data',
        lambda *a, **k: started.append(a) or 1 / 0)
    for argv, why in ((['-pc'], 'two or more'),
            (['-pc', '-n', '1'], 'two or more'),
            (['-pc', '-n', '2', '--debug'], '--debug'),
            (['-pc', '-n', '2', '-e', 'ML'], 'posterior'),
            (['-pc', '-n', '2', '-e', 'ML', 'MAP'], 'posterior')):
        args = run_BnpC.parse_args(['d.csv'] + argv)
        with pytest.raises(SystemExit, match=why):
            run_BnpC.check_args(args)
        # main() stops there: before the input is looked at
        with pytest.raises(SystemExit, match='--posterior_chains'):
            run_BnpC.main(args)
    assert not started


def test_binding_and_header_list_the_entry_points():
    for name in ('bnpc_post_chain_agreement',
            'bnpc_post_chain_agreement_times'):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    assert hasattr(_lib.Posterior, 'chain_agreement')
    assert hasattr(_lib.Posterior, 'chain_agreement_times')
    with open(os.path.join(ROOT, 'include', 'bnpc_hip.h')) as f:
        header = f.read()
    assert re.search(r'\bint bnpc_post_chain_agreement\(bnpc_post \*post, '
        r'const int64_t \*bounds', header)
    assert re.search(r'\bint bnpc_post_chain_agreement_times\(bnpc_post '
        r'\*post', header)
    assert _lib.ABI_VERSION == 12
