"""Per-mutation posterior fit and error rates (-pm): the host side.
postproc.host_mutation_fit against a per-entry evaluation that uses no counts,
against host_cell_fit (the same total likelihood, summed along the other
axis) and against the ML trace the chains recorded; hand-computed columns,
the routing of postproc.mutation_fit, the two files save_outputs writes, and
the flag.  CPU only: the clustering handle is the NumPy stand-in of
tests/fake_device.py, which has no mutation_fit method."""
import math
import os
import re

import numpy as np
import pytest

import run_BnpC
from bnpc_amd import _lib, postproc
from bnpc_amd import io as bio
from fake_device import FakePosterior
from test_cell_fit import small_case
from test_outputs import load_case
from test_support import save

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FILES = ('mutation_fit_posterior_mean.tsv',
    'mutation_summary_posterior_mean.txt')
COLUMNS = ['n_obs', 'n_ones', 'n_zeros', 'mean_ll', 'sd_ll',
    'mean_ll_per_obs', 'prevalence', 'FN_model', 'FP_model', 'FN_call',
    'FP_call']
SUMS = ('sum_ll', 'sum_ll2', 'efn', 'efp', 'eg1')
COUNTS = ('call1_obs1', 'call1_obs0', 'n1', 'n0')


def brute_force(data, a, params, FN, FP):
    """every observed entry on its own, no counts: per (s, m) the entries'
    L, qfn, qfp and carrier probability summed with math.fsum"""
    S, N = a.shape
    M = data.shape[1]
    ll, efn, efp, eg1 = (np.empty((S, M)) for _ in range(4))
    call = np.zeros((2, M), dtype=np.int64)
    for s in range(S):
        present = sorted(set(a[s].tolist()))
        for m in range(M):
            terms = [[], [], [], []]
            for i in range(N):
                if np.isnan(data[i, m]):
                    continue
                th = np.float32(params[s][present.index(a[s, i])][m])
                t, o = float(th), float(np.float32(1) - th)
                if data[i, m] == 1:
                    a1, b1 = t * (1 - FN[s]), o * FP[s]
                    terms[0].append(math.log(a1 + b1))
                    terms[2].append(b1 / (a1 + b1))
                    terms[3].append(a1 / (a1 + b1))
                    call[0, m] += th > 0.5
                else:
                    a0, b0 = t * FN[s], o * (1 - FP[s])
                    terms[0].append(math.log(a0 + b0))
                    terms[1].append(a0 / (a0 + b0))
                    terms[3].append(a0 / (a0 + b0))
                    call[1, m] += th > 0.5
            ll[s, m], efn[s, m], efp[s, m], eg1[s, m] = map(math.fsum, terms)
    return {'ll': ll, 'sum_ll': ll.sum(axis=0),
        'sum_ll2': (ll * ll).sum(axis=0), 'efn': efn.sum(axis=0),
        'efp': efp.sum(axis=0), 'eg1': eg1.sum(axis=0),
        'call1_obs1': call[0], 'call1_obs0': call[1],
        'n1': (data == 1).sum(axis=0), 'n0': (data == 0).sum(axis=0)}


def test_host_loop_against_the_per_entry_evaluation():
    data, a, params, FN, FP = small_case()
    S, M = a.shape[0], data.shape[1]
    fit = postproc.host_mutation_fit(data, a, params, FN, FP)
    assert sorted(fit) == sorted(SUMS + COUNTS + ('ll',))
    assert fit['ll'].shape == (S, M) and fit['ll'].dtype == np.float64
    for key in SUMS:
        assert fit[key].shape == (M,) and fit[key].dtype == np.float64, key
    for key in COUNTS:
        assert fit[key].shape == (M,) and fit[key].dtype == np.int64, key
    want = brute_force(data, a, params, FN, FP)
    for key in COUNTS:
        assert np.array_equal(fit[key], want[key]), key
    for key in SUMS + ('ll',):
        np.testing.assert_allclose(fit[key], want[key], rtol=1e-12, atol=0,
            err_msg=key)
    assert fit['call1_obs1'].any() and fit['call1_obs0'].any()
    # the reductions are those of the matrix, in sample order
    sums = postproc.mutation_fit_sums(fit['ll'])
    acc, acc2 = np.zeros(M), np.zeros(M)
    for s in range(S):
        acc = acc + fit['ll'][s]
        acc2 = acc2 + fit['ll'][s] * fit['ll'][s]
    for got in (fit, sums):
        assert np.array_equal(got['sum_ll'], acc)
        assert np.array_equal(got['sum_ll2'], acc2)
    # swapped error rates are another model
    swapped = postproc.host_mutation_fit(data, a, params, FP, FN)
    for key in SUMS + ('ll',):
        assert not np.allclose(swapped[key], want[key], rtol=1e-12, atol=0), \
            key


def test_both_axes_sum_to_the_same_total():
    data, a, params, FN, FP = small_case()
    by_mut = postproc.host_mutation_fit(data, a, params, FN, FP)['ll']
    by_cell = postproc.host_cell_fit(data, a, params, FN, FP)['ll']
    np.testing.assert_allclose(by_mut.sum(axis=1), by_cell.sum(axis=1),
        rtol=1e-12, atol=0)
    swapped = postproc.host_mutation_fit(data, a, params, FP, FN)['ll']
    assert not np.allclose(swapped.sum(axis=1), by_cell.sum(axis=1),
        rtol=1e-12, atol=0)


def test_matrix_sums_to_the_chains_own_trace(golden_dir, tmp_path):
    """as tests/test_cell_fit.py: every term is <= 0, so two orders of
    summation differ by at most N * M * 2**-52 relative"""
    d, case, results = load_case(golden_dir, 'fixture', tmp_path / 'ref')
    data = bio.load_data(os.path.join(d, 'input.tsv'))
    pooled = postproc.concat_chain_results(results)
    fit = postproc.host_mutation_fit(data, pooled['assignments'],
        pooled['params'], pooled['FN'], pooled['FP'])
    S = pooled['ML'].size
    assert S > 60 and fit['ll'].shape == (S, data.shape[1])
    np.testing.assert_allclose(fit['ll'].sum(axis=1), pooled['ML'],
        rtol=data.size * 2.0 ** -52, atol=0)
    swapped = postproc.host_mutation_fit(data, pooled['assignments'],
        pooled['params'], pooled['FP'], pooled['FN'])
    assert not np.allclose(swapped['ll'].sum(axis=1), pooled['ML'],
        rtol=data.size * 2.0 ** -52, atol=0)
    # the identities
    t = postproc.mutation_fit(None, data, pooled['assignments'],
        pooled['params'], pooled['FN'], pooled['FP'])
    assert (fit['efn'] <= fit['eg1']).all()
    assert (fit['call1_obs1'] <= S * fit['n1']).all()
    assert (fit['call1_obs0'] <= S * fit['n0']).all()
    seen = t['n_obs'] > 0
    assert ((t['prevalence'][seen] >= 0) & (t['prevalence'][seen] <= 1)).all()


def test_hand_computed_columns():
    """column 0 all missing; column 1 all ones under th = 1; column 2 all
    zeros under th = 0; column 3 mixed under th = 1/2"""
    S, N = 3, 4
    data = np.array([[np.nan, 1, 0, 1], [np.nan, 1, 0, 0], [np.nan, 1, 0, 1],
        [np.nan, 1, 0, np.nan]])
    a = np.zeros((S, N), dtype=int)
    params = np.tile(np.float32([0.3, 1.0, 0.0, 0.5]), (S, 1, 1))
    FN = np.array([0.25, 0.125, 0.5])
    FP = np.array([0.125, 0.25, 0.0625])
    fit = postproc.host_mutation_fit(data, a, params, FN, FP)
    t = postproc.mutation_fit(None, data, a, params, FN, FP)
    assert list(t) == COLUMNS + ['eg1', 'total']
    assert np.array_equal(t['n_obs'], [0, 4, 4, 3])
    assert np.array_equal(t['n_ones'], [0, 4, 0, 2])
    assert np.array_equal(t['n_zeros'], [0, 0, 4, 1])
    # nothing observed: zeros, nan rates, 0 per observation
    for key in SUMS + ('call1_obs1', 'call1_obs0'):
        assert fit[key][0] == 0, key
    assert not fit['ll'][:, 0].any()
    for key in ('mean_ll', 'sd_ll', 'mean_ll_per_obs'):
        assert t[key][0] == 0, key
    for key in ('prevalence', 'FN_model', 'FP_model', 'FN_call', 'FP_call'):
        assert np.isnan(t[key][0]), key
    # th = 1, all ones: L1 = log(1 - FN), no false positive, every cell a
    # carrier, called 1
    np.testing.assert_array_equal(fit['ll'][:, 1], 4 * np.log(1 - FN))
    assert fit['efp'][1] == 0 and fit['efn'][1] == 0
    assert fit['eg1'][1] == 4 * S
    assert fit['call1_obs1'][1] == 4 * S and fit['call1_obs0'][1] == 0
    assert t['prevalence'][1] == 1 and t['FN_model'][1] == 0
    assert np.isnan(t['FP_model'][1]) and np.isnan(t['FP_call'][1])
    assert t['FN_call'][1] == 0
    # th = 0, all zeros: L0 = log(1 - FP), nobody carries it
    np.testing.assert_array_equal(fit['ll'][:, 2], 4 * np.log(1 - FP))
    assert fit['efp'][2] == 0 and fit['efn'][2] == 0 and fit['eg1'][2] == 0
    assert fit['call1_obs1'][2] == 0 and fit['call1_obs0'][2] == 0
    assert t['prevalence'][2] == 0 and np.isnan(t['FN_model'][2])
    assert t['FP_model'][2] == 0 and np.isnan(t['FN_call'][2])
    assert t['FP_call'][2] == 0
    # th = 1/2 (not called: 0.5 > 0.5 is false)
    l1 = np.log(0.5 * (1 - FN) + 0.5 * FP)
    l0 = np.log(0.5 * FN + 0.5 * (1 - FP))
    np.testing.assert_allclose(fit['ll'][:, 3], 2 * l1 + l0, rtol=1e-15)
    qfp = FP / (1 - FN + FP)
    qfn = FN / (FN + 1 - FP)
    np.testing.assert_allclose(fit['efp'][3], (2 * qfp).sum(), rtol=1e-15)
    np.testing.assert_allclose(fit['efn'][3], qfn.sum(), rtol=1e-15)
    np.testing.assert_allclose(fit['eg1'][3], (2 * (1 - qfp) + qfn).sum(),
        rtol=1e-15)
    assert fit['call1_obs1'][3] == 0 and fit['call1_obs0'][3] == 0
    assert t['FP_call'][3] == 2 * S / (3 * S)
    np.testing.assert_allclose(t['mean_ll'], fit['ll'].mean(axis=0),
        rtol=1e-15)
    np.testing.assert_allclose(t['sd_ll'], fit['ll'].std(axis=0, ddof=1),
        rtol=1e-9, atol=1e-12)
    total = t['total']
    assert total['samples'] == S and total['mutations'] == 4
    assert total['observations'] == 11
    assert total['FN'] == FN.mean() and total['FP'] == FP.mean()
    assert total['FN_model'] == fit['efn'].sum() / fit['eg1'].sum()
    assert total['FP_model'] == fit['efp'].sum() / (S * 11 - fit['eg1'].sum())
    assert total['FN_call'] == 0 and total['FP_call'] == 2 * S / (7 * S)


def test_one_sample():
    data, a, params, FN, FP = small_case(S=1)
    t = postproc.mutation_fit(None, data, a, params, FN, FP)
    fit = postproc.host_mutation_fit(data, a, params, FN, FP)
    assert not t['sd_ll'].any()
    assert np.array_equal(t['mean_ll'], fit['ll'][0])


def test_handle_without_the_method_takes_the_host_loop():
    data, a, params, FN, FP = small_case()
    post = FakePosterior(a)
    assert not hasattr(post, 'mutation_fit')
    got = postproc.mutation_fit(post, data, a, params, FN, FP, order=a[0])
    fit = postproc.host_mutation_fit(data, a, params, FN, FP)
    S = a.shape[0]
    n_obs = fit['n1'] + fit['n0']
    assert np.array_equal(got['n_obs'], n_obs)
    assert np.array_equal(got['mean_ll'], fit['sum_ll'] / S)
    assert np.array_equal(got['prevalence'], fit['eg1'] / (S * n_obs))
    assert np.array_equal(got['FN_model'], fit['efn'] / fit['eg1'])
    assert np.array_equal(got['FP_model'],
        fit['efp'] / (S * n_obs - fit['eg1']))
    assert np.array_equal(got['FN_call'], fit['call1_obs0']
        / (fit['call1_obs1'] + fit['call1_obs0']))
    assert np.array_equal(got['FP_call'], (S * fit['n1'] - fit['call1_obs1'])
        / (S * n_obs - fit['call1_obs1'] - fit['call1_obs0']))
    mean = fit['sum_ll'] / S
    assert np.array_equal(got['sd_ll'], np.sqrt(np.maximum(
        fit['sum_ll2'] / S - mean ** 2, 0) * S / (S - 1)))
    assert np.array_equal(got['mean_ll_per_obs'], mean / n_obs)


def test_handle_with_the_method_is_asked():
    data, a, params, FN, FP = small_case()
    fit = postproc.host_mutation_fit(data, a, params, FN, FP)
    hint = a[1]

    class Handle(FakePosterior):
        calls = 0

        def mutation_fit(self, d, trace, fn, fp, order=None):
            assert np.array_equal(d, postproc.data_codes(data))
            assert trace is params and fn is FN and fp is FP
            assert order is hint
            self.calls += 1
            # (marked, so that the host loop cannot have made them)
            return (fit['sum_ll'] - 1, fit['sum_ll2'], fit['efn'],
                fit['efp'], fit['eg1'] + 1, fit['call1_obs1'],
                fit['call1_obs0'], None)
    post = Handle(a)
    got = postproc.mutation_fit(post, data, a, params, FN, FP, order=hint)
    assert post.calls == 1
    S = a.shape[0]
    assert np.array_equal(got['mean_ll'], (fit['sum_ll'] - 1) / S)
    assert np.array_equal(got['FN_model'], fit['efn'] / (fit['eg1'] + 1))
    assert np.array_equal(got['eg1'], fit['eg1'] + 1)
    assert np.array_equal(got['n_obs'], fit['n1'] + fit['n0'])


@pytest.fixture
def host_posterior(monkeypatch):
    monkeypatch.setattr(_lib, 'Posterior', FakePosterior)


def same(got, want):
    assert got.keys() == want.keys()
    for key in want:
        if key != 'total':
            assert np.array_equal(got[key], want[key], equal_nan=True), key
    assert got['total'].keys() == want['total'].keys()
    for key, val in want['total'].items():
        assert got['total'][key] == val or (val != val
            and got['total'][key] != got['total'][key]), key


def test_posterior_estimate_mutations(golden_dir, tmp_path, host_posterior):
    d, case, results = load_case(golden_dir, 'fixture', tmp_path / 'ref')
    data = bio.load_data(os.path.join(d, 'input.tsv'))
    plain = postproc.posterior_estimate(results, data)
    assert plain.keys() == postproc.posterior_estimate(results, data,
        mutations=False).keys()
    inf = postproc.posterior_estimate(results, data, mutations=True)
    assert sorted(set(inf) - set(plain)) == ['mutation_fit']
    for key in plain:
        assert np.array_equal(inf[key], plain[key]), key
    pooled = postproc.concat_chain_results(results)
    want = postproc.mutation_fit(None, data, pooled['assignments'],
        pooled['params'], pooled['FN'], pooled['FP'])
    same(inf['mutation_fit'], want)
    every = postproc.posterior_estimate(results, data, support=True,
        cells=True, fit=True, mutations=True)
    assert sorted(set(every) - set(plain)) == ['cell_genotypes', 'fit',
        'mutation_fit', 'support']


def test_save_outputs_writes_the_two_files(golden_dir, tmp_path,
        host_posterior, capsys):
    d, case, results = load_case(golden_dir, 'fixture', tmp_path / 'ref')
    out = tmp_path / 'out'
    args, names = save(d, case, results, out, posterior_mutations=True)
    assert capsys.readouterr().out == ''            # verbosity 0
    data = bio.load_data(os.path.join(d, 'input.tsv'))
    pooled = postproc.concat_chain_results(results)
    want = postproc.mutation_fit(None, data, pooled['assignments'],
        pooled['params'], pooled['FN'], pooled['FP'])
    M = data.shape[1]
    S = pooled['ML'].size
    rows = [ln.split('\t') for ln in
        (out / NEW_FILES[0]).read_text().splitlines()]
    assert rows[0] == ['mutation'] + COLUMNS
    assert len(rows) == M + 1 and all(len(r) == len(rows[0]) for r in rows)
    assert [r[0] for r in rows[1:]] == [str(x) for x in names[1].tolist()]
    for col, key in enumerate(COLUMNS, 1):
        got = [r[col] for r in rows[1:]]
        if col <= 3:
            assert got == [str(x) for x in want[key].tolist()], key
            continue
        digits = 8 if key in ('FP_model', 'FP_call') else 4
        assert all(re.fullmatch(r'-?\d+\.\d{%d}|nan' % digits, x)
            for x in got), key
        assert got == [f'{x:.{digits}f}' for x in want[key].tolist()], key
    lines = (out / NEW_FILES[1]).read_text().splitlines()
    assert [ln.split(': ')[0] for ln in lines] == ['samples', 'mutations',
        'observations', 'FN_model', 'FP_model', 'FN_call', 'FP_call', 'FN',
        'FP', 'worst_mutations', 'highest_FN']
    model = dict(ln.split(': ', 1) for ln in lines)
    total = want['total']
    assert int(model['samples']) == S == total['samples']
    assert int(model['mutations']) == M
    assert int(model['observations']) == int((~np.isnan(data)).sum())
    for key in ('FN_model', 'FN_call', 'FN'):
        assert model[key] == f'{total[key]:.4f}', key
    for key in ('FP_model', 'FP_call'):
        assert model[key] == f'{total[key]:.8f}', key
    assert 0 < total['FN_model'] < 1 and 0 < total['FP_model'] < 1
    per_obs = want['mean_ll_per_obs']
    seen = np.flatnonzero(want['n_obs'] > 0)
    order = seen[np.argsort(per_obs[seen], kind='stable')[:10]]
    worst = [p.rsplit(':', 1) for p in model['worst_mutations'].split(' ')]
    assert len(worst) == min(10, seen.size)
    assert [w[0] for w in worst] == [str(names[1][m]) for m in order]
    assert [w[1] for w in worst] == [f'{per_obs[m]:.4f}' for m in order]
    carried = np.flatnonzero(want['eg1'] / S >= 1)
    order = carried[np.argsort(-want['FN_model'][carried],
        kind='stable')[:10]]
    assert order.size
    high = [p.rsplit(':', 1) for p in model['highest_FN'].split(' ')]
    assert [h[0] for h in high] == [str(names[1][m]) for m in order]
    assert [h[1] for h in high] \
        == [f'{want["FN_model"][m]:.4f}' for m in order]
    assert 'posterior_mutations: True\n' in (out / 'args.txt').read_text()
    # everything else is what a run without the flag writes, byte for byte
    plain, false = tmp_path / 'plain', tmp_path / 'false'
    save(d, case, results, plain)
    save(d, case, results, false, posterior_mutations=False)
    for other in (plain, false):
        assert sorted(os.listdir(other)) \
            == sorted(set(os.listdir(out)) - set(NEW_FILES))
        for name in os.listdir(other):
            if name != 'args.txt':
                assert (other / name).read_bytes() \
                    == (out / name).read_bytes(), name
        assert 'posterior_mutations' not in (other / 'args.txt').read_text()
    # a namespace from before the flag existed (no such attribute) and one
    # that parsed it write the same directory
    assert (plain / 'args.txt').read_bytes() \
        == (false / 'args.txt').read_bytes()


def test_mutations_without_names_are_numbered(tmp_path):
    data, a, params, FN, FP = small_case()
    t = postproc.mutation_fit(None, data, a, params, FN, FP)
    paths = bio.save_mutation_fit(str(tmp_path), 'mean', 'posterior', t)
    assert [os.path.basename(p) for p in paths] == list(NEW_FILES)
    with open(paths[0]) as f:
        rows = [ln.split('\t') for ln in f.read().splitlines()]
    assert [r[0] for r in rows[1:]] == [str(m) for m in range(data.shape[1])]


def test_verbose_run_prints_one_line(golden_dir, tmp_path, host_posterior,
        capsys):
    d, case, results = load_case(golden_dir, 'fixture', tmp_path / 'ref')
    data, names = bio.load_data(os.path.join(d, 'input.tsv'), get_names=True)
    out = tmp_path / 'out'
    out.mkdir()
    args = run_BnpC.parse_args(['d.csv', '-pm', '-v', '1', '-e', 'posterior'])
    run_BnpC.save_outputs(args, results, data, str(out), names)
    lines = [ln for ln in capsys.readouterr().out.splitlines()
        if ln.startswith('posterior mutations: ')]
    assert len(lines) == 1
    assert re.fullmatch(r'posterior mutations: FN_model \d\.\d{4}, FP_model '
        r'\d\.\d{6} \(run: FN \d\.\d{4}, FP \d\.\d{6}\)', lines[0])
    model = dict(ln.split(': ', 1) for ln in
        (out / NEW_FILES[1]).read_text().splitlines())
    assert f'FN_model {model["FN_model"]},' in lines[0]
    assert f'(run: FN {model["FN"]},' in lines[0]


def test_flag_and_its_check():
    """(the input path is a required argument: `d.csv` stands for it)"""
    args = run_BnpC.parse_args(['d.csv'])
    assert args.posterior_mutations is False
    assert 'posterior_mutations' not in vars(args)
    run_BnpC.check_args(args)
    for flag in ('-pm', '--posterior_mutations'):
        args = run_BnpC.parse_args(['d.csv', flag])
        assert vars(args)['posterior_mutations'] is True
        run_BnpC.check_args(args)
    run_BnpC.check_args(run_BnpC.parse_args('d.csv -pm -e ML posterior'
        .split()))
    for ests in ('ML', 'ML MAP'):
        args = run_BnpC.parse_args(['d.csv', '-pm', '-e'] + ests.split())
        with pytest.raises(SystemExit, match='posterior'):
            run_BnpC.check_args(args)
        # main() stops there: before the input is looked at
        with pytest.raises(SystemExit, match='--posterior_mutations'):
            run_BnpC.main(args)


def test_binding_and_header_list_the_entry_points():
    for name in ('bnpc_post_mutation_fit', 'bnpc_post_mutation_fit_times'):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    assert hasattr(_lib.Posterior, 'mutation_fit')
    assert hasattr(_lib.Posterior, 'mutation_fit_times')
    with open(os.path.join(ROOT, 'include', 'bnpc_hip.h')) as f:
        header = f.read()
    assert re.search(r'\bint bnpc_post_mutation_fit\(bnpc_post \*post, '
        r'const uint8_t \*codes', header)
    assert re.search(r'\bint bnpc_post_mutation_fit_times\(bnpc_post \*post',
        header)
    with open(os.path.join(ROOT, 'bnpc_amd', 'csrc', 'bnpc_post_passes.hip')) as f:
        source = f.read()
    assert f'#define MF_ROWS {_lib.MUT_FIT_ROWS} ' in source
    assert _lib.ABI_VERSION == 12
