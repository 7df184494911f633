"""Per-cell posterior fit and WAIC (-pf): the host side.
postproc.host_cell_fit against the oracle's likelihood of one cell, hand
computed cases, the pointwise matrix against the ML trace the chains recorded
themselves, the routing of postproc.cell_fit, the two files save_outputs
writes, and the flag.  CPU only: the clustering handle is the NumPy stand-in
of tests/fake_device.py, which has no cell_fit method."""
import os
import re

import numpy as np
import pytest

import run_BnpC
from bnpc_amd import _lib, postproc
from bnpc_amd import io as bio
from fake_device import FakePosterior
from oracle.likelihood import Likelihood
from test_outputs import load_case
from test_support import posterior_row, save

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FILES = ('cell_fit_posterior_mean.tsv', 'model_fit_posterior_mean.txt')
HEADER = ['cell', 'cluster', 'n_obs', 'mean_ll', 'sd_ll', 'lppd', 'p_waic',
    'mean_ll_per_obs']


class Emission(Likelihood):
    """the oracle's likelihood of rows of data under given error rates"""

    def __init__(self, FN, FP):
        self.FN, self.FP = FN, FP


def small_case(S=6, N=9, M=13, seed=11):
    """labels from {0, 4, 7} (not compact), a sample with one cluster;
    missing entries as NaN; error rates that differ in every sample"""
    rng = np.random.RandomState(seed)
    a = np.array([0, 4, 7])[rng.randint(0, 3, (S, N))]
    a[S // 2] = 4
    a[-1, :3] = [7, 0, 4]
    params = rng.random_sample((S, 3, M)).astype(np.float32)
    params[0, 0, 0], params[0, 1, 1], params[-1, 2, 2] = 0.0, 1.0, 0.5
    data = (rng.random_sample((N, M)) < 0.4).astype(np.float64)
    data[rng.random_sample((N, M)) < 0.25] = np.nan
    FN = rng.uniform(0.05, 0.4, S)
    FP = rng.uniform(1e-6, 1e-3, S)
    return data, a, params, FN, FP


def host_reduction(ll):
    """the per-cell reductions of the definition, one cell at a time"""
    S, N = ll.shape
    mean, m2, lme = np.empty(N), np.empty(N), np.empty(N)
    for i in range(N):
        acc = 0.0
        for s in range(S):
            acc += ll[s, i]
        mean[i] = acc / S
        dev, es, mx = 0.0, 0.0, ll[:, i].max()
        for s in range(S):
            dev += (ll[s, i] - mean[i]) ** 2
            es += np.exp(ll[s, i] - mx)
        m2[i] = dev
        lme[i] = mx + np.log(es) - np.log(S)
    return mean, m2, lme


def test_host_loop_against_the_oracle():
    """one likelihood evaluation of the project: rtol = atol = 1e-12
    (tests/test_gpu_parity.py)"""
    data, a, params, FN, FP = small_case()
    S, N = a.shape
    fit = postproc.host_cell_fit(data, a, params, FN, FP)
    assert sorted(fit) == ['ll', 'lme', 'm2', 'mean', 'n_obs']
    assert fit['ll'].shape == (S, N) and fit['ll'].dtype == np.float64
    assert fit['n_obs'].dtype == np.int64
    assert np.array_equal(fit['n_obs'], (~np.isnan(data)).sum(axis=1))
    want = np.empty((S, N))
    for s in range(S):
        present = sorted(set(a[s].tolist()))
        om = Emission(FN[s], FP[s])
        for i in range(N):
            theta = params[s][present.index(a[s, i])]
            assert theta.dtype == np.float32
            want[s, i] = om._calc_ll(data[[i]], theta)[0]
    np.testing.assert_allclose(fit['ll'], want, rtol=1e-12, atol=1e-12)
    assert (fit['ll'] < 0).all()
    mean, m2, lme = host_reduction(fit['ll'])
    assert np.array_equal(fit['mean'], mean)
    assert np.array_equal(fit['m2'], m2)
    assert np.array_equal(fit['lme'], lme)
    # swapped error rates are another model
    swapped = postproc.host_cell_fit(data, a, params, FP, FN)['ll']
    assert np.abs(swapped - want).min() > 1e-3


def test_missing_as_3_and_codes_give_the_same_bits():
    data, a, params, FN, FP = small_case()
    want = postproc.host_cell_fit(data, a, params, FN, FP)
    threes = np.where(np.isnan(data), 3, data)
    for other in (threes, threes.astype(np.uint8), threes.astype(np.int64)):
        got = postproc.host_cell_fit(other, a, params, FN, FP)
        for key in want:
            assert np.array_equal(got[key], want[key]), key
    bad = threes.copy()
    bad[2, 3] = 2
    with pytest.raises(ValueError, match='missing'):
        postproc.host_cell_fit(bad, a, params, FN, FP)


def test_hand_computed_cases():
    """one cluster with parameter 1/2: every observed entry has likelihood
    (1 - FN + FP) / 2 as a 1 and (FN + 1 - FP) / 2 as a 0"""
    S, M = 4, 5
    data = np.array([[np.nan] * M, [1, 1, 0, np.nan, 0], [0] * M, [1] * M])
    a = np.zeros((S, 4), dtype=int)
    params = np.full((S, 1, M), 0.5, dtype=np.float32)
    FN = np.array([0.25, 0.25, 0.5, 0.125])
    FP = np.array([0.25, 0.125, 0.5, 0.125])
    fit = postproc.host_cell_fit(data, a, params, FN, FP)
    l1 = np.log(0.5 * (1 - FN) + 0.5 * FP)
    l0 = np.log(0.5 * FN + 0.5 * (1 - FP))
    assert np.array_equal(fit['n_obs'], [0, 4, 5, 5])
    assert np.array_equal(fit['ll'][:, 0], np.zeros(S))
    np.testing.assert_allclose(fit['ll'][:, 1], 2 * l1 + 2 * l0, rtol=1e-14)
    np.testing.assert_allclose(fit['ll'][:, 2], 5 * l0, rtol=1e-14)
    np.testing.assert_allclose(fit['ll'][:, 3], 5 * l1, rtol=1e-14)
    # the missing-only cell
    assert fit['lme'][0] == 0 and fit['m2'][0] == 0 and fit['mean'][0] == 0
    t = postproc.cell_fit(None, data, a, params, FN, FP)
    assert t['mean_ll_per_obs'][0] == 0 and t['sd_ll'][0] == 0
    for key, val in t.items():
        if key != 'total':
            assert val.shape == (4,) and np.isfinite(val).all(), key
    # lme is the log of the mean likelihood
    np.testing.assert_allclose(fit['lme'],
        np.log(np.exp(fit['ll']).mean(axis=0)), rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(t['p_waic'], fit['ll'].var(axis=0, ddof=1),
        rtol=1e-12, atol=1e-15)
    total = t['total']
    assert total['samples'] == S and total['cells'] == 4
    assert total['observations'] == 14
    assert total['lppd'] == t['lppd'].sum()
    assert total['p_waic'] == t['p_waic'].sum()
    assert total['waic'] == -2 * (total['lppd'] - total['p_waic'])


def test_one_sample():
    data, a, params, FN, FP = small_case(S=1)
    t = postproc.cell_fit(None, data, a, params, FN, FP)
    assert not t['sd_ll'].any() and not t['p_waic'].any()
    assert t['total']['p_waic'] == 0
    fit = postproc.host_cell_fit(data, a, params, FN, FP)
    assert np.array_equal(t['lppd'], fit['ll'][0])
    assert np.array_equal(t['mean_ll'], fit['ll'][0])
    assert all(np.isfinite(v).all() for k, v in t.items() if k != 'total')


def test_matrix_sums_to_the_chains_own_trace(golden_dir, tmp_path):
    """The recorded ML of a step is the likelihood of all the data under that
    step's clusters, parameters and error rates: the row sums of ll.  Every
    term is <= 0, so two orders of summation differ by at most
    N * M * 2**-52 relative - a wrong rank, another sample's error rates or
    an offset against the burn-in are far outside."""
    d, case, results = load_case(golden_dir, 'fixture', tmp_path / 'ref')
    data = bio.load_data(os.path.join(d, 'input.tsv'))
    pooled = postproc.concat_chain_results(results)
    fit = postproc.host_cell_fit(data, pooled['assignments'],
        pooled['params'], pooled['FN'], pooled['FP'])
    S = pooled['ML'].size
    assert S > 60 and fit['ll'].shape == (S, data.shape[0])
    np.testing.assert_allclose(fit['ll'].sum(axis=1), pooled['ML'],
        rtol=data.size * 2.0 ** -52, atol=0)
    # (the check can fail: one step further it does)
    assert not np.allclose(fit['ll'].sum(axis=1)[1:], pooled['ML'][:-1],
        rtol=1e-9, atol=0)


def test_handle_without_the_method_takes_the_host_loop():
    data, a, params, FN, FP = small_case()
    post = FakePosterior(a)
    assert not hasattr(post, 'cell_fit')
    got = postproc.cell_fit(post, data, a, params, FN, FP)
    fit = postproc.host_cell_fit(data, a, params, FN, FP)
    S = a.shape[0]
    assert np.array_equal(got['mean_ll'], fit['mean'])
    assert np.array_equal(got['sd_ll'], np.sqrt(fit['m2'] / (S - 1)))
    assert np.array_equal(got['p_waic'], fit['m2'] / (S - 1))
    assert np.array_equal(got['lppd'], fit['lme'])
    assert np.array_equal(got['n_obs'], fit['n_obs'])
    assert np.array_equal(got['mean_ll_per_obs'], fit['mean'] / fit['n_obs'])


def test_handle_with_the_method_is_asked():
    data, a, params, FN, FP = small_case()
    fit = postproc.host_cell_fit(data, a, params, FN, FP)

    class Handle(FakePosterior):
        calls = 0

        def cell_fit(self, d, trace, fn, fp):
            assert d is data and trace is params and fn is FN and fp is FP
            self.calls += 1
            # (marked, so that the host loop cannot have made them)
            return fit['mean'] - 1, fit['m2'], fit['lme'], None
    post = Handle(a)
    got = postproc.cell_fit(post, data, a, params, FN, FP)
    assert post.calls == 1
    assert np.array_equal(got['mean_ll'], fit['mean'] - 1)
    assert np.array_equal(got['lppd'], fit['lme'])
    assert np.array_equal(got['n_obs'], fit['n_obs'])


@pytest.fixture
def host_posterior(monkeypatch):
    monkeypatch.setattr(_lib, 'Posterior', FakePosterior)


def test_posterior_estimate_fit(golden_dir, tmp_path, host_posterior):
    d, case, results = load_case(golden_dir, 'fixture', tmp_path / 'ref')
    data = bio.load_data(os.path.join(d, 'input.tsv'))
    plain = postproc.posterior_estimate(results, data)
    assert plain.keys() == postproc.posterior_estimate(results, data,
        fit=False).keys()
    inf = postproc.posterior_estimate(results, data, fit=True)
    assert sorted(set(inf) - set(plain)) == ['fit']
    for key in plain:
        assert np.array_equal(inf[key], plain[key]), key
    pooled = postproc.concat_chain_results(results)
    want = postproc.cell_fit(None, data, pooled['assignments'],
        pooled['params'], pooled['FN'], pooled['FP'])
    assert inf['fit'].keys() == want.keys()
    for key in want:
        if key != 'total':
            assert np.array_equal(inf['fit'][key], want[key]), key
    assert inf['fit']['total'] == want['total']
    every = postproc.posterior_estimate(results, data, support=True,
        cells=True, fit=True)
    assert sorted(set(every) - set(plain)) == ['cell_genotypes', 'fit',
        'support']


def test_save_outputs_writes_the_two_files(golden_dir, tmp_path,
        host_posterior, capsys):
    d, case, results = load_case(golden_dir, 'fixture', tmp_path / 'ref')
    out = tmp_path / 'out'
    args, names = save(d, case, results, out, posterior_fit=True)
    assert capsys.readouterr().out == ''            # verbosity 0
    data = bio.load_data(os.path.join(d, 'input.tsv'))
    pooled = postproc.concat_chain_results(results)
    want = postproc.cell_fit(None, data, pooled['assignments'],
        pooled['params'], pooled['FN'], pooled['FP'])
    N = data.shape[0]
    rows = [ln.split('\t') for ln in
        (out / NEW_FILES[0]).read_text().splitlines()]
    assert rows[0] == HEADER
    assert len(rows) == N + 1 and all(len(r) == len(HEADER) for r in rows)
    assert [r[0] for r in rows[1:]] == [str(x) for x in names[0].tolist()]
    assert [int(r[1]) for r in rows[1:]] \
        == posterior_row(out / 'assignment.txt')
    assert [int(r[2]) for r in rows[1:]] == want['n_obs'].tolist()
    for col, key in enumerate(HEADER[3:], 3):
        assert all(re.fullmatch(r'-?\d+\.\d{4}', r[col]) for r in rows[1:])
        assert [r[col] for r in rows[1:]] \
            == [f'{x:.4f}' for x in want[key].tolist()], key
    lines = (out / NEW_FILES[1]).read_text().splitlines()
    keys = [ln.split(': ')[0] for ln in lines]
    assert keys == ['samples', 'cells', 'observations', 'lppd', 'p_waic',
        'WAIC', 'worst_cells']
    model = dict(ln.split(': ', 1) for ln in lines)
    total = want['total']
    assert int(model['samples']) == pooled['ML'].size == total['samples']
    assert int(model['cells']) == N
    assert int(model['observations']) == int((~np.isnan(data)).sum())
    for key in ('lppd', 'p_waic', 'WAIC'):
        assert re.fullmatch(r'-?\d+\.\d{4}', model[key]), key
        assert model[key] == f'{total[key.lower()]:.4f}'
    # to the printed digits: three roundings of 5e-5, two of them doubled
    assert abs(float(model['WAIC']) + 2 * (float(model['lppd'])
        - float(model['p_waic']))) <= 2.5e-4 + 1e-9
    worst = [pair.rsplit(':', 1) for pair in model['worst_cells'].split(' ')]
    assert len(worst) == 10
    order = np.argsort(want['mean_ll_per_obs'], kind='stable')[:10]
    assert [w[0] for w in worst] == [str(names[0][i]) for i in order]
    assert [w[1] for w in worst] \
        == [f'{want["mean_ll_per_obs"][i]:.4f}' for i in order]
    assert 'posterior_fit: True\n' in (out / 'args.txt').read_text()
    # everything else is what a run without the flag writes, byte for byte
    plain, false = tmp_path / 'plain', tmp_path / 'false'
    save(d, case, results, plain)
    save(d, case, results, false, posterior_fit=False)
    for other in (plain, false):
        assert sorted(os.listdir(other)) \
            == sorted(set(os.listdir(out)) - set(NEW_FILES))
        for name in os.listdir(other):
            if name != 'args.txt':
                assert (other / name).read_bytes() \
                    == (out / name).read_bytes(), name
        assert 'posterior_fit' not in (other / 'args.txt').read_text()


def test_verbose_run_prints_one_line(golden_dir, tmp_path, host_posterior,
        capsys):
    d, case, results = load_case(golden_dir, 'fixture', tmp_path / 'ref')
    data, names = bio.load_data(os.path.join(d, 'input.tsv'), get_names=True)
    out = tmp_path / 'out'
    out.mkdir()
    args = run_BnpC.parse_args(['d.csv', '-pf', '-v', '1', '-e', 'posterior'])
    run_BnpC.save_outputs(args, results, data, str(out), names)
    lines = [ln for ln in capsys.readouterr().out.splitlines()
        if ln.startswith('posterior fit: ')]
    assert len(lines) == 1
    model = dict(ln.split(': ', 1) for ln in
        (out / NEW_FILES[1]).read_text().splitlines())
    assert lines[0] == (f'posterior fit: WAIC {model["WAIC"]}, lppd '
        f'{model["lppd"]}, p_waic {model["p_waic"]}')


def test_flag_and_its_check():
    """(the input path is a required argument: `d.csv` stands for it)"""
    args = run_BnpC.parse_args(['d.csv'])
    assert args.posterior_fit is False
    assert 'posterior_fit' not in vars(args)
    run_BnpC.check_args(args)
    for flag in ('-pf', '--posterior_fit'):
        args = run_BnpC.parse_args(['d.csv', flag])
        assert vars(args)['posterior_fit'] is True
        run_BnpC.check_args(args)
    run_BnpC.check_args(run_BnpC.parse_args('d.csv -pf -e ML posterior'
        .split()))
    for ests in ('ML', 'ML MAP'):
        args = run_BnpC.parse_args(['d.csv', '-pf', '-e'] + ests.split())
        with pytest.raises(SystemExit, match='posterior'):
            run_BnpC.check_args(args)
        # main() stops there: before the input is looked at
        with pytest.raises(SystemExit, match='--posterior_fit'):
            run_BnpC.main(args)


def test_binding_and_header_list_the_entry_point():
    assert 'bnpc_post_cell_fit' in _lib.SIGNATURES
    assert hasattr(_lib.Posterior, 'cell_fit')
    with open(os.path.join(ROOT, 'include', 'bnpc_hip.h')) as f:
        header = f.read()
    assert re.search(r'\bint bnpc_post_cell_fit\(bnpc_post \*post, '
        r'const uint8_t \*codes', header)
    assert _lib.ABI_VERSION == 12
