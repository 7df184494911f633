"""Per-cell posterior genotypes (-pg): the host side.
postproc.host_cell_genotypes against a triple loop over its definition, the
mean / sd / prob tables against NumPy on the gathered samples x cells x
mutations array, the fall-back of postproc.cell_genotypes to the host loop,
the three tables save_outputs writes, and the flag.  CPU only: the clustering
handle is the NumPy stand-in of tests/fake_device.py, which has no
cell_genotypes method."""
import os
import re

import numpy as np
import pytest

import run_BnpC
from bnpc_amd import _lib, postproc
from bnpc_amd import io as bio
from fake_device import FakePosterior
from test_outputs import load_case
from test_support import save

NEW_FILES = tuple(f'genotypes_cell_{kind}_posterior_mean.tsv'
    for kind in ('prob', 'cont', 'sd'))


def small_case():
    """S, N, M = 5, 6, 4; labels from {0, 3, 5} (not compact), a sample with
    one cluster, one with all three; entries of exactly 0.5, 0 and 1"""
    S, N, M = 5, 6, 4
    rng = np.random.RandomState(56)
    a = np.array([0, 3, 5])[rng.randint(0, 3, (S, N))]
    a[1] = 3
    a[2] = [5, 0, 3, 3, 0, 5]
    params = rng.random_sample((S, 3, M)).astype(np.float32)
    params[0, 0, 0] = 0.5
    params[2, :, 1] = 0.5
    params[3, 1, 2] = 0.0
    params[4, 0, 3] = 1.0
    params[1, 0, :] = [0.5, np.nextafter(np.float32(0.5), np.float32(1)),
        np.nextafter(np.float32(0.5), np.float32(0)), 0.75]
    return a, params


def gathered(a, params):
    """G[s][i][m]: the parameter of cell i's cluster in sample s, float64"""
    S, N = a.shape
    G = np.empty((S, N, params.shape[2]))
    for s in range(S):
        present = sorted(set(a[s].tolist()))
        for i in range(N):
            G[s, i] = params[s][present.index(a[s, i])]
    return G


def test_host_loop_is_the_definition():
    a, params = small_case()
    S, N = a.shape
    M = params.shape[2]
    sum1, sum2, ones = postproc.host_cell_genotypes(a, params)
    assert sum1.dtype == sum2.dtype == np.float64 and ones.dtype == np.uint32
    assert sum1.shape == sum2.shape == ones.shape == (N, M)
    for i in range(N):
        for m in range(M):
            t1, t2, n = 0.0, 0.0, 0
            for s in range(S):
                row = sorted(set(a[s].tolist())).index(a[s, i])
                v = float(params[s, row, m])
                t1 += v
                t2 += v * v
                n += int(np.round(v) == 1)
            assert sum1[i, m] == t1 and sum2[i, m] == t2 and ones[i, m] == n
    # sample 2 puts 0.5 under every cell at mutation 1: never counted
    G = gathered(a, params)
    assert (G == 0.5).sum() >= N + 2
    assert np.array_equal(ones, (G > 0.5).sum(axis=0))
    assert not np.array_equal(ones, (G >= 0.5).sum(axis=0))


def test_float64_padded_trace_gives_the_same_bits():
    a, params = small_case()
    wide = np.pad(params.astype(np.float64), [(0, 0), (0, 2), (0, 0)])
    for got, want in zip(postproc.host_cell_genotypes(a, wide),
            postproc.host_cell_genotypes(a, params)):
        assert np.array_equal(got, want)


def test_tables_against_numpy():
    """float64 sums of at most a few dozen values in [0, 1]: 1e-12"""
    rng = np.random.RandomState(7)
    for a, params in (small_case(), (rng.randint(0, 40, (30, 17)) * 3,
            rng.random_sample((30, 17, 9)).astype(np.float32))):
        G = gathered(a, params)
        t = postproc.cell_genotypes(None, a, params)
        assert sorted(t) == ['mean', 'prob', 'sd']
        assert np.abs(t['mean'] - G.mean(axis=0)).max() <= 1e-12
        assert np.abs(t['sd'] - G.std(axis=0)).max() <= 1e-12
        assert np.abs(t['prob'] - (np.round(G) == 1).mean(axis=0)).max() \
            <= 1e-12
        assert (t['sd'] >= 0).all()


def test_sd_of_a_constant_is_zero_not_nan():
    a = np.zeros((3, 2), dtype=int)
    params = np.full((3, 1, 2), 0.1, dtype=np.float32)
    t = postproc.cell_genotypes(None, a, params)
    assert np.isfinite(t['sd']).all() and t['sd'].max() < 1e-7


def test_handle_without_the_method_takes_the_host_loop():
    a, params = small_case()
    post = FakePosterior(a)
    assert not hasattr(post, 'cell_genotypes')
    got = postproc.cell_genotypes(post, a, params)
    sum1, sum2, ones = postproc.host_cell_genotypes(a, params)
    S = a.shape[0]
    mean = sum1 / S
    assert np.array_equal(got['mean'], mean)
    assert np.array_equal(got['sd'],
        np.sqrt(np.maximum(sum2 / S - mean * mean, 0)))
    assert np.array_equal(got['prob'], ones / S)


def test_handle_with_the_method_is_asked():
    a, params = small_case()
    want = postproc.host_cell_genotypes(a, params)

    class Handle:
        calls = 0

        def cell_genotypes(self, trace):
            assert trace is params
            self.calls += 1
            return want
    post = Handle()
    got = postproc.cell_genotypes(post, a, params)
    assert post.calls == 1
    assert np.array_equal(got['prob'], want[2] / a.shape[0])


@pytest.fixture
def host_posterior(monkeypatch):
    monkeypatch.setattr(_lib, 'Posterior', FakePosterior)


def test_posterior_estimate_cells(golden_dir, tmp_path, host_posterior):
    d, case, results = load_case(golden_dir, 'fixture', tmp_path / 'ref')
    data = bio.load_data(os.path.join(d, 'input.tsv'))
    plain = postproc.posterior_estimate(results, data)
    assert plain.keys() == postproc.posterior_estimate(results, data,
        cells=False).keys()
    inf = postproc.posterior_estimate(results, data, cells=True)
    assert sorted(set(inf) - set(plain)) == ['cell_genotypes']
    for key in plain:
        assert np.array_equal(inf[key], plain[key]), key
    pooled = postproc.concat_chain_results(results)
    want = postproc.cell_genotypes(None, pooled['assignments'],
        pooled['params'])
    for key in ('mean', 'sd', 'prob'):
        assert np.array_equal(inf['cell_genotypes'][key], want[key]), key
    both = postproc.posterior_estimate(results, data, support=True,
        cells=True)
    assert sorted(set(both) - set(plain)) == ['cell_genotypes', 'support']


def test_save_outputs_writes_the_three_tables(golden_dir, tmp_path,
        host_posterior):
    d, case, results = load_case(golden_dir, 'fixture', tmp_path / 'ref')
    out = tmp_path / 'out'
    args, names = save(d, case, results, out, posterior_genotypes=True)
    pooled = postproc.concat_chain_results(results)
    want = postproc.cell_genotypes(None, pooled['assignments'],
        pooled['params'])
    N, M = want['mean'].shape
    for name, key in zip(NEW_FILES, ('prob', 'mean', 'sd')):
        rows = [ln.split('\t') for ln in
            (out / name).read_text().splitlines()]
        assert rows[0] == [''] + [str(x) for x in names[0].tolist()]
        assert [r[0] for r in rows[1:]] == [str(x) for x in names[1].tolist()]
        assert len(rows) == M + 1 and all(len(r) == N + 1 for r in rows)
        assert all(re.fullmatch(r'\d+\.\d{4}', x) for r in rows[1:]
            for x in r[1:])
        table = np.array([[float(x) for x in r[1:]] for r in rows[1:]])
        assert np.abs(table - want[key].T).max() <= 5e-5
    assert 'posterior_genotypes: True\n' in (out / 'args.txt').read_text()
    # everything else is what a run without the flag writes, byte for byte
    plain, false = tmp_path / 'plain', tmp_path / 'false'
    save(d, case, results, plain)
    save(d, case, results, false, posterior_genotypes=False)
    for other in (plain, false):
        assert sorted(os.listdir(other)) \
            == sorted(set(os.listdir(out)) - set(NEW_FILES))
        for name in os.listdir(other):
            if name != 'args.txt':
                assert (other / name).read_bytes() \
                    == (out / name).read_bytes(), name
        assert 'posterior_genotypes' not in (other / 'args.txt').read_text()


def test_flag_and_its_check():
    """(the input path is a required argument: `d.csv` stands for it)"""
    args = run_BnpC.parse_args(['d.csv'])
    assert args.posterior_genotypes is False
    assert 'posterior_genotypes' not in vars(args)
    run_BnpC.check_args(args)
    for flag in ('-pg', '--posterior_genotypes'):
        args = run_BnpC.parse_args(['d.csv', flag])
        assert vars(args)['posterior_genotypes'] is True
        run_BnpC.check_args(args)
    run_BnpC.check_args(run_BnpC.parse_args('d.csv -pg -e ML posterior'
        .split()))
    for ests in ('ML', 'ML MAP'):
        args = run_BnpC.parse_args(['d.csv', '-pg', '-e'] + ests.split())
        with pytest.raises(SystemExit, match='posterior'):
            run_BnpC.check_args(args)
        # main() stops there: before the input is looked at
        with pytest.raises(SystemExit, match='--posterior_genotypes'):
            run_BnpC.main(args)


def test_binding_and_header_list_the_entry_point():
    assert 'bnpc_post_cell_genotypes' in _lib.SIGNATURES
    assert hasattr(_lib.Posterior, 'cell_genotypes')
