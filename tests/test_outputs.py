"""The CLI's genotype tables and -tc / -td metrics against the reference's own
writers (tests/golden/make_output_golden.py -> outputs.npz: dpmmIO.save_geno,
save_v_measure, save_ARI, save_hamming_dist on small runs) and against
scikit-learn.  CPU only: the posterior's device passes are replaced by the
exact NumPy stand-in of tests/fake_device.py."""
import argparse
import json
import os

import numpy as np
import pytest

from bnpc_amd import _lib, postproc
from bnpc_amd import io as bio

CASES = ('fixture', 'fixture_sc', 'named', 'learned', 'square')
WRITTEN = ('genotypes_', 'V_measure.txt', 'ARI.txt', 'hammingDist.txt')


def load_case(golden_dir, name, dest):
    """Case `name` of outputs.npz unpacked into the directory dest: its input
    files and the files the reference wrote; (dest, case, results)."""
    g = np.load(os.path.join(golden_dir, 'outputs.npz'))
    os.makedirs(dest, exist_ok=True)
    for key in g.files:
        case_name, f = key.split('/')
        if case_name == name and '.' in f:
            with open(os.path.join(dest, f), 'wb') as fh:
                fh.write(g[key].tobytes())
    with open(os.path.join(dest, 'case.json')) as f:
        case = json.load(f)
    results = []
    for i in range(case['chains']):
        r = {k: g[f'{name}/r{i}_{k}'] for k in ('assignments', 'params',
            'DP_alpha', 'FN', 'FP', 'ML', 'MAP')}
        r['burn_in'] = int(g[f'{name}/r{i}_burn_in'])
        results.append(r)
    return str(dest), case, results


def golden_files(d):
    return sorted(f for f in os.listdir(d) if f.startswith(WRITTEN))


@pytest.fixture
def host_posterior(monkeypatch):
    from fake_device import FakePosterior
    monkeypatch.setattr(_lib, 'Posterior', FakePosterior)


def run_save_outputs(d, case, results, out_dir, tc=True, td=True):
    import run_BnpC
    data, names = bio.load_data(os.path.join(d, 'input.tsv'), get_names=True)
    args = argparse.Namespace(estimator=case['estimator'],
        single_chains=case['single_chains'], verbosity=0, transpose=True,
        true_clusters=os.path.join(d, 'true_clusters.txt') if tc else '',
        true_data=os.path.join(d, 'true_data.tsv') if td else '')
    run_BnpC.save_outputs(args, results, data, str(out_dir), names)


@pytest.mark.parametrize('name', CASES)
def test_save_outputs_writes_the_references_files(name, golden_dir, tmp_path,
        host_posterior):
    d, case, results = load_case(golden_dir, name, tmp_path / 'ref')
    out = tmp_path / 'out'
    out.mkdir()
    run_save_outputs(d, case, results, out)
    want = golden_files(d)
    assert want and golden_files(out) == want
    for f in want:
        with open(os.path.join(d, f), 'rb') as a, \
                open(os.path.join(out, f), 'rb') as b:
            got, ref = b.read(), a.read()
        if f.startswith('genotypes_'):
            assert got == ref, f
            continue
        # metric tables: the same rows; the scores are the reference's to
        # 1e-12 (on the reference's NumPy / SciPy the same bits - the log
        # and sum kernels differ in the last ulp between NumPy versions)
        got, ref = got.decode().splitlines(), ref.decode().splitlines()
        assert got[0] == ref[0] and len(got) == len(ref), f
        for g, r in zip(got[1:], ref[1:]):
            g, r = g.split('\t'), r.split('\t')
            assert g[:2] == r[:2], f
            assert abs(float(g[2]) - float(r[2])) <= 1e-12, (f, g, r)


def test_no_metric_files_without_truth(golden_dir, tmp_path, host_posterior):
    d, case, results = load_case(golden_dir, 'fixture', tmp_path / 'ref')
    out = tmp_path / 'out'
    out.mkdir()
    run_save_outputs(d, case, results, out, tc=False, td=False)
    written = golden_files(out)
    assert written and all(f.startswith('genotypes_') for f in written)
    for f in ('args.txt', 'assignment.txt', 'errors.txt'):
        assert os.path.exists(out / f)


def test_genotype_table_kinds(tmp_path):
    """All-integer values: only the 0/1 table, written from the values
    themselves; otherwise the 4-decimal table (half-to-even) as well."""
    values = np.array([[0., 1., 1.], [1., 0., 0.]])
    cols = np.array([1, 0, 0, 1])
    paths = bio.save_geno(str(tmp_path), 'mean', 'posterior', values, cols,
        [5, 2, 2, 5])
    assert [os.path.basename(p) for p in paths] == \
        ['genotypes_posterior_mean.tsv']
    assert open(paths[0]).read() == \
        '\t5\t2\t2\t5\n0\t1\t0\t0\t1\n1\t0\t1\t1\t0\n2\t0\t1\t1\t0\n'
    values = np.array([[0.00005, 0.5, 2.5, 0.123449999], [0.5001, 1., 0., 1.]])
    paths = bio.save_geno(str(tmp_path), 3, 'ML', values, np.array([1, 0]),
        [7, 1], names=['a', 'b', 'c', 'd'])
    assert [os.path.basename(p) for p in paths] == \
        ['genotypes_cont_ML_03.tsv', 'genotypes_ML_03.tsv']
    assert open(paths[0]).read() == \
        '\t7\t1\na\t0.5001\t0.0\nb\t1.0\t0.5\nc\t0.0\t2.5\nd\t1.0\t0.1234\n'
    assert open(paths[1]).read() == \
        '\t7\t1\na\t1\t0\nb\t1\t0\nc\t0\t2\nd\t1\t0\n'


def test_names_used_only_when_one_per_mutation(tmp_path):
    values = np.array([[0., 1.]])
    p = bio.save_geno(str(tmp_path), 'mean', 'MAP', values, np.zeros(2, int),
        [0, 0], names=np.array(['x', 'y', 'z'], dtype=object))
    assert open(p[0]).read() == '\t0\t0\n0\t0\t0\n1\t1\t1\n'


def labelings():
    rng = np.random.RandomState(0)
    out = []
    for n, kt, kp in ((10, 3, 4), (100, 5, 5), (1000, 30, 12), (7, 1, 3)):
        out.append((rng.randint(0, kt, n), rng.randint(0, kp, n)))
    t = rng.randint(0, 6, 300)
    perm = rng.permutation(6) * 17 + 1000           # permuted, non-contiguous
    out.append((t, perm[t]))
    out.append((t, np.where(t == 2, 5, t)))
    out.append((np.arange(50), rng.randint(0, 4, 50)))          # singletons
    out.append((np.arange(50), np.arange(50)[::-1]))
    out.append((np.zeros(40, int), rng.randint(0, 3, 40)))      # one cluster
    out.append((np.zeros(40, int), np.zeros(40, int)))
    out.append((rng.randint(0, 40, 50000), rng.randint(0, 55, 50000)))
    big = rng.randint(0, 3, 50000)
    out.append((big, np.where(rng.random_sample(50000) < .01, 3, big)))
    return out


@pytest.mark.parametrize('i', range(12))
def test_metrics_match_scikit_learn(i):
    sk = pytest.importorskip('sklearn.metrics')
    true, pred = labelings()[i]
    np.testing.assert_allclose(postproc.v_measure(pred, true),
        sk.v_measure_score(true, pred), rtol=0, atol=1e-12)
    np.testing.assert_allclose(postproc.adjusted_rand(pred, true),
        sk.adjusted_rand_score(true, pred), rtol=0, atol=1e-12)
    assert isinstance(postproc.adjusted_rand(pred, true), float)


def test_ari_pair_counts_do_not_overflow():
    """At 50 000 cells in two halves the pair products pass 2**63."""
    n = 50000
    true = np.repeat([0, 1], n // 2)
    pred = np.repeat([0, 1, 0, 1], n // 4)
    # exact: tp = 4 C(12500, 2) pairs, fp = fn = pairs split once
    score = postproc.adjusted_rand(pred, true)
    sk = pytest.importorskip('sklearn.metrics')
    np.testing.assert_allclose(score, sk.adjusted_rand_score(true, pred),
        rtol=0, atol=1e-12)


def read_metric(path):
    with open(path) as f:
        lines = f.read().splitlines()
    return lines[0], [ln.split('\t') for ln in lines[1:]]


def test_metrics_match_the_golden_files(golden_dir, tmp_path):
    for name in CASES:
        d, case, results = load_case(golden_dir, name, tmp_path / name)
        true = bio.load_txt(os.path.join(d, 'true_clusters.txt'))
        _, rows = read_metric(os.path.join(d, 'V_measure.txt'))
        _, rows_ari = read_metric(os.path.join(d, 'ARI.txt'))
        assign = read_assignments(d, case, results, rows)
        for (c, e, v), (_, _, a) in zip(rows, rows_ari):
            pred = assign[(c, e)]
            np.testing.assert_allclose(postproc.v_measure(pred, true),
                float(v), rtol=0, atol=1e-12)
            np.testing.assert_allclose(postproc.adjusted_rand(pred, true),
                float(a), rtol=0, atol=1e-12)


def read_assignments(d, case, results, rows):
    """(chain, estimator) -> the labels in the header of its genotype table"""
    out = {}
    for c, e, _ in rows:
        with open(os.path.join(d, f'genotypes_{e}_{c:0>2}.tsv')) as f:
            out[(c, e)] = [int(x) for x in f.readline().rstrip('\n')
                .split('\t')[1:]]
    return out


def test_hamming_orientation_square_and_nan():
    values = np.array([[1., 0., 0.9], [0.2, 1., 0.5]])      # K = 2, M = 3
    cols = np.array([0, 1, 1, 0])                            # N = 4
    called = np.round(values)[cols]                          # cells x muts
    truth = called.copy()
    truth[0, 0] = 0                  # one mismatch
    truth[1, 2] = np.nan             # missing truth: a mismatch
    assert postproc.hamming_similarity(values, cols, truth) == 1 - 2 / 12
    # square: the smaller count of both orientations
    values = np.array([[1., 0., 1.], [0., 1., 1.]])
    cols = np.array([0, 1, 1])
    called = np.round(values)[cols]
    assert postproc.hamming_similarity(values, cols, called) == 1.0
    assert postproc.hamming_similarity(values, cols, called.T) == 1.0
    t = called.T.copy()
    t[0, 0] = np.nan
    want = 1 - min(np.count_nonzero(called != t),
        np.count_nonzero(called.T != t)) / 9
    assert postproc.hamming_similarity(values, cols, t) == want
    # half-to-even: 0.5 calls 0, 1.5 calls 2
    assert postproc.hamming_similarity(np.array([[0.5, 1.5]]),
        np.array([0]), np.array([[0., 2.]])) == 1.0


POSTERIOR_FLAGS = {'-ps': 'posterior_support', '-pg': 'posterior_genotypes',
    '-pf': 'posterior_fit', '-pm': 'posterior_mutations',
    '-pd': 'posterior_doublets', '-pc': 'posterior_chains'}
FILES_PER_FLAG = {'-ps': 2, '-pg': 3, '-pf': 2, '-pm': 2, '-pd': 2, '-pc': 2}
SUMMARY_LINES = ['posterior fit', 'posterior mutations', 'posterior doublets',
    'posterior chains']


def listed(out):
    """the posterior flags of an output directory's args.txt"""
    return [ln.split(':')[0] for ln in (out / 'args.txt').read_text()
        .splitlines() if ln.startswith('posterior_')]


def test_all_posterior_flags_write_what_each_writes_alone(tmp_path,
        monkeypatch, capsys):
    """The run with every optional table of the posterior writes what the
    runs with one flag each write, lists the flags in args.txt and prints
    each summary line once.  Every pass takes its host loop (FakePosterior);
    the two chains are those of test_chain_agreement's command-line runs."""
    import run_BnpC
    from test_chain_agreement import ROOT, run_cli
    golden = os.path.join(ROOT, 'tests', 'golden', 'example_data.csv')
    _, results = run_cli(tmp_path, monkeypatch, 'chains', '-v', '0')
    data, names = bio.load_data(golden, get_names=True)

    def save(name, *flags):
        out = tmp_path / name
        out.mkdir()
        args = run_BnpC.parse_args([golden, '-n', '2', '-o', str(out),
            *flags])
        run_BnpC.save_outputs(args, results, data, str(out), names)
        return out

    plain = save('plain', '-v', '0')
    assert listed(plain) == []
    alone = {flag: save(flag[1:], flag, '-v', '0')
        for flag in POSTERIOR_FLAGS}
    capsys.readouterr()
    every = save('every', *POSTERIOR_FLAGS, '-v', '1')
    printed = capsys.readouterr().out.splitlines()

    union = set(os.listdir(plain))
    for flag, out in alone.items():
        new = set(os.listdir(out)) - set(os.listdir(plain))
        assert len(new) == FILES_PER_FLAG[flag], flag
        assert not new & union, flag
        union |= new
        assert listed(out) == [POSTERIOR_FLAGS[flag]]
        for name in os.listdir(out):
            if name != 'args.txt':
                assert (out / name).read_bytes() \
                    == (every / name).read_bytes(), (flag, name)
    assert set(os.listdir(every)) == union
    assert listed(every) == list(POSTERIOR_FLAGS.values())
    assert 'posterior_doublets: 0.05\n' in (every / 'args.txt').read_text()
    # `posterior: <n> clusters ...` is the estimator's own line
    assert [ln.split(':')[0] for ln in printed
        if ln.startswith('posterior ')] == SUMMARY_LINES
