#!/opt/conda/bin/python3.9
"""Golden output files (genotype tables, V-measure, ARI, Hamming), written by
the imported reference's own writers:

    /opt/conda/bin/python3.9 tests/golden/make_output_golden.py

Pinned functions (/root/reference/libs/dpmmIO.py): load_data :27-98,
load_txt :101-112, _infer_results :199-225, save_geno :491-511,
save_v_measure / save_ARI :514-530, save_hamming_dist :533-542.
Written to outputs.npz: per case, its inputs (input.tsv, true_clusters.txt,
true_data.tsv, case.json as `<case>/<file>` bytes, the chains' results as
`<case>/r<i>_<key>` arrays) and the files the reference wrote from them
(`<case>/<file>` bytes):
  fixture      the 60 x 40 posterior fixture (posterior.npz), all estimators
  fixture_sc   the same with -sc (ML / MAP per chain; the reference's
               per-chain posterior raises IndexError, utils.py:228-229)
  named        the fixture's data with row and column names
  learned      a learned-error run (CRP_learning_errors), 45 x 30
  square       a fixed-error run on 24 cells x 24 mutations (Hamming's
               orientation rule)
The true data carry missing entries (3) in every case."""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'outputs.npz')
sys.path.insert(0, REF)
sys.path.insert(0, HERE)

from libs.CRP import CRP  # noqa: E402
from libs.CRP_learning_errors import CRP_errors_learning  # noqa: E402
from libs.MCMC import MCMC  # noqa: E402
import libs.dpmmIO as rio  # noqa: E402

KEYS = ('assignments', 'params', 'DP_alpha', 'FN', 'FP', 'ML', 'MAP')


def synth_truth(seed, N, M, C, miss, FP_true=0.001, FN_true=0.1):
    """make_golden.synth, also returning the true clusters and genotypes"""
    rng = np.random.RandomState(seed)
    geno = (rng.random_sample((C, M)) < 0.3)
    z = rng.randint(0, C, N)
    X = geno[z]
    u = rng.random_sample((N, M))
    obs = np.where(X == 1, u >= FN_true, u < FP_true).astype(np.float64)
    obs[rng.random_sample((N, M)) < miss] = np.nan
    return obs, z, X.astype(np.float64)


def write_matrix(path, cells_x_muts, row_names=None, col_names=None):
    """mutations x cells, 3 for missing (the reference's input format)"""
    mat = np.where(np.isnan(cells_x_muts), 3, cells_x_muts).astype(int).T
    with open(path, 'w') as f:
        if col_names is not None:
            f.write('\t'.join(['mutation'] + list(col_names)) + '\n')
        for i, row in enumerate(mat):
            toks = [str(x) for x in row]
            if row_names is not None:
                toks = [row_names[i]] + toks
            f.write('\t'.join(toks) + '\n')


def run_chains(data, seeds, learned, steps=(80, 25)):
    results = []
    for seed in seeds:
        if learned:
            model = CRP_errors_learning(data, DP_alpha=[-1, -1],
                param_beta=[.25, .25], FP_mean=0.001, FP_sd=0.001,
                FN_mean=0.2, FN_sd=0.1)
            eup = .25
        else:
            model = CRP(data, DP_alpha=[-1, -1], param_beta=[.25, .25],
                FN_error=0.1, FP_error=0.001)
            eup = 0
        mcmc = MCMC(model, sm_prob=.33, dpa_prob=.25, error_prob=eup,
            sm_ratios=[.75, .25], sm_steps=3)
        with contextlib.redirect_stdout(io.StringIO()):
            mcmc.run(steps, seed, 1, 0, '', True)
        results.append(mcmc.get_results()[0])
    return results


def write_case(out, name, data, results, true_z, true_X, estimators, single,
        row_names=None, col_names=None, seed=0):
    d = tempfile.mkdtemp()
    write_matrix(os.path.join(d, 'input.tsv'), data, row_names, col_names)
    rng = np.random.RandomState(seed)
    truth = true_X.copy()
    truth[rng.random_sample(truth.shape) < 0.05] = np.nan
    write_matrix(os.path.join(d, 'true_data.tsv'), truth)
    with open(os.path.join(d, 'true_clusters.txt'), 'w') as f:
        # assignment.txt's layout: the reference's load_txt takes a bare
        # line of labels only where pandas raises ValueError for it
        f.write('chain\testimator\tAssignment\n0\ttrue\t'
            + ' '.join(str(int(x)) for x in true_z) + '\n')
    for i, r in enumerate(results):
        for k in KEYS:
            out[f'{name}/r{i}_{k}'] = np.asarray(r[k])
        out[f'{name}/r{i}_burn_in'] = np.array(r['burn_in'])
    with open(os.path.join(d, 'case.json'), 'w') as f:
        json.dump({'chains': len(results), 'estimator': estimators,
            'single_chains': single}, f)

    # what the reference's generate_output does with these (run_BnpC.py:
    # 203-222), its files only
    data_ref, names = rio.load_data(os.path.join(d, 'input.tsv'),
        get_names=True)
    args = argparse.Namespace(single_chains=single, chains=len(results),
        estimator=list(estimators), transpose=True)
    inferred = rio._infer_results(args, results, data_ref)
    rio.save_geno(inferred, d, names[1])
    true_assign = rio.load_txt(os.path.join(d, 'true_clusters.txt'))
    rio.save_v_measure(inferred, true_assign, d)
    rio.save_ARI(inferred, true_assign, d)
    data_true = rio.load_data(os.path.join(d, 'true_data.tsv'),
        transpose=True)
    rio.save_hamming_dist(inferred, data_true, d)
    for f in sorted(os.listdir(d)):
        with open(os.path.join(d, f), 'rb') as fh:
            out[f'{name}/{f}'] = np.frombuffer(fh.read(), dtype=np.uint8)
        os.remove(os.path.join(d, f))
    os.rmdir(d)


def main():
    out = {}
    g = np.load(os.path.join(HERE, 'posterior.npz'))
    results = []
    for i in range(2):
        r = {k: g[f'r{i}_{k}'] for k in KEYS}
        r['burn_in'] = int(g[f'r{i}_burn_in'])
        results.append(r)
    # posterior.npz's data: make_golden.synth(3, 60, 40, 3, 0.1)
    data, z, X = synth_truth(3, 60, 40, 3, 0.1)
    codes = g['data']
    assert np.array_equal(np.where(np.isnan(data), 3, data), codes)
    write_case(out, 'fixture', data, results, z, X,
        ['posterior', 'ML', 'MAP'], False, seed=1)
    write_case(out, 'fixture_sc', data, results, z, X, ['ML', 'MAP'], True,
        seed=2)
    write_case(out, 'named', data, results, z, X, ['posterior', 'ML', 'MAP'],
        False, row_names=[f'chr1_{100 + 7 * m}' for m in range(40)],
        col_names=[f'cell{n}' for n in range(60)], seed=3)

    data, z, X = synth_truth(11, 45, 30, 4, 0.1)
    write_case(out, 'learned', data, run_chains(data, (21, 22), True), z, X,
        ['posterior', 'ML', 'MAP'], False, seed=4)
    data, z, X = synth_truth(12, 24, 24, 3, 0.05)
    write_case(out, 'square', data, run_chains(data, (31,), False), z, X,
        ['posterior', 'ML', 'MAP'], False, seed=5)
    np.savez_compressed(OUT, **out)
    print(sorted(out))


if __name__ == '__main__':
    main()
