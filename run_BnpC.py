#!/usr/bin/env python3
"""Command line of the reference (/root/reference/run_BnpC.py:13-196), same
flags and defaults, driving the MI355X model classes (libs/CRP.py,
libs/CRP_learning_errors.py of this repo).

    python run_BnpC.py <DATA> [options]

Kept verbatim from the reference: every flag, its destination name, type,
default and choices - including the defaults that differ from their help text
(-FP_m 0.01, -sms 3) and `-t` being store_false.  Outputs (dpmmIO.py
save_run, save_geno, save_v_measure, save_ARI, save_hamming_dist): args.txt,
assignment.txt and errors.txt for the posterior (MPEAR, chains pooled), ML
and MAP estimators; per estimator the inferred genotypes
(genotypes_<est>_<chain>.tsv, and genotypes_cont_<est>_<chain>.tsv when they
are not all 0/1); with -tc V_measure.txt and ARI.txt, with -td
hammingDist.txt.  Plots, the similarity PDF and -tr tree colouring are not
part of this build; -ps (not a reference flag) writes the similarity PDF's
data summed per cluster: cell_support_posterior_mean.tsv and
cluster_similarity_posterior_mean.tsv; -pg (not a reference flag either)
writes the per-cell posterior genotypes, averaged over the samples instead of
taken from the cell's MPEAR cluster: genotypes_cell_prob_posterior_mean.tsv,
genotypes_cell_cont_posterior_mean.tsv, genotypes_cell_sd_posterior_mean.tsv;
-pf (not a reference flag either) writes how well the model explains every
cell and the run's WAIC, from the log-likelihood of every cell in every
posterior sample: cell_fit_posterior_mean.tsv, model_fit_posterior_mean.txt;
-pm (not a reference flag either) writes how well the model explains every
mutation and the error rates its column implies:
mutation_fit_posterior_mean.tsv, mutation_summary_posterior_mean.txt;
-pd [RATE] (not a reference flag either) scores every cell against every
cluster of the posterior clustering and every pair of them - is the cell a
doublet? - with RATE (0.05) the prior share of doublets:
doublets_posterior_mean.tsv, doublet_summary_posterior_mean.txt;
-pc (not a reference flag either) compares every chain's co-clustering with
that of the other chains pooled - did the chains find the same clustering?
(needs -n 2 or more): chain_agreement_posterior_mean.tsv,
chain_summary_posterior_mean.txt;
-po [MIN] (not a reference flag either) relates every pair of mutations - is
one nested in the other, are they carried by the same clusters, by disjoint
ones, or do they break a perfect phylogeny? - counted over the posterior
samples on clusters of MIN (2) cells or more: mutation_order_posterior_mean.tsv,
mutation_order_summary_posterior_mean.txt, mutation_pairs_posterior_mean.tsv
(up to 1000 mutations).
"""
import argparse
from datetime import datetime
import os

VERSION = '0.2.1'


def _ratio(val):
    val = float(val)
    if val <= 0 or val >= 1:
        raise argparse.ArgumentTypeError(
            f'Invalid value: {val}. Values need to be 0 < x < 1')
    return val


def _min_cells(val):
    val = int(val)
    if val < 1:
        raise argparse.ArgumentTypeError(
            f'Invalid value: {val}. Values need to be 1 or more')
    return val


def _percent(val):
    val = float(val)
    if val < 0 or val > 1:
        raise argparse.ArgumentTypeError(
            f'Invalid value: {val}. Values need to be 0 <= x <= 1')
    return val


def _psrf_cutoff(val):
    val = float(val)
    if val < 1 or val > 1.5:
        raise argparse.ArgumentTypeError(
            f'Invalid value: {val}. Values need to be 1 <= x <= 1.5')
    return val


# (group, short, long, keyword arguments) - one row per reference flag
FLAGS = [
    (None, '-t', '--transpose', dict(action='store_false',
        help='Transpose the input matrix. Default = True.')),
    (None, None, '--debug', dict(action='store_true', default=False,
        help='Run single chain in main python thread.')),
    ('model', '-FN', '--falseNegative', dict(type=float, default=-1,
        help='Fixed error rate for false negatives.')),
    ('model', '-FP', '--falsePositive', dict(type=float, default=-1,
        help='Fixed error rate for false positives.')),
    ('model', '-FN_m', '--falseNegative_mean', dict(type=_ratio, default=0.2,
        help='Prior mean of the false negative rate. Default = 0.2.')),
    ('model', '-FN_sd', '--falseNegative_std', dict(type=_ratio, default=0.1,
        help='Prior standard dev. of the false negative rate.')),
    ('model', '-FP_m', '--falsePositive_mean', dict(type=_ratio, default=0.01,
        help='Prior mean of the false positive rate.')),
    ('model', '-FP_sd', '--falsePositive_std', dict(type=_ratio, default=0.01,
        help='Prior standard dev. of the false positive rate.')),
    ('model', '-ap', '--DPa_prior', dict(type=float, nargs=2,
        default=[-1, -1], help='Gamma(a, b) prior of the CRP concentration. '
        'Default = (sqrt(#cells), 1).')),
    ('model', '-pp', '--param_prior', dict(type=float, nargs=2,
        default=[.25, .25], help='Beta(a, b) parameter prior.')),
    ('model', '-fa', '--fixed_assignment', dict(type=str, default='',
        help='File with a cluster assignment that is used and not updated.')),
    ('MCMC', '-n', '--chains', dict(type=int, default=1,
        help='Number of chains (one per GPU). Default = 1.')),
    ('MCMC', '-s', '--steps', dict(type=int, default=5000,
        help='Number of MCMC steps. Default = 5000.')),
    ('MCMC', '-r', '--runtime', dict(type=int, default=-1,
        help='Runtime in minutes; overrides steps. Default = -1.')),
    ('MCMC', '-ls', '--lugsail', dict(type=_psrf_cutoff, default=-1,
        help='Lugsail batch means PSRF threshold (e.g. 1.05).')),
    ('MCMC', '-b', '--burn_in', dict(type=_percent, default=0.33,
        help='Ratio of MCMC steps treated as burn-in. Default = 0.33.')),
    ('MCMC', '-cup', '--conc_update_prob', dict(type=_percent, default=0.25,
        help='Probability of updating the CRP concentration parameter.')),
    ('MCMC', '-eup', '--error_update_prob', dict(type=_percent, default=0.25,
        help='Probability of updating the error rates.')),
    ('MCMC', '-smp', '--split_merge_prob', dict(type=_percent, default=0.33,
        help='Probability of a split/merge step instead of Gibbs.')),
    ('MCMC', '-sms', '--split_merge_steps', dict(type=int, default=3,
        help='Restricted Gibbs scans during a split-merge move.')),
    ('MCMC', '-smr', '--split_merge_ratios', dict(type=_percent, nargs=2,
        default=[0.75, 0.25], help='Ratio of splits/merges.')),
    ('MCMC', '-e', '--estimator', dict(type=str, default='posterior',
        nargs='+', choices=['posterior', 'ML', 'MAP'],
        help='Estimator(s) used for inference.')),
    ('MCMC', '-sc', '--single_chains', dict(action='store_true',
        default=False, help='Infer a result for each chain individually.')),
    ('MCMC', None, '--seed', dict(type=int, default=-1,
        help='Seed for random number generation. Default = random.')),
    ('output', '-o', '--output', dict(type=str, default='',
        help='Output directory. Default = "<DATA_DIR>/<TIMESTAMP>".')),
    ('output', '-v', '--verbosity', dict(type=int, default=1,
        choices=[0, 1, 2], help='Print status messages. Default = 1.')),
    ('output', '-np', '--no_plots', dict(action='store_true', default=False,
        help='Accepted for compatibility (this build never plots).')),
    ('output', '-tr', '--tree', dict(type=str, default='',
        help='Accepted for compatibility (tree colouring is out of scope).')),
    ('output', '-tc', '--true_clusters', dict(type=str, default='',
        help='File with the true cluster assignment: writes V_measure.txt '
        'and ARI.txt.')),
    ('output', '-td', '--true_data', dict(type=str, default='',
        help='File with the true (error-free) data: writes hammingDist.txt.')),
    # not a reference flag: absent from the arguments (and from args.txt)
    # unless it is given - see Args
    ('output', '-ps', '--posterior_support', dict(action='store_true',
        default=argparse.SUPPRESS, help='Write the support of every cell '
        'for every cluster of the posterior clustering and the clusters\' '
        'mean posterior similarity (needs -e posterior).')),
    ('output', '-pg', '--posterior_genotypes', dict(action='store_true',
        default=argparse.SUPPRESS, help='Write the genotype of every cell '
        'averaged over the posterior samples - the probability of a 1, the '
        'mean and the standard deviation of its cluster\'s parameter - '
        'instead of the genotype of its cluster (needs -e posterior; one '
        'more pass over samples x cells x mutations on the GPU: minutes at '
        '50 000 cells x 5000 mutations).')),
    ('output', '-pf', '--posterior_fit', dict(action='store_true',
        default=argparse.SUPPRESS, help='Write how well the model explains '
        'every cell - mean and spread of its log-likelihood over the '
        'posterior samples, per observed entry too - and the WAIC of the '
        'run, with the cell as its unit (needs -e posterior; one more pass '
        'over samples x cells x mutations on the GPU).')),
    ('output', '-pm', '--posterior_mutations', dict(action='store_true',
        default=argparse.SUPPRESS, help='Write how well the model explains '
        'every mutation - mean and spread of its column\'s log-likelihood '
        'over the posterior samples - and the false-negative and '
        'false-positive rates the column implies, beside the run\'s global '
        'pair (needs -e posterior; one more pass over the samples on the '
        'GPU, over column counts per cluster).')),
    ('output', '-pd', '--posterior_doublets', dict(type=_ratio, nargs='?',
        const=0.05, default=argparse.SUPPRESS, metavar='RATE', help='Score '
        'every cell against every cluster of the posterior clustering and '
        'against every pair of them - a doublet shows the union of two '
        'clones\' mutations - and write the best pair, the gain over the '
        'best single cluster and the probability of a doublet per cell, with '
        'RATE (default 0.05) the prior share of doublets (needs -e '
        'posterior; one more pass over cells x mutations x cluster pairs on '
        'the GPU).')),
    ('output', '-pc', '--posterior_chains', dict(action='store_true',
        default=argparse.SUPPRESS, help='Compare the posterior co-clustering '
        'of every chain with that of the other chains pooled and write, per '
        'cell and chain, the mean and the largest difference and the pairs '
        'the two sides call differently: a chain that stands out has not '
        'mixed (needs -e posterior and -n 2 or more; one more pass over '
        'samples x pairs of cells on the GPU).')),
    ('output', '-po', '--posterior_order', dict(type=_min_cells, nargs='?',
        const=2, default=argparse.SUPPRESS, metavar='MIN', help='Relate every '
        'pair of mutations under the three-gamete rule in every posterior '
        'sample - one nested in the other, on the same clusters, on disjoint '
        'clusters, or in conflict with a perfect phylogeny - and write the '
        'probabilities, the mutation forest they imply and how often every '
        'mutation breaks the phylogeny; a cluster counts from MIN cells '
        '(default 2: a transient one-cell cluster is ignored; 1 is the '
        'strict reading) (needs -e posterior; one more pass over samples x '
        'pairs of mutations on the GPU).')),
]


class Args(argparse.Namespace):
    """The parsed arguments: the reference's flags as attributes set by the
    parser; a flag of this build alone reads as its default until given."""
    posterior_support = False
    posterior_genotypes = False
    posterior_fit = False
    posterior_mutations = False
    posterior_doublets = False
    posterior_chains = False
    posterior_order = False


def build_parser():
    parser = argparse.ArgumentParser(prog='BnpC',
        usage='python3 run_BnpC.py <DATA> [options]',
        description='*** Clustering of single cell data based on a '
            'Dirichlet process (MI355X build). ***')
    parser.add_argument('--version', action='version', version=VERSION)
    parser.add_argument('input', help='Path to the input matrix (mutations x '
        'cells by default, entries 0|1, 3 or empty for missing).')
    groups = {None: parser}
    for group, short, long_, kw in FLAGS:
        if group not in groups:
            groups[group] = parser.add_argument_group(group)
        names = [n for n in (short, long_) if n]
        groups[group].add_argument(*names, **kw)
    return parser


def parse_args(argv=None):
    return build_parser().parse_args(argv, namespace=Args())


def check_args(args):
    """Combinations of flags that cannot run: raises SystemExit with the
    reason (before any chain starts)."""
    ests = [args.estimator] if isinstance(args.estimator, str) \
        else list(args.estimator)
    if getattr(args, 'posterior_support', False) and 'posterior' not in ests:
        raise SystemExit('-ps / --posterior_support writes tables of the '
            'posterior clustering: it needs `posterior` among the estimators '
            f'(-e), which are: {" ".join(ests)}')
    if getattr(args, 'posterior_genotypes', False) \
            and 'posterior' not in ests:
        raise SystemExit('-pg / --posterior_genotypes writes tables of the '
            'posterior samples: it needs `posterior` among the estimators '
            f'(-e), which are: {" ".join(ests)}')
    if getattr(args, 'posterior_fit', False) and 'posterior' not in ests:
        raise SystemExit('-pf / --posterior_fit writes tables of the '
            'posterior samples: it needs `posterior` among the estimators '
            f'(-e), which are: {" ".join(ests)}')
    if getattr(args, 'posterior_mutations', False) and 'posterior' not in ests:
        raise SystemExit('-pm / --posterior_mutations writes tables of the '
            'posterior samples: it needs `posterior` among the estimators '
            f'(-e), which are: {" ".join(ests)}')
    if getattr(args, 'posterior_doublets', False) and 'posterior' not in ests:
        raise SystemExit('-pd / --posterior_doublets writes tables of the '
            'posterior samples: it needs `posterior` among the estimators '
            f'(-e), which are: {" ".join(ests)}')
    if getattr(args, 'posterior_order', False) and 'posterior' not in ests:
        raise SystemExit('-po / --posterior_order writes tables of the '
            'posterior samples: it needs `posterior` among the estimators '
            f'(-e), which are: {" ".join(ests)}')
    if getattr(args, 'posterior_chains', False):
        if 'posterior' not in ests:
            raise SystemExit('-pc / --posterior_chains writes tables of the '
                'posterior samples: it needs `posterior` among the estimators '
                f'(-e), which are: {" ".join(ests)}')
        if getattr(args, 'debug', False):
            raise SystemExit('-pc / --posterior_chains compares chains with '
                'each other: --debug runs a single chain')
        if getattr(args, 'chains', 1) < 2:
            raise SystemExit('-pc / --posterior_chains compares chains with '
                'each other: it needs two or more (-n), not '
                f'{getattr(args, "chains", 1)}')


def save_outputs(args, results, data, out_dir, names=None):
    """The output files of one run; names: the loader's (cell, mutation)
    names, which name the genotype tables' rows."""
    from bnpc_amd import io as bio
    from bnpc_amd import postproc
    ests = [args.estimator] if isinstance(args.estimator, str) \
        else list(args.estimator)
    chains = list(enumerate(results)) if args.single_chains else [('mean', None)]
    rows_a, rows_e, inferred = [], [], []
    for est in ests:
        if est == 'posterior':
            # the reference's per-chain posterior (-sc) indexes its parameter
            # trace inconsistently (utils.py:228-229); chains are pooled here
            inf = postproc.posterior_estimate(results, data,
                support=getattr(args, 'posterior_support', False),
                cells=getattr(args, 'posterior_genotypes', False),
                fit=getattr(args, 'posterior_fit', False),
                mutations=getattr(args, 'posterior_mutations', False),
                doublets=getattr(args, 'posterior_doublets', False),
                chains=getattr(args, 'posterior_chains', False),
                ordering=getattr(args, 'posterior_order', False))
            rows_a.append(('mean', est,
                ' '.join(str(i) for i in inf['assignment'])))
            inferred.append(('mean', est, inf))
            rows_e.append(('mean', est,
                f'{inf["FN"][0]:.4f}+-{inf["FN"][1]:.4f}',
                round(float(inf['FN_geno']), 4),
                f'{inf["FP"][0]:.8f}+-{inf["FP"][1]:.8f}',
                round(float(inf['FP_geno']), 8)))
            if args.verbosity > 0:
                print(f'posterior: {len(set(inf["assignment"]))} clusters, '
                    f'FN {inf["FN"][0]:.4f}, FP {inf["FP"][0]:.6f}')
                if 'fit' in inf:
                    total = inf['fit']['total']
                    print(f'posterior fit: WAIC {total["waic"]:.4f}, lppd '
                        f'{total["lppd"]:.4f}, p_waic {total["p_waic"]:.4f}')
                if 'mutation_fit' in inf:
                    total = inf['mutation_fit']['total']
                    print('posterior mutations: FN_model '
                        f'{total["FN_model"]:.4f}, FP_model '
                        f'{total["FP_model"]:.6f} (run: FN {total["FN"]:.4f}, '
                        f'FP {total["FP"]:.6f})')
                if 'doublets' in inf:
                    total = inf['doublets']['total']
                    print(f'posterior doublets: {total["called"]} called, '
                        f'{total["expected_doublets"]:.4f} expected (rate '
                        f'{total["rate"]})')
                if 'chains' in inf:
                    total = inf['chains']['total']
                    print('posterior chains: mean difference '
                        f'{total["mean_diff"]:.4f}, worst chain '
                        f'{total["worst_chain"]} '
                        f'({total["worst_mean_diff"]:.4f}), flip share '
                        f'{total["flip_share"]:.4f}')
                if 'mutation_order' in inf:
                    total = inf['mutation_order']['total']
                    print(f'posterior order: {total["roots"]} roots, depth '
                        f'{total["max_depth"]}, conflict share '
                        f'{total["conflict"]:.4f}')
            continue
        for chain, res in chains:
            res = res if res is not None else postproc.best_chain(results, est)
            inf = postproc.point_estimate(res, est, data)
            rows_a.append((chain, est,
                ' '.join(str(i) for i in inf['assignment'])))
            inferred.append((chain, est, inf))
            rows_e.append((chain, est, round(float(inf['FN']), 4),
                round(float(inf['FN_geno']), 4), round(float(inf['FP']), 8),
                round(float(inf['FP_geno']), 8)))
            if args.verbosity > 0:
                print(f'{est} (chain {chain}): step {inf["step"]}, '
                    f'{len(set(inf["assignment"]))} clusters, '
                    f'FN {inf["FN"]:.4f}, FP {inf["FP"]:.6f}')
    with open(os.path.join(out_dir, 'assignment.txt'), 'w') as f:
        f.write('chain\testimator\tAssignment\n')
        for row in rows_a:
            f.write('\t'.join(str(x) for x in row) + '\n')
    with open(os.path.join(out_dir, 'errors.txt'), 'w') as f:
        f.write('chain\testimator\tFN_model\tFN_data\tFP_model\tFP_data\n')
        for row in rows_e:
            f.write('\t'.join(str(x) for x in row) + '\n')
    with open(os.path.join(out_dir, 'args.txt'), 'w') as f:
        for key, val in vars(args).items():
            if key == 'time':
                val = [f'{t:%Y%m%d_%H:%M:%S}' for t in val]
            if key in ('posterior_support', 'posterior_genotypes',
                    'posterior_fit', 'posterior_mutations',
                    'posterior_doublets', 'posterior_chains',
                    'posterior_order') and not val:
                continue        # listed only when it is set
            f.write(f'{key}: {val}\n')
    mut_names = names[1] if names is not None else None
    for chain, est, inf in inferred:
        bio.save_geno(out_dir, chain, est, inf['cluster_genotypes'],
            inf['cluster_of'], inf['assignment'], mut_names)
        if 'support' in inf:
            bio.save_support(out_dir, chain, est, inf['support'],
                inf['assignment'], names[0] if names is not None else None)
        if 'cell_genotypes' in inf:
            bio.save_cell_geno(out_dir, chain, est, inf['cell_genotypes'],
                names)
        if 'fit' in inf:
            bio.save_cell_fit(out_dir, chain, est, inf['fit'],
                inf['assignment'], names[0] if names is not None else None)
        if 'mutation_fit' in inf:
            bio.save_mutation_fit(out_dir, chain, est, inf['mutation_fit'],
                mut_names)
        if 'doublets' in inf:
            bio.save_doublets(out_dir, chain, est, inf['doublets'],
                names[0] if names is not None else None)
        if 'chains' in inf:
            bio.save_chain_agreement(out_dir, chain, est, inf['chains'],
                names[0] if names is not None else None)
        if 'mutation_order' in inf:
            bio.save_mutation_order(out_dir, chain, est,
                inf['mutation_order'], mut_names)
    # the metric tables list their rows chain by chain, as the reference
    # does (its per-chain dictionary, dpmmIO.py:524-530); the pooled
    # posterior first
    inferred.sort(key=lambda row: -1 if row[0] == 'mean' else row[0])
    if args.true_clusters:
        true_assign = bio.load_txt(args.true_clusters)
        bio.save_metric(os.path.join(out_dir, 'V_measure.txt'), 'V-measure',
            [(c, e, postproc.v_measure(inf['assignment'], true_assign))
                for c, e, inf in inferred])
        bio.save_metric(os.path.join(out_dir, 'ARI.txt'), 'ARI',
            [(c, e, postproc.adjusted_rand(inf['assignment'], true_assign))
                for c, e, inf in inferred])
    if args.true_data:
        true_data = bio.load_data(args.true_data, transpose=args.transpose)
        bio.save_metric(os.path.join(out_dir, 'hammingDist.txt'),
            '1 - norm Hamming distance',
            [(c, e, postproc.hamming_similarity(inf['cluster_genotypes'],
                inf['cluster_of'], true_data)) for c, e, inf in inferred])


def main(args):
    from bnpc_amd import io as bio
    from bnpc_amd import postproc
    from libs.MCMC import MCMC

    check_args(args)
    if os.path.getsize(args.input) > (4 << 20):
        # large matrices (no row / column names): the packed bit planes, read
        # from the file next to the input when it is current, else scanned
        # natively and written there for the next run; the model and the
        # device take them as they are (no float64 matrix)
        from bnpc_amd import bitplanes
        data = bitplanes.load_matrix(args.input, transpose=args.transpose)
        names = None
    else:
        data, names = bio.load_data(args.input, transpose=args.transpose,
            get_names=True)
    assert data.size > 0, f'Could not read data from file: {args.input}'

    # fixed error rates only if BOTH are given (run_BnpC.py:249-262)
    if args.falsePositive > 0 and args.falseNegative > 0:
        args.error_update_prob = 0
        import libs.CRP as mod
        model = mod.CRP(data, DP_alpha=args.DPa_prior,
            param_beta=args.param_prior, FN_error=args.falseNegative,
            FP_error=args.falsePositive)
    else:
        import libs.CRP_learning_errors as mod
        model = mod.CRP_errors_learning(data, DP_alpha=args.DPa_prior,
            param_beta=args.param_prior, FP_mean=args.falsePositive_mean,
            FP_sd=args.falsePositive_std, FN_mean=args.falseNegative_mean,
            FN_sd=args.falseNegative_std)

    args.time = [datetime.now()]
    run_var, run_str = bio.get_mcmc_termination(args)
    mcmc = MCMC(model, sm_prob=args.split_merge_prob,
        dpa_prob=args.conc_update_prob, error_prob=args.error_update_prob,
        sm_ratios=args.split_merge_ratios, sm_steps=args.split_merge_steps)
    if args.verbosity > 0:
        print(model)
        print(mcmc)
        print(f'Run MCMC with ({args.chains} chains {run_str}):')
    if args.debug:
        args.chains = 1

    mcmc.run(run_var, args.seed, args.chains, args.verbosity,
        args.fixed_assignment, args.debug)
    args.chain_seeds = [int(s) for s in mcmc.get_seeds()]
    results = mcmc.get_results()
    args.time.append(datetime.now())

    args.PSRF = float(postproc.get_lugsail_batch_means_est(
        [(r['ML'], r['burn_in']) for r in results]))
    args.steps = [int(r['ML'].size) for r in results]
    out_dir = bio.get_out_dir(args)
    if args.verbosity > 0:
        bio.show_MCMC_summary(args.time[0], args.time[1], results)
        print(f'Lugsail PSRF:\t\t{args.PSRF:.5f}')
        print(f'\nWriting output to: {out_dir}\n')
    if hasattr(data, 'planes'):
        data = data.codes()     # 0 | 1 | 3: all the estimators compare with
    save_outputs(args, results, data, out_dir, names)
    return results


if __name__ == '__main__':
    main(parse_args())
