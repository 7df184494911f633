"""Minimal input / reporting helpers the driver and the CLI need.

Restates, as far as the CLI requires, the reference's
/root/reference/libs/dpmmIO.py: ``load_data`` :27-98 (separator / header /
index sniffing, ``3`` or blank -> NaN, ``2`` -> 1, transpose by default),
``load_txt`` :101-112, ``show_MH_acceptance`` :343-348, run-time summary
:310-315, ``_get_mcmc_termination`` :157-169.  Plotting, tree colouring and
the simulation-folder conventions are out of scope.
"""
from datetime import timedelta
import os

import numpy as np

_CODES = (0.0, 1.0, 2.0, 3.0)


def _sniff_separator(first_line):
    tabs, spaces, commas = (first_line.count(c) for c in '\t ,')
    if tabs > spaces and tabs > commas:
        return '\t'
    if commas > spaces:
        return ','
    return ' '


def _is_code(token):
    """True if the token is one of the matrix codes 0|1|2|3."""
    try:
        return float(token) in _CODES
    except ValueError:
        return False


def _sniff_layout(head):
    """(separator, header_row, index_col) from the first lines of the file."""
    sep = _sniff_separator(head[0])
    header_row = any(not _is_code(tok) for tok in head[0].split(sep)
        if tok not in ('', ' '))
    body_probe = head[1:] if header_row else head
    index_col = any(not _is_code(ln.split(sep)[0]) for ln in body_probe
        if ln.split(sep)[0] not in ('', ' '))
    return sep, header_row, index_col


def _sniff_head(lines, in_file):
    """What the layout is sniffed from: the first five lines, stripped, the
    blank ones left out."""
    head = [ln.strip() for ln in lines[:5] if ln.strip()]
    if not head:
        raise ValueError(f'Could not read data from file: {in_file}')
    return head


def _is_blank(line, sep):
    """pandas.read_csv's skip_blank_lines, the reader the reference rests on:
    a line is no row (and no header) if it is empty or holds only spaces and
    tabs that do not separate."""
    return all(ch in ' \t' and ch != sep for ch in line)


def load_codes_native(in_file, transpose=True):
    """The same matrix as `load_data`, as int8 codes 0 | 1 | 3 (missing),
    cells x mutations, scanned by libbnpc_hip.so's byte scanner
    (bnpc_parse_matrix).  No names."""
    import ctypes as C
    from bnpc_amd import _lib
    with open(in_file, 'r') as f:
        head = _sniff_head([f.readline() for _ in range(5)], in_file)
    sep, header_row, index_col = _sniff_layout(head)
    lib = _lib.load()
    rows, cols = C.c_int64(0), C.c_int64(0)
    path = os.fsencode(in_file)
    bsep = sep.encode()
    _lib.check(lib.bnpc_parse_matrix(path, bsep, int(header_row),
        int(index_col), None, C.byref(rows), C.byref(cols)), 'parse_matrix')
    if rows.value < 1 or cols.value < 1:
        raise ValueError(f'Could not read data from file: {in_file}')
    codes = np.empty((rows.value, cols.value), dtype=np.int8)
    _lib.check(lib.bnpc_parse_matrix(path, bsep, int(header_row),
        int(index_col), _lib.ptr(codes, C.c_int8), C.byref(rows),
        C.byref(cols)), 'parse_matrix')
    if transpose:
        codes = np.ascontiguousarray(codes.T)
    return codes


def codes_to_data(codes):
    """int8 codes 0 | 1 | 3 -> the reference's float64 matrix with NaN."""
    data = codes.astype(np.float64)
    data[codes == 3] = np.nan
    return data


def data_to_codes(data):
    codes = np.where(np.isnan(data), 3, data).astype(np.int8)
    return codes


def load_data(in_file, transpose=True, get_names=False):
    """Read a 0|1|2|3 matrix; returns cells x mutations float64 with NaN.

    On disk the reference format is mutations x cells, hence the default
    transpose (dpmmIO.py:27-98; run_BnpC.py:50-53 passes ``-t`` as
    store_false).
    """
    with open(in_file, 'r') as f:
        lines = [ln.rstrip('\r\n') for ln in f]
    sep, header_row, index_col = _sniff_layout(_sniff_head(lines, in_file))
    # the lines are read_csv's: blank ones are skipped wherever they stand,
    # every other line is a row (a lone separator: a row of missing
    # entries), no line is stripped, and one with more fields than the first
    # is refused (bnpc_parse_matrix reads the same way)
    lines = [ln for ln in lines if not _is_blank(ln, sep)]

    col_names, allowed = None, None
    if header_row:
        col_names = lines[0].strip().split(sep)
        allowed = len(lines[0].split(sep))
        lines = lines[1:]
    if not lines:
        raise ValueError(f'Could not read data from file: {in_file}')

    rows, row_names = [], []
    for ln in lines:
        toks = ln.split(sep)
        if allowed is None or (not rows and header_row and index_col
                and len(toks) == allowed + 1):
            allowed = len(toks)
        if len(toks) > allowed:
            raise ValueError(f'{in_file}: row {len(rows)} holds {len(toks)} '
                f'fields, the lines before it {allowed}')
        if index_col:
            row_names.append(toks[0])
            toks = toks[1:]
        rows.append([np.nan if t.strip() == '' else float(t) for t in toks])
    width = max(len(r) for r in rows)
    mat = np.full((len(rows), width), np.nan)
    for i, r in enumerate(rows):
        mat[i, :len(r)] = r

    if col_names is not None:
        if index_col and len(col_names) == width + 1:
            col_names = col_names[1:]
        col_names = np.array(col_names[:width], dtype=object)
    else:
        col_names = np.arange(1 if index_col else 0,
            width + (1 if index_col else 0))
    row_names = np.array(row_names, dtype=object) if index_col \
        else np.arange(len(rows))

    if transpose:
        mat = mat.T
        row_names, col_names = col_names, row_names

    mat = np.ascontiguousarray(mat, dtype=np.float64)
    mat[mat == 3] = np.nan
    mat[mat == 2] = 1
    if get_names:
        return mat, (row_names, col_names)
    return mat


def load_txt(path):
    """Cluster assignment file: space separated ints, optionally in a
    tab-separated table with an ``Assignment`` column (dpmmIO.py:101-112)."""
    with open(path, 'r') as f:
        text = f.read()
    lines = [ln for ln in text.splitlines() if ln.strip()]
    if lines and 'Assignment' in lines[0].split('\t'):
        col = lines[0].split('\t').index('Assignment')
        text = lines[1].split('\t')[col]
    return [int(tok) for tok in text.split()]


def get_mcmc_termination(args):
    """(run_var, description) from CLI arguments (dpmmIO.py:157-169)."""
    if args.runtime > 0:
        span = timedelta(minutes=args.runtime)
        return (args.time[0] + span, args.time[0] + args.burn_in * span), \
            f'for {args.runtime} mins'
    if args.lugsail > 0:
        return (args.lugsail, 0), f'until PSRF < {args.lugsail:.4f}'
    return (args.steps, int(args.steps * args.burn_in)), \
        f'for {args.steps} steps'


def show_MH_acceptance(counter, name, tab_no=2):
    """dpmmIO.py:343-348"""
    try:
        rate = counter[0] / counter.sum()
    except (ZeroDivisionError, FloatingPointError):
        rate = np.nan
    print('\t\t{}:{}{:.2f}'.format(name, '\t' * tab_no, rate))


def show_MCMC_summary(start, end, results):
    """Run-time line of the reference (dpmmIO.py:310-315): total wall time
    over the number of recorded steps of the first chain."""
    total = sum(r['ML'].size for r in results)
    step_time = (end - start) / results[0]['ML'].size
    print(f'\nClustering time:\t{end - start}\t'
        f'({step_time.total_seconds():.2f} secs. per MCMC step)')
    print(f'Steps recorded (all chains):\t{total}')


def get_out_dir(args, prefix=''):
    """dpmmIO.py:172-192"""
    if args.output:
        if any(args.output.endswith(s) for s in ('.txt', '.gv', '.csv')):
            out_dir = os.path.dirname(args.output)
        else:
            out_dir = args.output
    else:
        stamp = f'BnpC_{args.time[0]:%Y%m%d_%H:%M:%S}{prefix}'
        base = os.path.join(os.path.dirname(args.input), stamp)
        out_dir, i = base, 1
        while os.path.exists(out_dir):
            out_dir = f'{base}_{i}'
            i += 1
    os.makedirs(out_dir, exist_ok=True)
    return out_dir


# ---------------------------------------------------------------------------
# genotype tables (dpmmIO.py:491-511)
# ---------------------------------------------------------------------------
def _write_rows(path, header, tokens, cols):
    """The header line, then one row per row of `tokens` (rows x (1 + K)
    strings: the row's name, then its K distinct entries), each cell c
    taking entry cols[c] (libbnpc_hip.so's bnpc_write_table)."""
    from bnpc_amd import _lib
    with open(path, 'w') as f:
        f.write('\t'.join([''] + [str(h) for h in header]) + '\n')
    R, K1 = tokens.shape
    enc = [t.encode() for t in tokens.ravel().tolist()]
    off = np.zeros(len(enc) + 1, dtype=np.int64)
    np.cumsum([len(e) for e in enc], out=off[1:])
    blob = b''.join(enc)
    col = np.ascontiguousarray(cols, dtype=np.int32)
    _lib.check(_lib.load().bnpc_write_table(os.fsencode(path), R, K1 - 1,
        blob, _lib.ptr(off), col.size, _lib.ptr(col)), 'write_table')


def _row_names(names, n):
    """The names of n rows: `names` where there is one per row, else
    0..n-1."""
    if names is not None and np.asarray(names).size == n:
        return np.asarray(names)
    return np.arange(n)


def _paths(out_dir, files, est, chain):
    """The output paths of one (chain, estimator) row: <stem>_<est>_<chain>
    with its extension for every <stem>.<ext> of `files`."""
    tag = f'{chain:0>2}'
    return [os.path.join(out_dir, f'{stem}_{est}_{tag}{ext}')
        for stem, ext in map(os.path.splitext, files)]


def _name_values(index, values, rows):
    """`name:value` of the selected rows, values %.4f, space separated."""
    return ' '.join(f'{index[i]}:{values[i]:.4f}' for i in rows)


def save_geno(out_dir, chain, est, values, cols, header, names=None):
    """`save_geno` of the reference for one (chain, estimator) row: the
    mutations x cells genotype table whose cell c is column cols[c] of
    `values` (clusters x mutations, float64 for the posterior, the trace's
    float32 for ML / MAP), under a header of the cells' cluster labels.
    genotypes_<est>_<chain>.tsv holds the rounded 0/1 calls;
    genotypes_cont_<est>_<chain>.tsv the values rounded to 4 decimals, if
    any is not an integer.  Rows are named by `names` (the loader's mutation
    names) when there is one per mutation, else 0..M-1.  Entries are
    formatted as pandas' to_csv formats them (`astype(str)` of the dtype;
    `round` is half-to-even, as DataFrame.round), once per distinct value."""
    values = np.asarray(values)
    M = values.shape[1]
    index = np.arange(M)
    if names is not None and np.asarray(names).size == M:
        index = np.asarray(names)
    index = np.array([str(x) for x in index.tolist()], dtype=object)
    tag = f'{chain:0>2}'
    rounded = np.round(values)

    def table(entries):
        return np.concatenate([index[:, None],
            np.asarray(entries).T.astype(object)], axis=1)

    paths = []
    if not np.array_equal(rounded, values):
        path = os.path.join(out_dir, f'genotypes_cont_{est}_{tag}.tsv')
        _write_rows(path, header, table(np.round(values, 4).astype(str)),
            cols)
        paths.append(path)
    path = os.path.join(out_dir, f'genotypes_{est}_{tag}.tsv')
    _write_rows(path, header, table(rounded.astype(np.int64).astype(str)),
        cols)
    paths.append(path)
    return paths


def save_support(out_dir, chain, est, tables, assignment, names=None):
    """The -ps tables of postproc.cluster_support for one (chain, estimator)
    row.  cell_support_<est>_<chain>.tsv: per cell its name (`names`, the
    loader's cell names, when there is one per cell, else 0..N-1), its
    cluster, the support of that cluster, the best other cluster with its
    support, then the support of every cluster;
    cluster_similarity_<est>_<chain>.tsv: clusters x clusters.  Cluster ids
    are the labels of `assignment` (cluster k of the tables is the k-th
    smallest), values %.4f."""
    assignment = np.asarray(assignment)
    ids = np.unique(assignment)
    cluster_of = np.searchsorted(ids, assignment)
    support = tables['support']
    N, K = support.shape
    index = np.arange(N)
    if names is not None and np.asarray(names).size == N:
        index = np.asarray(names)
    tag = f'{chain:0>2}'
    head = '\t'.join(str(i) for i in ids.tolist())
    paths = [os.path.join(out_dir, f'cell_support_{est}_{tag}.tsv'),
        os.path.join(out_dir, f'cluster_similarity_{est}_{tag}.tsv')]
    nxt = tables['next_cluster']
    with open(paths[0], 'w') as f:
        f.write('cell\tcluster\tsupport\tnext_cluster\tnext_support\t'
            + head + '\n')
        for i, name in enumerate(index.tolist()):
            other = ids[nxt[i]] if nxt[i] >= 0 else -1
            f.write(f'{name}\t{ids[cluster_of[i]]}\t{tables["own"][i]:.4f}\t'
                f'{other}\t{tables["next_support"][i]:.4f}\t'
                + '\t'.join(f'{x:.4f}' for x in support[i].tolist()) + '\n')
    with open(paths[1], 'w') as f:
        f.write('\t' + head + '\n')
        for k, row in enumerate(tables['similarity'].tolist()):
            f.write(f'{ids[k]}\t' + '\t'.join(f'{x:.4f}' for x in row)
                + '\n')
    return paths


def save_cell_geno(out_dir, chain, est, tables, names=None):
    """The -pg tables of postproc.cell_genotypes for one (chain, estimator)
    row, each mutations x cells, values %.4f:
    genotypes_cell_prob_<est>_<chain>.tsv the share of the samples in which
    the cell's parameter rounds to 1, genotypes_cell_cont_<est>_<chain>.tsv
    its posterior mean, genotypes_cell_sd_<est>_<chain>.tsv its posterior
    standard deviation.  names: the loader's (cell, mutation) names - columns
    and rows are named by them where there is one per cell / mutation, else
    0..N-1 / 0..M-1."""
    N, M = tables['mean'].shape
    cells, muts = (_row_names(None if names is None else names[k], n)
        for k, n in enumerate((N, M)))
    index = np.array([str(x) for x in muts.tolist()], dtype=object)
    paths = _paths(out_dir, ('genotypes_cell_prob.tsv',
        'genotypes_cell_cont.tsv', 'genotypes_cell_sd.tsv'), est, chain)
    for path, key in zip(paths, ('prob', 'mean', 'sd')):
        entries = np.char.mod('%.4f', np.asarray(tables[key]).T)
        _write_rows(path, cells.tolist(), np.concatenate([index[:, None],
            entries.astype(object)], axis=1), np.arange(N))
    return paths


def save_cell_fit(out_dir, chain, est, fit, assignment, names=None):
    """The -pf files of postproc.cell_fit for one (chain, estimator) row.
    cell_fit_<est>_<chain>.tsv: per cell its name (`names`, the loader's cell
    names, when there is one per cell, else 0..N-1), its cluster (the label
    of `assignment`), its observed entries, the mean and the standard
    deviation of its log-likelihood over the samples, its share of lppd and
    of p_waic, and the mean log-likelihood per observed entry; floats %.4f.
    model_fit_<est>_<chain>.txt: `key: value` lines - samples, cells,
    observations, lppd, p_waic, WAIC (= -2 (lppd - p_waic); the unit is the
    cell) and worst_cells, the ten cells with the smallest mean
    log-likelihood per observed entry as name:value pairs."""
    assignment = np.asarray(assignment)
    index = _row_names(names, assignment.size).tolist()
    paths = _paths(out_dir, ('cell_fit.tsv', 'model_fit.txt'), est, chain)
    columns = ('mean_ll', 'sd_ll', 'lppd', 'p_waic', 'mean_ll_per_obs')
    with open(paths[0], 'w') as f:
        f.write('cell\tcluster\tn_obs\t' + '\t'.join(columns) + '\n')
        for i, name in enumerate(index):
            f.write(f'{name}\t{assignment[i]}\t{fit["n_obs"][i]}\t'
                + '\t'.join(f'{fit[k][i]:.4f}' for k in columns) + '\n')
    total = fit['total']
    per_obs = fit['mean_ll_per_obs']
    worst = np.argsort(per_obs, kind='stable')[:10]
    with open(paths[1], 'w') as f:
        for key in ('samples', 'cells', 'observations'):
            f.write(f'{key}: {total[key]}\n')
        for key, val in (('lppd', total['lppd']), ('p_waic', total['p_waic']),
                ('WAIC', total['waic'])):
            f.write(f'{key}: {val:.4f}\n')
        f.write('worst_cells: ' + _name_values(index, per_obs, worst.tolist())
            + '\n')
    return paths


def save_mutation_fit(out_dir, chain, est, fit, names=None):
    """The -pm files of postproc.mutation_fit for one (chain, estimator) row.
    mutation_fit_<est>_<chain>.tsv: per mutation its name (`names`, the
    loader's mutation names, when there is one per mutation, else 0..M-1) and
    the columns of postproc.MUTATION_FIT_COLUMNS: integers plain, floats
    %.4f, FP_model and FP_call %.8f (as errors.txt).
    mutation_summary_<est>_<chain>.txt: `key: value` lines - samples,
    mutations, observations, the pooled FN_model, FP_model, FN_call, FP_call,
    the posterior means FN and FP of the run's own rates, worst_mutations
    (the ten with the smallest mean log-likelihood per observed entry among
    those with observations) and highest_FN (the ten with the largest
    FN_model among those with at least one expected carrier per sample), as
    name:value pairs."""
    from bnpc_amd.postproc import MUTATION_FIT_COLUMNS as columns
    index = _row_names(names, fit['n_obs'].size).tolist()
    paths = _paths(out_dir, ('mutation_fit.tsv', 'mutation_summary.txt'),
        est, chain)
    fine = ('FP_model', 'FP_call')

    def cell(key, val):
        if key.startswith('n_'):
            return str(int(val))
        return f'{val:.8f}' if key in fine else f'{val:.4f}'
    with open(paths[0], 'w') as f:
        f.write('mutation\t' + '\t'.join(columns) + '\n')
        for m, name in enumerate(index):
            f.write(f'{name}\t'
                + '\t'.join(cell(k, fit[k][m]) for k in columns) + '\n')
    total = fit['total']
    per_obs = fit['mean_ll_per_obs']
    seen = np.flatnonzero(fit['n_obs'] > 0)
    worst = seen[np.argsort(per_obs[seen], kind='stable')[:10]]
    carried = np.flatnonzero(fit['eg1'] / total['samples'] >= 1)
    high = carried[np.argsort(-fit['FN_model'][carried], kind='stable')[:10]]
    with open(paths[1], 'w') as f:
        for key in ('samples', 'mutations', 'observations'):
            f.write(f'{key}: {total[key]}\n')
        for key in ('FN_model', 'FP_model', 'FN_call', 'FP_call', 'FN', 'FP'):
            f.write(f'{key}: {cell(key, total[key])}\n')
        f.write('worst_mutations: '
            + _name_values(index, per_obs, worst.tolist()) + '\n')
        f.write('highest_FN: '
            + _name_values(index, fit['FN_model'], high.tolist()) + '\n')
    return paths


def save_doublets(out_dir, chain, est, tables, names=None):
    """The -pd files of postproc.doublets for one (chain, estimator) row.
    doublets_<est>_<chain>.tsv: per cell its name (`names`, the loader's cell
    names, when there is one per cell, else 0..N-1), `cluster` (its label of
    assignment.txt, as every cluster id here), `n_obs`, `ll_cluster`,
    `best_cluster`, `ll_best`, `pair_a`, `pair_b`, `ll_pair`, `delta`,
    `p_doublet`; floats %.4f.  doublet_summary_<est>_<chain>.txt: `key:
    value` lines - cells, clusters, candidates, rate, expected_doublets,
    called, pair_counts (the pairs with called cells as a-b:count) and
    top_cells, the ten cells with the largest p_doublet (ties: the larger
    delta, then the smaller index) as name:value pairs."""
    N = tables['p_doublet'].size
    index = _row_names(names, N).tolist()
    paths = _paths(out_dir, ('doublets.tsv', 'doublet_summary.txt'), est,
        chain)
    columns = ('cluster', 'n_obs', 'll_cluster', 'best_cluster', 'll_best',
        'pair_a', 'pair_b', 'll_pair', 'delta', 'p_doublet')
    whole = ('cluster', 'n_obs', 'best_cluster', 'pair_a', 'pair_b')
    with open(paths[0], 'w') as f:
        f.write('cell\t' + '\t'.join(columns) + '\n')
        for i, name in enumerate(index):
            f.write(f'{name}\t' + '\t'.join(str(int(tables[k][i]))
                if k in whole else f'{tables[k][i]:.4f}' for k in columns)
                + '\n')
    total = tables['total']
    p, delta = tables['p_doublet'], tables['delta']
    top = sorted(range(N), key=lambda i: (-p[i], -delta[i], i))[:10]
    with open(paths[1], 'w') as f:
        for key in ('cells', 'clusters', 'candidates'):
            f.write(f'{key}: {total[key]}\n')
        f.write(f'rate: {total["rate"]}\n')
        f.write(f'expected_doublets: {total["expected_doublets"]:.4f}\n')
        f.write(f'called: {total["called"]}\n')
        f.write('pair_counts: ' + ' '.join(f'{a}-{b}:{n}'
            for (a, b), n in total['pair_counts'].items()) + '\n')
        f.write('top_cells: ' + _name_values(index, p, top) + '\n')
    return paths


def save_placement(out_dir, chain, est, tables, assignment, names=None):
    """The placement files of postproc.place_cells for one (chain, estimator) row.
    placement_<est>_<chain>.tsv: per new cell its name (`names`, the names of
    the file of new cells, when there is one per cell, else 0..Q-1),
    `cluster` (`new` where the cell opens a cluster of its own), `prob`,
    `next_cluster`, `next_prob`, `p_new`, `entropy`, `n_obs`, `lpd`,
    `lpd_per_obs`, then the probability of every cluster; cluster ids are the
    labels of `assignment` (cluster k of the tables is the k-th smallest),
    floats %.4f.  placement_summary_<est>_<chain>.txt: `key: value` lines -
    samples, cells, clusters, placed (per cluster id:count), new, lpd,
    mean_lpd_per_obs and worst_cells, the ten cells with the smallest lpd per
    observed entry as name:value pairs."""
    ids = np.unique(np.asarray(assignment))
    prob = tables['prob']
    index = _row_names(names, prob.shape[0]).tolist()
    paths = _paths(out_dir, ('placement.tsv', 'placement_summary.txt'), est,
        chain)

    def cluster_id(k):
        return 'new' if k < 0 else str(ids[k])
    nxt = tables['next_cluster']
    with open(paths[0], 'w') as f:
        f.write('cell\tcluster\tprob\tnext_cluster\tnext_prob\tp_new\t'
            'entropy\tn_obs\tlpd\tlpd_per_obs\t'
            + '\t'.join(str(i) for i in ids.tolist()) + '\n')
        for i, name in enumerate(index):
            other = ids[nxt[i]] if nxt[i] >= 0 else -1
            f.write(f'{name}\t{cluster_id(tables["cluster"][i])}\t'
                f'{tables["cluster_prob"][i]:.4f}\t{other}\t'
                f'{tables["next_prob"][i]:.4f}\t{tables["p_new"][i]:.4f}\t'
                f'{tables["entropy"][i]:.4f}\t{int(tables["n_obs"][i])}\t'
                f'{tables["lpd"][i]:.4f}\t{tables["lpd_per_obs"][i]:.4f}\t'
                + '\t'.join(f'{x:.4f}' for x in prob[i].tolist()) + '\n')
    total = tables['total']
    per_obs = tables['lpd_per_obs']
    with open(paths[1], 'w') as f:
        for key in ('samples', 'cells', 'clusters'):
            f.write(f'{key}: {total[key]}\n')
        f.write('placed: ' + ' '.join(f'{ids[k]}:{n}'
            for k, n in enumerate(total['placed'])) + '\n')
        f.write(f'new: {total["new"]}\n')
        f.write(f'lpd: {total["lpd"]:.4f}\n')
        f.write(f'mean_lpd_per_obs: {total["mean_lpd_per_obs"]:.4f}\n')
        f.write('worst_cells: '
            + _name_values(index, per_obs, total['worst_cells']) + '\n')
    return paths


# the most mutations whose pairs save_mutation_order lists one by one
# (M (M - 1) / 2 lines: half a million at the limit)
MUTATION_PAIRS_MAX = 1000


def save_mutation_order(out_dir, chain, est, tables, names=None):
    """The -po files of postproc.mutation_order for one (chain, estimator)
    row.  mutation_order_<est>_<chain>.tsv: per mutation its name (`names`,
    the loader's mutation names, when there is one per mutation, else
    0..M-1), `carried`, `depth`, `parent` (a name, or `root`), `p_parent`,
    `same_as` (a name, or `-`), `n_same`, `n_descendants`, `n_exclusive`,
    `conflict`, `worst_conflict` (a name, or `-`), `p_worst_conflict`; floats
    %.4f.  mutation_order_summary_<est>_<chain>.txt: `key: value` lines -
    samples, mutations, pairs, min_cells, the shares of the pairs that are
    ancestral, same, exclusive, conflict, absent or undecided, mean_conflict,
    roots, max_depth, skipped_ancestors, most_conflicting (name:value pairs)
    and pairs_table (`written`, or `skipped` above MUTATION_PAIRS_MAX
    mutations).  mutation_pairs_<est>_<chain>.tsv, up to that limit: every
    pair a < b with `p_anc` (a ancestral to b), `p_desc` (b to a), `p_same`,
    `p_excl`, `p_conflict`."""
    M = tables['carried'].size
    index = _row_names(names, M).tolist()
    paths = _paths(out_dir, ('mutation_order.tsv',
        'mutation_order_summary.txt', 'mutation_pairs.tsv'), est, chain)
    columns = ('carried', 'depth', 'parent', 'p_parent', 'same_as', 'n_same',
        'n_descendants', 'n_exclusive', 'conflict', 'worst_conflict',
        'p_worst_conflict')
    named = {'parent': 'root', 'same_as': '-', 'worst_conflict': '-'}
    whole = ('depth', 'n_same', 'n_descendants', 'n_exclusive')

    def cell(key, val):
        if key in named:
            return str(index[int(val)]) if val >= 0 else named[key]
        return str(int(val)) if key in whole else f'{val:.4f}'
    with open(paths[0], 'w') as f:
        f.write('mutation\t' + '\t'.join(columns) + '\n')
        for m, name in enumerate(index):
            f.write(f'{name}\t'
                + '\t'.join(cell(k, tables[k][m]) for k in columns) + '\n')
    total = tables['total']
    S = total['samples']
    listed = M <= MUTATION_PAIRS_MAX
    with open(paths[1], 'w') as f:
        for key in ('samples', 'mutations', 'pairs', 'min_cells'):
            f.write(f'{key}: {total[key]}\n')
        for key in ('ancestral', 'same', 'exclusive', 'conflict', 'absent',
                'undecided', 'mean_conflict'):
            f.write(f'{key}: {total[key]:.4f}\n')
        for key in ('roots', 'max_depth', 'skipped_ancestors'):
            f.write(f'{key}: {total[key]}\n')
        f.write('most_conflicting: ' + _name_values(index,
            tables['conflict'], total['most_conflicting']) + '\n')
        f.write(f'pairs_table: {"written" if listed else "skipped"}\n')
    if not listed:
        return paths[:2]
    anc, same, excl, conf = (tables[k] for k in ('anc', 'same', 'excl',
        'conf'))
    with open(paths[2], 'w') as f:
        f.write('a\tb\tp_anc\tp_desc\tp_same\tp_excl\tp_conflict\n')
        for a in range(M):
            for b in range(a + 1, M):
                f.write(f'{index[a]}\t{index[b]}\t' + '\t'.join(
                    f'{int(t[a, b]) / S:.4f}'
                    for t in (anc, anc.T, same, excl, conf)) + '\n')
    return paths


def save_chain_agreement(out_dir, chain, est, tables, names=None):
    """The -pc files of postproc.chain_agreement for one (chain, estimator)
    row.  chain_agreement_<est>_<chain>.tsv: per cell its name (`names`, the
    loader's cell names, when there is one per cell, else 0..N-1), `cluster`
    (its label of assignment.txt), `worst_chain`, `worst_diff`, then per
    chain c `diff_<c>`, `max_<c>`, `flips_<c>`; floats %.4f, flips as
    integers.  chain_summary_<est>_<chain>.txt: `key: value` lines - chains,
    samples (per chain), cells, pairs, per chain mean_diff, max_diff and
    flip_share, worst_chain (the largest mean_diff, as chain:value),
    cluster_diff (per cluster its label and the chains' values, clusters
    separated by `;`) and unstable_cells, the ten cells with the largest
    worst_diff (ties: the smaller index) as name:value pairs."""
    N, C = tables['diff'].shape
    index = _row_names(names, N).tolist()
    paths = _paths(out_dir, ('chain_agreement.tsv', 'chain_summary.txt'),
        est, chain)
    with open(paths[0], 'w') as f:
        f.write('cell\tcluster\tworst_chain\tworst_diff\t' + '\t'.join(
            f'diff_{c}\tmax_{c}\tflips_{c}' for c in range(C)) + '\n')
        for i, name in enumerate(index):
            f.write(f'{name}\t{int(tables["cluster"][i])}\t'
                f'{int(tables["worst_chain"][i])}\t'
                f'{tables["worst_diff"][i]:.4f}\t' + '\t'.join(
                f'{tables["diff"][i, c]:.4f}\t{tables["max_diff"][i, c]:.4f}'
                f'\t{int(tables["flips"][i, c])}' for c in range(C)) + '\n')
    total = tables['total']
    worst = tables['worst_diff']
    top = np.argsort(-worst, kind='stable')[:10]
    with open(paths[1], 'w') as f:
        f.write(f'chains: {total["chains"]}\n')
        f.write('samples: ' + ' '.join(str(int(x))
            for x in tables['samples']) + '\n')
        f.write(f'cells: {total["cells"]}\n')
        f.write(f'pairs: {total["pairs"]}\n')
        for key, name in (('mean_diff_c', 'mean_diff'),
                ('max_diff_c', 'max_diff'), ('flip_share_c', 'flip_share')):
            f.write(f'{name}: ' + ' '.join(f'{x:.4f}'
                for x in tables[key]) + '\n')
        f.write(f'worst_chain: {total["worst_chain"]}:'
            f'{total["worst_mean_diff"]:.4f}\n')
        f.write('cluster_diff: ' + '; '.join(f'{int(k)} ' + ' '.join(
            f'{x:.4f}' for x in row) for k, row in zip(tables['clusters'],
            tables['cluster_diff'])) + '\n')
        f.write('unstable_cells: '
            + _name_values(index, worst, top.tolist()) + '\n')
    return paths


def save_metric(path, column, rows):
    """V_measure.txt / ARI.txt / hammingDist.txt (dpmmIO.py:514-542): a
    tab-separated `chain  estimator  <column>` table, floats as to_csv
    writes float64 (their repr)."""
    with open(path, 'w') as f:
        f.write(f'chain\testimator\t{column}\n')
        for chain, est, score in rows:
            f.write(f'{chain}\t{est}\t{float(score)!r}\n')
