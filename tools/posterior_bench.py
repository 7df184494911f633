#!/usr/bin/env python3
"""Phases of the posterior estimator's clustering step (postproc.get_MPEAR) on
synthetic posterior samples: N cells, S samples around C true clusters.
usage: posterior_bench.py N S [C]

With GENO_M=<mutations> the genotype pass follows on the best cut, with a
random float32 trace of GENO_W (default C + 8) rows per sample: the device
pass (bnpc_post_genotypes, trace upload included; its kernels alone:
rocprofv3 --kernel-trace --stats) and - GENO_HOST=1 - the host loop
(postproc.host_genotypes).
GENO_TABLE=<dir>: the genotype table writer (io.save_geno) into that
directory, files removed afterwards.
SUPPORT=1: right after the pair counts are made, the three passes that read
all of them - k_differ_sum, one k_mpear_sums pass, the support pass
(k_post_support) - beside each other on that matrix for the C true clusters,
by device events (Posterior.pass_times), and Posterior.support as a call
(table to the host included) checked against the two others; then exit.
CELLS_M=<mutations>: right after the pair counts are made, the per-cell
genotype pass (bnpc_post_cell_genotypes) with a random float32 trace of
CELLS_W (default C + 8) rows per sample, CELLS_CHUNK samples per upload and
CELLS_SLAB cells per pass over the trace (0: the defaults): CELLS_REPS
(default 5) calls without the tables' way back, each by device events
(Posterior.cell_genotypes_times) - the fastest one's trace uploads, rank
kernel and accumulation kernel, the element-steps per second of the kernels
against the device's FP64 vector add rate, the uploads' share - then the call
with its three tables brought to the host, and - CELLS_HOST=1 - the host loop
(postproc.host_cell_genotypes) compared with it; then - CELLS_FIT=1 - the
per-cell fit pass (bnpc_post_cell_fit) over the same trace with random data
(30 % missing) and error rates, CELLS_REPS calls by device events
(Posterior.cell_fit_times): the fastest one's uploads and its four kernels,
the table bytes per second k_cf_sums reads (8 per observed entry, cell and
sample) beside the trace bytes per second of k_cg_accum (4 per cell, mutation
and sample), then the call with its results brought to the host; then -
MUT_FIT=1 - the per-mutation fit pass (bnpc_post_mutation_fit) over the same
trace, data and error rates, CELLS_REPS calls by device events
(Posterior.mutation_fit_times) for each of three hints - the true clusters
(sorted), the last sample's labels (the default) and random labels: the
fastest one's uploads and mask kernel, k_cg_rank, k_mf_count, k_mf_reduce
beside k_cf_sums of the same run, then the call with its vectors brought to
the host; then exit.
With DOUBLETS=1 and DOUBLETS_M=<mutations> (two samples are enough: the pass
reads none): the doublet pass (bnpc_post_doublets) for the base clustering of C
clusters with random genotypes (a tenth of them soft), random data (30 %
missing), DOUBLETS_CHUNK candidates and DOUBLETS_SLAB cells at a time (0: the
defaults): DOUBLETS_REPS calls by device events (Posterior.doublets_times) -
the fastest one's uploads and mask kernel, k_db_tables, k_db_sums,
k_db_reduce, the (cell, candidate, mutation) steps per second of k_db_sums
(two float64 FMAs each) beside the device's FP64 vector rate - then the call
with its seven vectors brought to the host, and - DOUBLETS_HOST=1 - the host
loop (postproc.host_doublets); then exit.
CHAINS=<C>: right after the pair counts are made, the between-chain agreement
pass (bnpc_post_chain_agreement) with the S samples cut into C chains of equal
length (the first S mod C one longer): the pass - the tables' zeroing and
k_chain_agree - beside one k_codist launch over the same samples, by device
events, the fastest of CHAINS_REPS (default 5) each
(Posterior.chain_agreement_times), the label compares per second of both and
the atomics the pass issues at most; then the call with its three tables
brought to the host and - CHAINS_HOST=1 - the host loop
(postproc.host_chain_agreement) compared with it; then exit.
PLACE=1: right after the pair counts are made, the placement pass
(bnpc_post_place) of PLACE_Q (default N) new cells x PLACE_M (default 1000)
mutations of random data (30 % missing) against a random float32 trace of
PLACE_W (default C + 8) rows per sample, PLACE_CHUNK samples and PLACE_SLAB new
cells at a time (0: the defaults): PLACE_REPS (default 3) calls by device
events (Posterior.place_times) - the fastest one's uploads and mask kernel,
k_cg_rank, k_pn_tables, k_pn_counts, k_db_sums and the reductions, the scores
per second of k_db_sums - then the call with its results brought to the host,
then k_db_sums of the doublet pass at the same new cells and the nearest
number of candidates, its scores per second and the ratio of the two; with
PLACE_HOST=<samples>,<new cells> the host loop (postproc.host_place) and the
device on that many of both; then exit.
ORDER=1: right after the pair counts are made, the mutation-order pass
(bnpc_post_mutation_order) of ORDER_M (default 1000) mutations against a
random float32 trace of ORDER_W (default C + 8) rows per sample - every row a
random subset of the mutations, so that all relations occur - with ORDER_MIN
(default 2) cells a live cluster, ORDER_CHUNK samples and ORDER_SLAB table rows
at a time (0: the defaults): ORDER_REPS (default 5) calls by device events
(Posterior.mutation_order_times) - the fastest one's uploads, ranks and live
rows, k_po_masks and k_po_pairs, the pair-samples per second of k_po_pairs
(the unordered pairs with the diagonal where one slab holds all rows, else all
ordered pairs) and their share of the device's 32-bit vector issue rate at the
24 vector instructions a pair-sample costs in the one-word kernel - then the
call with its four tables brought to the host; with ORDER_HOST=<samples> the
host loop (postproc.host_mutation_order) and the device on that many samples,
compared; then exit."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from scipy.cluster.hierarchy import cut_tree, linkage  # noqa: E402

from bnpc_amd import _lib, postproc  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 5000
S = int(sys.argv[2]) if len(sys.argv) > 2 else 400
C = int(sys.argv[3]) if len(sys.argv) > 3 else 10
rng = np.random.RandomState(0)
base = rng.randint(0, C, N)
a = np.tile(base, (S, 1)).astype(np.int32)
flip = rng.random_sample((S, N)) < 0.03
a[flip] = rng.randint(0, C, flip.sum())


def lap(label, t0):
    t1 = time.perf_counter()
    print(f'  {label:46s} {t1 - t0:8.3f} s', flush=True)
    return t1


print(f'N={N} S={S} C={C}: {N * (N - 1) // 2:.3e} pairs')
t0 = t_all = time.perf_counter()
post = _lib.Posterior(a)
t0 = lap('pair counts on the device (k_codist) + their sum', t0)
if os.environ.get('SUPPORT') == '1':
    labels = np.unique(base, return_inverse=True)[1]
    K = int(labels.max()) + 1
    read = 4 * post.pairs
    t_sum, t_mpear, t_sup = post.pass_times(labels, reps=5)
    print(f'  passes over the {read / 1e9:.2f} GB of pair counts, K={K} '
        '(device events, fastest of 5):')
    for name, t, times in (('k_differ_sum', t_sum, 1),
            ('k_mpear_sums, 1 candidate', t_mpear, 1),
            ('k_post_support (reads twice)', t_sup, 2)):
        print(f'    {name:32s} {t * 1e3:9.3f} ms  '
            f'{times * read / t / 1e9:8.1f} GB/s', flush=True)
    print(f'    support / differ_sum time: {t_sup / t_sum:.2f}x')
    t0 = time.perf_counter()
    differ_to = post.support(labels)
    t0 = lap('Posterior.support (call, N x K table to the host)', t0)
    print('  sum == 2 differ_sum:', int(differ_to.sum()) == 2 * post.differ_sum,
        '; own == 2 mpear sum:', int(differ_to[np.arange(N), labels].sum())
        == 2 * int(post.mpear_sums(labels[None])[0]))
    post.close()
    sys.exit(0)
if os.environ.get('CHAINS'):
    n_chains = int(os.environ['CHAINS'])
    reps = int(os.environ.get('CHAINS_REPS', '5'))
    lengths = np.full(n_chains, S // n_chains)
    lengths[:S % n_chains] += 1
    bounds = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    compares = S * N * (N - 1) // 2
    tiles = ((N + 63) // 64) * ((N + 63) // 64 + 1) // 2
    t_pass, t_codist = post.chain_agreement_times(bounds, reps)
    print(f'chain agreement: {n_chains} chains of {lengths.min()}..'
        f'{lengths.max()} samples, {compares:.3e} label compares, at most '
        f'{384 * tiles * n_chains:.3e} 64-bit atomics, tables '
        f'{24 * n_chains * N / 1e6:.2f} MB (device events, fastest of '
        f'{reps}):')
    for name, t in (('k_chain_agree + zeroing', t_pass),
            ('k_codist', t_codist)):
        print(f'    {name:32s} {t * 1e3:9.3f} ms  {compares / t:.3e} '
            'compares/s', flush=True)
    print(f'    pass / k_codist time: {t_pass / t_codist:.3f}x')
    t0 = time.perf_counter()
    got = post.chain_agreement(bounds)
    t0 = lap('Posterior.chain_agreement (call, three tables to the host)', t0)
    if os.environ.get('CHAINS_HOST') == '1':
        want = postproc.host_chain_agreement(a, bounds)
        t0 = lap('host loop (postproc.host_chain_agreement)', t0)
        print('  device == host:', all(np.array_equal(g, w)
            for g, w in zip(got, want)))
    post.close()
    sys.exit(0)
if os.environ.get('DOUBLETS') == '1':
    # FP64 vector operations per second: 256 compute units x 4 SIMDs x 32
    # lanes at 2.4 GHz retire one float32 operation per lane and cycle (157.3
    # TFLOPS of FMA), a float64 one every other cycle
    F64_OPS = 256 * 4 * 32 * 2.4e9 / 2
    M = int(os.environ.get('DOUBLETS_M', '1000'))
    chunk = int(os.environ.get('DOUBLETS_CHUNK', '0'))
    slab = int(os.environ.get('DOUBLETS_SLAB', '0'))
    reps = int(os.environ.get('DOUBLETS_REPS', '5'))
    labels = np.unique(base, return_inverse=True)[1]
    K = int(labels.max()) + 1
    P = K + K * (K - 1) // 2
    theta = (rng.random_sample((K, M)) < 0.3).astype(np.float64)
    soft = rng.random_sample((K, M)) < 0.1
    theta[soft] = rng.random_sample(int(soft.sum()))
    data = (rng.random_sample((N, M)) < 0.3).astype(np.uint8)
    data[rng.random_sample((N, M)) < 0.3] = 3
    FN, FP = 0.2, 0.001
    steps = N * P * M
    print(f'doublets: M={M} K={K} P={P} chunk={chunk} slab={slab}, tables '
        f'{P * M * 16 / 1e9:.3f} GB, scores {N * P * 8 / 1e9:.3f} GB, '
        f'{steps:.3e} (cell, candidate, mutation) steps')
    runs = []
    for r in range(reps):
        t = post.doublets_times(data, labels, theta, FN, FP, chunk=chunk,
            slab=slab)
        runs.append((sum(t),) + t)
        print(f'  rep {r}: uploads + k_mf_masks {t[0] * 1e3:.3f} ms  '
            f'k_db_tables {t[1] * 1e3:.3f} ms  k_db_sums {t[2] * 1e3:.3f} ms  '
            f'k_db_reduce {t[3] * 1e3:.3f} ms', flush=True)
    total, d_up, d_tab, d_sum, d_red = min(runs)
    print(f'  fastest of {reps} (device events): pass {total * 1e3:.3f} ms; '
        f'k_db_sums {steps / d_sum:.3e} steps/s = {2 * steps / d_sum:.3e} '
        f'float64 FMAs/s, {2 * steps / d_sum / F64_OPS:.1%} of the FP64 '
        f'vector rate {F64_OPS:.3e}/s', flush=True)
    t0 = time.perf_counter()
    got = post.doublets(data, labels, theta, FN, FP, chunk=chunk, slab=slab)
    t0 = lap('Posterior.doublets (call, seven vectors to the host)', t0)
    if os.environ.get('DOUBLETS_HOST') == '1':
        want = postproc.host_doublets(data, labels, theta, FN, FP)
        t0 = lap('host loop (postproc.host_doublets)', t0)
        print('  best single and pair, device == host:',
            np.array_equal(got[5], want['best_single']),
            np.array_equal(got[6], want['best_pair']),
            '; max |ll_pair dev - host| =',
            float(np.abs(got[3] - want['ll_pair']).max()))
    post.close()
    sys.exit(0)
if os.environ.get('ORDER') == '1':
    # 32-bit vector instructions per second, per lane: 256 compute units x 4
    # SIMDs x 32 lanes at 2.4 GHz
    INT_OPS = 256 * 4 * 32 * 2.4e9
    PAIR_OPS = 24       # of the one-word k_po_pairs, counted in its ISA
    M = int(os.environ.get('ORDER_M', '1000'))
    W = int(os.environ.get('ORDER_W', str(C + 8)))
    min_cells = int(os.environ.get('ORDER_MIN', '2'))
    chunk = int(os.environ.get('ORDER_CHUNK', '0'))
    slab = int(os.environ.get('ORDER_SLAB', '0'))
    reps = int(os.environ.get('ORDER_REPS', '5'))
    params = np.empty((S, W, M), dtype=np.float32)
    rate = rng.random_sample(M) ** 2
    for s in range(S):
        params[s] = np.where(rng.random_sample((W, M)) < rate, 0.9, 0.1)
    sym = slab == 0 or slab >= M
    pairs = M * (M + 1) // 2 if sym else M * M
    print(f'mutation order: M={M} W={W} ({(W + 63) // 64} mask words) '
        f'min_cells={min_cells} chunk={chunk} slab={slab}, trace '
        f'{params.nbytes / 1e9:.2f} GB, tables {16 * M * M / 1e9:.2f} GB, '
        f'{S * pairs:.3e} pair-samples')
    runs = []
    for r in range(reps):
        t = post.mutation_order_times(params, min_cells, chunk, slab)
        runs.append((sum(t),) + t)
        print(f'  rep {r}: uploads {t[0] * 1e3:.3f} ms  k_cg_rank + k_po_live '
            f'{t[1] * 1e3:.3f} ms  k_po_masks {t[2] * 1e3:.3f} ms  k_po_pairs '
            f'{t[3] * 1e3:.3f} ms', flush=True)
    total, _, _, _, t_pairs = min(runs)
    t_pairs = min(r[4] for r in runs)
    print(f'  fastest of {reps} (device events): pass {total * 1e3:.3f} ms; '
        f'k_po_pairs {t_pairs * 1e3:.3f} ms = {S * pairs / t_pairs:.3e} '
        f'pair-samples/s, {PAIR_OPS * S * pairs / t_pairs / INT_OPS:.1%} of '
        f'the 32-bit vector issue rate {INT_OPS:.3e}/s', flush=True)
    t0 = time.perf_counter()
    got = post.mutation_order(params, min_cells, chunk, slab)
    t0 = lap('Posterior.mutation_order (call, four tables to the host)', t0)
    post.close()
    if os.environ.get('ORDER_HOST'):
        Sh = int(os.environ['ORDER_HOST'])
        t0 = time.perf_counter()
        want = postproc.host_mutation_order(a[:Sh], params[:Sh], min_cells)
        t0 = lap(f'host loop (postproc.host_mutation_order) at S={Sh}', t0)
        small = _lib.Posterior(a[:Sh])
        t0 = time.perf_counter()
        have = small.mutation_order(params[:Sh], min_cells, chunk, slab)
        t0 = lap(f'Posterior.mutation_order at S={Sh}', t0)
        small.close()
        print('  device == host:', all(np.array_equal(g, w)
            for g, w in zip(have, want)), '; counted:',
            [int(w.astype(np.int64).sum()) for w in want])
    sys.exit(0)
if os.environ.get('PLACE') == '1':
    M = int(os.environ.get('PLACE_M', '1000'))
    Q = int(os.environ.get('PLACE_Q', str(N)))
    W = int(os.environ.get('PLACE_W', str(C + 8)))
    chunk = int(os.environ.get('PLACE_CHUNK', '0'))
    slab = int(os.environ.get('PLACE_SLAB', '0'))
    reps = int(os.environ.get('PLACE_REPS', '3'))
    labels = np.unique(base, return_inverse=True)[1]
    params = np.empty((S, W, M), dtype=np.float32)
    for s in range(S):
        params[s] = np.clip(rng.random_sample((W, M)), 1e-3, 1 - 1e-3)
    new = (rng.random_sample((Q, M)) < 0.3).astype(np.uint8)
    new[rng.random_sample((Q, M)) < 0.3] = 3
    FN, FP = rng.uniform(0.1, 0.3, S), rng.uniform(1e-4, 1e-2, S)
    alpha = rng.uniform(0.5, 5.0, S)
    cands = int(sum(np.unique(row).size + 1 for row in a))
    steps = Q * cands * M
    print(f'placement: Q={Q} M={M} W={W} chunk={chunk} slab={slab}, trace '
        f'{params.nbytes / 1e9:.2f} GB, {cands} candidates over the samples, '
        f'{steps:.3e} (cell, candidate, mutation) steps')
    runs = []
    for r in range(reps):
        t = post.place_times(new, labels, params, FN, FP, alpha, chunk=chunk,
            slab=slab)
        runs.append((sum(t),) + t)
        print(f'  rep {r}: uploads + k_mf_masks {t[0] * 1e3:.3f} ms  k_cg_rank '
            f'{t[1] * 1e3:.3f} ms  k_pn_tables {t[2] * 1e3:.3f} ms  '
            f'k_pn_counts {t[3] * 1e3:.3f} ms  k_db_sums {t[4] * 1e3:.3f} ms  '
            f'k_pn_soft + k_pn_accum + k_pn_lpd {t[5] * 1e3:.3f} ms', flush=True)
    total, _, _, _, _, p_sum, _ = min(runs)
    print(f'  fastest of {reps} (device events): pass {total * 1e3:.3f} ms; '
        f'k_db_sums {Q * cands / p_sum:.3e} scores/s', flush=True)
    t0 = time.perf_counter()
    got = post.place(new, labels, params, FN, FP, alpha, chunk=chunk,
        slab=slab)
    t0 = lap('Posterior.place (call, Q x K table and vectors to the host)', t0)
    post.close()
    # the doublet pass' k_db_sums at the same Q and M and the smallest number
    # of candidates K (K + 1) / 2 that is not below the placement's
    K = 1
    while K * (K + 1) // 2 < cands:
        K += 1
    P = K * (K + 1) // 2
    dlab = rng.permutation(np.arange(Q) % K).astype(np.int32)
    theta = np.clip(rng.random_sample((K, M)), 1e-3, 1 - 1e-3)
    other = _lib.Posterior(np.stack([dlab, dlab]))
    runs = []
    for r in range(reps):
        t = other.doublets_times(new, dlab, theta, 0.2, 0.001)
        runs.append((t[2], t))
    d_sum = min(runs)[0]
    other.close()
    print(f'  doublets at Q={Q} M={M} K={K} P={P}: k_db_sums '
        f'{d_sum * 1e3:.3f} ms, {Q * P / d_sum:.3e} scores/s; placement / '
        f'doublets scores per second {(Q * cands / p_sum) / (Q * P / d_sum):.3f}',
        flush=True)
    if os.environ.get('PLACE_HOST'):
        Sh, Qh = (int(x) for x in os.environ['PLACE_HOST'].split(','))
        t0 = time.perf_counter()
        want = postproc.host_place(new[:Qh], a[:Sh], labels, params[:Sh],
            FN[:Sh], FP[:Sh], alpha[:Sh], (.25, .25), keep=False)
        t0 = lap(f'host loop (postproc.host_place) at S={Sh} Q={Qh}', t0)
        small = _lib.Posterior(a[:Sh])
        t0 = time.perf_counter()
        have = small.place(new[:Qh], labels, params[:Sh], FN[:Sh], FP[:Sh],
            alpha[:Sh])
        t0 = lap(f'Posterior.place at S={Sh} Q={Qh}', t0)
        small.close()
        print('  max |prob_sum dev - host| =',
            float(np.abs(have[0] - want['prob_sum']).max()),
            '; max |lpd dev - host| =',
            float(np.abs(have[3] - want['lpd']).max()))
    sys.exit(0)
CELLS_M = int(os.environ.get('CELLS_M', '0'))
if CELLS_M:
    # FP64 vector adds per second: 256 compute units x 4 SIMDs x 32 lanes at
    # 2.4 GHz retire one float32 operation per lane and cycle (157.3 TFLOPS
    # of FMA), a float64 one every other cycle
    F64_ADDS = 256 * 4 * 32 * 2.4e9 / 2
    W = int(os.environ.get('CELLS_W', str(C + 8)))
    chunk = int(os.environ.get('CELLS_CHUNK', '0'))
    slab = int(os.environ.get('CELLS_SLAB', '0'))
    reps = int(os.environ.get('CELLS_REPS', '5'))
    params = np.empty((S, W, CELLS_M), dtype=np.float32)
    for s in range(S):
        params[s] = rng.random_sample((W, CELLS_M))
    steps = N * CELLS_M * S
    print(f'cell genotypes: M={CELLS_M} W={W} chunk={chunk} slab={slab}, '
        f'trace {params.nbytes / 1e9:.2f} GB, tables '
        f'{N * CELLS_M * 20 / 1e9:.2f} GB, {steps:.3e} element-steps')
    runs = []
    for r in range(reps):
        t0 = time.perf_counter()
        t_up, t_rank, t_acc = post.cell_genotypes_times(params, chunk, slab)
        wall = time.perf_counter() - t0
        runs.append((t_up + t_rank + t_acc, t_up, t_rank, t_acc, wall))
        print(f'  rep {r}: uploads {t_up:.4f} s  k_cg_rank {t_rank:.4f} s  '
            f'k_cg_accum {t_acc:.4f} s  (host clock, whole call {wall:.4f} s)',
            flush=True)
    total, t_up, t_rank, t_acc, wall = min(runs)
    kern = t_rank + t_acc
    print(f'  fastest of {reps} (device events): pass {total:.4f} s = uploads '
        f'{t_up:.4f} s ({100 * t_up / total:.1f} %) + kernels {kern:.4f} s')
    print(f'    kernels: {steps / kern:.3e} element-steps/s = '
        f'{100 * steps / kern / F64_ADDS:.1f} % of {F64_ADDS:.3e} FP64 vector '
        f'adds/s (two float64 operations per element-step: '
        f'{100 * 2 * steps / kern / F64_ADDS:.1f} %); whole pass '
        f'{steps / total:.3e} element-steps/s', flush=True)
    t0 = time.perf_counter()
    got = post.cell_genotypes(params, chunk, slab)
    t0 = lap('Posterior.cell_genotypes (call, three tables to the host)', t0)
    if os.environ.get('CELLS_HOST') == '1':
        want = postproc.host_cell_genotypes(a, params)
        t0 = lap('host loop (postproc.host_cell_genotypes)', t0)
        print('  device == host:', all(np.array_equal(g, w)
            for g, w in zip(got, want)))
    fits = [k for k in ('CELLS_FIT', 'MUT_FIT') if os.environ.get(k) == '1']
    if fits:
        data = (rng.random_sample((N, CELLS_M)) < 0.3).astype(np.uint8)
        data[rng.random_sample((N, CELLS_M)) < 0.3] = 3
        FN, FP = rng.uniform(0.1, 0.3, S), rng.uniform(1e-4, 1e-2, S)
        seen = int((data != 3).sum()) * S
        f_sum = None
    if 'CELLS_FIT' in fits:
        print(f'cell fit: {seen:.3e} observed element-steps of {steps:.3e}, '
            f'LL {S * N * 8 / 1e9:.2f} GB')
        runs = []
        for r in range(reps):
            t = post.cell_fit_times(data, params, FN, FP, chunk, slab)
            runs.append((sum(t),) + t)
            print(f'  rep {r}: uploads {t[0]:.4f} s  k_cg_rank {t[1]:.4f} s  '
                f'k_cf_tables {t[2]:.4f} s  k_cf_sums {t[3]:.4f} s  '
                f'k_cf_reduce {t[4]:.4f} s', flush=True)
        total, f_up, f_rank, f_tab, f_sum, f_red = min(runs)
        print(f'  fastest of {reps} (device events): pass {total:.4f} s; '
            f'k_cf_sums reads {8 * seen / f_sum / 1e9:.1f} GB/s of tables, '
            f'k_cg_accum {4 * steps / t_acc / 1e9:.1f} GB/s of trace; '
            f'k_cf_sums / k_cg_accum time {f_sum / t_acc:.2f}x', flush=True)
        t0 = time.perf_counter()
        post.cell_fit(data, params, FN, FP, chunk, slab)
        t0 = lap('Posterior.cell_fit (call, three vectors to the host)', t0)
    if 'MUT_FIT' in fits:
        if f_sum is None:
            f_sum = post.cell_fit_times(data, params, FN, FP, chunk, slab)[3]
        print(f'mutation fit: lane masks {(N + 63) // 64 * CELLS_M * 16 / 1e9:.2f}'
            f' GB; k_cf_sums of this run {f_sum:.4f} s')
        hints = (('sorted hint (true clusters)', base),
            ('no hint (last sample)', None),
            ('random hint', rng.randint(0, C, N)))
        for name, hint in hints:
            runs = []
            for r in range(reps):
                t = post.mutation_fit_times(data, params, FN, FP, hint, chunk)
                runs.append((sum(t),) + t)
            total, m_up, m_rank, m_cnt, _, m_red = min(runs)
            print(f'  {name}, fastest of {reps} (device events): pass '
                f'{total:.4f} s = uploads + k_mf_masks {m_up:.4f} s  '
                f'k_cg_rank {m_rank:.4f} s  k_mf_count {m_cnt:.4f} s  '
                f'k_mf_reduce {m_red:.4f} s; k_mf_count / k_cf_sums time '
                f'{m_cnt / f_sum:.3f}x', flush=True)
        t0 = time.perf_counter()
        post.mutation_fit(data, params, FN, FP, base, chunk)
        t0 = lap('Posterior.mutation_fit (call, seven vectors to the host)',
            t0)
    post.close()
    sys.exit(0)
tree = post.ward()
t0 = lap('Ward linkage on the device (k_ward_chain|work) + relabel', t0)
scans, steps = post.ward_stats()
print(f'    ({scans} full row scans for {N - 1} merges and {steps} chain '
    'steps: the other steps took the row\'s cached nearest neighbour)')
if os.environ.get('WARD_CHECK'):
    dist = post.dist()
    t0 = lap('mean distance divided on the device -> host f64', t0)
    want = linkage(dist, method='ward')
    t0 = lap('Ward linkage (SciPy, host)', t0)
    print('  device linkage == SciPy linkage:', np.array_equal(tree, want))
    del dist
sizable = [int((np.unique(r, return_counts=True)[1] > 2).sum()) for r in a]
avg = np.mean(sizable)
cand = np.arange(max(2, avg * 0.2), min(avg * 2.5, N), dtype=int)
cuts = postproc.cut_tree_labels(tree, cand)
t0 = lap(f'tree cuts for {cand.size} candidates (cut_tree_labels)', t0)
labels = np.ascontiguousarray(cuts.T)
sums = post.mpear_sums(labels)
t0 = lap(f'MPEAR sums of {cand.size} candidates (k_mpear_sums)', t0)
scores = postproc.mpear_scores(sums, labels, post.differ_sum, S)
best = int(np.argmax(scores))
t0 = lap('scores from the integers (host)', t0)
print(f'  total {time.perf_counter() - t_all:.3f} s; best cut: '
    f'{cand[best]} clusters, MPEAR {scores[best]:.6f}')
GENO_M = int(os.environ.get('GENO_M', '0'))
if GENO_M:
    W = int(os.environ.get('GENO_W', str(C + 8)))
    assign = np.ascontiguousarray(cuts[:, best])
    params = np.empty((S, W, GENO_M), dtype=np.float32)
    for s in range(S):
        params[s] = rng.random_sample((W, GENO_M))
    print(f'genotypes: K={cand[best]} M={GENO_M} W={W}, trace '
        f'{params.nbytes / 1e9:.2f} GB')
    t0 = time.perf_counter()
    geno = post.genotypes(assign, params)
    t0 = lap('device pass (bnpc_post_genotypes, upload included)', t0)
    if os.environ.get('GENO_HOST') == '1':
        want = postproc.host_genotypes(a, assign, params)
        t0 = lap('host loop (postproc.host_genotypes)', t0)
        print('  device == host:', np.array_equal(geno, want))
    out_dir = os.environ.get('GENO_TABLE')
    if out_dir:
        from bnpc_amd import io as bio
        os.makedirs(out_dir, exist_ok=True)
        t0 = time.perf_counter()
        paths = bio.save_geno(out_dir, 'mean', 'posterior', geno, assign,
            assign.tolist())
        t0 = lap('genotype tables written (io.save_geno)', t0)
        for path in paths:
            print(f'    {os.path.basename(path)}: '
                f'{os.path.getsize(path) / 1e9:.2f} GB')
            os.remove(path)
post.close()
if len(sys.argv) > 4:       # the reference-order host evaluation, one candidate
    d = _lib.codist(a) / S
    t0 = time.perf_counter()
    s = postproc.calc_MPEAR(1 - d, labels[best])
    print(f'  host calc_MPEAR of ONE candidate: {time.perf_counter() - t0:.3f}'
        f' s (x {cand.size} candidates in the old path); score {s:.6f}')
