"""Post-processing the driver and the CLI need.

Restated from /root/reference/libs/utils.py: the lugsail batch-means PSRF
(:427-467, used by the -ls termination mode and the run summary), the ML / MAP
point estimates (:248-282) and the posterior estimator (:90-244: mean
co-clustering distance, MPEAR-selected Ward clustering, averaged cluster
genotypes).  The O(samples x cells^2) co-clustering distance - the next
data-parallel kernel after the likelihood path (SURVEY.md section 8(f) rank
4) - and the MPEAR score of every candidate cut run on the GPU (bnpc_post:
the pair counts stay there, each candidate is one term of ONE pass over
them); Ward's linkage and the tree cuts are SciPy on the host.
The per-cluster genotype averaging that follows is a device pass as well
(bnpc_post_genotypes; host_genotypes is the host loop it is pinned to).
The -ps tables (per-cell cluster support, cluster similarity: the data of the
reference's similarity heat map, dpmmIO.py:245-274, summed per cluster) come
from one more device pass over the pair counts (bnpc_post_support;
host_support is the host loop it is pinned to).
The -pg tables (per-cell posterior genotypes: the parameter of whichever
cluster a cell was in, averaged over the samples - not a reference output)
are a device pass over the samples and the parameter trace
(bnpc_post_cell_genotypes; host_cell_genotypes is the host loop it is pinned
to).
The -pf tables (per-cell posterior fit and the run's WAIC, from the pointwise
log-likelihood of every cell in every sample - not a reference output) are a
device pass over the samples, the parameter trace and the data
(bnpc_post_cell_fit; host_cell_fit is the host loop it is pinned to).
The -pm tables (per-mutation posterior fit and the error rates every column
implies - not a reference output) are a device pass over the same inputs
(bnpc_post_mutation_fit; host_mutation_fit is the host loop it is pinned to).
The -pd tables (doublet scores: every cell against every cluster of the MPEAR
clustering and every pair of them - not a reference output) are a device pass
over the data and the cluster genotypes (bnpc_post_doublets; host_doublets is
the host loop it is pinned to).
The -pc tables (every chain's co-clustering against that of the other chains
pooled - not a reference output) are one more pass of the pair-count tile loop
over the samples, chain by chain (bnpc_post_chain_agreement;
host_chain_agreement is the host loop it is pinned to).
The -po tables (the relation of every pair of mutations under the
three-gamete rule, counted over the samples, and the mutation forest they
imply - not a reference output) are a device pass over the samples and the
parameter trace, on cluster bit masks (bnpc_post_mutation_order;
host_mutation_order is the host loop it is pinned to).
The -tc / -td metrics (V-measure, ARI, Hamming; utils.py:49-72) are
restated from integer counts at the end; tree helpers are out of scope.
"""
import numpy as np

EPSILON = np.finfo(np.float64).resolution


def _tau_lugsail(b, data, chain_mean):
    """Batch-means variance estimate with batch size b (utils.py:463-466)."""
    a = data.size // b
    batch_mean = np.mean(np.reshape(data[:a * b], (a, b)), axis=1)
    return (b / (a - 1)) * np.sum(np.square(batch_mean - chain_mean))


def get_lugsail_batch_means_est(data_in, steps=None):
    """Lugsail PSRF of Vats & Knudson (2018), eq. 5, over the ML traces of the
    chains: data_in = [(trace, burn_in), ...]  (utils.py:427-461)."""
    T_iL, s_i, n_i = [], [], []
    for trace, burn_in in data_in:
        data = trace[burn_in:steps]
        if data.size < 9:
            return np.inf
        n = data.size
        b = int(n ** 0.5)
        n_i.append(n)
        mean = np.mean(data)
        T_iL.append(2 * _tau_lugsail(b, data, mean)
            - _tau_lugsail(b // 3, data, mean))
        s_i.append(np.var(data, ddof=1))
    T_L, s, n = np.mean(T_iL), np.mean(s_i), np.round(np.mean(n_i))
    sigma_L = ((n - 1) * s + T_L) / n
    try:
        with np.errstate(divide='raise', invalid='raise'):
            return np.sqrt(sigma_L / s)
    except FloatingPointError:
        return np.inf


def point_estimate(result, est, data):
    """The sample with the best ML / MAP after burn-in (utils.py:262-282)."""
    burn_in = result['burn_in']
    k = int(np.argmax(result[est][burn_in:]))
    step = k + burn_in
    assignment = np.asarray(result['assignments'][step])
    clusters = np.unique(assignment)
    params = result['params'][k][np.arange(clusters.size)]
    row_of = {c: i for i, c in enumerate(clusters)}
    cluster_of = np.array([row_of[c] for c in assignment], dtype=np.int64)
    geno = params[cluster_of]                               # cells x muts
    called = geno.round()
    FN_geno = (((called == 1) & (data == 0)).sum() + EPSILON) \
        / (called.sum() + EPSILON)
    FP_geno = (((called == 0) & (data == 1)).sum() + EPSILON) \
        / ((1 - called).sum() + EPSILON)
    return {'step': step, 'a': result['DP_alpha'][step],
        'assignment': assignment.tolist(), 'genotypes': geno,
        'cluster_genotypes': params, 'cluster_of': cluster_of,
        'FN': result['FN'][step], 'FP': result['FP'][step],
        'FN_geno': FN_geno, 'FP_geno': FP_geno}


def best_chain(results, est):
    scores = [np.max(r[est][r['burn_in']:]) for r in results]
    return results[int(np.argmax(scores))]


# ---------------------------------------------------------------------------
# posterior estimator (utils.py:90-244)
# ---------------------------------------------------------------------------
def get_dist(assignments):
    """Mean posterior co-clustering distance of all cell pairs, condensed in
    pdist order (utils.py:90-97); exact integer counts from the GPU."""
    from bnpc_amd import _lib
    differ = _lib.codist(assignments)
    return differ / np.asarray(assignments).shape[0]


def _same_cluster(labels):
    """Condensed (pdist order) indicator of the pairs that share a label:
    what `1 - pdist(stack([labels, labels]).T, 'hamming')` holds
    (utils.py:137-138), built row by row from integer comparisons instead of
    a 2-column float distance."""
    labels = np.asarray(labels)
    n = labels.size
    same = np.empty(n * (n - 1) // 2, dtype=bool)
    at = 0
    for i in range(n - 1):
        np.equal(labels[i + 1:], labels[i], out=same[at:at + n - 1 - i])
        at += n - 1 - i
    return same


def calc_MPEAR(pi, labels):
    """Posterior expected adjusted Rand index of a clustering
    (Fritsch & Ickstadt 2009, eq. 13; utils.py:133-145).  Same elementwise
    products and the same NumPy reductions as the reference, so the score has
    the same bits."""
    from scipy.special import binom
    same = _same_cluster(labels)
    I_sum, pi_sum = float(same.sum()), pi.sum()
    expected = (I_sum * pi_sum) / binom(labels.size, 2)
    return ((same * pi).sum() - expected) \
        / (.5 * (I_sum + pi_sum) - expected)


def mpear_scores(same_differ, labels, differ_sum, S):
    """MPEAR (Fritsch & Ickstadt 2009, eq. 13; utils.py:133-145) of C
    candidate clusterings from exact integers: with pi = 1 - differ / S over
    the P pairs,
        I_sum  = pairs that share a label        (from the label counts)
        pi_sum = P - differ_sum / S
        index  = sum of pi over those pairs = I_sum - same_differ / S.
    labels: (C, N)."""
    from scipy.special import binom
    labels = np.asarray(labels)
    N = labels.shape[1]
    P = binom(N, 2)
    pi_sum = P - differ_sum / S
    scores = np.empty(labels.shape[0])
    for c, lab in enumerate(labels):
        n_k = np.bincount(lab).astype(np.float64)
        I_sum = float((n_k * (n_k - 1) / 2).sum())
        index = I_sum - same_differ[c] / S
        expected = (I_sum * pi_sum) / P
        scores[c] = (index - expected) / (.5 * (I_sum + pi_sum) - expected)
    return scores


def cut_tree_labels(tree, n_clusters):
    """`scipy.cluster.hierarchy.cut_tree(tree, n_clusters=...)` for several
    cluster counts: (cells, len(n_clusters)) labels.  SciPy replays all N - 1
    merges with an O(N) relabelling each (12 s at 50 000 cells).  What it
    does, restated:
      * the merges are replayed in the order of `_order_cluster_tree`: by
        height, and among equal heights in REVERSE order of a breadth-first
        walk from the root that visits right children first (every internal
        node is `insort_left`-ed as the walk meets it);
      * a merged cluster takes the smaller of the two labels and the labels
        above the larger one move down - which keeps the clusters numbered
        in the order of their smallest member at every step.
    So a cut into n clusters is: the first N - n merges of that order as a
    union-find whose roots are the smallest members, clusters ranked by
    root.  Same labels (tests: Ward / average / single trees with tied
    heights), one pass over the merges + O(N) per cut."""
    from collections import deque
    tree = np.asarray(tree)
    N = tree.shape[0] + 1
    left = tree[:, 0].astype(np.int64)
    right = tree[:, 1].astype(np.int64)
    height = tree[:, 2]
    wanted = [min(max(int(n), 1), N) for n in n_clusters]
    out = np.empty((N, len(wanted)), dtype=np.int64)
    # breadth-first visiting rank of the internal nodes (root first, right
    # child before left)
    visit = np.zeros(N - 1, dtype=np.int64)
    queue, seen = deque([2 * N - 2] if N > 1 else []), 0
    while queue:
        node = queue.popleft()
        if node >= N:
            visit[node - N] = seen
            seen += 1
            queue.append(int(right[node - N]))
            queue.append(int(left[node - N]))
    order = np.lexsort((-visit, height))        # by height, ties reversed
    # smallest member of every node
    low = np.arange(2 * N - 1, dtype=np.int64)
    for i in range(N - 1):
        low[N + i] = min(low[left[i]], low[right[i]])
    parent = np.arange(N, dtype=np.int64)       # union-find over the cells
    stops = {}
    for col, n in enumerate(wanted):
        stops.setdefault(N - n, []).append(col)

    def snapshot(cols):
        root = parent.copy()
        while True:                             # pointer jumping
            nxt = root[root]
            if np.array_equal(nxt, root):
                break
            root = nxt
        labels = np.unique(root, return_inverse=True)[1]
        for col in cols:
            out[:, col] = labels

    if 0 in stops:
        snapshot(stops[0])
    for done, i in enumerate(order, start=1):
        a, b = low[left[i]], low[right[i]]      # roots: smallest members
        parent[max(a, b)] = min(a, b)
        if done in stops:
            snapshot(stops[done])
    return out


def get_MPEAR(assignments, dist=None):
    """The MPEAR clustering (utils.py:100-130); see _mpear."""
    assign, post = _mpear(assignments, dist)
    if post is not None:
        post.close()
    return assign


def _mpear(assignments, dist=None):
    """(MPEAR clustering, the open Posterior or None): Ward tree on the mean
    distance, cut where MPEAR is largest (utils.py:100-130).  Product path (dist is None): the pair counts are
    made and kept on the device, the mean distance comes to the host once
    for the linkage, and ALL candidate cuts are scored in one device pass
    over the counts (bnpc_post_mpear) - the float64 similarity `1 - dist`
    and the reference's pass over it per candidate are never made.  With a
    given `dist` the scores are evaluated on the host (calc_MPEAR).  The
    product path hands its Posterior, samples still on the device, to the
    caller, who closes it (mean_hierarchy_assignment: the genotype pass)."""
    from scipy.cluster.hierarchy import linkage
    from bnpc_amd import _lib
    assignments = np.asarray(assignments)
    post = None
    done = False
    try:
        if dist is None:
            import os
            post = _lib.Posterior(assignments)
            tree = None
            if os.environ.get('BNPC_WARD_DEVICE', '1') != '0':   # ('plain': no graph)
                # the linkage on the device too: the distance vector (10 GB at
                # 50 000 cells) is never brought to the host
                try:
                    tree = post.ward()
                except _lib.DeviceMemoryError as err:
                    # the full distance matrix (8 N^2 bytes) does not fit the
                    # device: SciPy's own routine on the condensed vector -
                    # the reference's call, the same tree.  Any OTHER failure
                    # (a device fault, a chain that did not close) is raised.
                    print(f'[bnpc] Ward linkage on the device: {err}; '
                        'using scipy.cluster.hierarchy.linkage')
            if tree is None:
                dist = post.dist()
                tree = linkage(dist, method='ward')
        else:
            tree = linkage(dist, method='ward')
        sizable = [int((np.unique(a, return_counts=True)[1] > 2).sum())
            for a in assignments]
        avg = np.mean(sizable)
        candidates = np.arange(max(2, avg * 0.2),
            min(avg * 2.5, assignments.shape[1]), dtype=int)
        if candidates.size == 0:
            # no candidate cut: the reference's loop does not run and its
            # best_assignment stays None (utils.py:116-130)
            done = True
            return None, post
        # every candidate cut of the tree (cut_tree's labels, without its
        # O(N^2) replay of the merges: 12 s at 50 000 cells)
        cuts = cut_tree_labels(tree, candidates)
        if post is not None and cuts.max() < 65534:
            dist = None
            labels = np.ascontiguousarray(cuts.T)
            scores = mpear_scores(post.mpear_sums(labels), labels,
                post.differ_sum, assignments.shape[0])
            done = True
            return _first_maximum(cuts, scores), post
        if dist is None:        # labels beyond uint16: the host scores
            dist = post.dist()
        sim = 1 - dist
        scores = np.array([calc_MPEAR(sim, np.ascontiguousarray(cuts[:, col]))
            for col in range(candidates.size)])
        done = True
        return _first_maximum(cuts, scores), post
    finally:
        if post is not None and not done:
            post.close()


def _first_maximum(cuts, scores):
    """The cut the reference's loop keeps (utils.py:119-128: `if score >
    best: ...` from -inf): the FIRST of the largest scores; a NaN score never
    passes `>`, so it is skipped, and if nothing passes the result is None."""
    scores = np.asarray(scores, dtype=np.float64)
    usable = ~np.isnan(scores) & (scores > -np.inf)
    if not usable.any():
        return None
    best = int(np.argmax(np.where(usable, scores, -np.inf)))
    return np.ascontiguousarray(cuts[:, best])


def mean_hierarchy_assignment(assignments, params_full, dist=None):
    """utils.py:148-192: the MPEAR clustering and, per cluster, the mean of
    the sampled parameter vectors of the posterior samples in which the
    cluster's cells sit together (and alone, if such samples exist).
    Product path (dist is None): the Posterior of the MPEAR scoring, its
    samples still on the device, runs the genotype pass too
    (bnpc_post_genotypes, bit-identical to host_genotypes); with a given
    `dist`, or cluster labels past uint16, the host loop."""
    assign, params = _mean_hierarchy(assignments, params_full, dist)
    return assign, params[assign].T


def _mean_hierarchy(assignments, params_full, dist=None, while_open=None,
        with_genotypes=None):
    """(MPEAR clustering, per-cluster mean parameters (clusters, muts));
    while_open(post, assign) is called before the genotype pass and
    with_genotypes(post, assign, params) after it, both before the Posterior
    is closed."""
    assign, post = _mpear(assignments, dist)
    # the device pass runs on the samples the Posterior holds on the device;
    # a clustering handle without it (a host stand-in for the pair counts)
    # leaves the averaging to the host loop
    device = getattr(post, 'genotypes', None)
    try:
        if while_open is not None:
            while_open(post, assign)
        if device is not None and assign is not None \
                and int(np.max(assign)) < 65534:
            params = device(assign, params_full)
        else:
            params = host_genotypes(assignments, assign, params_full)
        if with_genotypes is not None:
            with_genotypes(post, assign, params)
    finally:
        if post is not None:
            post.close()
    return assign, params


def host_genotypes(assignments, assign, params_full):
    """The per-cluster mean parameters of utils.py:148-192 on the host:
    (clusters, muts) float64, row i for the i-th smallest label of assign."""
    steps = assignments.shape[0]
    clusters = np.unique(assign)
    params = np.zeros((clusters.size, params_full.shape[2]))
    for row, cluster in enumerate(clusters):
        member = assign == cluster
        cells = np.flatnonzero(member)
        sub = assignments[:, cells]
        others = assignments[:, np.flatnonzero(~member)]
        together = (sub == sub[:, :1]).all(axis=1)
        major = np.array([np.argmax(np.bincount(r)) for r in sub])
        alone = ~(others == major[:, None]).any(axis=1)
        if together.any():
            pick = together & alone
            if not pick.any():
                pick = together
            chosen = np.flatnonzero(pick)
            for s in chosen:
                present = np.append(np.unique(others[s]), major[s])
                rank = np.argwhere(np.sort(present) == major[s])[0][0]
                params[row] += params_full[s][rank]
            params[row] /= chosen.size
        else:
            for s, sample in enumerate(assignments):
                all_ids = np.unique(sample)
                ids, cnt = np.unique(sample[cells], return_counts=True)
                rows = np.flatnonzero(np.isin(all_ids, ids))
                params[row] += np.dot(cnt, params_full[s][rows])
            params[row] /= steps * cells.size
    return params


def concat_chain_results(results):
    """Pool the post-burn-in samples of all chains (utils.py:206-223)."""
    pooled = {k: np.concatenate([r[k][r['burn_in']:] for r in results])
        for k in ('assignments', 'DP_alpha', 'ML', 'MAP', 'FN', 'FP')}
    width = max(r['params'].shape[1] for r in results)
    pooled['params'] = np.concatenate([np.pad(r['params'],
        [(0, 0), (0, width - r['params'].shape[1]), (0, 0)])
        for r in results])
    pooled['burn_in'] = 0
    return pooled


def posterior_estimate(results, data, support=False, cells=False, fit=False,
        mutations=False, doublets=False, chains=False, ordering=False):
    """`-e posterior` (the default estimator), chains pooled
    (utils.py:195-244).  support=True: the key 'support' holds the tables of
    cluster_support for the MPEAR clustering, made from the pair counts of
    the MPEAR scoring while they are still on the device.  cells=True: the
    key 'cell_genotypes' holds the tables of cell_genotypes, made from the
    samples the same handle keeps on the device.  fit=True: the key 'fit'
    holds the tables of cell_fit, from the same samples, the data and the
    samples' error rates.  mutations=True: the key 'mutation_fit' holds the
    tables of mutation_fit, from the same inputs, the cells sorted by the
    MPEAR clustering.  doublets: a rate in (0, 1), the prior share of
    doublets among the cells, adds the key 'doublets' with the tables of
    doublets(), made from the data, the MPEAR clustering, its genotypes and
    the posterior means of the error rates on the same handle.  chains=True:
    the key 'chains' holds the tables of chain_agreement, every chain's
    samples against the other chains', with the bounds of results_bounds, on
    the same handle.  ordering: a cluster size of 1 or more (min_cells) adds
    the key 'mutation_order' with the tables of mutation_order, from the
    samples and their parameter trace on the same handle."""
    res = concat_chain_results(results)
    tables = {}
    if doublets:
        def with_genotypes(post, assign, params):
            tables['doublets'] = _doublet_tables(post, data, assign,
                params, np.mean(res['FN']), np.mean(res['FP']), doublets)
    else:
        with_genotypes = None
    if support or cells or fit or mutations or chains or ordering:
        def while_open(post, assign):
            if support:
                tables['support'] = posterior_support(post, assign)
            if chains:
                tables['chains'] = chain_agreement(post, res['assignments'],
                    results_bounds(results), assign)
            if cells:
                tables['cell_genotypes'] = cell_genotypes(post,
                    res['assignments'], res['params'])
            if fit:
                tables['fit'] = cell_fit(post, data, res['assignments'],
                    res['params'], res['FN'], res['FP'])
            if mutations:
                tables['mutation_fit'] = mutation_fit(post, data,
                    res['assignments'], res['params'], res['FN'], res['FP'],
                    order=assign)
            if ordering:
                tables['mutation_order'] = mutation_order(post,
                    res['assignments'], res['params'], int(ordering))
    else:
        while_open = None
    assign, params = _mean_hierarchy(res['assignments'], res['params'],
        while_open=while_open, with_genotypes=with_genotypes)
    geno = params[assign].T
    called = geno.T.round()
    FN_geno = (((called == 1) & (data == 0)).sum() + EPSILON) \
        / (called.sum() + EPSILON)
    FP_geno = (((called == 0) & (data == 1)).sum() + EPSILON) \
        / ((1 - called).sum() + EPSILON)
    return {'a': (np.mean(res['DP_alpha']), np.std(res['DP_alpha'])),
        'assignment': assign.tolist(), 'genotypes': geno.T,
        'cluster_genotypes': params, 'cluster_of': assign,
        'FN': (np.mean(res['FN']), np.std(res['FN'])),
        'FP': (np.mean(res['FP']), np.std(res['FP'])),
        'FN_geno': FN_geno, 'FP_geno': FP_geno, **tables}


# ---------------------------------------------------------------------------
# per-cell cluster support and cluster similarity (-ps): the reference's
# N x N posterior similarity heat map (dpmmIO.py:245-274, drawn below 300
# cells only), summed per cluster
# ---------------------------------------------------------------------------
def host_support(differ, labels):
    """differ_to[i][k] = sum over cells j != i with labels[j] == k of
    differ_ij, int64 (N, K), from the condensed pair counts: row by row, no
    N x N matrix.  (The per-row sums go through np.bincount's float64
    weights: integers below (N - 1) * S < 2**53, so they are exact.)"""
    labels = np.asarray(labels, dtype=np.int64)
    differ = np.asarray(differ)
    N = labels.size
    K = int(labels.max()) + 1
    out = np.zeros((N, K), dtype=np.int64)
    at = 0
    for i in range(N - 1):
        row = differ[at:at + N - 1 - i].astype(np.int64)    # pairs (i, j > i)
        at += N - 1 - i
        out[i] += np.bincount(labels[i + 1:], weights=row, minlength=K) \
            .astype(np.int64)
        out[i + 1:, labels[i]] += row
    return out


def posterior_support(post, labels):
    """cluster_support of a clustering from an open clustering handle: the
    device pass (Posterior.support) where the handle has one and the labels
    fit it, else the host loop on the fetched pair counts."""
    labels = np.asarray(labels)
    device = getattr(post, 'support', None)
    if device is not None and int(labels.max()) + 1 < 65534:
        differ_to = device(labels)
    else:
        differ_to = host_support(post.differ(), labels)
    return cluster_support(differ_to, labels, post.S)


def cluster_support(differ_to, labels, S):
    """The -ps tables of a clustering (labels compact in [0, K)) from
    differ_to (host_support / Posterior.support) and the number of samples S.
    With n_k the size of cluster k and m_ik = n_k - [labels[i] == k]:
      support[i][k]    = 1 - differ_to[i][k] / (S m_ik): the mean posterior
                         probability that cell i shares a label with a member
                         of cluster k (1.0 for a singleton's own cluster)
      own              support of every cell's own cluster
      next_cluster,    the best other cluster (ties: the smallest index) and
      next_support     its support; -1 and 0 if there is one cluster only
      similarity[k][l] = 1 - block[k][l] / (S p_kl), block[k][l] the sum of
                         differ_to[i][l] over the cells of k, p_kl = n_k n_l,
                         p_kk = n_k (n_k - 1) (1.0 for a singleton's own)."""
    differ_to = np.asarray(differ_to, dtype=np.int64)
    labels = np.asarray(labels, dtype=np.int64)
    N, K = differ_to.shape
    cells = np.arange(N)
    n_k = np.bincount(labels, minlength=K).astype(np.int64)
    m = np.tile(n_k, (N, 1))
    m[cells, labels] -= 1
    support = np.ones((N, K))
    np.divide(differ_to, S * m, out=support, where=m > 0)
    np.subtract(1.0, support, out=support, where=m > 0)
    own = support[cells, labels]
    if K > 1:
        others = support.copy()
        others[cells, labels] = -np.inf
        next_cluster = np.argmax(others, axis=1).astype(np.int64)
        next_support = others[cells, next_cluster]
    else:
        next_cluster = np.full(N, -1, dtype=np.int64)
        next_support = np.zeros(N)
    block = np.zeros((K, K), dtype=np.int64)
    np.add.at(block, labels, differ_to)
    pairs = np.outer(n_k, n_k) - np.diag(n_k)
    similarity = np.ones((K, K))
    np.divide(block, S * pairs, out=similarity, where=pairs > 0)
    np.subtract(1.0, similarity, out=similarity, where=pairs > 0)
    return {'support': support, 'own': own, 'next_cluster': next_cluster,
        'next_support': next_support, 'similarity': similarity}


# ---------------------------------------------------------------------------
# per-cell posterior genotypes (-pg): what the model says about one cell and
# one mutation, averaged over the posterior samples - independent of the
# MPEAR cut; not a reference output, so the summation order below is the
# specification
# ---------------------------------------------------------------------------
def host_cell_genotypes(assignments, params_full):
    """(sum1, sum2, ones), each (cells, muts): with v the float32 parameter
    params_full[s][r][m] of the row r of cell i's cluster in sample s (r: the
    distinct labels of the sample below the cell's - any integer labels), as
    float64, the sums of v and of v * v over the samples, one sample at a
    time in increasing s from 0.0, and the uint32 count of the samples with
    v > 0.5 (np.round(v) == 1: half-to-even sends 0.5 to 0).  The plain loop
    bnpc_post_cell_genotypes is pinned to."""
    assignments = np.asarray(assignments)
    S, N = assignments.shape
    M = params_full.shape[2]
    sum1 = np.zeros((N, M))
    sum2 = np.zeros((N, M))
    ones = np.zeros((N, M), dtype=np.uint32)
    for s in range(S):
        rank = np.unique(assignments[s], return_inverse=True)[1].ravel()
        v = np.asarray(params_full[s], dtype=np.float32)[rank] \
            .astype(np.float64)
        sum1 += v
        sum2 += v * v
        ones += v > 0.5
    return sum1, sum2, ones


def cell_genotypes(post, assignments, params_full):
    """The -pg tables, each (cells, muts) float64: 'mean' and 'sd' of the
    parameter of the cell's cluster over the posterior samples, 'prob' the
    share of the samples in which it rounds to 1.  From an open clustering
    handle: the device pass (Posterior.cell_genotypes) where the handle has
    one, else the host loop; the same arithmetic on the sums either way."""
    device = getattr(post, 'cell_genotypes', None)
    if device is not None:
        sum1, sum2, ones = device(params_full)
    else:
        sum1, sum2, ones = host_cell_genotypes(assignments, params_full)
    S = np.asarray(assignments).shape[0]
    mean = sum1 / S
    sd = np.sqrt(np.maximum(sum2 / S - mean * mean, 0))
    return {'mean': mean, 'sd': sd, 'prob': ones / S}


# ---------------------------------------------------------------------------
# posterior ordering of every pair of mutations (-po): which mutation came
# first, which share a branch, which sit on separate lineages - the relation
# of the two under the three-gamete rule in every posterior sample, counted;
# not a reference output, so the definition below is the specification
# ---------------------------------------------------------------------------
def host_mutation_order(assignments, params_full, min_cells=2):
    """(anc, same, excl, conf), each (M, M) uint32: the samples in which the
    pair of mutations (a, b) stands in each relation.  In sample s the
    distinct labels in increasing order are the rows r < D_s of
    params_full[s] (rows >= D_s are padding, never read); row r is live iff
    its label has at least min_cells cells; A_m is the set of live rows with
    the float32 params_full[s][r][m] > 0.5 (0.5 itself and NaN are not
    carried).  With x11 = A_a and A_b meet, x10 = A_a minus A_b is not empty,
    x01 = A_b minus A_a is not empty: same is x11 alone, anc[a][b] (a strictly
    ancestral to b) x11 and x10, anc[b][a] x11 and x01, excl x10 and x01,
    conf all three; any other case (a or b carried by no live row) counts
    nowhere.  The plain loop bnpc_post_mutation_order is pinned to."""
    assignments = np.asarray(assignments)
    min_cells = int(min_cells)
    if min_cells < 1:
        raise ValueError('min_cells must be 1 or more')
    S = assignments.shape[0]
    M = params_full.shape[2]
    tables = [np.zeros((M, M), dtype=np.uint32) for _ in range(4)]
    anc, same, excl, conf = tables
    for s in range(S):
        sizes = np.unique(assignments[s], return_counts=True)[1]
        rows = np.asarray(params_full[s][:sizes.size], dtype=np.float32)
        with np.errstate(invalid='ignore'):
            g = (rows > np.float32(0.5))[sizes >= min_cells]
        # (counts of rows, below 2 ** 24: exact in float32)
        g = g.astype(np.float32)
        n11 = g.T @ g
        n10 = g.T @ (1 - g)
        x11, x10, x01 = n11 > 0, n10 > 0, n10.T > 0
        same += x11 & ~x10 & ~x01
        anc += x11 & x10 & ~x01
        excl += ~x11 & x10 & x01
        conf += x11 & x10 & x01
    return anc, same, excl, conf


def mutation_order(post, assignments, params_full, min_cells=2):
    """The -po tables.  'anc', 'same', 'excl', 'conf': the (M, M) uint32
    counts of host_mutation_order - from the device pass
    (Posterior.mutation_order) where the open clustering handle has one, else
    from the host loop.  From them, with S the samples and p = count / S, per
    mutation m (arrays of M):
      carried            same[m][m] / S: the share of the samples that carry m
      depth              |Anc(m)|, Anc(m) = {b != m: anc[b][m] > S / 2}
      n_descendants      |{b: anc[m][b] > S / 2}|
      parent, p_parent   the b of Anc(m) with depth(b) < depth(m) that has the
                         largest depth (ties: the larger anc[b][m], then the
                         smaller index) and anc[b][m] / S; -1 and 0 for a
                         root.  The strict depth makes the parents a forest
                         even where the majorities are not transitive
      skipped_ancestors  the members of Anc(m) that condition excludes
      same_as            the smallest b < m with same[b][m] > S / 2, else -1
      n_same,            the b != m whose same / excl exceeds S / 2
      n_exclusive
      conflict           the mean over b != m of conf[m][b] / S (0 for M = 1)
      worst_conflict,    the b with the largest conf[m][b] (ties: the smaller
      p_worst_conflict   index) and conf[m][b] / S; -1 and 0 if all are 0
    and 'total': samples, mutations, pairs, min_cells; the shares of the
    M (M - 1) / 2 pairs whose relation has p > 0.5 - ancestral (either way),
    same, exclusive, conflict, absent - and undecided, the rest;
    mean_conflict, roots, max_depth, skipped_ancestors (summed) and
    most_conflicting, the ten mutations with the largest conflict (ties: the
    smaller index)."""
    assignments = np.asarray(assignments)
    S = int(assignments.shape[0])
    min_cells = int(min_cells)
    device = getattr(post, 'mutation_order', None)
    if device is not None:
        anc, same, excl, conf = device(params_full, min_cells)
    else:
        anc, same, excl, conf = host_mutation_order(assignments, params_full,
            min_cells)
    M = anc.shape[0]
    idx = np.arange(M)
    off = ~np.eye(M, dtype=bool)
    # count > S / 2 in integers
    major = lambda t: (2 * t.astype(np.int64) > S) & off
    anc_of = major(anc).T                   # anc_of[m][b]: b in Anc(m)
    depth = anc_of.sum(axis=1)
    parent = np.full(M, -1, dtype=np.int64)
    p_parent = np.zeros(M)
    skipped = np.zeros(M, dtype=np.int64)
    for m in range(M):
        cand = np.flatnonzero(anc_of[m])
        ok = cand[depth[cand] < depth[m]]
        skipped[m] = cand.size - ok.size
        if ok.size:
            best = min(ok.tolist(),
                key=lambda b: (-depth[b], -int(anc[b, m]), b))
            parent[m] = best
            p_parent[m] = anc[best, m] / S
    same_major = major(same)
    same_as = np.full(M, -1, dtype=np.int64)
    for m in range(M):
        below = np.flatnonzero(same_major[m, :m])
        if below.size:
            same_as[m] = below[0]
    conf_off = np.where(off, conf, 0).astype(np.int64)
    conflict = conf_off.sum(axis=1) / S / (M - 1) if M > 1 else np.zeros(M)
    worst = np.argmax(conf_off, axis=1).astype(np.int64)   # first maximum
    worst_n = conf_off[idx, worst]
    worst[worst_n == 0] = -1
    upper = np.triu(np.ones((M, M), dtype=bool), 1)
    pairs = M * (M - 1) // 2
    absent = S - (anc.astype(np.int64) + anc.T + same + excl + conf)

    def share(mask):
        return float((mask & upper).sum() / pairs) if pairs else 0.0
    shares = {'ancestral': share(major(anc) | major(anc).T),
        'same': share(same_major), 'exclusive': share(major(excl)),
        'conflict': share(major(conf)), 'absent': share(major(absent))}
    top = sorted(range(M), key=lambda m: (-conflict[m], m))[:10]
    total = {'samples': S, 'mutations': M, 'pairs': pairs,
        'min_cells': min_cells, **shares,
        'undecided': (1.0 - sum(shares.values())) if pairs else 0.0,
        'mean_conflict': float(conflict.mean()),
        'roots': int((parent < 0).sum()), 'max_depth': int(depth.max()),
        'skipped_ancestors': int(skipped.sum()), 'most_conflicting': top}
    return {'anc': anc, 'same': same, 'excl': excl, 'conf': conf,
        'carried': same[idx, idx] / S, 'depth': depth.astype(np.int64),
        'n_descendants': major(anc).sum(axis=1).astype(np.int64),
        'parent': parent, 'p_parent': p_parent,
        'skipped_ancestors': skipped, 'same_as': same_as,
        'n_same': same_major.sum(axis=1).astype(np.int64),
        'n_exclusive': major(excl).sum(axis=1).astype(np.int64),
        'conflict': conflict, 'worst_conflict': worst,
        'p_worst_conflict': worst_n / S, 'total': total}


# ---------------------------------------------------------------------------
# per-cell posterior fit and WAIC (-pf): how well the model explains every
# cell, from the pointwise log-likelihood of every cell in every sample; not
# a reference output, so the arithmetic and the summation order below are the
# specification
# ---------------------------------------------------------------------------
def data_codes(data):
    """cells x mutations uint8: 1, 0, and 3 for a missing entry (NaN or 3 in
    `data`); any other value raises ValueError."""
    from bnpc_amd import _lib
    codes = _lib.data_codes(data)
    if not np.isin(codes, (0, 1, 3)).all():
        raise ValueError('the data must be 0, 1 or missing (NaN or 3)')
    return codes


def host_cell_fit(data, assignments, params_full, FN, FP):
    """The pointwise log-likelihood of every cell in every posterior sample
    and its per-cell reductions; the plain loop bnpc_post_cell_fit is pinned
    to.  data: cells x mutations, 0 / 1 / missing (NaN or 3); assignments:
    S x N, any integer labels; params_full: S x W x M, the row of a cell in
    sample s the rank of its label among the sample's distinct labels (as in
    host_cell_genotypes); FN, FP: the S error rates of the samples.  With
    th = float32 params_full[s][r][m], t = float64(th) and
    o = float64(float32(1) - th),
      L1 = log(t * (1 - FN[s]) + o * FP[s])     an observed 1
      L0 = log(t * FN[s] + o * (1 - FP[s]))     an observed 0
    (the expressions of k_tables_theta, each operation rounded on its own),
    ll[s][i] is the sum over the mutations of L1 where the cell shows a 1 and
    L0 where it shows a 0.  Per cell, over the column ll[:, i] one sample at
    a time in increasing s: mean (the sum from 0.0, divided by S), m2 (the
    sum of (ll - mean)**2), lme = mx + log(sum of exp(ll - mx)) - log(S) with
    mx the column's maximum - the log of the mean likelihood; n_obs counts
    the cell's observed entries.
    -> {'ll': (S, N), 'mean', 'm2', 'lme': (N,) float64, 'n_obs': (N,) int64}
    """
    codes = data_codes(data)
    assignments = np.asarray(assignments)
    S, N = assignments.shape
    FN = np.asarray(FN, dtype=np.float64)
    FP = np.asarray(FP, dtype=np.float64)
    ll = np.empty((S, N))
    for s in range(S):
        rank = np.unique(assignments[s], return_inverse=True)[1].ravel()
        th = np.asarray(params_full[s], dtype=np.float32)[:rank.max() + 1]
        t = th.astype(np.float64)
        o = (np.float32(1) - th).astype(np.float64)
        L1 = np.log(t * (1 - FN[s]) + o * FP[s])
        L0 = np.log(t * FN[s] + o * (1 - FP[s]))
        # (where: an entry that is not there adds nothing, whatever its log)
        el = np.where(codes == 1, L1[rank], np.where(codes == 0, L0[rank], 0))
        ll[s] = el.sum(axis=1)
    acc = np.zeros(N)
    for s in range(S):
        acc += ll[s]
    mean = acc / S
    m2 = np.zeros(N)
    for s in range(S):
        m2 += (ll[s] - mean) ** 2
    mx = ll.max(axis=0)
    esum = np.zeros(N)
    for s in range(S):
        esum += np.exp(ll[s] - mx)
    lme = mx + np.log(esum) - np.log(S)
    return {'ll': ll, 'mean': mean, 'm2': m2, 'lme': lme,
        'n_obs': (codes != 3).sum(axis=1).astype(np.int64)}


def cell_fit(post, data, assignments, params_full, FN, FP):
    """The -pf tables: how well the model explains every cell, and WAIC
    (Watanabe 2010; Gelman, Hwang & Vehtari 2014) of the run.  The unit of
    WAIC here is the cell - its whole row of the matrix is one observation,
    ll[s][i] its pointwise log-likelihood - not the single entry.  Per cell,
    (N,) arrays: 'mean_ll' and 'sd_ll' (sqrt(m2 / (S - 1)); 0 for S = 1) of
    ll over the samples, 'lppd' (the log of the mean likelihood), 'p_waic'
    (the sample variance m2 / (S - 1); 0 for S = 1), 'n_obs',
    'mean_ll_per_obs' (mean_ll / n_obs; 0 for a cell without observations).
    'total': {'samples', 'cells', 'observations', 'lppd', 'p_waic', 'waic'}
    with waic = -2 (lppd - p_waic), the sums over the cells.  From an open
    clustering handle: the device pass (Posterior.cell_fit) where the handle
    has one, else the host loop (host_cell_fit); the same arithmetic on
    (mean, m2, lme) either way."""
    device = getattr(post, 'cell_fit', None)
    if device is not None:
        mean, m2, lme, _ = device(data, params_full, FN, FP)
        n_obs = (data_codes(data) != 3).sum(axis=1).astype(np.int64)
    else:
        fit = host_cell_fit(data, assignments, params_full, FN, FP)
        mean, m2, lme, n_obs = (fit[k] for k in ('mean', 'm2', 'lme', 'n_obs'))
    S, N = np.asarray(assignments).shape
    var = m2 / (S - 1) if S > 1 else np.zeros(N)
    per_obs = np.zeros(N)
    np.divide(mean, n_obs, out=per_obs, where=n_obs > 0)
    lppd, p_waic = float(lme.sum()), float(var.sum())
    return {'mean_ll': mean, 'sd_ll': np.sqrt(var), 'lppd': lme,
        'p_waic': var, 'n_obs': n_obs, 'mean_ll_per_obs': per_obs,
        'total': {'samples': int(S), 'cells': int(N),
            'observations': int(n_obs.sum()), 'lppd': lppd, 'p_waic': p_waic,
            'waic': -2 * (lppd - p_waic)}}


# ---------------------------------------------------------------------------
# per-mutation posterior fit and error rates (-pm): how well the model
# explains every column, and the error rates the column implies; not a
# reference output, so the arithmetic and the summation order below are the
# specification
# ---------------------------------------------------------------------------
def host_mutation_fit(data, assignments, params_full, FN, FP):
    """The log-likelihood of every mutation's column in every posterior
    sample, the error rates the fitted model implies for it, and their
    reductions over the samples; the plain loop bnpc_post_mutation_fit is
    pinned to.  Inputs as host_cell_fit.  All cells of a cluster share their
    parameter row, so per sample s, row r and mutation m everything follows
    from c1, c0 - the row's cells that show a 1 / a 0 at m - and, with
    th = float32 params_full[s][r][m], t = float64(th) and
    o = float64(float32(1) - th),
      a1 = t * (1 - FN[s])  b1 = o * FP[s]        d1 = a1 + b1  L1 = log(d1)
      a0 = t * FN[s]        b0 = o * (1 - FP[s])  d0 = a0 + b0  L0 = log(d0)
      qfp = b1 / d1     an observed 1 is a false positive
      qfn = a0 / d0     an observed 0 is a false negative
    (host_cell_fit's expressions, each operation rounded on its own).  Per
    (s, m), over the rows in increasing r from 0.0:
      ll[s][m] = sum of c1 * L1 + c0 * L0      efn_s = sum of c0 * qfn
      efp_s = sum of c1 * qfp      eg1_s = sum of c1 * (a1 / d1) + c0 * qfn
    (eg1: the expected number of observed cells that carry the mutation), and
    per mutation over the samples in increasing s from 0.0: sum_ll, sum_ll2
    (of ll * ll), efn, efp, eg1; call1_obs1, call1_obs0 add c1 and c0 of the
    rows with th > 0.5 (the rounding of host_cell_genotypes); n1, n0 count
    the column's ones and zeros.
    -> {'ll': (S, M) float64, 'sum_ll', 'sum_ll2', 'efn', 'efp', 'eg1': (M,)
    float64, 'call1_obs1', 'call1_obs0', 'n1', 'n0': (M,) int64}"""
    codes = data_codes(data)
    assignments = np.asarray(assignments)
    S = assignments.shape[0]
    M = codes.shape[1]
    FN = np.asarray(FN, dtype=np.float64)
    FP = np.asarray(FP, dtype=np.float64)
    is1, is0 = codes == 1, codes == 0
    ll = np.empty((S, M))
    sub = np.empty((3, S, M))
    call = np.zeros((2, M), dtype=np.int64)
    for s in range(S):
        rank = np.unique(assignments[s], return_inverse=True)[1].ravel()
        acc = np.zeros((4, M))
        for r in range(rank.max() + 1):
            member = rank == r
            k1 = is1[member].sum(axis=0, dtype=np.int64)
            k0 = is0[member].sum(axis=0, dtype=np.int64)
            c1, c0 = k1.astype(np.float64), k0.astype(np.float64)
            th = np.asarray(params_full[s][r], dtype=np.float32)
            t = th.astype(np.float64)
            o = (np.float32(1) - th).astype(np.float64)
            a1, b1 = t * (1 - FN[s]), o * FP[s]
            a0, b0 = t * FN[s], o * (1 - FP[s])
            d1, d0 = a1 + b1, a0 + b0
            qfp, qfn = b1 / d1, a0 / d0
            acc[0] += c1 * np.log(d1) + c0 * np.log(d0)
            acc[1] += c0 * qfn
            acc[2] += c1 * qfp
            acc[3] += c1 * (a1 / d1) + c0 * qfn
            called = th > 0.5
            call[0] += np.where(called, k1, 0)
            call[1] += np.where(called, k0, 0)
        ll[s] = acc[0]
        sub[:, s] = acc[1:]
    out = {'ll': ll, **mutation_fit_sums(ll)}
    for k, key in enumerate(('efn', 'efp', 'eg1')):
        out[key] = np.zeros(M)
        for s in range(S):
            out[key] += sub[k, s]
    out.update(call1_obs1=call[0], call1_obs0=call[1],
        n1=is1.sum(axis=0, dtype=np.int64), n0=is0.sum(axis=0, dtype=np.int64))
    return out


def mutation_fit_sums(ll):
    """host_mutation_fit's reductions of an (S, M) matrix ll over the samples,
    one sample at a time in increasing s from 0.0: {'sum_ll', 'sum_ll2'}."""
    sum_ll, sum_ll2 = np.zeros(ll.shape[1]), np.zeros(ll.shape[1])
    for row in ll:
        sum_ll += row
        sum_ll2 += row * row
    return {'sum_ll': sum_ll, 'sum_ll2': sum_ll2}


def _rate(num, den):
    """num / den as float64, nan where den is 0 (arrays or scalars)."""
    num = np.asarray(num, dtype=np.float64)
    den = np.asarray(den, dtype=np.float64)
    out = np.full(np.broadcast(num, den).shape, np.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out if out.ndim else float(out)


MUTATION_FIT_COLUMNS = ('n_obs', 'n_ones', 'n_zeros', 'mean_ll', 'sd_ll',
    'mean_ll_per_obs', 'prevalence', 'FN_model', 'FP_model', 'FN_call',
    'FP_call')


def mutation_fit(post, data, assignments, params_full, FN, FP, order=None):
    """The -pm tables: how well the model explains every mutation, and the
    error rates its column implies, where the model has one global pair.  Per
    mutation, (M,) arrays (MUTATION_FIT_COLUMNS): 'n_obs', 'n_ones',
    'n_zeros' of the column; 'mean_ll' and 'sd_ll' (the sample standard
    deviation; 0 for S = 1) of the column's log-likelihood over the samples,
    'mean_ll_per_obs' (0 without observations); 'prevalence', the expected
    share of the observed cells that carry the mutation (eg1 / (S n_obs));
    'FN_model' = efn / eg1 and 'FP_model' = efp / (S n_obs - eg1), the rates
    the fitted model implies - expected false negatives per expected carrier,
    expected false positives per expected non-carrier; 'FN_call' =
    call1_obs0 / (call1_obs1 + call1_obs0) and 'FP_call' = (S n1 -
    call1_obs1) / (S n_obs - call1_obs1 - call1_obs0), the per-column,
    posterior-averaged form of FN_data / FP_data of errors.txt, from the
    genotypes called at th > 0.5.  A rate is nan where its denominator is 0.
    'eg1' is the sum itself.  'total': {'samples', 'mutations',
    'observations', the four rates pooled from the column sums, 'FN', 'FP':
    the posterior means of the run's own rates}.  From an open clustering
    handle: the device pass (Posterior.mutation_fit, the cells sorted by
    `order`, any clustering's labels) where the handle has one, else the host
    loop (host_mutation_fit); the same arithmetic on the sums either way."""
    codes = data_codes(data)
    n1 = (codes == 1).sum(axis=0, dtype=np.int64)
    n0 = (codes == 0).sum(axis=0, dtype=np.int64)
    device = getattr(post, 'mutation_fit', None)
    if device is not None:
        sum_ll, sum_ll2, efn, efp, eg1, c11, c10, _ = device(codes,
            params_full, FN, FP, order=order)
    else:
        fit = host_mutation_fit(codes, assignments, params_full, FN, FP)
        sum_ll, sum_ll2, efn, efp, eg1, c11, c10 = (fit[k] for k in (
            'sum_ll', 'sum_ll2', 'efn', 'efp', 'eg1', 'call1_obs1',
            'call1_obs0'))
    S = int(np.asarray(assignments).shape[0])
    M = n1.size
    n_obs = n1 + n0
    mean = sum_ll / S
    sd = np.zeros(M)
    if S > 1:
        sd = np.sqrt(np.maximum(sum_ll2 / S - mean ** 2, 0) * S / (S - 1))
    per_obs = np.zeros(M)
    np.divide(mean, n_obs, out=per_obs, where=n_obs > 0)

    def rates(n_obs, n1, efn, efp, eg1, c11, c10):
        return {'FN_model': _rate(efn, eg1),
            'FP_model': _rate(efp, S * n_obs - eg1),
            'FN_call': _rate(c10, c11 + c10),
            'FP_call': _rate(S * n1 - c11, S * n_obs - c11 - c10)}
    total = {'samples': S, 'mutations': int(M),
        'observations': int(n_obs.sum()),
        **rates(int(n_obs.sum()), int(n1.sum()), efn.sum(), efp.sum(),
            eg1.sum(), int(c11.sum()), int(c10.sum())),
        'FN': float(np.mean(FN)), 'FP': float(np.mean(FP))}
    return {'n_obs': n_obs, 'n_ones': n1, 'n_zeros': n0, 'mean_ll': mean,
        'sd_ll': sd, 'mean_ll_per_obs': per_obs,
        'prevalence': _rate(eg1, S * n_obs),
        **rates(n_obs, n1, efn, efp, eg1, c11, c10), 'eg1': eg1,
        'total': total}


# ---------------------------------------------------------------------------
# doublet scores (-pd): is a cell explained by two clusters at once?  Every
# cell against every cluster of a clustering and every unordered pair of them;
# not a reference output, so the arithmetic and the summation order below are
# the specification
# ---------------------------------------------------------------------------
def doublet_pairs(K):
    """The pairs (a, b), a < b, of K clusters in lexicographic order: (a, b)
    int64 arrays of K (K - 1) / 2.  Pair (a, b) is candidate
    K + a (2K - a - 1) / 2 + (b - a - 1); the K singles come first."""
    a, b = np.triu_indices(K, 1)
    return a.astype(np.int64), b.astype(np.int64)


def doublet_tables(theta, FN, FP):
    """The (P, M) float64 tables L1, L0 of host_doublets: the K singles, then
    the pairs."""
    theta = np.asarray(theta, dtype=np.float64)
    a, b = doublet_pairs(theta.shape[0])
    o = np.concatenate([1.0 - theta, (1.0 - theta[a]) * (1.0 - theta[b])])
    t = np.concatenate([theta, 1.0 - o[theta.shape[0]:]])
    return np.log(t * (1 - FN) + o * FP), np.log(t * FN + o * (1 - FP))


def doublet_reduce(scores, labels, K, logw, lN, lT):
    """host_doublets' per-cell reductions of an (N, P) matrix of scores, each
    a walk over the cell's candidates in index order."""
    scores = np.asarray(scores, dtype=np.float64)
    N, P = scores.shape
    a, b = doublet_pairs(K)

    def group(sc, prior):
        best = np.argmax(sc, axis=1)            # the first of the largest
        y = sc + prior
        mx = y.max(axis=1)
        es = np.zeros(N)
        for c in range(sc.shape[1]):
            es += np.exp(y[:, c] - mx)
        return best, sc[np.arange(N), best], mx + np.log(es)
    best, ll_single, lse_single = group(scores[:, :K], logw - lN)
    out = {'own': scores[np.arange(N), labels],
        'best_single': best.astype(np.int32), 'll_single': ll_single,
        'lse_single': lse_single}
    if K > 1:
        best, ll_pair, lse_pair = group(scores[:, K:], (logw[a] + logw[b]) - lT)
        best_pair = np.stack([a[best], b[best]], axis=1).astype(np.int32)
    else:
        best_pair = np.full((N, 2), -1, dtype=np.int32)
        ll_pair, lse_pair = np.full(N, -np.inf), np.full(N, -np.inf)
    out.update(best_pair=best_pair, ll_pair=ll_pair, lse_pair=lse_pair)
    return out


def _doublet_weights(labels, K, logw):
    """(labels, logw, lN, lT) of host_doublets: the default log-weights are
    the logs of the cluster sizes, lN = log N, lT = log of the sum of
    n_a n_b over a < b (-inf for K = 1)."""
    labels = np.asarray(labels)
    sizes = np.bincount(labels, minlength=K) if labels.size \
        and labels.min() >= 0 else np.zeros(K + 1, dtype=np.int64)
    if sizes.size != K or not sizes.all():
        raise ValueError(f'the labels must be compact in [0, {K}) with no '
            'empty cluster')
    logw = np.log(sizes.astype(np.float64)) if logw is None \
        else np.asarray(logw, dtype=np.float64)
    if logw.shape != (K,) or not np.isfinite(logw).all():
        raise ValueError(f'logw must hold {K} finite log-weights')
    n = int(labels.size)
    both = (n * n - int((sizes.astype(object) ** 2).sum())) // 2
    with np.errstate(divide='ignore'):
        return labels, logw, np.log(np.float64(n)), np.log(np.float64(both))


def host_doublets(data, labels, theta, FN, FP, logw=None):
    """The log-likelihood of every cell under every single cluster and under
    every unordered pair of clusters, and its per-cell reductions; the plain
    loop bnpc_post_doublets is pinned to.  data: cells x mutations, 0 / 1 /
    missing (NaN or 3); labels: N labels, compact in [0, K), no cluster
    empty; theta: K x M float64 in [0, 1]; FN, FP: two scalars strictly
    inside (0, 1).  Candidate c < K is the cluster c; then the pairs (a, b),
    a < b, in lexicographic order (doublet_pairs); P = K + K (K - 1) / 2.
      single  t = theta[k][m], o = 1.0 - t
      pair    o = (1.0 - theta[a][m]) * (1.0 - theta[b][m]), t = 1.0 - o
              (the union: the mutation is there if either cell carries it)
      L1 = log(t * (1 - FN) + o * FP)       an observed 1
      L0 = log(t * FN + o * (1 - FP))       an observed 0
    (float64, each operation rounded on its own).  scores[i][c] is the sum
    over the mutations, strictly in increasing m from 0.0, of L1[c][m] where
    the cell shows a 1 and L0[c][m] where it shows a 0.  With logw the K
    log-weights (None: log n_k, the cluster sizes), lN = log N and lT = log
    of the sum of n_a n_b over a < b - the priors of drawing one cell, or two
    cells of different clusters - a single weighs y = score + (logw[k] - lN)
    and a pair y = score + ((logw[a] + logw[b]) - lT).  Per cell, over its
    candidates in index order: 'own' (the score of its own cluster),
    'best_single' and 'll_single' (the largest single score and its cluster,
    the first on ties), 'best_pair' (a, b) and 'll_pair' (the same over the
    pairs), 'lse_single' and 'lse_pair' (mx + log(sum of exp(y - mx)), mx the
    group's largest y).  K = 1 has no pair: best_pair (-1, -1), ll_pair and
    lse_pair -inf.
    -> these and 'scores' (N, P), 'n_obs' (N,) int64"""
    codes = data_codes(data)
    theta = np.asarray(theta, dtype=np.float64)
    K = theta.shape[0]
    if theta.ndim != 2 or codes.shape[1] != theta.shape[1] \
            or not ((theta >= 0) & (theta <= 1)).all():
        raise ValueError('theta must be K x M values in [0, 1]')
    if not (0 < FN < 1 and 0 < FP < 1):
        raise ValueError('FN and FP must lie strictly inside (0, 1)')
    labels, logw, lN, lT = _doublet_weights(labels, K, logw)
    if labels.shape != (codes.shape[0],):
        raise ValueError('one label per cell')
    L1, L0 = doublet_tables(theta, FN, FP)
    is1, is0 = codes == 1, codes == 0
    scores = np.zeros((codes.shape[0], L1.shape[0]))
    for m in range(codes.shape[1]):
        # (adding 0.0 leaves every bit: no partial sum is -0.0)
        scores += np.where(is1[:, m, None], L1[:, m],
            np.where(is0[:, m, None], L0[:, m], 0.0))
    return {'scores': scores, 'n_obs': (codes != 3).sum(axis=1).astype(np.int64),
        **doublet_reduce(scores, labels, K, logw, lN, lT)}


def doublets(post, data, labels, theta, FN, FP, rate):
    """The -pd tables: is a cell explained by two clusters at once?  A
    doublet shows the union of two clones' mutations.  Per cell, (N,) arrays:
    'cluster' (its label), 'n_obs', 'll_cluster' (its score under its own
    cluster), 'best_cluster' and 'll_best' (the best single cluster),
    'pair_a', 'pair_b' and 'll_pair' (the best pair; -1, -1, -inf for one
    cluster), 'delta' = ll_pair - ll_best, and 'p_doublet' =
    1 / (1 + exp((log(1 - rate) + lse_single) - (log(rate) + lse_pair))), the
    posterior probability of a doublet under the prior share `rate` (0 where
    there is one cluster).  'total': {'cells', 'clusters', 'candidates',
    'rate', 'expected_doublets' (the sum of p_doublet), 'called' (cells with
    p_doublet > 0.5), 'pair_counts' ({(a, b): called cells whose best pair it
    is})}.  From an open clustering handle: the device pass
    (Posterior.doublets) where the handle has one, else the host loop
    (host_doublets); the same arithmetic on the reductions either way."""
    if not 0 < rate < 1:
        raise ValueError(f'the doublet rate {rate} is not inside (0, 1)')
    codes = data_codes(data)
    theta = np.asarray(theta, dtype=np.float64)
    K = int(theta.shape[0])
    labels = np.asarray(labels)
    FN, FP = float(FN), float(FP)
    device = getattr(post, 'doublets', None)
    if device is not None:
        own, ll_single, lse_single, ll_pair, lse_pair, best_single, \
            best_pair = device(codes, labels, theta, FN, FP)[:7]
    else:
        red = host_doublets(codes, labels, theta, FN, FP)
        own, ll_single, lse_single, ll_pair, lse_pair, best_single, \
            best_pair = (red[k] for k in ('own', 'll_single', 'lse_single',
                'll_pair', 'lse_pair', 'best_single', 'best_pair'))
    N = codes.shape[0]
    if K > 1:
        with np.errstate(over='ignore'):
            p = 1 / (1 + np.exp((np.log(1 - rate) + lse_single)
                - (np.log(rate) + lse_pair)))
        delta = ll_pair - ll_single
    else:
        p, delta = np.zeros(N), np.full(N, -np.inf)
    called = p > 0.5
    pair_counts = {}
    for a, b in best_pair[called].tolist():
        pair_counts[(a, b)] = pair_counts.get((a, b), 0) + 1
    return {'cluster': labels, 'n_obs': (codes != 3).sum(axis=1)
            .astype(np.int64), 'll_cluster': own,
        'best_cluster': np.asarray(best_single), 'll_best': ll_single,
        'pair_a': np.asarray(best_pair)[:, 0],
        'pair_b': np.asarray(best_pair)[:, 1], 'll_pair': ll_pair,
        'delta': delta, 'p_doublet': p,
        'total': {'cells': int(N), 'clusters': K,
            'candidates': K + K * (K - 1) // 2, 'rate': float(rate),
            'expected_doublets': float(p.sum()), 'called': int(called.sum()),
            'pair_counts': dict(sorted(pair_counts.items()))}}


_doublet_tables = doublets      # (posterior_estimate's keyword has the name)


# ---------------------------------------------------------------------------
# placement of held-out cells: the Gibbs conditional of one cell that was
# not part of the run (libs/CRP.py:223-234 with the weights of :84-85 and the
# mixing constants of :42-44), in every posterior sample, averaged; not a
# reference output, so the arithmetic and the summation order below are the
# specification
# ---------------------------------------------------------------------------
def place_scores(new_data, assignments, params_full, FN, FP, prior):
    """host_place's scores: (S, Q, W + 1) float64.  Per sample s, with K_s
    its distinct labels, slot r < K_s holds the score of the new cells under
    row r of the trace, slot W their score under a new cluster and every
    other slot NaN.  With th = float32 params_full[s][r][m], t = float64(th),
    o = float64(float32(1) - th) for a row and t = mix1 = p / (p + q),
    o = mix0 = q / (p + q) for the new cluster ((p, q) = prior),
      L1 = log(t * (1 - FN[s]) + o * FP[s])     an observed 1
      L0 = log(t * FN[s] + o * (1 - FP[s]))     an observed 0
    each operation rounded on its own, and a score is the sum over the
    mutations, strictly in increasing m from 0.0, of L1 where the cell shows
    a 1 and L0 where it shows a 0."""
    codes = data_codes(new_data)
    assignments = np.asarray(assignments)
    S = assignments.shape[0]
    Q, M = codes.shape
    W = params_full.shape[1]
    FN = np.asarray(FN, dtype=np.float64)
    FP = np.asarray(FP, dtype=np.float64)
    p, q = (float(x) for x in prior)
    mix1, mix0 = p / (p + q), q / (p + q)
    is1, is0 = codes == 1, codes == 0
    scores = np.full((S, Q, W + 1), np.nan)
    for s in range(S):
        Ks = np.unique(assignments[s]).size
        th = np.asarray(params_full[s], dtype=np.float32)[:Ks]
        t = np.append(th.astype(np.float64), np.full((1, M), mix1), axis=0)
        o = np.append((np.float32(1) - th).astype(np.float64),
            np.full((1, M), mix0), axis=0)
        L1 = np.log(t * (1 - FN[s]) + o * FP[s])
        L0 = np.log(t * FN[s] + o * (1 - FP[s]))
        sc = np.zeros((Q, Ks + 1))
        for m in range(M):
            # (adding 0.0 leaves every bit: no partial sum is -0.0)
            sc += np.where(is1[:, m, None], L1[:, m],
                np.where(is0[:, m, None], L0[:, m], 0.0))
        scores[s, :, :Ks] = sc[:, :Ks]
        scores[s, :, W] = sc[:, Ks]
    return scores


def place_reduce(scores, assignments, labels, K, alpha, keep=False):
    """host_place's reductions of an (S, Q, W + 1) array of scores (the
    layout of place_scores): per sample the candidates in order - the rows
    r < K_s, then the new cluster - and per cell one sample at a time in
    increasing s.  -> {'prob_sum' (Q, K), 'new_sum', 'ent_sum', 'lpd' (Q,),
    'lp' (S, Q)} and, with keep=True, 'y' (S, Q, W + 1): the candidates'
    y_c in the layout of the scores."""
    scores = np.asarray(scores, dtype=np.float64)
    assignments = np.asarray(assignments)
    labels = np.asarray(labels, dtype=np.int64)
    alpha = np.asarray(alpha, dtype=np.float64)
    S, N = assignments.shape
    Q, W = scores.shape[1], scores.shape[2] - 1
    prob_sum = np.zeros((Q, K))
    new_sum, ent_sum = np.zeros(Q), np.zeros(Q)
    lp = np.empty((S, Q))
    ys = np.full(scores.shape, np.nan) if keep else None
    for s in range(S):
        rank = np.unique(assignments[s], return_inverse=True)[1].ravel()
        Ks = int(rank.max()) + 1
        cnt = np.zeros((Ks, K), dtype=np.int64)
        np.add.at(cnt, (rank, labels), 1)
        n = cnt.sum(axis=1)
        share = cnt.astype(np.float64) / n.astype(np.float64)[:, None]
        y = np.empty((Q, Ks + 1))
        y[:, :Ks] = scores[s, :, :Ks] + np.log(n.astype(np.float64))
        y[:, Ks] = scores[s, :, W] + np.log(alpha[s])
        mx = y.max(axis=1)
        e = np.empty_like(y)
        es, h = np.zeros(Q), np.zeros(Q)
        for c in range(Ks + 1):
            d = y[:, c] - mx
            e[:, c] = np.exp(d)
            es += e[:, c]
            h += e[:, c] * d
        pr = e / es[:, None]
        t = np.zeros((Q, K))
        for r in range(Ks):
            t += pr[:, r, None] * share[r]
        prob_sum += t
        new_sum += pr[:, Ks]
        les = np.log(es)
        ent_sum += les - h / es
        lp[s] = (mx + les) - np.log(N + alpha[s])
        if keep:
            ys[s, :, :Ks] = y[:, :Ks]
            ys[s, :, W] = y[:, Ks]
    mxs = lp.max(axis=0)
    acc = np.zeros(Q)
    for s in range(S):
        acc += np.exp(lp[s] - mxs)
    out = {'prob_sum': prob_sum, 'new_sum': new_sum, 'ent_sum': ent_sum,
        'lpd': mxs + np.log(acc) - np.log(S), 'lp': lp}
    if keep:
        out['y'] = ys
    return out


def host_place(new_data, assignments, labels, params_full, FN, FP, alpha,
        prior, keep=True):
    """Where cells that were not part of the run belong: the Gibbs
    conditional of one cell in every posterior sample, averaged; the plain
    loop bnpc_post_place is pinned to.  new_data: Q x M, 0 / 1 / missing (NaN
    or 3); assignments: S x N, any integer labels; labels: the N labels of
    the MPEAR clustering, compact in [0, K); params_full: S x W x M float32;
    FN, FP, alpha: the S error rates and concentrations of the samples; prior:
    the Beta (p, q) of the parameters.  Per sample s, r(i) is the rank of
    training cell i's label among the sample's K_s distinct labels, n_r the
    cells of row r and cnt[r][k] those of them with MPEAR label k; the
    candidates c of a new cell are the rows r < K_s, then a new cluster, and
    their scores those of place_scores.  Then
      y_c = score_c + log(n_c), or score + log(alpha[s]) for the new cluster
      mx = max y_c, e_c = exp(y_c - mx), es = the sum of e_c in candidate
      order from 0.0, pr_c = e_c / es
    and per new cell j, one sample at a time in increasing s from 0.0,
      prob_sum[j][k] += the sum over r, in increasing r from 0.0, of
                        pr_r * (cnt[r][k] / n_r)
      new_sum[j]     += pr of the new cluster
      ent_sum[j]     += log(es) - (the sum of e_c * (y_c - mx)) / es
      lp[s][j]        = (mx + log(es)) - log(N + alpha[s])
      lpd[j]          = mxs + log(sum over s of exp(lp[s][j] - mxs)) - log(S)
    with mxs the column's maximum.  lp[s][j] is the log predictive density of
    the row in sample s; an all-missing row has score 0 everywhere, the CRP
    weights n_k / (N + alpha) as its probabilities and lp = 0.
    -> {'prob_sum', 'new_sum', 'ent_sum', 'lpd', 'lp', 'n_obs' (Q,) int64} and,
    with keep=True, 'scores' and 'y' (S, Q, W + 1)."""
    codes = data_codes(new_data)
    labels = np.asarray(labels, dtype=np.int64)
    assignments = np.asarray(assignments)
    if labels.shape != (assignments.shape[1],) or labels.min() < 0:
        raise ValueError('one label >= 0 per training cell')
    alpha = np.asarray(alpha, dtype=np.float64)
    if not (np.isfinite(alpha) & (alpha > 0)).all():
        raise ValueError('alpha must be finite and > 0')
    if codes.shape[1] != params_full.shape[2]:
        raise ValueError(f'the new cells must have the {params_full.shape[2]} '
            f'mutations of the trace, not {codes.shape[1]}')
    K = int(labels.max()) + 1
    scores = place_scores(codes, assignments, params_full, FN, FP, prior)
    out = place_reduce(scores, assignments, labels, K, alpha, keep=keep)
    out['n_obs'] = (codes != 3).sum(axis=1).astype(np.int64)
    if keep:
        out['scores'] = scores
    return out


def place_cells(post, new_data, assignments, labels, params_full, FN, FP,
        alpha, prior=(.25, .25)):
    """The placement tables: where do cells that were not clustered belong?  Per
    new cell: 'prob' (Q, K), the posterior probability that a cell drawn at
    random from the cluster the new cell joins belongs to MPEAR cluster k,
    and 'p_new', that it opens a cluster of its own (together they sum to
    1); 'cluster' (the arg-max of prob, ties to the smaller index, or -1
    where p_new exceeds every prob) and 'cluster_prob' (its probability);
    'next_cluster' and 'next_prob' (the best MPEAR cluster other than
    `cluster`; -1 and 0 with one cluster); 'entropy' (the mean entropy of the
    allocation over the samples), 'n_obs', 'lpd' (the out-of-sample log
    predictive density of the row) and 'lpd_per_obs' (0 without
    observations).  'total': {'samples', 'cells', 'clusters', 'placed' (the
    count per cluster), 'new', 'lpd', 'mean_lpd_per_obs' (the sum of lpd over
    the observed entries of all new cells), 'worst_cells' (the ten with the
    smallest lpd_per_obs, ties to the smaller index)}.  From an open
    clustering handle: the device pass (Posterior.place) where the handle has
    one, else the host loop (host_place); the same arithmetic on the sums
    either way."""
    codes = data_codes(new_data)
    labels = np.asarray(labels, dtype=np.int64)
    S = np.asarray(assignments).shape[0]
    device = getattr(post, 'place', None)
    if device is not None:
        prob_sum, new_sum, ent_sum, lpd = device(codes, labels, params_full,
            FN, FP, alpha, prior)[:4]
    else:
        red = host_place(codes, assignments, labels, params_full, FN, FP,
            alpha, prior, keep=False)
        prob_sum, new_sum, ent_sum, lpd = (red[k] for k in ('prob_sum',
            'new_sum', 'ent_sum', 'lpd'))
    n_obs = (codes != 3).sum(axis=1).astype(np.int64)
    Q, K = prob_sum.shape
    cells = np.arange(Q)
    prob, p_new = prob_sum / S, new_sum / S
    best = np.argmax(prob, axis=1).astype(np.int64)
    cluster = np.where(p_new > prob[cells, best], -1, best)
    cluster_prob = np.where(cluster < 0, p_new, prob[cells, best])
    if K > 1:
        others = prob.copy()
        placed = cluster >= 0
        others[cells[placed], cluster[placed]] = -np.inf
        next_cluster = np.argmax(others, axis=1).astype(np.int64)
        next_prob = others[cells, next_cluster]
    else:
        next_cluster = np.full(Q, -1, dtype=np.int64)
        next_prob = np.zeros(Q)
    per_obs = np.zeros(Q)
    np.divide(lpd, n_obs, out=per_obs, where=n_obs > 0)
    observed = int(n_obs.sum())
    return {'prob': prob, 'p_new': p_new, 'cluster': cluster,
        'cluster_prob': cluster_prob, 'next_cluster': next_cluster,
        'next_prob': next_prob, 'entropy': ent_sum / S, 'n_obs': n_obs,
        'lpd': lpd, 'lpd_per_obs': per_obs,
        'total': {'samples': int(S), 'cells': int(Q), 'clusters': int(K),
            'placed': np.bincount(cluster[cluster >= 0], minlength=K).tolist(),
            'new': int((cluster < 0).sum()), 'lpd': float(lpd.sum()),
            'mean_lpd_per_obs': float(lpd.sum()) / observed if observed
                else 0.0,
            'worst_cells': np.argsort(per_obs, kind='stable')[:10].tolist()}}


# ---------------------------------------------------------------------------
# between-chain agreement of the clustering (-pc): every chain's co-clustering
# against that of the other chains pooled - not a reference output, so the
# integers below are the specification
# ---------------------------------------------------------------------------
def chain_bounds(bounds, S, N):
    """The bounds of C chains in S pooled samples of N cells as Python
    integers, checked: C + 1 integers rising strictly from 0 to S (so C >= 2
    chains, none empty), and S_c R_c N (N - 1) < 2**63 for every chain, which
    keeps every sum of host_chain_agreement inside int64.  ValueError
    otherwise."""
    b = np.asarray(bounds)
    if b.ndim != 1 or b.size < 1 or b.dtype.kind not in 'iu':
        raise ValueError('the chain bounds must be a vector of integers')
    b = [int(x) for x in b.tolist()]
    C = len(b) - 1
    if C < 2:
        raise ValueError(f'the chain agreement compares chains: {C} chain '
            'has no others (it needs C >= 2)')
    if b[0] != 0 or b[-1] != S:
        raise ValueError(f'the chain bounds run from {b[0]} to {b[-1]}, not '
            f'from 0 to the {S} samples')
    for c in range(C):
        if b[c + 1] <= b[c]:
            raise ValueError(f'chain {c} is empty: the bounds {b[c]}, '
                f'{b[c + 1]} do not increase')
        Sc = b[c + 1] - b[c]
        if Sc * (S - Sc) * N * (N - 1) >= 2 ** 63:
            raise ValueError(f'S_c R_c N (N - 1) of chain {c} does not fit '
                '63 bits')
    return b


def host_chain_agreement(assignments, bounds):
    """(abs_sum, max_abs, flips), int64 (C, N) each - the definition the
    device pass (bnpc_post_chain_agreement) is pinned to.  assignments: the
    pooled S x N samples; chain c owns the samples [bounds[c], bounds[c + 1]).
    With S_c its length, R_c = S - S_c and, for cells i != j, d_c the samples
    of chain c in which they differ in label and d = sum_c d_c:
      same_c = S_c - d_c,  same_r = (S - d) - same_c
      x      = same_c R_c - same_r S_c  (x / (S_c R_c): the pair's
               co-clustering probability in chain c minus that in the rest)
      flip   = [2 same_c > S_c] != [2 same_r > R_c]  (exactly half: apart)
      abs_sum[c][i] = sum_{j != i} |x|, max_abs[c][i] = max_{j != i} |x|,
      flips[c][i] = sum_{j != i} flip.
    Row by row: a chain's samples against one cell's column at a time."""
    a = np.asarray(assignments)
    if a.ndim != 2:
        raise ValueError('the samples must be samples x cells')
    S, N = a.shape
    b = chain_bounds(bounds, S, N)
    C = len(b) - 1
    Sc = np.diff(np.array(b, dtype=np.int64))
    Rc = S - Sc
    abs_sum = np.zeros((C, N), dtype=np.int64)
    max_abs = np.zeros((C, N), dtype=np.int64)
    flips = np.zeros((C, N), dtype=np.int64)
    others = np.ones(N, dtype=bool)
    for i in range(N):
        d_c = np.stack([np.count_nonzero(
            a[b[c]:b[c + 1]] != a[b[c]:b[c + 1], i:i + 1], axis=0)
            for c in range(C)]).astype(np.int64)            # C x N
        same_c = Sc[:, None] - d_c
        same_r = (S - d_c.sum(axis=0))[None, :] - same_c
        x = np.abs(same_c * Rc[:, None] - same_r * Sc[:, None])
        flip = (2 * same_c > Sc[:, None]) != (2 * same_r > Rc[:, None])
        others[i] = False
        if N > 1:
            abs_sum[:, i] = x[:, others].sum(axis=1)
            max_abs[:, i] = x[:, others].max(axis=1)
            flips[:, i] = flip[:, others].sum(axis=1)
        others[i] = True
    return abs_sum, max_abs, flips


def chain_agreement(post, assignments, bounds, labels):
    """The -pc tables: did the chains find the same clustering?  From the
    integers of host_chain_agreement - the device pass
    (Posterior.chain_agreement) where the open clustering handle has one, else
    the host loop on the samples - in float64, the same arithmetic either
    way.  Per cell and chain, (N, C): 'diff' = abs_sum / (S_c R_c (N - 1)), the
    mean absolute difference between the co-clustering probabilities of the
    cell's pairs in chain c and in the other chains; 'max_diff' = max_abs /
    (S_c R_c); 'flips' (integers) and 'flip_share' = flips / (N - 1), the
    pairs the two sides call differently at 0.5.  Per cell: 'cluster' (labels,
    the MPEAR clustering), 'worst_chain' (the largest diff, ties: the smallest
    index) and 'worst_diff'.  Per chain, (C,): 'samples', 'mean_diff_c' =
    (sum_i abs_sum) / (S_c R_c N (N - 1)) with the integer sum taken first,
    'max_diff_c', 'flip_share_c' = sum_i flips / (N (N - 1)).  'clusters' (the
    sorted labels) and 'cluster_diff' (clusters x chains): the mean diff of a
    cluster's cells.  'total': {'chains', 'cells', 'pairs', 'samples',
    'mean_diff' (the mean of the chains'), 'worst_chain', 'worst_mean_diff',
    'flip_share' (all chains pooled)}."""
    a = np.asarray(assignments)
    S, N = a.shape
    b = chain_bounds(bounds, S, N)
    C = len(b) - 1
    device = getattr(post, 'chain_agreement', None)
    if device is not None:
        abs_sum, max_abs, flips = device(np.array(b, dtype=np.int64))
    else:
        abs_sum, max_abs, flips = host_chain_agreement(a, b)
    abs_sum, max_abs, flips = (np.asarray(x, dtype=np.int64)
        for x in (abs_sum, max_abs, flips))
    labels = np.asarray(labels)
    Sc = [b[c + 1] - b[c] for c in range(C)]
    span = [Sc[c] * (S - Sc[c]) for c in range(C)]          # S_c R_c, exact
    diff = np.empty((N, C))
    max_diff = np.empty((N, C))
    for c in range(C):
        diff[:, c] = abs_sum[c] / float(span[c] * (N - 1))
        max_diff[:, c] = max_abs[c] / float(span[c])
    flip_share = flips.T / float(N - 1)
    worst = np.argmax(diff, axis=1).astype(np.int64)
    mean_diff_c = np.array([sum(abs_sum[c].tolist())
        / (span[c] * N * (N - 1)) for c in range(C)])
    flip_share_c = np.array([sum(flips[c].tolist()) / (N * (N - 1))
        for c in range(C)])
    clusters = np.unique(labels)
    cluster_diff = np.array([diff[labels == k].mean(axis=0)
        for k in clusters]).reshape(clusters.size, C)
    worst_c = int(np.argmax(mean_diff_c))
    return {'cluster': labels, 'worst_chain': worst,
        'worst_diff': diff[np.arange(N), worst], 'diff': diff,
        'max_diff': max_diff, 'flips': np.ascontiguousarray(flips.T),
        'flip_share': flip_share,
        'samples': np.array(Sc, dtype=np.int64), 'mean_diff_c': mean_diff_c,
        'max_diff_c': max_diff.max(axis=0), 'flip_share_c': flip_share_c,
        'clusters': clusters, 'cluster_diff': cluster_diff,
        'total': {'chains': C, 'cells': int(N), 'pairs': N * (N - 1) // 2,
            'samples': int(S), 'mean_diff': float(mean_diff_c.mean()),
            'worst_chain': worst_c,
            'worst_mean_diff': float(mean_diff_c[worst_c]),
            'flip_share': sum(flips.ravel().tolist())
                / (C * N * (N - 1))}}


def results_bounds(results):
    """The bounds of the chains in concat_chain_results' pooled samples:
    every chain's post-burn-in length, in the order of results."""
    return np.concatenate([[0], np.cumsum([len(r['assignments'])
        - int(r['burn_in']) for r in results])]).astype(np.int64)


# ---------------------------------------------------------------------------
# -tc / -td metrics (utils.py:49-72): scikit-learn's v_measure_score and
# adjusted_rand_score restated from an integer contingency table (the
# product does not import scikit-learn), the Hamming count of get_hamming_dist
# ---------------------------------------------------------------------------
def _contingency(labels_true, labels_pred):
    """Non-zero cells of the contingency table (rows: true classes, columns:
    inferred clusters) in column-major order - the order SciPy's sparse
    `find` returns them in on the stack the golden files were written with
    (its coo.sum_duplicates sorts by column first), which sets the
    summation order of the mutual information; there the restatement is
    bit-identical to scikit-learn, elsewhere within a few ulp.  Returns
    (row, col, count), row sums, column sums."""
    t = np.unique(np.asarray(labels_true), return_inverse=True)[1].ravel()
    p = np.unique(np.asarray(labels_pred), return_inverse=True)[1].ravel()
    if t.size != p.size:
        raise ValueError('true and inferred clusterings differ in length: '
            f'{t.size} != {p.size}')
    height = int(t.max()) + 1 if t.size else 1
    cells, count = np.unique(p.astype(np.int64) * height + t,
        return_counts=True)
    return cells % height, cells // height, count.astype(np.int64), \
        np.bincount(t).astype(np.int64), np.bincount(p).astype(np.int64)


def _entropy(counts):
    """sklearn.metrics.cluster.entropy from the label counts"""
    from math import log
    pi = counts[counts > 0].astype(np.float64)
    if pi.size <= 1:
        return 0.0
    pi_sum = np.sum(pi)
    return -np.sum((pi / pi_sum) * (np.log(pi) - log(pi_sum)))


def v_measure(labels_pred, labels_true):
    """`v_measure_score(labels_true, labels_pred)` (utils.get_v_measure,
    beta = 1): mutual information over the entropies of both clusterings."""
    from math import log
    if np.asarray(labels_true).size == 0:
        return 1.0
    row, col, nz, n_c, n_k = _contingency(labels_true, labels_pred)
    h_c, h_k = _entropy(n_c), _entropy(n_k)
    if n_c.size == 1 or n_k.size == 1:
        mi = 0.0
    else:
        total = int(nz.sum())
        log_nz = np.log(nz)
        nz_frac = nz / total
        outer = n_c.take(row) * n_k.take(col)
        log_outer = -np.log(outer) + log(n_c.sum()) + log(n_k.sum())
        terms = nz_frac * (log_nz - log(total)) + nz_frac * log_outer
        terms = np.where(np.abs(terms) < np.finfo(terms.dtype).eps, 0.0,
            terms)
        mi = float(np.clip(terms.sum(), 0.0, None))
    homogeneity = mi / h_c if h_c else 1.0
    completeness = mi / h_k if h_k else 1.0
    if homogeneity + completeness == 0.0:
        return 0.0
    return 2 * homogeneity * completeness / (homogeneity + completeness)


def adjusted_rand(labels_pred, labels_true):
    """`adjusted_rand_score(labels_true, labels_pred)` (utils.get_ARI) from
    the pair confusion counts, in Python integers: at 50 000 cells the
    products reach ~1e18."""
    n = np.asarray(labels_true).size
    row, col, nz, n_c, n_k = _contingency(labels_true, labels_pred)
    nz = [int(x) for x in nz.tolist()]
    sum_squares = sum(x * x for x in nz)
    n_c, n_k = n_c.tolist(), n_k.tolist()
    tp = sum_squares - n
    fp = sum(x * n_k[j] for x, j in zip(nz, col.tolist())) - sum_squares
    fn = sum(x * n_c[i] for x, i in zip(nz, row.tolist())) - sum_squares
    tn = n * n - fp - fn - sum_squares
    if fn == 0 and fp == 0:
        return 1.0
    return 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn)
        + (tp + fp) * (fp + tn))


def hamming_similarity(values, cols, true_data):
    """`1 - get_hamming_dist(geno, true) / true.size` (dpmmIO.py:533-542,
    utils.py:63-72): geno is the mutations x cells table whose cell c is
    column cols[c] of `values` (clusters x mutations), rounded half-to-even;
    true_data as loaded (cells x mutations by default).  Compared with the
    truth transposed; if the shapes are equal, the smaller count of both
    orientations; NaN in the truth is a mismatch."""
    true_data = np.asarray(true_data)
    called = np.round(np.asarray(values))[np.asarray(cols)]     # cells x muts
    if true_data.shape != called.shape[::-1]:
        score = np.count_nonzero(called != true_data)
    else:
        score = np.count_nonzero(called.T != true_data)
        if called.shape == true_data.shape:
            score = min(score, np.count_nonzero(called != true_data))
    return 1 - score / true_data.size
