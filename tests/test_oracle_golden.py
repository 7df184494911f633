"""Pin the CPU oracle (oracle/crp_numpy.py) to the golden vectors captured from
the imported reference (tests/golden/make_golden.py, numpy 1.26.4 / scipy 1.7.1
/ bottleneck 1.3.2).

Tolerances: the golden stack's np.log differs from this stack's in the last
ulp for ~16 % of arguments (measured), so sums agree to ~1e-15 relative, not
bit for bit; 1e-12 relative is asserted (the north-star bar is 1e-6).  On the
golden stack itself the oracle is bit-identical (oracle/check_same_stack.py).
"""
import hashlib
import os

import numpy as np
import pytest

from oracle import crp_numpy as O
from bnpc_amd.mcmc import MCMC

RTOL = 1e-12


def decode(codes):
    x = codes.astype(np.float64)
    x[codes == 3] = np.nan
    return x


def close(a, b, rtol=RTOL, atol=1e-12):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol)


@pytest.fixture(scope='module')
def G(golden_dir):
    return {n: np.load(os.path.join(golden_dir, n + '.npz'))
        for n in ('calc_ll', 'state_functions', 'normalisers', 'rng',
            'trajectories')}


def test_seqsum_is_sequential():
    rng = np.random.RandomState(0)
    v = np.log(rng.random_sample((13, 257)))
    v[rng.random_sample(v.shape) < 0.2] = np.nan
    clean = np.where(np.isnan(v), 0, v)
    assert np.array_equal(O.seqsum(v, axis=1), np.cumsum(clean, axis=1)[:, -1])
    assert np.array_equal(O.seqsum(v, axis=0), np.cumsum(clean, axis=0)[-1])
    assert O.seqsum(v) == np.cumsum(clean.ravel())[-1]
    assert O.seqsum(np.array([])) == 0.0
    assert O.seqsum(np.full((3, 4), np.nan), axis=1).tolist() == [0, 0, 0]
    assert np.array_equal(O._seqsum_np(v, 1), O.seqsum(v, axis=1))
    assert np.array_equal(O._seqsum_np(v, 0), O.seqsum(v, axis=0))
    assert O.seqsum(np.array([1, 0, 1, -1])) == 1



def _table_sums_cumsum(x, L1, L0):
    """Independent form: per cluster the elements, NaN -> 0, a cumulative
    sum along the mutations (a sequential scan), its last column."""
    out = np.zeros((x.shape[0], L1.shape[0]))
    for k in range(L1.shape[0]):
        el = np.where(x == 1, L1[k], np.where(x == 0, L0[k], np.nan))
        el = np.where(np.isnan(el), 0.0, el)
        if el.shape[1]:
            out[:, k] = np.cumsum(el, axis=1)[:, -1]
    return out


@pytest.mark.parametrize('threads', ['1', '3', '16'])
def test_table_sums_helper_is_the_strict_order_sum(threads, monkeypatch):
    """oracle.seqsum.table_sums (the compiled helper, row slices on threads)
    gives the bits of the NumPy form on ragged shapes, all-missing rows and
    columns, and tables holding -inf, +0.0, -0.0 and NaN."""
    from oracle import seqsum as S
    assert S._LIB is not None, 'oracle/_build/liboracle_seqsum.so not built'
    monkeypatch.setenv('OMP_NUM_THREADS', threads)
    rng = np.random.RandomState(int(threads))
    for n, M, K in ((1, 1, 1), (7, 3, 1), (63, 64, 2), (65, 65, 3),
            (130, 127, 9), (517, 301, 37), (1000, 17, 130), (9, 0, 4)):
        x = (rng.random_sample((n, M)) < 0.35).astype(np.float64)
        x[rng.random_sample(x.shape) < 0.2] = np.nan
        if n > 2 and M > 2:
            x[1] = np.nan                   # an all-missing row
            x[:, M - 2] = np.nan            # an all-missing column
            x[2] = 1.0
        L1 = np.log(rng.uniform(size=(K, M)))
        L0 = np.log(rng.uniform(size=(K, M)))
        if M > 3:
            L1[0, 1] = -np.inf
            L0[K - 1, M - 1] = 0.0
            L1[K - 1, 0] = -0.0
            L0[0, 3] = np.nan
        got = S.table_sums(x, L1, L0)
        assert got.shape == (n, K)
        assert np.array_equal(got, S._table_sums_np(x, L1, L0),
            equal_nan=True), (n, M, K)
        assert np.array_equal(got, _table_sums_cumsum(x, L1, L0),
            equal_nan=True), (n, M, K)
        if n > 2 and M > 2:
            assert np.all(got[1] == 0.0) and not np.any(np.signbit(got[1]))
        if M > 3:
            assert np.all(got[x[:, 1] == 1, 0] == -np.inf)
    # one-dimensional tables are one cluster
    x = (rng.random_sample((5, 6)) < .5).astype(np.float64)
    l1, l0 = np.log(rng.uniform(size=6)), np.log(rng.uniform(size=6))
    assert np.array_equal(S.table_sums(x, l1, l0),
        S._table_sums_np(x, l1[None], l0[None]))

def test_calc_ll(G):
    g = G['calc_ll']
    for ci in range(int(g['n_cases'])):
        data = decode(g[f'c{ci}_data'])
        theta = g[f'c{ci}_theta']
        FP, FN = g[f'c{ci}_FPFN']
        m = O.CRP(data, [-1, -1], [1, 1], FN_error=FN, FP_error=FP)
        ll = np.stack([m._calc_ll(data[[r]], theta)
            for r in range(data.shape[0])])
        close(ll, g[f'c{ci}_ll'])
        flat = m._calc_ll(data, theta[g[f'c{ci}_assign']], True)
        close(flat, g[f'c{ci}_flat'])


def _model_at(g, pre, data, pb, state=1):
    m = O.CRP(data, [-1, -1], list(pb), FN_error=0.1, FP_error=1e-3)
    m.DP_a = float(g[pre + 'DP_a0'])
    m.init_DP_prior()
    m.parameters = np.zeros(data.shape, dtype=np.float32)
    if state == 0:
        m.assignment = g[pre + 'assignment0'].copy()
        m.parameters = g[pre + 'parameters0'].copy()
        ids, cnt = np.unique(m.assignment, return_counts=True)
        m.cells_per_cluster = dict(zip(ids.tolist(), cnt.tolist()))
    else:
        m.assignment = g[pre + 'assignment1'].copy()
        cl = g[pre + 'clusters1']
        m.parameters[cl] = g[pre + 'parameters1']
        m.cells_per_cluster = dict(
            zip(cl.tolist(), g[pre + 'sizes1'].tolist()))
    return m


def test_state_functions(G):
    g = G['state_functions']
    data = decode(g['data'])
    for pi, pb in enumerate(g['param_betas']):
        pre = f'p{pi}_'
        m0 = _model_at(g, pre, data, pb, state=0)
        close(m0._beta_mix_const, g[pre + 'beta_mix'])
        close(m0.CRP_prior, g[pre + 'CRP_prior0'])
        close(m0.get_lpost_single_new_cluster(), g[pre + 'new_cluster'])
        close(m0.get_ll_full(), g[pre + 'll_full0'])
        close(m0.get_lprior_full(), g[pre + 'lprior0'], rtol=1e-10)

        m = _model_at(g, pre, data, pb, state=1)
        close(m.get_ll_full(), g[pre + 'll_full1'])
        close(m.get_lprior_full(), g[pre + 'lprior1'], rtol=1e-10)
        cl = g[pre + 'clusters1']
        got = np.stack([m.get_lpost_single(c, cl)
            for c in range(0, data.shape[0], 7)])
        close(got, g[pre + 'lpost_single'])

        for j in range(int(g[pre + 'n_logA'])):
            cells = g[pre + f'logA{j}_cells']
            new, old = g[pre + f'logA{j}_new'], g[pre + f'logA{j}_old']
            std = g[pre + f'logA{j}_std']
            a = (O.TMIN - old) / std
            b = (O.TMAX - old) / std
            for clip in (0, 1):
                A = m._get_log_A(new, old, cells, a, b, std, bool(clip))
                # includes SciPy truncnorm/beta logpdf of another version
                close(A, g[pre + f'logA{j}_A{clip}'], rtol=1e-9, atol=1e-9)
            x = data[cells]
            mut, wt = m._Bernoulli_FN(x), m._Bernoulli_FP(x)
            close(O.seqsum(np.log(new * mut + (1 - new) * wt), axis=0),
                g[pre + f'logA{j}_newll'])
            close(O.seqsum(np.log(old * mut + (1 - old) * wt), axis=0),
                g[pre + f'logA{j}_oldll'])

        # restricted Gibbs primitives
        cells = g[pre + 'rg_cells']
        i, j, S = cells[0], cells[-1], cells[1:-1]
        fill = m._beta_mix_const[0]
        ll_i = m._calc_ll(data[S], np.nan_to_num(data[i], nan=fill))
        ll_j = m._calc_ll(data[S], np.nan_to_num(data[j], nan=fill))
        close(ll_i, g[pre + 'rg_init_ll_i'])
        close(ll_j, g[pre + 'rg_init_ll_j'])
        m.rg_assignment = g[pre + 'rg_assignment_init'].astype(int)
        m.rg_params_split = g[pre + 'rg_params_split'].copy()
        m.rg_params_merge = g[pre + 'rg_params_merge'].copy()
        close(m._rg_get_ll(S, m.rg_params_split), g[pre + 'rg_ll'])
        close(m._get_ll_ratio(cells, 'split'), g[pre + 'rg_ll_ratio_split'],
            rtol=1e-10, atol=1e-9)
        close(m._get_ll_ratio(cells, 'merge'), g[pre + 'rg_ll_ratio_merge'],
            rtol=1e-10, atol=1e-9)
        close(m._get_lprior_ratio_split(cells), g[pre + 'rg_lprior_split'],
            rtol=1e-10)
        close(m._get_lprior_ratio_merge(cells), g[pre + 'rg_lprior_merge'],
            rtol=1e-10)


def test_rg_init_split_assignment_matches_reference(G):
    """The one DISCRETE decision of the path (ll_j > ll_i, CRP.py:561)."""
    g = G['state_functions']
    data = decode(g['data'])
    for pi, pb in enumerate(g['param_betas']):
        pre = f'p{pi}_'
        m = _model_at(g, pre, data, pb, state=1)
        np.random.seed(99 + pi)
        m._rg_init_split(g[pre + 'rg_cells'].copy())
        ref = g[pre + 'rg_assignment_init'].astype(int)
        # ties decided by rounding noise can differ across numpy versions;
        # require agreement wherever the two log-likelihoods are not within
        # a few ulp of each other
        gap = np.abs(g[pre + 'rg_init_ll_j'] - g[pre + 'rg_init_ll_i'])
        firm = gap > 1e-9
        assert np.array_equal(m.rg_assignment[firm], ref[firm])
        if np.array_equal(m.rg_assignment, ref):
            # Beta draws from identical counts on the identical stream
            close(m.rg_params_split, g[pre + 'rg_params_split'], rtol=1e-6)


def test_ll_full_error(G):
    g = G['state_functions']
    data = decode(g['data'])
    m = O.CRP_errors_learning(data, [-1, -1], [.25, .25], FP_mean=0.01,
        FP_sd=0.01, FN_mean=0.2, FN_sd=0.1)
    m.assignment = g['le_assignment'].copy()
    m.parameters = np.zeros(data.shape, dtype=np.float32)
    m.parameters[g['le_clusters']] = g['le_parameters']
    m.cells_per_cluster = dict(
        zip(g['le_clusters'].tolist(), g['le_sizes'].tolist()))
    m.DP_a = float(g['le_DP_a'])
    m.init_DP_prior()
    got = [m.get_ll_full_error(fp, fn) for fp, fn in g['le_trials']]
    close(got, g['le_ll'])
    close(m.get_lprior_full(), g['le_lprior'], rtol=1e-10)


def test_normalisers(G):
    g = G['normalisers']
    for i in range(int(g['n_vecs'])):
        close(O.CRP._normalize_log_probs(g[f'v{i}']), g[f'np{i}'],
            rtol=1e-13, atol=0)
    for i in range(int(g['n_two'])):
        close(np.asarray(O.CRP._normalize_log(g[f't{i}']), dtype=float),
            g[f'nl{i}'], rtol=1e-13, atol=1e-300)
    for N in (10, 1000):
        a = float(g[f'crp_a_{N}'])
        sizes = np.append(np.arange(1, N + 1), a)
        close(np.append(0, O.CRP.log_CRP_prior(sizes, N, a)),
            g[f'crp_prior_{N}'], rtol=1e-14)


def test_legacy_rng_stream_is_stable(G):
    """The legacy np.random stream the sampler consumes is bit-stable across
    the golden numpy (1.26.4) and this one."""
    g = G['rng']
    for seed in (1, 42, 1608637542):
        pre = f's{seed}_'
        np.random.seed(seed)
        assert np.array_equal(np.random.random(5), g[pre + 'random'])
        assert np.array_equal(np.random.permutation(37), g[pre + 'perm'])
        assert np.array_equal(np.random.randint(0, 1000, size=11),
            g[pre + 'randint'])
        assert np.array_equal(np.random.randint(0, 2 ** 32 - 1, 3),
            g[pre + 'randint_big'])
        p = np.array([.1, .2, .3, .25, .15])
        got = [np.random.choice(np.arange(5), p=p) for _ in range(20)]
        assert np.array_equal(got, g[pre + 'choice_p'])
        assert np.array_equal(
            np.random.choice(np.array([.1, .25, .5]), size=50),
            g[pre + 'choice_sd'])
        assert np.array_equal(np.random.choice(17, size=2, replace=False),
            g[pre + 'choice2'])
        assert np.array_equal(np.random.permutation(1000), g[pre + 'perm2'])
        assert np.array_equal(np.random.random(3), g[pre + 'random_after'])
        close(np.random.beta(np.array([.25, 1.25, 7.25, .25]),
            np.array([.25, .25, 3.25, 9.25])), g[pre + 'beta'], rtol=1e-14)
        close([np.random.gamma(3.5, 0.7), np.random.gamma(0.4, 2.0)],
            g[pre + 'gamma'], rtol=1e-14)
        assert np.array_equal(np.random.random(2), g[pre + 'random_end'])


def run_oracle_chain(kind, data, steps, seed, pb=(.25, .25), sm_prob=.33,
        sm_steps=3):
    if kind == 'fixed':
        model = O.CRP(data, DP_alpha=[-1, -1], param_beta=list(pb),
            FN_error=0.1, FP_error=0.001)
        eup = 0
    else:
        model = O.CRP_errors_learning(data, DP_alpha=[-1, -1],
            param_beta=list(pb), FP_mean=0.01, FP_sd=0.01, FN_mean=0.2,
            FN_sd=0.1)
        eup = .25
    mcmc = MCMC(model, sm_prob=sm_prob, dpa_prob=.25, error_prob=eup,
        sm_ratios=[.75, .25], sm_steps=sm_steps)
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        mcmc.run((steps, int(steps * .33)), seed, 1, 0, '', True)
    return mcmc.get_results()[0], mcmc.get_seeds()[0]


def sha16(assignments):
    return hashlib.sha256(np.ascontiguousarray(
        assignments, dtype=np.int64).tobytes()).hexdigest()[:16]


def test_trajectory_example_fixed_errors(G, golden_dir):
    """example_data, seed 42, 200 steps, fixed errors:
    identical assignment trajectory (sha ec91db5ad46ef182), ML to 1e-9."""
    from bnpc_amd.io import load_data
    g = G['trajectories']
    data = load_data(os.path.join(golden_dir, 'example_data.csv'),
        transpose=True)
    assert data.shape == (100, 100)
    assert np.isnan(data).sum() == 948 and np.nansum(data) == 2445
    res, seed = run_oracle_chain('fixed', data, 200, 42)
    assert seed == 1608637542 == int(g['ex_fixed_chain_seed'])
    assert np.array_equal(res['assignments'], g['ex_fixed_assignments'])
    assert sha16(res['assignments']) == 'ec91db5ad46ef182'
    close(res['ML'], g['ex_fixed_ML'], rtol=1e-9)
    close(res['MAP'], g['ex_fixed_MAP'], rtol=1e-9)
    close(res['DP_alpha'], g['ex_fixed_DP_alpha'], rtol=1e-9)
    close(res['params'][-1], g['ex_fixed_params_last'], rtol=1e-5)


def test_trajectory_small_fixed_errors(G):
    """60 x 40 synthetic, split-merge heavy.  On the golden stack the oracle
    is bit-identical over all 120 steps (oracle/check_same_stack.py); on a
    newer numpy the run with -smp 0.5 leaves the golden trajectory at step 63
    (a last-ulp np.log difference decides a tie), so the prefix is pinned."""
    g = G['trajectories']
    data = decode(g['small_data'])
    res, _ = run_oracle_chain('fixed', data, 120, 7, sm_prob=.5, sm_steps=2)
    n = 50
    assert np.array_equal(res['assignments'][:n],
        g['sm_fixed_assignments'][:n])
    close(res['ML'][:n], g['sm_fixed_ML'][:n], rtol=1e-9)
    res, _ = run_oracle_chain('fixed', data, 80, 5, pb=(1, 1))
    assert np.array_equal(res['assignments'], g['uni_fixed_assignments'])
    close(res['ML'], g['uni_fixed_ML'], rtol=1e-9)
    res, _ = run_oracle_chain('learn', data, 120, 7, sm_prob=.5, sm_steps=2)
    assert np.array_equal(res['assignments'][:n],
        g['sm_learn_assignments'][:n])
    close(res['ML'][:n], g['sm_learn_ML'][:n], rtol=1e-8)


def test_trajectory_learned_errors_prefix(G, golden_dir):
    """Learned-error traces depend on SciPy's scalar truncnorm.rvs, which
    differs in the last ulp between the golden SciPy (1.7.1) and newer ones
    and diverges after ~100 steps: the prefix must
    still agree."""
    from bnpc_amd.io import load_data
    g = G['trajectories']
    data = load_data(os.path.join(golden_dir, 'example_data.csv'),
        transpose=True)
    res, _ = run_oracle_chain('learn', data, 200, 42)
    n = 40
    assert np.array_equal(res['assignments'][:n],
        g['ex_learn_assignments'][:n])
    close(res['ML'][:n], g['ex_learn_ML'][:n], rtol=1e-8)
    close(res['FN'][:n], g['ex_learn_FN'][:n], rtol=1e-8)
    close(res['FP'][:n], g['ex_learn_FP'][:n], rtol=1e-8)


def test_config5_first_cells_fixture_is_what_its_maker_describes(golden_dir):
    """c5_first_cells.npz (tests/golden/make_c5_first_cells.py: the oracle's
    first cells of config 5's first sweep at full size; re-making it takes
    ten CPU-minutes, so here only its shape): distinct cells, the cluster each
    drew, a new cluster = the lowest free id at that moment, the cluster
    count moving by at most one per cell."""
    g = np.load(os.path.join(golden_dir, 'c5_first_cells.npz'))
    cells, drawn, K_after, born = (g[k] for k in ('cells', 'drawn', 'K_after',
        'born'))
    n = cells.size
    assert n >= 64 and drawn.size == K_after.size == born.size == n
    assert np.unique(cells).size == n and cells.min() >= 0 \
        and cells.max() < 50000
    assert int(g['seed']) == 42 and 31000 < int(g['K0']) < 32000
    assert 8 <= born.sum() <= n
    steps = np.diff(np.concatenate([[int(g['K0'])], K_after]))
    assert np.all(np.abs(steps) <= 1)
    # a cell that opens a cluster never lowers the count; one that joins an
    # existing cluster never raises it
    assert np.all(steps[born] >= 0) and np.all(steps[~born] <= 0)
    assert 0.0 <= float(g['peek']) < 1.0


# ------------------------- the extended-precision reference of the flat total
def _total_forms():
    import test_total_and_screen_forms as T
    from oracle import likelihood as L
    if L.TOTAL_REFERENCE is None:
        pytest.skip('no arithmetic with a 64-bit significand on this host')
    return T, L


def test_total_reference_is_the_sum_it_says():
    """total_ll_reference against decimal arithmetic (50 digits) element by
    element - float32 `1 - theta` taken as an input, the bounds of theta,
    extreme error rates - and against the oracle's get_ll_full on a matrix."""
    import decimal
    T, L = _total_forms()
    D = decimal.Decimal
    theta = np.array([[T.TMIN, 0.5, T.TMAX, 0.3, 0.7]], dtype=np.float32)
    n1 = np.array([[3, 0, 1, 0, 7]], dtype=np.int32)
    n0 = np.array([[0, 2, 5, 0, 11]], dtype=np.int32)
    with decimal.localcontext() as dc:
        dc.prec = 50
        for fp, fn in T.RATES:
            want = mag = D(0)
            for th, c1, c0 in zip(theta[0], n1[0], n0[0]):
                t, o = D(float(th)), D(float(np.float32(1) - th))
                term = int(c1) * (t * (1 - D(fn)) + o * D(fp)).ln() \
                    + int(c0) * (t * D(fn) + o * (1 - D(fp))).ln()
                want += term
                mag += abs(term)
            total, got_mag, mass = L.total_ll_reference(theta, n1, n0, fp, fn)
            assert mass == 29
            assert abs(D(float(got_mag)) - mag) < D(2) ** -45 * mag
            # the total itself carries more than a float64 holds: both halves
            hi = float(total)
            lo = float(total - type(total)(hi))
            assert abs(D(hi) + D(lo) - want) < D(2) ** -58 * mag, (fp, fn)
            assert L.total_ll_distance(hi, total) <= abs(hi) * 2.0 ** -53
    # theta without counts is not read
    other = theta.copy()
    other[0, 3] = 0.9
    assert L.total_ll_reference(other, n1, n0, .01, .2)[0] \
        == L.total_ll_reference(theta, n1, n0, .01, .2)[0]
    # the oracle's flat total from the matrix itself
    case = T.total_case(257, 255)
    x = T.total_data(257)[0]
    m = O.CRP(x, [-1, -1], [1, 1], FN_error=.2, FP_error=.01)
    flat = m._calc_ll(x, case.theta[case.assign], True)
    total, mag, _ = T.total_reference(case, 0)
    assert T.RATES[0] == (.01, .2)
    assert abs(flat - float(total)) < 1e-12 * mag
    # ... and the float64 evaluation in the kernel's grouping on a shape small
    # enough to write the grouping out: 257 elements = block 0 full, block 1
    # one element; thread j of block 0 meets thread j + 128, + 64, ...
    case = T.total_case(257, 1)
    t = case.theta.astype(np.float64).ravel()
    o = (1 - case.theta).astype(np.float64).ravel()
    term = case.n1.ravel() * np.log(t * (1.0 - .2) + o * .01) \
        + case.n0.ravel() * np.log(t * .2 + o * (1.0 - .01))
    red = list(term[:256])
    for s in (128, 64, 32, 16, 8, 4, 2, 1):
        red = [red[j] + red[j + s] for j in range(s)]
    assert L.total_ll_kernel_order(case.theta, case.n1, case.n0, .01, .2) \
        == (0.0 + red[0]) + term[256]


def test_total_bound_holds_for_float64_in_the_kernels_order():
    """The bound of the GPU tests (oracle.likelihood.total_ll_bound, derived
    from k_ll_total's arithmetic) against a NumPy float64 evaluation in the
    kernel's grouping, at every shape and rate pair of
    test_total_and_screen_forms.py: inside it with room to spare.  Observed:
    |float64 - reference| / bound is at most 0.08 over the 52 cases (the
    roundings do not all point the same way); a ratio above 0.25 would mean
    the derivation is wrong, not that the margin is too small."""
    T, L = _total_forms()
    worst = 0.0
    for shape in T.SHAPES:
        case = T.total_case(*shape)
        assert case.KM == shape[0] * shape[1]
        blocks = min(-(-case.KM // 256), 256)
        assert L.total_ll_chain(case.KM) \
            == -(-case.KM // 65536) + 8 + blocks
        for j, (fp, fn) in enumerate(T.RATES):
            total, mag, mass = T.total_reference(case, j)
            assert mass == case.n1.sum() + case.n0.sum() and mag > 0
            emu = L.total_ll_kernel_order(case.theta, case.n1, case.n0,
                fp, fn)
            bound = L.total_ll_bound(case.KM, mag, mass)
            ratio = L.total_ll_distance(emu, total) / bound
            print(f'[total bound] M {case.M} K {case.K} rates {fp, fn}: '
                f'{emu!r}, ratio {ratio:.4f}')
            assert ratio < 0.25, (shape, fp, fn, ratio)
            worst = max(worst, ratio)
    print(f'[total bound] worst ratio {worst:.4f}')


# ------------------- the pdist-free references of tests/test_posterior_forms
def _pdist_counts(a):
    from scipy.spatial.distance import pdist
    out = np.zeros(a.shape[1] * (a.shape[1] - 1) // 2, dtype=np.int32)
    for row in a:
        out += pdist(np.stack([row, row]).T, 'hamming').astype(np.int32)
    return out


def test_differ_rows_is_the_pdist_accumulation(golden_dir):
    """oracle.posterior_numpy.differ_rows (row by row, no pdist) against the
    per-sample pdist accumulation on ragged small shapes, with and without
    labels that fit an int8, and against the reference's own mean distance
    of the golden samples."""
    from oracle import posterior_numpy as Q
    rng = np.random.RandomState(11)
    for S, N, lo, hi in ((1, 2, 0, 2), (1, 3, 0, 2), (3, 5, -3, 4),
            (7, 66, 0, 5), (33, 131, -200, 200), (2, 17, 0, 1)):
        a = rng.randint(lo, hi, size=(S, N))
        got = Q.differ_rows(a)
        assert got.dtype == np.int32 and got.shape == (N * (N - 1) // 2,)
        assert np.array_equal(got, _pdist_counts(a)), (S, N)
    g = np.load(os.path.join(golden_dir, 'posterior.npz'))
    a0 = g['r0_assignments'][int(g['r0_burn_in']):]
    assert np.array_equal(Q.differ_rows(a0) / a0.shape[0], g['dist0'])


def test_same_label_sums_is_the_fake_devices():
    """oracle.posterior_numpy.same_label_sums (group by group through the
    condensed index) against FakePosterior.mpear_sums (a pdist mask): random
    candidates, everything in one cluster (the sum of all counts), all
    singletons (0), labels at the ends of the device's range."""
    from fake_device import FakePosterior
    from oracle import posterior_numpy as Q
    rng = np.random.RandomState(12)
    for S, N in ((1, 2), (4, 3), (9, 66), (20, 131)):
        a = rng.randint(0, 4, size=(S, N))
        fake = FakePosterior(a)
        lab = rng.randint(0, rng.randint(1, 9, size=(7, 1)), size=(7, N))
        lab[0] = 0
        lab[1] = np.arange(N)
        lab[2] = np.where(lab[2] == 0, 65533, lab[2])
        got = Q.same_label_sums(fake.differ(), lab)
        assert got.dtype == np.int64
        assert np.array_equal(got, fake.mpear_sums(lab)), (S, N)
        assert got[0] == fake.differ_sum and got[1] == 0
    assert Q.same_label_sums(fake.differ(), lab[:0]).shape == (0,)


def test_differ_rows_takes_labels_at_the_int32_extremes():
    """Only equality matters: samples whose labels are drawn from [-64, -1],
    0, INT32_MIN and INT32_MAX count like a copy relabelled to 0 .. 66."""
    from oracle import posterior_numpy as Q
    info = np.iinfo(np.int32)
    pool = np.concatenate([np.arange(-64, 0), [info.min, info.max, 0]]) \
        .astype(np.int32)
    rng = np.random.RandomState(13)
    pick = rng.randint(0, pool.size, size=(9, 70))
    a = pool[pick]
    assert a.dtype == np.int32 and a.min() == info.min and a.max() == info.max
    want = Q.differ_rows(pick)
    assert np.array_equal(Q.differ_rows(a), want)
    assert np.array_equal(want, _pdist_counts(pick))
