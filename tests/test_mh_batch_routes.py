"""Every route of the screened parameter batch's driver (bnpc_mh_batch_dev,
bnpc_label_counts_and_batch: bnpc_amd/csrc/bnpc_mhbatch.cpp; mh_counts and
mh_screen_launch: bnpc_kernels.hip), each reached on purpose and compared over
its WHOLE output with the plain host batch from the same stream position.

The contract is exact - a screened batch returns the bits of the plain batch
and leaves the stream where the plain batch leaves it - so nothing here has a
tolerance.  The driver reports no route: `plan` below restates, line by line,
how mh_batch_dev_impl cuts a batch into slices (rows under the pinned budget),
parts (the pipeline) and one team job or part after part.  Every case carries
the route it is meant to reach as a string (`describe`), the unmarked tests
assert through `plan` alone that its shape and knobs reach it, and a guard
reads the thresholds `plan` restates out of the sources: when one is retuned
the guard fails and the cases are re-aimed, not dropped.  The one thing the
device tells is Context.mh_screen_stats(): `screened` grows by exactly the
entries of the slices the plan calls screened.  (Nothing is asserted about
the share the screen leaves to the host: that would measure the code under
test.)

References, all compared bit for bit:
  1. the plain host batch, _lib.mh_batch(..., ctx=None), from the same seed:
     status, new parameters, declined counts, prior densities, the stream
     position (one np.random.random() behind the call);
  2. the SciPy-level arithmetic CRP._mh_math on the reference's draws: new,
     declined, the prior table - independent of the C library;
  3. the draws: _lib.mh_draws(G, M, n_sd) from the same seed, row by row.  A
     screened batch that ends with status 0 keeps its draws in the pinned
     block and hands none back, so on the device they are compared where the
     driver hands them back - unscreened batches, caller-given draws and every
     status-1 batch (group G runs those with stream draws on the threaded and
     the sliced route as well) - and are held by the new parameters and the
     stream position everywhere else;
  4. the counts of the label route: n1 / n0 go in as -7 and come back as
     NumPy's (data[assign == id] == 1).sum(0) / (== 0).sum(0), and ll_total
     gives the same bits as after a plain colcounts_by_label.

Groups: A the 512-entry threshold and the part count; B part after part
without completion words, BNPC_MH_SCREEN = 0 / 2; C parts issued by rank 0 and
the three ways the label route's counts arrive; D row slices under the pinned
budget (with the prior cache and the chained sum of the densities); E
counts_src 1 with a summed row; F priors, rates, proposal widths; G status 1;
H one pinned block through a history of capacities.

A one-row batch at M = 256 is 256 entries and therefore NOT screened (plan
says so); the screened one-row batch is the M = 2048, G = 1 case.

Not covered, for the record:
  * the walker that takes draws ahead (MhAhead) is posted from inside
    bnpc_chain_step only: test_draws_taken_ahead_change_nothing;
  * bnpc_rg_counts_and_batch needs a restricted scan in front:
    test_fused_restricted_scan_changes_nothing;
  * the min(8, G) bound on the parts needs more than 32 768 mutations;
  * the fallback without pinned memory needs the host to refuse an
    allocation.
"""
import collections
import contextlib
import os
import re

import numpy as np
import pytest

from bnpc_amd import _lib
from bnpc_amd import fastdist
from bnpc_amd import model as P
import test_host_logic as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'bnpc_amd', 'csrc')

# what `plan` restates (test_the_plan_restates_the_sources reads them back)
MH_SCREEN_MIN = 512
MH_THREADED_MIN = 65536
ZC_OUT_MAX = 512 << 10
PIN_BYTES_PER_ENTRY = 29            # mh_pin_offsets: 8 + 8 + 4 + 4 + 4 + 1
SWEEP_BYTES_DEFAULT = 256 << 20     # mh_pin_max = 2 * BNPC_SWEEP_BYTES
MASK_COUNTS_MAX = 64

KNOBS = ('BNPC_MH_SCREEN', 'BNPC_DONE_WORDS', 'BNPC_SWEEP_BYTES',
    'BNPC_ZERO_COPY', 'BNPC_MASK_COUNTS_MAX')
N_CELLS = 640
SD3 = (0.1, 0.25, 0.5)
PRIOR, RATES = (.25, .25), (.01, .2)
ROWS4 = {'BNPC_SWEEP_BYTES': '14848'}       # M = 256: rows_max = 4
ROWS5 = {'BNPC_SWEEP_BYTES': '9280'}        # M = 128: rows_max = 5
ROWS1 = {'BNPC_SWEEP_BYTES': '1'}           # rows_max = 1
NO_WORDS = {'BNPC_DONE_WORDS': '0'}


# ------------------------------------------------------------------ the plan
Slice = collections.namedtuple('Slice',
    'g0 G screened parts cuts threaded one_job')
Plan = collections.namedtuple('Plan', 'screened rows_max slices')


def roundup16(n):
    return (n + 15) & ~15


def plan(G, M, counts_src=0, knobs=None, given=False):
    """mh_batch_dev_impl, restated: (screened at all, rows_max, slices).
    `given`: the caller brings the draws (rng == NULL)."""
    knobs = knobs or {}
    screen = int(knobs.get('BNPC_MH_SCREEN', 1))
    words = int(knobs.get('BNPC_DONE_WORDS', 1)) != 0
    b = int(knobs.get('BNPC_SWEEP_BYTES', 0))
    pin_max = 2 * (b if b > 0 else SWEEP_BYTES_DEFAULT)
    # rows_max (mhbatch.cpp: "the pinned block has a budget")
    rows_max = max(1, pin_max // (PIN_BYTES_PER_ENTRY * roundup16(M)))
    # mh_screen_applies (the batch is not scored here)
    if not screen or G * M < MH_SCREEN_MIN:
        return Plan(False, rows_max, (Slice(0, G, False, 0, (), False,
            False),))
    if G > rows_max and counts_src == 0:
        rows = [(g0, min(rows_max, G - g0)) for g0 in range(0, G, rows_max)]
    else:
        rows = [(0, G)]
    slices = []
    for g0, Gs in rows:
        E = Gs * M
        if E < MH_SCREEN_MIN:       # a slice is a batch of its own
            slices.append(Slice(g0, Gs, False, 0, (), False, False))
            continue
        threaded = not given and words and Gs >= 4 and counts_src == 0 \
            and E >= MH_THREADED_MIN
        parts = 2 if Gs >= 4 and counts_src == 0 else 1
        if threaded:
            parts = max(2, min(8, Gs, E // (MH_THREADED_MIN // 2)))
        cuts = tuple(Gs * p // parts for p in range(parts + 1))
        slices.append(Slice(g0, Gs, True, parts, cuts, threaded,
            words and parts >= 2))
    return Plan(True, rows_max, tuple(slices))


def describe(pl):
    """'plain', or per slice '<rows>r:<parts>[cuts]' + 'T' (rank 0 issues
    parts) + 'J' (one team job) / 'P' (part after part), or '<rows>r:plain'"""
    if not pl.screened:
        return 'plain'
    out = []
    for s in pl.slices:
        if not s.screened:
            out.append(f'{s.G}r:plain')
        else:
            out.append(f'{s.G}r:{s.parts}[{",".join(map(str, s.cuts))}]'
                + ('T' if s.threaded else '') + ('J' if s.one_job else 'P'))
    return ' | '.join(out)


def screened_entries(pl, M, upto_row=None):
    """what Context.mh_screen_stats()[0] grows by (upto_row: the batch ends
    with the slice that holds this row - status 1)"""
    total = 0
    for s in pl.slices:
        if s.screened:
            total += s.G * M
        if upto_row is not None and s.g0 <= upto_row < s.g0 + s.G:
            break
    return total


def counts_arrival(G, M, knobs=None):
    """how the label route's counts reach the host (counts_from_masks,
    zc_result, colcounts_by_label_impl; 640 cells are one LDS range)"""
    knobs = knobs or {}
    if G > int(knobs.get('BNPC_MASK_COUNTS_MAX', MASK_COUNTS_MAX)):
        return 'cell list'
    if int(knobs.get('BNPC_ZERO_COPY', 1)) and 2 * G * M * 4 <= ZC_OUT_MAX:
        return 'pending'
    return 'synchronous'


# ----------------------------------------------------------------- the cases
# route: 'dev' bnpc_mh_batch_dev behind a separate colcounts_by_label,
# 'label' bnpc_label_counts_and_batch, 'given' bnpc_mh_batch_dev with the
# caller's draws.  want: describe(plan(...)).  arrival: counts_arrival(...) on
# the label route.
Case = collections.namedtuple('Case',
    'group M G route knobs threads want arrival')


def _c(group, M, G, route, want, knobs=None, threads=None, arrival=None):
    return Case(group, M, G, route, knobs or {}, threads, want, arrival)


def _three_ways(group, M, G, want, knobs=None, given_want=None):
    return [_c(group, M, G, 'dev', want, knobs),
        _c(group, M, G, 'label', want, knobs,
            arrival='pending' if want != 'plain' else None),
        _c(group, M, G, 'given', given_want or want, knobs)]


CASES = []
# A: the threshold and the part count, default knobs
for _M, _G, _want in (
        (128, 3, 'plain'), (128, 4, '4r:2[0,2,4]J'), (128, 5, '5r:2[0,2,5]J'),
        (256, 1, 'plain'), (256, 2, '2r:1[0,2]P'), (256, 3, '3r:1[0,3]P'),
        (256, 4, '4r:2[0,2,4]J'), (256, 5, '5r:2[0,2,5]J'),
        (256, 7, '7r:2[0,3,7]J'), (2048, 1, '1r:1[0,1]P')):
    CASES += _three_ways('A', _M, _G, _want)
# B: part after part (no completion words), BNPC_MH_SCREEN = 2 / 0
for _M, _G, _want in ((128, 4, '4r:2[0,2,4]P'), (128, 5, '5r:2[0,2,5]P'),
        (256, 4, '4r:2[0,2,4]P'), (256, 5, '5r:2[0,2,5]P'),
        (256, 7, '7r:2[0,3,7]P')):
    CASES += _three_ways('B', _M, _G, _want, NO_WORDS)
CASES += [
    _c('B', 256, 7, 'dev', '7r:2[0,3,7]P', NO_WORDS, threads=1),
    _c('B', 256, 7, 'label', '7r:2[0,3,7]P', NO_WORDS, threads=1,
        arrival='pending'),
    _c('B', 256, 7, 'dev', '7r:2[0,3,7]J', threads=1),
    _c('B', 256, 5, 'dev', '5r:2[0,2,5]J', {'BNPC_MH_SCREEN': '2'}),
    _c('B', 256, 5, 'label', '5r:2[0,2,5]J', {'BNPC_MH_SCREEN': '2'},
        arrival='pending'),
    _c('B', 256, 5, 'dev', 'plain', {'BNPC_MH_SCREEN': '0'}),
    _c('B', 256, 5, 'label', 'plain', {'BNPC_MH_SCREEN': '0'}),
]
# C: parts issued by rank 0 (M = 2048)
_C_SHAPES = (
    (31, '31r:2[0,15,31]J'), (32, '32r:2[0,16,32]TJ'),
    (48, '48r:3[0,16,32,48]TJ'), (50, '50r:3[0,16,33,50]TJ'),
    (128, '128r:8[0,16,32,48,64,80,96,112,128]TJ'),
    (129, '129r:8[0,16,32,48,64,80,96,112,129]TJ'))
for _G, _want in _C_SHAPES:
    _two = f'{_G}r:2[0,{_G // 2},{_G}]'
    CASES += [_c('C', 2048, _G, 'dev', _want),
        _c('C', 2048, _G, 'dev', _want, threads=1),
        _c('C', 2048, _G, 'dev', _two + 'P', NO_WORDS),
        _c('C', 2048, _G, 'given', _two + 'J')]
CASES += [
    _c('C', 2048, 32, 'label', '32r:2[0,16,32]TJ', arrival='pending'),
    _c('C', 2048, 33, 'label', '33r:2[0,16,33]TJ', arrival='synchronous'),
    _c('C', 2048, 64, 'label', '64r:4[0,16,32,48,64]TJ',
        arrival='synchronous'),
    _c('C', 2048, 65, 'label', '65r:4[0,16,32,48,65]TJ',
        arrival='cell list'),
    _c('C', 2048, 129, 'label', '129r:8[0,16,32,48,64,80,96,112,129]TJ',
        arrival='cell list'),
    _c('C', 2048, 32, 'label', '32r:2[0,16,32]TJ', {'BNPC_ZERO_COPY': '0'},
        arrival='synchronous'),
    _c('C', 2048, 32, 'label', '32r:2[0,16,32]TJ',
        {'BNPC_MASK_COUNTS_MAX': '0'}, arrival='cell list'),
    _c('C', 2048, 32, 'label', '32r:2[0,16,32]P', NO_WORDS,
        arrival='pending'),
]
# D: row slices under the pinned budget
_J4 = '4r:2[0,2,4]J'
_J5 = '5r:2[0,2,5]J'
_ONE = '1r:1[0,1]P'
_D_SHAPES = (
    (256, 9, ROWS4, f'{_J4} | {_J4} | 1r:plain'),
    (256, 10, ROWS4, f'{_J4} | {_J4} | 2r:1[0,2]P'),
    (256, 8, ROWS4, f'{_J4} | {_J4}'),
    (128, 11, ROWS5, f'{_J5} | {_J5} | 1r:plain'),
    (2048, 5, ROWS1, ' | '.join([_ONE] * 5)))
for _M, _G, _knobs, _want in _D_SHAPES:
    CASES += [_c('D', _M, _G, 'dev', _want, _knobs),
        _c('D', _M, _G, 'label', _want, _knobs, arrival='pending')]
CASES += [
    _c('D', 256, 10, 'given', f'{_J4} | {_J4} | 2r:1[0,2]P', ROWS4),
    _c('D', 256, 9, 'dev', '4r:2[0,2,4]P | 4r:2[0,2,4]P | 1r:plain',
        dict(ROWS4, **NO_WORDS)),
]


def _case_id(c):
    knobs = ','.join(f'{k[5:]}={v}' for k, v in c.knobs.items())
    return f'{c.group}-M{c.M}-G{c.G}-{c.route}' \
        + (f'-{knobs}' if knobs else '') \
        + (f'-threads{c.threads}' if c.threads else '')


# ---------------------------------------------------------- CPU: the guards
def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_plan_restates_the_sources():
    """The thresholds and the arithmetic `plan` restates, read out of the
    sources: a retuned threshold fails HERE, and the cases are then re-aimed
    at the routes their ids name."""
    ctx_h = _source('bnpc_ctx.h')
    mh = _source('bnpc_mhbatch.cpp')
    context = _source('bnpc_context.cpp')
    kernels = _source('bnpc_kernels.hip')

    def define(text, name):
        return re.search(rf'#define {name}\s+(.+?)\s*(?://|$)', text,
            re.M).group(1)
    assert define(ctx_h, 'MH_SCREEN_MIN') == str(MH_SCREEN_MIN)
    assert define(ctx_h, 'MH_THREADED_MIN') == str(MH_THREADED_MIN)
    assert define(ctx_h, 'ZC_OUT_MAX') == '((int64_t)512 << 10)' \
        and ZC_OUT_MAX == 512 << 10
    assert re.search(r'int mask_counts_max = (\d+);', ctx_h).group(1) \
        == str(MASK_COUNTS_MAX)
    assert re.search(r'env_int\("BNPC_MASK_COUNTS_MAX", (\d+)\)',
        context).group(1) == str(MASK_COUNTS_MAX)
    # bytes of the pinned block per entry, entries rounded up to 16
    body = re.search(r'static size_t mh_pin_offsets\(.*?\n}\n', mh,
        re.S).group(0)
    assert '(E + 15) & ~(size_t)15' in body
    assert 'return off[5] + Ea;' in body
    assert sum(int(f) for f in re.findall(r'Ea \* (\d+);', body)) + 1 \
        == PIN_BYTES_PER_ENTRY
    # the budget: twice BNPC_SWEEP_BYTES, 2 * 256 MiB without it
    m = re.search(r't\.mh_pin_max = (\d+) \* \(size_t\)\(b > 0 \? b : '
        r'\(long long\)(\d+) << (\d+)\);', context)
    assert int(m.group(1)) == 2 \
        and int(m.group(2)) << int(m.group(3)) == SWEEP_BYTES_DEFAULT
    assert re.search(r'size_t mh_pin_max = \(size_t\)512 << 20;', ctx_h)
    squeezed = re.sub(r'\s+', ' ', mh)
    for line in (
            'return !(a->trans_prob || !c->tun.mh_screen || a->screen '
            '|| a->G * a->M < MH_SCREEN_MIN);',
            'const size_t per_row = mh_pin_offsets((size_t)a->M, off);',
            'const int64_t rows_max = std::max<int64_t>( 1, '
            '(int64_t)(c->tun.mh_pin_max / per_row));',
            'if (a->G > rows_max && counts_src == 0 && row0 == 0 '
            '&& G_all < 0) {',
            'for (int64_t g0 = 0; g0 < a->G; g0 += rows_max) {',
            'const bool threaded = rng && c->tun.done_words && G >= 4 '
            '&& counts_src == 0 && E >= MH_THREADED_MIN;',
            'int parts = (G >= 4 && counts_src == 0) ? 2 : 1;',
            'parts = (int)std::max<int64_t>(2, std::min<int64_t>( '
            'std::min<int64_t>(8, G), (int64_t)(E / (MH_THREADED_MIN / 2))));',
            'for (int p = 0; p <= parts; p++) cut[p] = G * p / parts;',
            'const bool one_job = c->tun.done_words && parts >= 2;'):
        assert line in squeezed, line
    # how the label route's counts arrive
    squeezed = re.sub(r'\s+', ' ', context)
    assert 'if (!c->tun.zero_copy || (int64_t)bytes > ZC_OUT_MAX ' \
        '|| bytes > ZC_OUT_BYTES) return nullptr;' in squeezed
    squeezed = re.sub(r'\s+', ' ', kernels)
    assert 'if (K <= c->tun.mask_counts_max && c->views[0].nblk ' \
        '<= CM_RANGE_MAX) {' in squeezed
    assert int(define(kernels, 'CM_RANGE_MAX')) * 64 >= N_CELLS


@pytest.mark.parametrize('case', CASES, ids=_case_id)
def test_a_case_is_where_its_id_says(case):
    pl = plan(case.G, case.M, 0, case.knobs, case.route == 'given')
    assert describe(pl) == case.want, (
        f'{_case_id(case)} takes {describe(pl)!r}, not {case.want!r}: the '
        f'driver changed - re-aim this case (shape or knobs) instead of '
        f'dropping it')
    if case.arrival:
        assert case.route == 'label' \
            and counts_arrival(case.G, case.M, case.knobs) == case.arrival
    if case.group == 'D':
        assert len(pl.slices) >= 2 and pl.rows_max == pl.slices[0].G


def test_the_cases_cover_the_routes_between_them():
    """every kind of route is named by some case (none was lost in an edit)"""
    wants = ' ~ '.join(c.want for c in CASES)
    for piece in ('plain', '1r:1[0,1]P', '3r:1[0,3]P', '4r:2[0,2,4]J',
            '7r:2[0,3,7]P', '32r:2[0,16,32]TJ', '48r:3[0,16,32,48]TJ',
            '50r:3[0,16,33,50]TJ', '129r:8[', ' | 1r:plain',
            ' | 2r:1[0,2]P'):
        assert piece in wants, piece
    assert {c.arrival for c in CASES if c.route == 'label'} \
        >= {'pending', 'synchronous', 'cell list'}
    # the sizes the issue names
    assert 2 * 32 * 2048 * 4 == ZC_OUT_MAX and 4 * 128 == MH_SCREEN_MIN \
        and 32 * 2048 == MH_THREADED_MIN
    # counts_src 1 is never sliced and never cut
    assert describe(plan(3, 256, 1, ROWS1)) == '3r:1[0,3]P'
    assert describe(plan(2, 256, 1)) == '2r:1[0,2]P'
    assert describe(plan(3, 128, 1)) == 'plain'
    assert describe(plan(4, 256, 1)) == '4r:1[0,4]P'    # (refused: code 2)


# ------------------------------------------------- inputs and the references
_memo = {}


def _data(M):
    key = ('data', M)
    if key not in _memo:
        _memo[key] = H.synth(3 * M + 1, N_CELLS, M, 6, 0.2)
    return _memo[key]


Inputs = collections.namedtuple('Inputs', 'data assign ids n1 n0 old')


def _inputs(M, G):
    """G clusters by label on the M-mutation matrix (ids with gaps, in
    descending order), NumPy's counts, old parameters where a converged chain
    sits, a few of them ON the truncation bounds."""
    key = ('in', M, G)
    if key not in _memo:
        data = _data(M)
        rng = np.random.RandomState(1000 * G + M)
        ids = (3 * np.arange(G)[::-1] + 1).astype(np.int64)
        lab = rng.randint(0, G, N_CELLS)
        if G <= N_CELLS:
            lab[rng.permutation(N_CELLS)[:G]] = np.arange(G)
        assign = ids[lab]
        n1 = np.stack([(data[assign == i] == 1).sum(0) for i in ids]) \
            .astype(np.int32)
        n0 = np.stack([(data[assign == i] == 0).sum(0) for i in ids]) \
            .astype(np.int32)
        _memo[key] = Inputs(data, assign, ids, n1, n0, _old(rng, n1, n0))
    return _memo[key]


def _old(rng, n1, n0):
    G, M = n1.shape
    old = np.clip((n1 + .25) / (n1 + n0 + .5)
        + rng.normal(size=(G, M)) * 0.01, P.TMIN, P.TMAX).astype(np.float32)
    at = rng.choice(G * M, min(8, G * M), replace=False)
    old.ravel()[at[::2]] = np.float32(P.TMIN)
    old.ravel()[at[1::2]] = np.float32(P.TMAX)
    return old


def _table():
    table = P._native_kernels()
    if table is None:
        pytest.skip('native parameter batch not available')
    return table


def _seed(G, M):
    return 11 + 7 * G + M


def _given_draws(G, M, n_sd):
    """draws a caller brings: drawn elsewhere on the stream"""
    np.random.seed(90000 + _seed(G, M))
    return _lib.mh_draws(G, M, n_sd)


def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.int32)
    if a.dtype == np.float64:
        return a.view(np.int64)
    return a


def _same(got, want, what):
    """np.array_equal on the bits (NaN compares, -0.0 is not 0.0)"""
    got, want = _bits(got), _bits(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f'{what}: {len(bad)} entries differ, first at '
            f'(row, column) {tuple(bad[0])}, last at {tuple(bad[-1])}, rows '
            f'{sorted(set(bad[:, 0].tolist()))[:12]}')


Result = collections.namedtuple('Result',
    'status new declined prior draws position')


def _batch(table, old, n1, n0, par, seed, draws=None, **kw):
    """One _lib.mh_batch from `seed`: the draws copied (they are views of
    scratch), the stream position as one uniform behind the call."""
    prior, rates, sd = par
    uniform = prior[0] == prior[1] == 1
    np.random.seed(seed)
    out = _lib.mh_batch(table, old, n1, n0, np.array(sd), P.TMIN, P.TMAX,
        rates[0], rates[1], prior[0], prior[1], uniform, False,
        want_prior=True, draws=draws, **kw)
    status, new, _, declined, pr, d = out
    return Result(status, new, declined, pr, tuple(x.copy() for x in d),
        np.random.random())


def _exact(old, n1, n0, par, draws, old_prior=None):
    """reference 2: CRP._mh_math (new, declined per row, prior table)"""
    prior, rates, sd = par
    probe = P.CRP.__new__(P.CRP)
    probe.param_proposal_sd = np.array(sd)
    probe.p, probe.q = prior
    probe.beta_prior_uniform = bool(prior[0] == prior[1] == 1)
    probe.FP, probe.FN = rates
    new, _, decline, pri = probe._mh_math(old, probe.param_proposal_sd[
        draws[0]], draws[1], draws[2], n1, n0, False, old_prior)
    return new, decline.sum(axis=1), pri


def _reference(table, M, G, par, given, old=None, n1=None, n0=None,
            known=None, tag=None):
    """references 1 - 3 for one batch, made once: the plain host batch, the
    draws of the same seed, the SciPy-level arithmetic (status 0 only)"""
    key = ('ref', M, G, par, given, tag)
    if key in _memo:
        return _memo[key]
    inp = _inputs(M, G)
    old = inp.old if old is None else old
    n1 = inp.n1 if n1 is None else n1
    n0 = inp.n0 if n0 is None else n0
    seed = _seed(G, M)
    draws = _given_draws(G, M, len(par[2])) if given else None
    host = _batch(table, old, n1, n0, par, seed, draws=draws, known=known)
    np.random.seed(seed)
    if given:
        want_draws, want_pos = draws, np.random.random()    # the stream rests
    else:
        want_draws = _lib.mh_draws(G, M, len(par[2]))
        want_pos = np.random.random()
    for got, want, name in zip(host.draws, want_draws, ('sd_idx', 'U', 'u')):
        _same(got, want, f'host draws {name}')
    assert host.position == want_pos, 'host stream position'
    exact = None
    if host.status == 0:
        old_prior = None
        if known is not None and host.prior is not None:
            hit = _bits(known[0]) == _bits(old)
            old_prior = np.where(hit, known[1],
                fastdist.beta_logpdf(old, par[0][0], par[0][1]))
        exact = _exact(old, n1, n0, par, want_draws, old_prior)
        _same(host.new, exact[0], 'host new against CRP._mh_math')
        _same(host.declined, exact[1], 'host declined against CRP._mh_math')
        if host.prior is not None:
            _same(host.prior, exact[2], 'host prior against CRP._mh_math')
        else:
            assert exact[2] is None
    _memo[key] = (host, want_draws, exact)
    return _memo[key]


# ------------------------------------------------------------ the device side
class _Dev:
    """one context per width, made on first use"""

    def __init__(self):
        self.ctxs = {}

    def ctx(self, M):
        if M not in self.ctxs:
            self.ctxs[M] = _lib.Context(data=_data(M))
        return self.ctxs[M]

    def close(self):
        for c in self.ctxs.values():
            c.close()


@pytest.fixture(scope='module')
def dev():
    d = _Dev()
    yield d
    d.close()


@contextlib.contextmanager
def _knobs(monkeypatch, ctx, knobs):
    with monkeypatch.context() as mp:
        for k in KNOBS:
            mp.delenv(k, raising=False)
        for k, v in knobs.items():
            mp.setenv(k, v)
        ctx.reload_options()
        try:
            yield
        finally:
            mp.undo()
            ctx.reload_options()


def _run(table, ctx, M, G, route, par, knobs, threads=None, counts_src=0,
            old=None, n1=None, n0=None, known=None, bad_row=None, tag=None,
            seq=None, view_counts=None):
    """One batch on the device against its references.  The caller has set
    the knobs.  Returns (device Result, host Result)."""
    inp = _inputs(M, G) if counts_src == 0 else None
    old = inp.old if old is None else old
    n1 = inp.n1 if n1 is None else n1
    n0 = inp.n0 if n0 is None else n0
    given = route == 'given'
    pl = plan(G, M, counts_src, knobs, given)
    host, want_draws, exact = _reference(table, M, G, par, given, old, n1, n0,
        known, tag)
    seed = _seed(G, M)
    kw = dict(known=known, threads=threads, ctx=ctx, prior_seq_sum=seq)
    if counts_src == 1:
        view_counts()       # the resident view counts of this batch
    elif route != 'label':
        c1, c0 = ctx.colcounts_by_label(inp.assign, inp.ids)
        _same(c1, inp.n1, 'colcounts_by_label n1')
        _same(c0, inp.n0, 'colcounts_by_label n0')
    before = ctx.mh_screen_stats()[0]
    _poison_scratch(G, M)
    if route == 'label':
        c1 = np.full_like(n1, -7)
        c0 = np.full_like(n0, -7)
        got = _batch(table, old, c1, c0, par, seed,
            label=(inp.assign, inp.ids), **kw)
        _same(c1, n1, 'label route n1')     # reference 4
        _same(c0, n0, 'label route n0')
    else:
        got = _batch(table, old, n1, n0, par, seed,
            draws=want_draws if given else None, counts_src=counts_src, **kw)
    grown = ctx.mh_screen_stats()[0] - before
    assert grown == screened_entries(pl, M, bad_row), (
        f'screened grew by {grown}: the plan is {describe(pl)}')
    assert got.status == host.status == (0 if bad_row is None else 1)
    assert got.position == host.position, 'stream position'
    if got.status == 0:
        _same(got.new, host.new, 'new')
        _same(got.declined, host.declined, 'declined')
        _same(got.new, exact[0], 'new against CRP._mh_math')
        _same(got.declined, exact[1], 'declined against CRP._mh_math')
        if par[0] == (1, 1):
            assert got.prior is None and host.prior is None
        else:
            _same(got.prior, host.prior, 'prior')
            _same(got.prior, exact[2], 'prior against CRP._mh_math')
    # the draws, where the driver hands them back (reference 3)
    if got.status != 0 or given or not pl.screened:
        for g, w, name in zip(got.draws, want_draws, ('sd_idx', 'U', 'u')):
            _same(g, w, f'draws {name}')
    return got, host


def _poison_scratch(G, M):
    """the binding's draw arrays of this shape hold no earlier call's draws"""
    _, sd_idx, U, u, _ = _lib._mh_buffers(G, M)
    sd_idx[...] = -1
    U[...] = np.nan
    u[...] = np.nan


def _total_bits(ctx, inp, rates):
    return _bits(ctx.ll_total(inp.old, [rates[0]], [rates[1]]))


PAR = (PRIOR, RATES, SD3)


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=_case_id)
def test_route_whole_output(case, dev, monkeypatch):
    """groups A - D: see the module docstring and the case's id"""
    table = _table()
    ctx = dev.ctx(case.M)
    inp = _inputs(case.M, case.G)
    with _knobs(monkeypatch, ctx, case.knobs):
        _run(table, ctx, case.M, case.G, case.route, PAR, case.knobs,
            threads=case.threads)
        if case.route == 'label':
            # the resident copy of the counts is intact
            fused = _total_bits(ctx, inp, RATES)
            ctx.colcounts_by_label(inp.assign, inp.ids)
            assert np.array_equal(fused, _total_bits(ctx, inp, RATES))
        if case.knobs.get('BNPC_MH_SCREEN') == '2':
            # verdicts only: the screen vouches for no proposal's bits
            _, draws, _ = _reference(table, case.M, case.G, PAR, False)
            args = (0, inp.old, np.array(SD3), draws, P.TMIN, P.TMAX,
                RATES[0], RATES[1], PRIOR[0], PRIOR[1], False)
            flags = ctx.mh_screen(*args)
            assert not (flags == 3).any() and (flags == 2).any()
    if case.knobs.get('BNPC_MH_SCREEN') == '2':
        assert (ctx.mh_screen(*args) == 3).any()    # (the knob is off again)


# ----------------------------------------- D: the prior cache and the sum
def _known(inp, prior, shift):
    """A cache (known_theta, known_prior) that holds the bits of `old` on
    about half the entries, with the true density there.  The other half
    holds the parameter of the row `shift` rows further on - a hit for a
    driver that moved `old` with the slice or part and the cache not - beside
    a density no entry has."""
    G, M = inp.old.shape
    rng = np.random.RandomState(G + M)
    hit = rng.random_sample((G, M)) < 0.5
    other = np.roll(inp.old, -shift, axis=0)
    other = np.where(_bits(other) == _bits(inp.old), np.float32(0.321), other)
    kt = np.where(hit, inp.old, other).astype(np.float32)
    kp = np.where(hit, fastdist.beta_logpdf(inp.old, prior[0], prior[1]),
        777.0)
    return hit, (kt, kp)


_SUM_CASES = [
    (256, 9, 'dev', ROWS4, '4r:2[0,2,4]J | 4r:2[0,2,4]J | 1r:plain', 4),
    (256, 10, 'label', ROWS4, '4r:2[0,2,4]J | 4r:2[0,2,4]J | 2r:1[0,2]P', 4),
    (256, 10, 'given', ROWS4, '4r:2[0,2,4]J | 4r:2[0,2,4]J | 2r:1[0,2]P', 4),
    (2048, 5, 'dev', ROWS1, ' | '.join([_ONE] * 5), 1),
    (256, 7, 'dev', {}, '7r:2[0,3,7]J', 3),
    (256, 7, 'dev', NO_WORDS, '7r:2[0,3,7]P', 3),
    (2048, 48, 'dev', {}, '48r:3[0,16,32,48]TJ', 16),
    (2048, 48, 'label', NO_WORDS, '48r:2[0,24,48]P', 24),
]


def _sum_id(c):
    return f'M{c[0]}-G{c[1]}-{c[2]}-' + (','.join(f'{k[5:]}={v}'
        for k, v in c[3].items()) or 'default')


@pytest.mark.parametrize('c', _SUM_CASES, ids=_sum_id)
def test_a_cache_case_is_where_its_id_says(c):
    M, G, route, knobs, want, shift = c
    pl = plan(G, M, 0, knobs, route == 'given')
    assert describe(pl) == want
    # the cache's decoys point one slice (or first part) further on
    first = pl.slices[0]
    assert shift == (first.G if len(pl.slices) > 1 else first.cuts[1])
    hit, _ = _known(_inputs(M, G), (.75, 2.), shift)
    for s in pl.slices[1:3]:
        assert hit[s.g0:s.g0 + s.G].any() and not hit[s.g0:s.g0 + s.G].all()


@pytest.mark.gpu
@pytest.mark.parametrize('c', _SUM_CASES, ids=_sum_id)
def test_prior_cache_and_chained_sum_move_with_the_rows(c, dev, monkeypatch):
    """A non-uniform prior with want_prior and a `known` cache that hits on
    about half the entries of every slice and part (known_theta, known_prior
    and prior_out move with the rows), and the sum of the densities chained
    across parts and slices (bnpc_mh_args.prior_seq_sum) against a plain
    left-to-right sum of the returned table, from NaN and from a value."""
    M, G, route, knobs, _, shift = c
    table = _table()
    ctx = dev.ctx(M)
    par = ((.75, 2.), RATES, SD3)
    inp = _inputs(M, G)
    _, known = _known(inp, par[0], shift)
    with _knobs(monkeypatch, ctx, knobs):
        for start in (np.nan, -12.5):
            seq = np.array([start])
            got, _ = _run(table, ctx, M, G, route, par, knobs, known=known,
                tag=('cache', shift), seq=seq)
            assert not (got.prior == 777.0).any()
            flat = got.prior.ravel()
            want = flat[0] if np.isnan(start) else start + flat[0]
            for v in flat[1:].tolist():
                want = want + v         # one accumulator, index order
            assert seq[0] == want, (start, seq[0], want)


# ------------------------------------------------------------ E: counts_src 1
def _view_case(M):
    """a gathered view with repeats, slots of no segment among them"""
    key = ('view', M)
    if key not in _memo:
        data = _data(M)
        rng = np.random.RandomState(5 * M)
        cells = rng.randint(0, N_CELLS, 500)
        cells[:40] = cells[40:80]                   # repeats for certain
        labels = rng.choice([-1, 0, 1], 500, p=[.3, .4, .3]).astype(np.int64)
        rows = [data[cells[labels == g]] for g in (0, 1)]
        n1 = np.stack([(r == 1).sum(0) for r in rows]).astype(np.int32)
        n0 = np.stack([(r == 0).sum(0) for r in rows]).astype(np.int32)
        n1 = np.vstack([n1, n1.sum(0, keepdims=True)]).astype(np.int32)
        n0 = np.vstack([n0, n0.sum(0, keepdims=True)]).astype(np.int32)
        _memo[key] = (cells, labels, n1, n0, _old(rng, n1, n0))
    return _memo[key]


@pytest.mark.gpu
@pytest.mark.parametrize('M,G,knobs,want', [
    (256, 2, {}, '2r:1[0,2]P'), (256, 3, {}, '3r:1[0,3]P'),
    (128, 2, {}, 'plain'), (128, 3, {}, 'plain'),
    (256, 3, ROWS1, '3r:1[0,3]P')],
    ids=['M256-G2', 'M256-G3-summed', 'M128-G2-plain', 'M128-G3-plain',
        'M256-G3-rows_max1-whole'])
def test_view_counts_batch_with_a_summed_row(M, G, knobs, want, dev,
            monkeypatch):
    """counts_src 1: the two segments of the last view_counts, row 2 of a
    three-row batch their sum (mh_counts' sum_row, k_mh_screen's g ==
    sum_row); never sliced, whatever the budget."""
    table = _table()
    ctx = dev.ctx(M)
    assert describe(plan(G, M, 1, knobs)) == want
    cells, labels, n1, n0, old = _view_case(M)

    def view_counts():
        ctx.view_set(1, cells)
        c1, c0 = ctx.view_counts(1, labels, 2)
        _same(c1, n1[:2], 'view_counts n1')
        _same(c0, n0[:2], 'view_counts n0')
    with _knobs(monkeypatch, ctx, knobs):
        for route in ('dev', 'given'):
            _run(table, ctx, M, G, route, PAR, knobs, counts_src=1,
                old=old[:G], n1=n1[:G], n0=n0[:G], tag='view',
                view_counts=view_counts)


@pytest.mark.gpu
def test_four_rows_on_view_counts_are_refused(dev, monkeypatch):
    """G = 4 with counts_src 1: code 2, nothing screened, and the context
    goes on (the G = 3 batch behind it is right)."""
    table = _table()
    M = 256
    ctx = dev.ctx(M)
    cells, labels, n1, n0, old = _view_case(M)
    with _knobs(monkeypatch, ctx, {}):
        ctx.view_set(1, cells)
        ctx.view_counts(1, labels, 2)
        before = ctx.mh_screen_stats()[0]
        four = np.vstack([old, old[:1]])
        with pytest.raises(RuntimeError, match=r'code 2.*view counts'):
            _batch(table, four, np.vstack([n1, n1[:1]]),
                np.vstack([n0, n0[:1]]), PAR, 5, ctx=ctx, counts_src=1)
        assert ctx.mh_screen_stats()[0] == before

        def view_counts():
            ctx.view_counts(1, labels, 2)
        _run(table, ctx, M, 3, 'dev', PAR, {}, counts_src=1, old=old, n1=n1,
            n0=n0, tag='view', view_counts=view_counts)


# ------------------------------------------------ F: priors, rates and widths
_F_SHAPES = [(256, 3, {}, '3r:1[0,3]P'), (256, 5, {}, '5r:2[0,2,5]J'),
    (2048, 32, {}, '32r:2[0,16,32]TJ'),
    (256, 9, ROWS4, '4r:2[0,2,4]J | 4r:2[0,2,4]J | 1r:plain')]
_F_PRIORS = ((.25, .25), (1, 1), (.75, 2.))
_F_RATES = ((.01, .2), (1e-4, .45), (.3, 1e-3))
_F_SDS = ((0.25,), SD3, (0.02, 0.05, 0.1, 0.2, 0.3, 0.5, 0.7, 1.0))


@pytest.mark.parametrize('M,G,knobs,want', _F_SHAPES,
    ids=['one-part', 'two-part', 'threaded', 'sliced'])
def test_a_prior_case_is_where_its_id_says(M, G, knobs, want):
    assert describe(plan(G, M, 0, knobs)) == want
    assert [len(s) for s in _F_SDS] == [1, 3, 8]


@pytest.mark.gpu
@pytest.mark.parametrize('prior', _F_PRIORS, ids=str)
@pytest.mark.parametrize('M,G,knobs,want', _F_SHAPES,
    ids=['one-part', 'two-part', 'threaded', 'sliced'])
def test_priors_rates_and_proposal_widths(M, G, knobs, want, prior, dev,
            monkeypatch):
    """both Beta priors and the uniform one (no prior table on either side),
    mild and extreme error rates, 1, 3 and 8 proposal widths"""
    table = _table()
    ctx = dev.ctx(M)
    with _knobs(monkeypatch, ctx, knobs):
        for rates in _F_RATES:
            for sd in _F_SDS:
                for route in ('dev', 'label'):
                    _run(table, ctx, M, G, route, (prior, rates, sd), knobs)


# ------------------------------------------------------------------ G: status 1
# (M, G, knobs, the plan with stream draws, with given draws, the entry)
_G_CASES = [
    (256, 5, {}, '5r:2[0,2,5]J', '5r:2[0,2,5]J', (0, 17), 'first part'),
    (256, 5, NO_WORDS, '5r:2[0,2,5]P', '5r:2[0,2,5]P', (3, 250),
        'second part, part after part'),
    (2048, 48, {}, '48r:3[0,16,32,48]TJ', '48r:2[0,24,48]J', (40, 2047),
        'a later part of a threaded batch'),
    (256, 10, ROWS4, '4r:2[0,2,4]J | 4r:2[0,2,4]J | 2r:1[0,2]P',
        '4r:2[0,2,4]J | 4r:2[0,2,4]J | 2r:1[0,2]P', (6, 100),
        'second slice'),
    (256, 9, ROWS4, '4r:2[0,2,4]J | 4r:2[0,2,4]J | 1r:plain',
        '4r:2[0,2,4]J | 4r:2[0,2,4]J | 1r:plain', (8, 3),
        'the unscreened last slice'),
]


def _bad_old(M, G, at):
    old = _inputs(M, G).old.copy()
    old[at] = np.float32(P.TMIN / 4)        # an interval right of zero
    return old


@pytest.mark.parametrize('c', _G_CASES, ids=[c[-1] for c in _G_CASES])
def test_a_status_one_case_is_where_its_id_says(c):
    """the plans, and on the host route alone: an `old` entry below tmin
    makes the library hand the batch back (include/bnpc_hip.h, *status = 1),
    with all the draws and the stream behind them"""
    M, G, knobs, want, want_given, at, where = c
    assert describe(plan(G, M, 0, knobs)) == want
    assert describe(plan(G, M, 0, knobs, True)) == want_given
    pl = plan(G, M, 0, knobs)
    s = [s for s in pl.slices if s.g0 <= at[0] < s.g0 + s.G][0]
    if 'part' in where:
        p = sum(at[0] - s.g0 >= cut for cut in s.cuts[1:])
        assert p == (0 if where == 'first part' else s.parts - 1) \
            and (s.threaded or 'threaded' not in where)
    else:
        assert pl.slices.index(s) == (1 if where == 'second slice' else 2)
    table = _table()
    for given in (False, True):
        host, _, _ = _reference(table, M, G, PAR, given, _bad_old(M, G, at),
            tag=('bad', at))
        assert host.status == 1


@pytest.mark.gpu
@pytest.mark.parametrize('route', ['given', 'dev', 'label'])
@pytest.mark.parametrize('c', _G_CASES, ids=[c[-1] for c in _G_CASES])
def test_status_one_hands_the_whole_batch_back(c, route, dev, monkeypatch):
    """Status 1 on both routes, the three draw arrays whole - the given ones,
    or those of the stream in the reference's row order, with the stream
    behind ALL of them -, and the good batch behind it on the same context is
    right."""
    M, G, knobs, _, _, at, _ = c
    table = _table()
    ctx = dev.ctx(M)
    with _knobs(monkeypatch, ctx, knobs):
        _run(table, ctx, M, G, route, PAR, knobs, old=_bad_old(M, G, at),
            bad_row=at[0], tag=('bad', at))
        _run(table, ctx, M, G, route, PAR, knobs)


# ------------------------------------------------------- H: capacity history
_H_STEPS = [(1024, {}, '1024r:8[0,128,256,384,512,640,768,896,1024]TJ'),
    (2, {}, '2r:1[0,2]P'), (384, {}, '384r:3[0,128,256,384]TJ'),
    (9, ROWS4, '4r:2[0,2,4]J | 4r:2[0,2,4]J | 1r:plain'),
    (5, {}, '5r:2[0,2,5]J')]


def test_the_capacity_history_is_where_it_says():
    assert [G * 256 for G, _, _ in _H_STEPS[:3]] == [262144, 512, 98304]
    for G, knobs, want in _H_STEPS:
        assert describe(plan(G, 256, 0, knobs)) == want


@pytest.mark.gpu
def test_one_pinned_block_through_a_history_of_capacities(monkeypatch):
    """The pinned block is laid out for its CAPACITY (mh_pin_get): 262 144
    entries first, then 512, 98 304, a sliced batch and a small one on the
    same context - each equal to the same batch on a fresh context (and to
    the host batch)."""
    table = _table()
    M = 256
    ctx = _lib.Context(data=_data(M))
    try:
        for G, knobs, _ in _H_STEPS:
            with _knobs(monkeypatch, ctx, knobs):
                used, _ = _run(table, ctx, M, G, 'label', PAR, knobs)
            fresh_ctx = _lib.Context(data=_data(M))
            try:
                with _knobs(monkeypatch, fresh_ctx, knobs):
                    fresh, _ = _run(table, fresh_ctx, M, G, 'label', PAR,
                        knobs)
            finally:
                fresh_ctx.close()
            _same(used.new, fresh.new, f'G = {G}: new')
            _same(used.prior, fresh.prior, f'G = {G}: prior')
            _same(used.declined, fresh.declined, f'G = {G}: declined')
            assert used.position == fresh.position
    finally:
        ctx.close()
