"""Every route of a split / merge move's native driver (bnpc_sm_move:
bnpc_amd/csrc/bnpc_moves.cpp; bnpc_rg_scan_step_with: bnpc_sweeps.cpp;
bnpc_rg_counts_and_batch: bnpc_mhbatch.cpp), each reached on purpose at the
smallest shape that reaches it and compared with the oracle's move from the
same state and seed.

A move is a dozen host and device steps in one call: the proposal; the view
and the launch state from the two anchors' own rows; the view's column
counts; three Beta rows with the first scan's sums queued under the third;
`scan_no` intermediate restricted scans; a scored scan (split) or a scored
one-row batch and the reverse scan (merge); four ratios and the acceptance
draw; the writes of an accepted move - or the move handed back at any point,
the stream and the cached Gaussian put back.  The driver reports no route:
`plan` below restates its decisions, every case carries the event it is meant
to reach in its id, the unmarked tests assert with the oracle alone that it
does (and that no decision sits on a knife edge), and a guard reads the
thresholds `plan` restates out of the sources: when one is retuned the guard
fails and the cases are re-aimed, not dropped.

The routes:
  * handed back early (n <= 2: no device work), late (a merge of 3 cells,
    S - 1 <= 0, after all the device work; an element of the split's own row
    that bnpc_log_accept leaves to SciPy) - or done;
  * scan_no = 0 (a merge queues nothing ahead, a split's scored scan adopts
    the queued sums) / > 0 (the first intermediate scan adopts them);
  * every intermediate scan's second half: counts, then the batch (3 M < 512
    entries), counts and screen in one wait (3 M >= 512), with the draws taken
    ahead by a walker (3 M >= 2048; from 512 under BNPC_MH_AHEAD=2);
  * a split whose scan leaves one side empty (no acceptance uniform);
  * accepted (the writes) / declined.

References, none of them the code under test:
  1. the oracle (oracle.crp_numpy) for a whole move, through a recording
     subclass: the four terms of A, their sum, the cells of the move, whether
     the launch state ended degenerate, log(u) of the acceptance draw;
  2. NumPy for a single scan: reference_rg_scan (test_native_sweeps),
     CRP._mh_math on _lib.mh_draws from the reference's stream position, and
     (data[cells][labels == g] == 1).sum(0) / == 0 for the counts;
  3. the binding's own step-by-step walk (BNPC_NATIVE_MOVES=0): a second
     witness for the stream position only.

Compared with the oracle after every move, all exact: the result flags, the
assignment, the cluster table in dict order, the parameter rows of the live
clusters as float32 bits, one uniform peeked off the stream, the cells of the
move.  log_A is compared to 1e-9 (the project's bound for device
likelihoods) of the largest absolute value among the oracle's four terms - A
is their sum and may cancel.

Route evidence, exact: Context.mh_screen_stats()[0] grows by 3 M per
intermediate scan iff 3 M >= MH_SCREEN_MIN and the screen is on, by nothing
for the scored scan and the merge's one-row batch; bnpc_mh_ahead_stats
(begun, taken, rows) as `plan` says; the model's _native_moves by 1, by 0 for
a hand-back.  (Nothing is asserted about the share the screen leaves to the
host.)

Groups: A kind x scan_no x outcome; B the thresholds of the scan's second
half; C the cells of the move on the view's 64-slot edges and M on the mask
words; D degenerate and tied launch states; E hand-backs; F state shapes; G
the documented switches; H one context through a history of moves; I one scan
alone (bnpc_rg_scan_step) against reference 2, status 1 included; J a move
beside an issued tile.

Group J, for the record: with a tile in flight bnpc_rg_counts_and_batch does
not fuse (any_tile_pending) and no walker is posted, but the batch behind the
separate counts is still bnpc_mh_batch_dev, which screens from 512 entries on
the side lane: `screened` stays flat at M = 170 and grows by 3 M per scan at
M = 171.  `plan` says so (tile=True) and both widths are run.

Not covered: bnpc_move_last_draw_hook is set only inside bnpc_chain_step (the
walker of the step's parameter batch under a move's tail); it is held by
test_draws_taken_ahead_change_nothing (test_gpu_parity.py).  Two things on
the path show in no output and no counter, so nothing here can hold them:
WHICH call computes a scan's first sums (queued under the third Beta row or
made by the scan itself - the same sums), and the sum_rows() behind a split's
scored scan (the two sides always add up to the cells of the move: the third
row cannot have changed).
"""
import collections
import contextlib
import os
import re

import numpy as np
import pytest

from oracle import crp_numpy as O
from bnpc_amd import _lib
from bnpc_amd import model as P
from test_native_sweeps import reference_rg_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'bnpc_amd', 'csrc')

# what `plan` restates (test_the_plan_restates_the_sources reads them back)
MH_SCREEN_MIN = 512
MH_AHEAD_SCAN_MIN = 2048

KNOBS = ('BNPC_MH_SCREEN', 'BNPC_MH_AHEAD', 'BNPC_DONE_WORDS',
    'BNPC_ZERO_COPY', 'BNPC_HOST_THREADS', 'BNPC_LOOP_SHORTCUTS', 'BNPC_KW',
    'BNPC_MASK_COUNTS_MAX', 'BNPC_NATIVE_MOVES', 'BNPC_RG_FUSED')
N_CELLS = 200
N_A = 140               # cells 0 .. 139: clone A (cell 0: every entry missing)
RTOL = 1e-9             # the project's bound for device likelihoods
EDGE_A = 1e-6           # |log(u) - A| of the acceptance draw, relative
EDGE_PICK = 1e-9        # |c0 / c1 - u| of a scan's pick


# ------------------------------------------------------------------ the plan
Plan = collections.namedtuple('Plan',
    'handback fused walker screened begun taken rows native')


def plan(move, scan_no, n, M, knobs=None, late=False, tile=False):
    """bnpc_sm_move with its scans, restated: what one move of `n` cells does
    to the counters.  `late`: an element of the split's own row is left to
    SciPy (bnpc_log_accept, after every scan).  `tile`: an issued tile is in
    flight on the context."""
    knobs = knobs or {}
    screen = int(knobs.get('BNPC_MH_SCREEN', 1)) != 0
    ahead = int(knobs.get('BNPC_MH_AHEAD', 1))
    if n <= 2:                          # bnpc_moves.cpp: if (n <= 2) return 0
        return Plan('early', False, False, 0, 0, 0, 0, 0)
    handback = None
    if move == 'merge' and (n - 2) - 1 <= 0:    # if (S - 1 <= 0) return 0
        handback = 'late'
    if late:
        handback = 'late'
    E = 3 * M                           # an intermediate scan's batch: G = 3
    # bnpc_rg_counts_and_batch: fused = !trans_prob && mh_screen
    #   && G * M >= MH_SCREEN_MIN && !any_tile_pending()
    fused = screen and E >= MH_SCREEN_MIN and not tile
    # (not fused: bnpc_view_counts, then bnpc_mh_batch_dev on counts_src 1,
    # which screens by mh_screen_applies alone)
    screens = screen and E >= MH_SCREEN_MIN
    # bnpc_mh_ahead_begin from bnpc_mh_ahead_scan: mode, the screen, the size
    walker = ahead != 0 and screen and not tile \
        and E >= (MH_SCREEN_MIN if ahead >= 2 else MH_AHEAD_SCAN_MIN)
    begun = scan_no if walker else 0
    taken = begun if ahead in (1, 2) else 0     # mh_ahead_claim: mode 3 drops
    return Plan(handback, fused, walker, scan_no * E if screens else 0, begun,
        taken, 3 * taken, 0 if handback else 1)


def describe(pl):
    if pl.handback == 'early':
        return 'early'
    return ('fused' if pl.fused else 'unfused') \
        + ('+walker' if pl.walker else '') \
        + ('+late' if pl.handback else '')


# ------------------------------------------------------------------ the data
_memo = {}


def _data(M, variant='two'):
    """Two clones (140 and 60 cells) seen through false negatives, false
    positives and 15 % missing entries; cell 0 has no entry at all.  'same':
    200 identical rows (every launch tie goes to anchor i)."""
    key = ('data', M, variant)
    if key not in _memo:
        rng = np.random.RandomState(7 * M + 1)
        geno = rng.random_sample((2, M)) < 0.35
        if variant == 'same':
            row = np.where(geno[0], 1., 0.)
            row[rng.random_sample(M) < 0.15] = np.nan
            data = np.repeat(row[None, :], N_CELLS, axis=0)
        else:
            z = (np.arange(N_CELLS) >= N_A).astype(int)
            X = geno[z]
            u = rng.random_sample((N_CELLS, M))
            data = np.where(X, u >= 0.1, u < 0.001).astype(np.float64)
            data[rng.random_sample((N_CELLS, M)) < 0.15] = np.nan
            data[0] = np.nan
        _memo[key] = data
    return _memo[key]


State = collections.namedtuple('State', 'assignment items parameters target')


def _groups(name, n):
    """The clusters of a state as cell lists, the move's own first (`target`
    of them), then what is left of clone A and of clone B."""
    A = np.arange(1, N_A)
    B = np.arange(N_A, N_CELLS)
    nb = min(n // 2, 50)
    if name == 'all':               # K = 1
        return [np.arange(N_CELLS)], 1
    if name == 'lump':              # both clones in one cluster
        own = [np.concatenate([A[:n - nb], B[:nb]])]
    elif name == 'clone':           # one clone as one cluster
        own = [A[:n]]
    elif name == 'blank':           # ... with the cell that has no entry
        own = [np.concatenate([[0], A[:n - 1]])]
    elif name == 'halves':          # two halves of one clone
        own = [A[:n // 2], A[n // 2:n]]
    elif name == 'pair':            # two different clones
        own = [A[:n - nb], B[:nb]]
    else:
        raise ValueError(name)
    used = np.concatenate(own)
    rest = [np.setdiff1d(np.append(A, 0), used), np.setdiff1d(B, used)]
    return own + [r for r in rest if r.size], len(own)


def _state(name, n, M, variant='two', ids=None, low=False):
    """Assignment, cluster table (dict order = `ids`), parameter rows drawn
    where a chain sits.  `low`: one entry of the first cluster's row at
    TMIN / 4 (left to SciPy)."""
    key = ('state', name, n, M, variant, ids, low)
    if key not in _memo:
        data = _data(M, variant)
        groups, target = _groups(name, n)
        use = list(ids) if ids else list(range(len(groups)))
        assert len(use) == len(groups)
        assignment = np.full(N_CELLS, -1, dtype=np.int64)
        for cl, cells in zip(use, groups):
            assignment[cells] = cl
        assert (assignment >= 0).all()
        rng = np.random.RandomState(1000 + 3 * n + M)
        parameters = np.full((N_CELLS, M), np.float32(O.TMIN), np.float32)
        for cl, cells in zip(use, groups):
            n1 = (data[cells] == 1).sum(0)
            n0 = (data[cells] == 0).sum(0)
            parameters[cl] = np.clip(rng.beta(.25 + n1, .25 + n0), O.TMIN,
                O.TMAX).astype(np.float32)
        if low:
            parameters[use[0], min(5, M - 1)] = np.float32(O.TMIN / 4)
        items = [(int(cl), int(cells.size)) for cl, cells in zip(use, groups)]
        _memo[key] = State(assignment, items, parameters,
            tuple(use[:target]))
    return _memo[key]


# ----------------------------------------------------------------- the cases
# kind: 'split' do_split_move, 'merge' do_merge_move, 'auto'
# update_assignments_split_merge.  event: 'accepted', 'declined' (two sides),
# 'one-side' (a split whose scan left a side empty: declined without a
# uniform), 'early' / 'late' (handed back).  SEEDS holds, per case, the seed
# and the event it reaches: found with the oracle alone, asserted by the
# unmarked tests.
Case = collections.namedtuple('Case', 'group kind state n M scan_no want '
    'variant ids low pb model knobs prime tile')


def _c(group, kind, state, n, M, scan_no, want=None, variant='two', ids=None,
        low=False, pb=(.25, .25), model='fixed', knobs=None, prime=False,
        tile=False):
    return Case(group, kind, state, n, M, scan_no, want, variant, ids, low,
        pb, model, knobs or {}, prime, tile)


def _key(c):
    """what decides the oracle's move (the id without group and knobs)"""
    out = f'{c.kind}-{c.state}{c.n}-M{c.M}-s{c.scan_no}'
    if c.variant != 'two':
        out += f'-{c.variant}'
    if c.ids:
        out += '-ids' + '.'.join(map(str, c.ids))
    if c.low:
        out += '-low'
    if c.pb != (.25, .25):
        out += f'-pb{c.pb[0]}.{c.pb[1]}'
    if c.model != 'fixed':
        out += f'-{c.model}'
    if c.prime:
        out += '-gauss'
    if c.want:
        out += f'-{c.want}'
    return out


def _case_id(c):
    knobs = ','.join(f'{k[5:]}={v}' for k, v in c.knobs.items())
    return f'{c.group}-{_key(c)}' + (f'-{knobs}' if knobs else '') \
        + ('-tile' if c.tile else '')


CASES = []
# A: kind x scan_no x outcome at M = 171
for _s in (0, 1, 3):
    CASES += [_c('A', 'split', 'lump', 66, 171, _s, 'accepted'),
        _c('A', 'split', 'clone', 66, 171, _s, 'one-side'),
        _c('A', 'split', 'clone', 6, 171, _s, 'declined'),
        _c('A', 'merge', 'halves', 66, 171, _s, 'accepted'),
        _c('A', 'merge', 'pair', 66, 171, _s, 'declined')]
# B: the thresholds of the scan's second half
for _M in (170, 171, 682, 683):
    CASES += [_c('B', 'split', 'lump', 66, _M, 2, 'accepted'),
        _c('B', 'merge', 'halves', 66, _M, 2, 'accepted'),
        _c('B', 'merge', 'pair', 40, _M, 2, 'declined')]
# C: the cells of the move on the view's edges, M on the mask words
for _M in (63, 64, 65):
    for _n in (3, 4, 5, 63, 64, 65, 66, 129, 130):
        CASES += [_c('C', 'split', 'lump', _n, _M, 1),
            _c('C', 'merge', 'halves', _n, _M, 1)]
# D: degenerate and tied launch states
CASES += [
    _c('D', 'split', 'lump', 3, 171, 2, 'one-side'),
    _c('D', 'split', 'clone', 64, 171, 2, 'one-side'),
    _c('D', 'split', 'lump', 65, 171, 2, 'one-side', variant='same'),
    _c('D', 'merge', 'halves', 65, 171, 2, variant='same'),
    _c('D', 'split', 'blank', 5, 171, 2),
    _c('D', 'split', 'blank', 4, 683, 1),
]
# E: hand-backs (the stream starts with a cached Gaussian)
CASES += [
    _c('E', 'split', 'lump', 2, 171, 2, 'early', prime=True),
    _c('E', 'merge', 'halves', 2, 171, 2, 'early', prime=True),
    _c('E', 'merge', 'halves', 3, 171, 2, 'late', prime=True),
    _c('E', 'merge', 'pair', 3, 683, 0, 'late', prime=True),
    _c('E', 'split', 'lump', 66, 171, 2, 'late', low=True, prime=True),
    _c('E', 'split', 'lump', 40, 683, 0, 'late', low=True, prime=True),
]
# F: state shapes
CASES += [
    _c('F', 'split', 'lump', 66, 171, 1, 'accepted', ids=(7, 2, 5)),
    _c('F', 'split', 'lump', 66, 171, 1, 'accepted', ids=(1, 0, 4)),
    _c('F', 'merge', 'halves', 66, 171, 1, 'accepted', ids=(9, 3, 0, 6)),
    _c('F', 'merge', 'halves', 66, 171, 1, 'accepted', ids=(3, 9, 6, 0)),
    _c('F', 'auto', 'all', 200, 171, 1, 'accepted'),
    _c('F', 'auto', 'lump', 66, 171, 1),
    _c('F', 'split', 'lump', 66, 171, 1, 'accepted', pb=(1, 1)),
    _c('F', 'merge', 'halves', 66, 171, 1, 'accepted', pb=(1, 1)),
    _c('F', 'merge', 'pair', 66, 171, 1, 'declined', pb=(1, 1)),
    _c('F', 'split', 'lump', 66, 171, 1, 'accepted', pb=(.75, 2.)),
    _c('F', 'merge', 'halves', 66, 171, 1, 'accepted', pb=(.75, 2.)),
    _c('F', 'split', 'lump', 66, 171, 1, 'accepted', model='learn'),
    _c('F', 'merge', 'halves', 66, 171, 1, 'accepted', model='learn'),
]
# G: the documented switches, one at a time, on a fused, walker-sized case
_SWITCHES = [{'BNPC_MH_SCREEN': '0'}, {'BNPC_MH_SCREEN': '2'},
    {'BNPC_MH_AHEAD': '0'}, {'BNPC_MH_AHEAD': '2'}, {'BNPC_MH_AHEAD': '3'},
    {'BNPC_DONE_WORDS': '0'}, {'BNPC_ZERO_COPY': '0'},
    {'BNPC_HOST_THREADS': '1'}, {'BNPC_LOOP_SHORTCUTS': '0'},
    {'BNPC_KW': '2'}, {'BNPC_MASK_COUNTS_MAX': '1'}]
for _k in _SWITCHES:
    CASES += [_c('G', 'split', 'lump', 66, 683, 2, 'accepted', knobs=_k),
        _c('G', 'merge', 'halves', 66, 683, 2, 'accepted', knobs=_k)]
# (BNPC_MH_AHEAD=2 posts a walker from 512 entries on)
CASES += [_c('G', 'split', 'lump', 66, 171, 2, 'accepted',
        knobs={'BNPC_MH_AHEAD': '2'}),
    _c('G', 'merge', 'halves', 66, 171, 2, 'accepted',
        knobs={'BNPC_MH_AHEAD': '3'})]
# J: a move beside an issued tile
for _M in (170, 171):
    CASES += [_c('J', 'split', 'lump', 66, _M, 2, 'accepted', tile=True),
        _c('J', 'merge', 'halves', 66, _M, 2, 'accepted', tile=True)]

# H: one context through a history of moves (M = 171): large, 3 cells, across
# a block edge, a hand-back, fused after unfused
HISTORY = [
    _c('H', 'split', 'lump', 130, 171, 2),
    _c('H', 'split', 'lump', 3, 171, 2, 'one-side'),
    _c('H', 'merge', 'halves', 65, 171, 2),
    _c('H', 'merge', 'halves', 3, 171, 2, 'late', prime=True),
    _c('H', 'split', 'lump', 66, 171, 2, 'accepted',
        knobs={'BNPC_MH_SCREEN': '0'}),
    _c('H', 'split', 'lump', 66, 171, 2, 'accepted'),
    _c('H', 'merge', 'pair', 40, 171, 2, 'declined'),
    _c('H', 'split', 'clone', 64, 171, 2, 'one-side'),
]

# key -> (seed, event): the first seed from 0 whose proposal picks the state's
# own cluster(s), that reaches the wanted event and keeps every decision off
# the knife edge (tests/test_move_routes.py::test_a_case_reaches_its_event)
SEEDS = {
    'split-lump66-M171-s0-accepted': (5, 'accepted'),
    'split-clone66-M171-s0-one-side': (7, 'one-side'),
    'split-clone6-M171-s0-declined': (219, 'declined'),
    'merge-halves66-M171-s0-accepted': (11, 'accepted'),
    'merge-pair66-M171-s0-declined': (2, 'declined'),
    'split-lump66-M171-s1-accepted': (5, 'accepted'),
    'split-clone66-M171-s1-one-side': (7, 'one-side'),
    'split-clone6-M171-s1-declined': (417, 'declined'),
    'merge-halves66-M171-s1-accepted': (11, 'accepted'),
    'merge-pair66-M171-s1-declined': (2, 'declined'),
    'split-lump66-M171-s3-accepted': (5, 'accepted'),
    'split-clone66-M171-s3-one-side': (5, 'one-side'),
    'split-clone6-M171-s3-declined': (417, 'declined'),
    'merge-halves66-M171-s3-accepted': (11, 'accepted'),
    'merge-pair66-M171-s3-declined': (2, 'declined'),
    'split-lump66-M170-s2-accepted': (5, 'accepted'),
    'merge-halves66-M170-s2-accepted': (16, 'accepted'),
    'merge-pair40-M170-s2-declined': (1, 'declined'),
    'split-lump66-M171-s2-accepted': (5, 'accepted'),
    'merge-halves66-M171-s2-accepted': (11, 'accepted'),
    'merge-pair40-M171-s2-declined': (1, 'declined'),
    'split-lump66-M682-s2-accepted': (5, 'accepted'),
    'merge-halves66-M682-s2-accepted': (22, 'accepted'),
    'merge-pair40-M682-s2-declined': (1, 'declined'),
    'split-lump66-M683-s2-accepted': (5, 'accepted'),
    'merge-halves66-M683-s2-accepted': (60, 'accepted'),
    'merge-pair40-M683-s2-declined': (1, 'declined'),
    'split-lump3-M63-s1': (9, 'one-side'),
    'merge-halves3-M63-s1': (0, 'late'),
    'split-lump4-M63-s1': (9, 'accepted'),
    'merge-halves4-M63-s1': (0, 'declined'),
    'split-lump5-M63-s1': (9, 'accepted'),
    'merge-halves5-M63-s1': (0, 'declined'),
    'split-lump63-M63-s1': (5, 'accepted'),
    'merge-halves63-M63-s1': (2, 'declined'),
    'split-lump64-M63-s1': (5, 'accepted'),
    'merge-halves64-M63-s1': (2, 'declined'),
    'split-lump65-M63-s1': (5, 'accepted'),
    'merge-halves65-M63-s1': (2, 'accepted'),
    'split-lump66-M63-s1': (5, 'accepted'),
    'merge-halves66-M63-s1': (2, 'accepted'),
    'split-lump129-M63-s1': (0, 'accepted'),
    'merge-halves129-M63-s1': (11, 'declined'),
    'split-lump130-M63-s1': (0, 'accepted'),
    'merge-halves130-M63-s1': (11, 'accepted'),
    'split-lump3-M64-s1': (9, 'one-side'),
    'merge-halves3-M64-s1': (0, 'late'),
    'split-lump4-M64-s1': (9, 'accepted'),
    'merge-halves4-M64-s1': (0, 'declined'),
    'split-lump5-M64-s1': (9, 'accepted'),
    'merge-halves5-M64-s1': (0, 'declined'),
    'split-lump63-M64-s1': (5, 'accepted'),
    'merge-halves63-M64-s1': (2, 'declined'),
    'split-lump64-M64-s1': (5, 'accepted'),
    'merge-halves64-M64-s1': (2, 'declined'),
    'split-lump65-M64-s1': (5, 'accepted'),
    'merge-halves65-M64-s1': (2, 'declined'),
    'split-lump66-M64-s1': (5, 'accepted'),
    'merge-halves66-M64-s1': (2, 'declined'),
    'split-lump129-M64-s1': (0, 'accepted'),
    'merge-halves129-M64-s1': (11, 'declined'),
    'split-lump130-M64-s1': (0, 'accepted'),
    'merge-halves130-M64-s1': (11, 'accepted'),
    'split-lump3-M65-s1': (9, 'one-side'),
    'merge-halves3-M65-s1': (0, 'late'),
    'split-lump4-M65-s1': (9, 'accepted'),
    'merge-halves4-M65-s1': (0, 'declined'),
    'split-lump5-M65-s1': (9, 'accepted'),
    'merge-halves5-M65-s1': (0, 'declined'),
    'split-lump63-M65-s1': (5, 'accepted'),
    'merge-halves63-M65-s1': (2, 'declined'),
    'split-lump64-M65-s1': (5, 'accepted'),
    'merge-halves64-M65-s1': (2, 'declined'),
    'split-lump65-M65-s1': (5, 'accepted'),
    'merge-halves65-M65-s1': (2, 'declined'),
    'split-lump66-M65-s1': (5, 'accepted'),
    'merge-halves66-M65-s1': (2, 'declined'),
    'split-lump129-M65-s1': (0, 'accepted'),
    'merge-halves129-M65-s1': (11, 'accepted'),
    'split-lump130-M65-s1': (0, 'accepted'),
    'merge-halves130-M65-s1': (11, 'accepted'),
    'split-lump3-M171-s2-one-side': (9, 'one-side'),
    'split-clone64-M171-s2-one-side': (7, 'one-side'),
    'split-lump65-M171-s2-same-one-side': (5, 'one-side'),
    'merge-halves65-M171-s2-same': (2, 'accepted'),
    'split-blank5-M171-s2': (252, 'one-side'),
    'split-blank4-M683-s1': (9, 'one-side'),
    'split-lump2-M171-s2-gauss-early': (1, 'early'),
    'merge-halves2-M171-s2-gauss-early': (0, 'early'),
    'merge-halves3-M171-s2-gauss-late': (0, 'late'),
    'merge-pair3-M683-s0-gauss-late': (0, 'late'),
    'split-lump66-M171-s2-low-gauss-late': (1, 'late'),
    'split-lump40-M683-s0-low-gauss-late': (1, 'late'),
    'split-lump66-M171-s1-ids7.2.5-accepted': (5, 'accepted'),
    'split-lump66-M171-s1-ids1.0.4-accepted': (5, 'accepted'),
    'merge-halves66-M171-s1-ids9.3.0.6-accepted': (11, 'accepted'),
    'merge-halves66-M171-s1-ids3.9.6.0-accepted': (11, 'accepted'),
    'auto-all200-M171-s1-accepted': (0, 'accepted'),
    'auto-lump66-M171-s1': (0, 'accepted'),
    'split-lump66-M171-s1-pb1.1-accepted': (5, 'accepted'),
    'merge-halves66-M171-s1-pb1.1-accepted': (2, 'accepted'),
    'merge-pair66-M171-s1-pb1.1-declined': (2, 'declined'),
    'split-lump66-M171-s1-pb0.75.2.0-accepted': (5, 'accepted'),
    'merge-halves66-M171-s1-pb0.75.2.0-accepted': (2, 'accepted'),
    'split-lump66-M171-s1-learn-accepted': (5, 'accepted'),
    'merge-halves66-M171-s1-learn-accepted': (11, 'accepted'),
    'split-lump130-M171-s2': (0, 'accepted'),
    'merge-halves65-M171-s2': (2, 'accepted'),
}


def _seed(c):
    return SEEDS[_key(c)][0]


def _event(c):
    return SEEDS[_key(c)][1]


def _plan(c, n=None, kind=None):
    return plan(kind or c.kind, c.scan_no, c.n if n is None else n, c.M,
        c.knobs, late=c.low, tile=c.tile)


# ---------------------------------------------------------- CPU: the guards
def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_plan_restates_the_sources():
    """The thresholds and the conditions `plan` restates, read out of the
    sources: a retuned threshold fails HERE, and the cases are then re-aimed
    at the routes their ids name."""
    ctx_h = _source('bnpc_ctx.h')
    moves = re.sub(r'\s+', ' ', _source('bnpc_moves.cpp'))
    sweeps = re.sub(r'\s+', ' ', _source('bnpc_sweeps.cpp'))
    mh = re.sub(r'\s+', ' ', _source('bnpc_mhbatch.cpp'))

    def define(text, name):
        return re.search(rf'#define {name}\s+(.+?)\s*(?://|$)', text,
            re.M).group(1)
    assert define(ctx_h, 'MH_SCREEN_MIN') == str(MH_SCREEN_MIN)
    assert define(ctx_h, 'MH_AHEAD_SCAN_MIN') == str(MH_AHEAD_SCAN_MIN)
    assert re.search(r'int mh_ahead = 1;', ctx_h)
    for line in ('if (n <= 2) return 0;', 'if (S - 1 <= 0) return 0;',
            'const int64_t n = (int64_t)s.cells.size(), S = n - 2;',
            'const bool ahead = st->scan_no > 0 || split;',
            'for (int it = 0; it < st->scan_no; it++) { mh.G = 3;',
            'if (ones != 0 && ones != S) accept = '
            'np_log1(k, mt_double(rng)) < A;'):
        assert line in moves, line
    for line in ('|| n < 3 || (mh->G != 3 && mh->G != 2)',
            'if (!mh->trans_prob) bnpc_rg_scan_order_hook(&at_order);',
            'bnpc_mh_ahead_scan(ctx, rng, S, mh->G, mh->M, mh->n_sd);'):
        assert line in sweeps, line
    for line in ('const bool fused = !a->trans_prob && c->tun.mh_screen '
            '&& a->G * M >= MH_SCREEN_MIN && !c->any_tile_pending();',
            'return bnpc_mh_batch_dev(c, k, rng, a, 1, status);',
            'return !(a->trans_prob || !c->tun.mh_screen || a->screen '
            '|| a->G * a->M < MH_SCREEN_MIN);',
            'if (mode == 0 || !c->tun.mh_screen || rows > MH_AHEAD_MAX_ROWS '
            '|| E < (mode >= 2 ? MH_SCREEN_MIN : min_entries) '
            '|| mh_pin_offsets((size_t)E, off) > c->tun.mh_pin_max '
            '|| c->any_tile_pending()) return 0;',
            '(void)bnpc_mh_ahead_begin(c, rng, &no_gauss, way, rows, M, '
            'n_sd, &posted, MH_AHEAD_SCAN_MIN);',
            '&& c->tun.mh_ahead != 3;'):
        assert line in mh, line
    # the sizes the cases are aimed at
    assert 3 * 170 < MH_SCREEN_MIN <= 3 * 171
    assert 3 * 682 < MH_AHEAD_SCAN_MIN <= 3 * 683
    assert int(define(ctx_h, 'MH_AHEAD_MAX_ROWS')) >= 3


def test_the_plan_at_the_edges():
    assert describe(plan('split', 2, 66, 170)) == 'unfused'
    assert describe(plan('split', 2, 66, 171)) == 'fused'
    assert describe(plan('merge', 2, 66, 682)) == 'fused'
    assert describe(plan('merge', 2, 66, 683)) == 'fused+walker'
    assert describe(plan('split', 2, 2, 683)) == 'early'
    assert describe(plan('merge', 2, 3, 171)) == 'fused+late'
    assert describe(plan('split', 2, 3, 171)) == 'fused'
    assert describe(plan('split', 2, 66, 171, late=True)) == 'fused+late'
    assert plan('split', 2, 66, 171) == Plan(None, True, False, 1026, 0, 0,
        0, 1)
    assert plan('merge', 3, 66, 683) == Plan(None, True, True, 6147, 3, 3, 9,
        1)
    assert plan('merge', 0, 66, 683) == Plan(None, True, True, 0, 0, 0, 0, 1)
    two = {'BNPC_MH_AHEAD': '2'}
    assert plan('split', 2, 66, 171, two)[4:7] == (2, 2, 6)
    assert plan('split', 2, 66, 170, two)[4:7] == (0, 0, 0)
    assert plan('split', 2, 66, 683, {'BNPC_MH_AHEAD': '3'})[4:7] == (2, 0, 0)
    assert plan('split', 2, 66, 683, {'BNPC_MH_AHEAD': '0'})[4:7] == (0, 0, 0)
    off = plan('split', 2, 66, 683, {'BNPC_MH_SCREEN': '0'})
    assert describe(off) == 'unfused' and off.screened == off.begun == 0
    assert plan('split', 2, 66, 683, {'BNPC_MH_SCREEN': '2'}) \
        == plan('split', 2, 66, 683)
    beside = plan('split', 2, 66, 171, tile=True)
    assert describe(beside) == 'unfused' and beside.screened == 1026
    assert plan('split', 2, 66, 170, tile=True).screened == 0
    assert plan('split', 2, 66, 683, tile=True).begun == 0


def test_the_cases_cover_the_routes_between_them():
    """every kind of route and event is named by some case"""
    seen = {(c.kind, _event(c), describe(_plan(c, kind=c.kind)))
        for c in CASES + HISTORY if c.kind != 'auto'}
    for want in (('split', 'accepted', 'unfused'),
            ('split', 'accepted', 'fused'),
            ('split', 'accepted', 'fused+walker'),
            ('merge', 'accepted', 'unfused'), ('merge', 'accepted', 'fused'),
            ('merge', 'accepted', 'fused+walker'),
            ('merge', 'declined', 'fused'), ('split', 'declined', 'fused'),
            ('split', 'one-side', 'fused'), ('split', 'early', 'early'),
            ('merge', 'early', 'early'), ('merge', 'late', 'fused+late'),
            ('merge', 'late', 'fused+walker+late'),
            ('split', 'late', 'fused+late'),
            ('split', 'late', 'fused+walker+late')):
        assert want in seen, want
    by_scan = {(c.kind, c.scan_no, _event(c)) for c in CASES
        if c.group == 'A'}
    assert by_scan >= {(k, s, e) for s in (0, 1, 3) for k, e in (
        ('split', 'accepted'), ('split', 'one-side'), ('split', 'declined'),
        ('merge', 'accepted'), ('merge', 'declined'))}
    # S = 64 sits exactly on a block (n = 66), S = 1 and S = 128 too
    assert {c.n for c in CASES if c.group == 'C'} \
        == {3, 4, 5, 63, 64, 65, 66, 129, 130}
    assert len(HISTORY) == 8 and len({c.M for c in HISTORY}) == 1


# ------------------------------------------------- the oracle, made to record
class _Recording:
    """Mixed in front of an oracle class: the four terms of A, their sum, the
    cells of the move, whether the split's launch state ended on one side,
    log(u) of the acceptance draw (None: none was drawn)."""

    def run_rg_nc(self, move, cells, size_data, scan_no):
        self.rec = {'cells': np.array(cells), 'terms': [], 'log_u': None,
            'one_side': None, 'move': move, 'launch': None}
        return super().run_rg_nc(move, cells, size_data, scan_no)

    def _rg_init_split(self, cells, random=False):
        super()._rg_init_split(cells, random)
        self.rec['launch'] = np.array(self.rg_assignment, dtype=np.int64)

    def _term(self, value):
        self.rec['terms'].append(float(np.asarray(value).reshape(-1)[0]))
        return value

    def _get_trans_prob_ratio_split(self, cells):
        return self._term(super()._get_trans_prob_ratio_split(cells))

    def _get_trans_prob_ratio_merge(self, cells):
        return self._term(super()._get_trans_prob_ratio_merge(cells))

    def _get_lprior_ratio_split(self, cells):
        return self._term(super()._get_lprior_ratio_split(cells))

    def _get_lprior_ratio_merge(self, cells):
        return self._term(super()._get_lprior_ratio_merge(cells))

    def _get_ll_ratio(self, cells, move):
        return self._term(super()._get_ll_ratio(cells, move))

    def _get_ltrans_prob_size_ratio_split(self, ltrans_prob_size,
            cluster_size):
        return self._term(super()._get_ltrans_prob_size_ratio_split(
            ltrans_prob_size, cluster_size))

    def _get_ltrans_prob_size_ratio_merge(self, trans_prob_size):
        return self._term(super()._get_ltrans_prob_size_ratio_merge(
            trans_prob_size))

    def _with_the_uniform(self, call):
        real = np.random.random

        def random(*args):
            u = real(*args)
            if not args:        # (the parameter updates draw random(M))
                self.rec['log_u'] = float(np.log(u))
            return u
        np.random.random = random
        try:
            return call()
        finally:
            np.random.random = real

    def _do_rg_split_MH(self, cells, size_data):
        out = self._with_the_uniform(
            lambda: super(_Recording, self)._do_rg_split_MH(cells, size_data))
        self.rec['one_side'] = bool(np.unique(self.rg_assignment).size == 1)
        return out

    def _do_rg_merge_MH(self, cells, size_data):
        return self._with_the_uniform(
            lambda: super(_Recording, self)._do_rg_merge_MH(cells, size_data))


class _OracleFixed(_Recording, O.CRP):
    pass


class _OracleLearn(_Recording, O.CRP_errors_learning):
    pass


def _model(mod, c, ctx=None):
    """A model in the case's state (nothing is drawn, nothing runs on the
    device); `ctx`: the device context it is to use."""
    data = _data(c.M, c.variant)
    learn = c.model == 'learn'
    if mod is O:
        cls = _OracleLearn if learn else _OracleFixed
    else:
        cls = P.CRP_errors_learning if learn else P.CRP
    if learn:
        m = cls(data, DP_alpha=[-1, -1], param_beta=list(c.pb), FP_mean=0.01,
            FP_sd=0.01, FN_mean=0.2, FN_sd=0.1)
    else:
        m = cls(data, DP_alpha=[-1, -1], param_beta=list(c.pb), FN_error=0.1,
            FP_error=0.001)
    st = _state(c.state, c.n, c.M, c.variant, c.ids, c.low)
    m.assignment = st.assignment.copy()
    m.cells_per_cluster = dict(st.items)
    m.parameters = st.parameters.copy()
    m.init_DP_prior()
    if ctx is not None:
        m._ctx = ctx
    return m


def _start(c, seed=None):
    """the stream a case's move starts from"""
    np.random.seed(_seed(c) if seed is None else seed)
    if c.prime:
        np.random.standard_normal()     # (leaves a cached Gaussian)
        assert np.random.get_state()[3] == 1


def _do(m, c):
    if c.kind == 'split':
        return m.do_split_move(c.scan_no), 0
    if c.kind == 'merge':
        return m.do_merge_move(c.scan_no), 1
    res, kind = m.update_assignments_split_merge([.5, .5], c.scan_no)
    return res, int(kind)


Snap = collections.namedtuple('Snap', 'res kind assignment items rows peek')


def _snap(m, res, kind):
    ids = list(m.cells_per_cluster)
    return Snap([int(x) for x in res], kind, m.assignment.copy(),
        [(int(a), int(b)) for a, b in m.cells_per_cluster.items()],
        np.ascontiguousarray(m.parameters[ids]).view(np.int32).copy(),
        np.random.random())


def _same_snap(got, want, what):
    assert got.res == want.res and got.kind == want.kind, \
        (what, got.res, want.res)
    assert np.array_equal(got.assignment, want.assignment), what
    assert got.items == want.items, (what, got.items, want.items)
    assert got.rows.shape == want.rows.shape \
        and np.array_equal(got.rows, want.rows), \
        (what, np.argwhere(got.rows != want.rows)[:4])
    assert got.peek == want.peek, (what, 'the position of the stream')


def _oracle_run(c, seed):
    """(Snap, the recording) of the oracle's move from `seed`"""
    m = _model(O, c)
    m.rec = None
    _start(c, seed)
    res, kind = _do(m, c)
    return _snap(m, res, kind), m.rec


def _classify(c, snap, rec):
    """the event a move reached, from the oracle alone"""
    n = len(rec['cells'])
    if n <= 2:
        return 'early'
    if c.low or (rec['move'] == 'merge' and n == 3):
        return 'late'
    if snap.res == [1, 0]:
        return 'accepted'
    if rec['one_side']:
        return 'one-side'
    return 'declined'


def _on_target(c, rec):
    """the proposal picked the state's own cluster(s)"""
    if c.kind == 'auto' and c.state != 'all':
        return True                     # (whichever move the kind draw gives)
    st = _state(c.state, c.n, c.M, c.variant, c.ids, c.low)
    picked = set(st.assignment[rec['cells']].tolist())
    return picked == set(st.target) and len(rec['cells']) == c.n


def _off_the_edge(rec):
    """|log(u) - A| > 1e-6 of the largest term (no draw: nothing to decide)"""
    terms = rec['terms']
    if rec['log_u'] is None or len(terms) != 4:
        return True
    A = terms[0] + terms[1] + terms[2] + terms[3]
    if not np.isfinite(A):
        return True
    return abs(rec['log_u'] - A) > EDGE_A * max(abs(t) for t in terms)


def _oracle(c):
    key = ('oracle', _key(c))
    if key not in _memo:
        _memo[key] = _oracle_run(c, _seed(c))
    return _memo[key]


def find_seed(c, upto=2000):
    """The first seed that aims the case (used when a case is added or
    re-aimed; the table SEEDS holds the results)."""
    for seed in range(upto):
        snap, rec = _oracle_run(c, seed)
        if rec is None or not _on_target(c, rec):
            continue
        if c.state == 'blank' and 0 not in (rec['cells'][0],
                rec['cells'][-1]):
            continue
        event = _classify(c, snap, rec)
        if c.want and event != c.want:
            continue
        if not _off_the_edge(rec):
            continue
        return seed, event
    raise LookupError(_key(c))


_MOVE_CASES = list({_key(c): c for c in CASES + HISTORY}.values())


def test_the_seed_search_gives_the_tables_seeds():
    """find_seed, on the cases it answers at once"""
    quick = [c for c in _MOVE_CASES if _seed(c) <= 1 and c.M < 100]
    assert len(quick) >= 6
    for c in quick:
        assert find_seed(c) == SEEDS[_key(c)], _key(c)


@pytest.mark.parametrize('c', _MOVE_CASES, ids=_key)
def test_a_case_reaches_its_event(c):
    """With the oracle alone: the seed's proposal picks the clusters the
    state was built around, the move reaches the event in the case's id, and
    its acceptance draw is off the knife edge."""
    snap, rec = _oracle(c)
    assert rec is not None and _on_target(c, rec)
    event = _classify(c, snap, rec)
    assert event == _event(c) and (not c.want or event == c.want), event
    assert _off_the_edge(rec), (rec['log_u'], rec['terms'])
    if c.state == 'blank':
        assert 0 in (rec['cells'][0], rec['cells'][-1])
        assert np.isnan(_data(c.M)[0]).all()
    if event == 'one-side':
        assert rec['log_u'] is None
    if event in ('accepted', 'declined'):
        assert rec['log_u'] is not None and len(rec['terms']) == 4
    if c.kind == 'auto' and c.state == 'all':
        assert snap.kind == 0 and len(_state('all', c.n, c.M).items) == 1
    if c.ids and event == 'accepted' and c.kind == 'split':
        # the smallest unused id
        new = set(dict(snap.items)) - set(c.ids)
        assert new == {min(set(range(N_CELLS)) - set(c.ids))}
    if c.n == 3 and c.kind == 'split':
        assert event == 'one-side'      # S = 1: always
    if c.variant == 'same':
        # identical rows: every launch tie goes to anchor i
        assert rec['launch'].size == c.n - 2 and not rec['launch'].any()
        d = _data(c.M, 'same')
        assert (np.isnan(d) == np.isnan(d[0])).all() \
            and np.array_equal(np.nan_to_num(d), np.nan_to_num(
                np.repeat(d[:1], N_CELLS, axis=0)))


@pytest.mark.parametrize('c', [c for c in _MOVE_CASES if c.kind != 'auto'],
    ids=_key)
def test_the_proposal_alone_gives_the_oracles_cells(c):
    """bnpc_move_propose - the proposal bnpc_sm_move starts with - from the
    case's stream: the cells of the move in the oracle's order (host only)."""
    table = P._native_kernels()
    if table is None:
        pytest.skip('native kernel table not available')
    _, rec = _oracle(c)
    st = _state(c.state, c.n, c.M, c.variant, c.ids, c.low)
    _start(c)
    got = _lib.move_propose(table, 0 if c.kind == 'split' else 1,
        np.array([i for i, _ in st.items]), np.array([s for _, s in st.items]),
        st.assignment.copy())
    assert got is not None and np.array_equal(got[0], rec['cells'])


# --------------------------------------------- reference 2: one scan in NumPy
ScanCase = collections.namedtuple('ScanCase', 'G n M bad knobs scored')
# G = 3 unscored (an intermediate scan), G = 2 scored (a split's last scan)
SCAN_CASES = [ScanCase(G, n, M, None, {}, G == 2) for G in (3, 2)
    for n in (3, 66, 130) for M in (170, 171, 683)]
# status 1: an `old` entry at TMIN / 4 in each of the three rows, unfused and
# fused
SCAN_CASES += [ScanCase(3, 66, M, row, {}, False) for M in (170, 171)
    for row in (0, 1, 2)]
# G * M ON the threshold: two unscored rows of 256 are 512 entries (three rows
# never are).  Fused or not, the batch is screened; only a fused scan adopts
# a walker's rows, and BNPC_MH_AHEAD=2 posts one from 512 entries on.
_AHEAD2 = {'BNPC_MH_AHEAD': '2'}
SCAN_CASES += [ScanCase(2, 66, 256, None, _AHEAD2, False),
    ScanCase(2, 66, 255, None, _AHEAD2, False),
    ScanCase(2, 66, 256, None, {}, False),
    ScanCase(3, 66, 171, None, _AHEAD2, False),
    ScanCase(3, 66, 171, None, {'BNPC_MH_AHEAD': '3'}, False),
    ScanCase(3, 66, 683, None, {'BNPC_MH_AHEAD': '0'}, False)]


def _scan_id(s):
    knobs = ','.join(f'{k[5:]}={v}' for k, v in s.knobs.items())
    return f'G{s.G}-n{s.n}-M{s.M}' + ('-scored' if s.scored else '') \
        + (f'-bad{s.bad}' if s.bad is not None else '') \
        + (f'-{knobs}' if knobs else '')


ScanPlan = collections.namedtuple('ScanPlan', 'fused screened begun taken')


def scan_plan(G, M, scored, knobs=None):
    """bnpc_rg_scan_step_with and bnpc_rg_counts_and_batch for one scan"""
    knobs = knobs or {}
    screen = int(knobs.get('BNPC_MH_SCREEN', 1)) != 0
    ahead = int(knobs.get('BNPC_MH_AHEAD', 1))
    E = G * M
    fused = not scored and screen and E >= MH_SCREEN_MIN
    walker = not scored and ahead != 0 and screen \
        and E >= (MH_SCREEN_MIN if ahead >= 2 else MH_AHEAD_SCAN_MIN)
    # (a walker's rows are adopted by the fused second half alone)
    taken = 1 if walker and fused and ahead in (1, 2) else 0
    return ScanPlan(fused, E if fused else 0, int(walker), taken)


def _scan_seed(s):
    return 40 + s.n + s.M + 7 * s.G


Scan = collections.namedtuple('Scan', 'cells rg0 rows rg prob margins n1 n0 '
    'draws new probs position')
SCAN_PAR = dict(pb=(.25, .25), FP=0.001, FN=0.1, sd=(0.1, 0.25, 0.5))


def _scan_inputs(s):
    rng = np.random.RandomState(s.n * 1000 + s.M)
    cells = rng.permutation(N_CELLS)[:s.n].astype(np.int64)
    rg0 = rng.randint(0, 2, s.n - 2).astype(np.int64)
    data = _data(s.M)
    labels = np.concatenate([[0], rg0, [1]])
    rows = []
    for g in (0, 1, None):
        sub = data[cells] if g is None else data[cells[labels == g]]
        rows.append(np.clip(rng.beta(.25 + (sub == 1).sum(0),
            .25 + (sub == 0).sum(0)), O.TMIN, O.TMAX))
    rows = np.array(rows[:s.G], dtype=np.float32)
    if s.bad is not None:
        rows[s.bad, 11] = np.float32(O.TMIN / 4)
    return cells, rg0, rows


def _margins(ll, DP_a, rg, seed):
    """the picks of reference_rg_scan again, with |c0 / c1 - u| of each"""
    rg = rg.copy()
    S = ll.shape[0]
    np.random.seed(seed)
    out = np.zeros(S)
    for cell in np.random.permutation(S):
        rg[cell] = -1
        n_j = O.seqsum(rg) + 2
        n_i = S + 2 - n_j - 1
        p = np.exp(O.CRP._normalize_log(ll[cell]
            + O.CRP.log_CRP_prior([n_i, n_j], S + 2, DP_a)))
        u = np.random.random()
        out[cell] = abs(p[0] / (p[0] + p[1]) - u)
        rg[cell] = 0 if p[0] / (p[0] + p[1]) > u else 1
    return rg, out


def _scan_reference(s):
    key = ('scan', s.G, s.n, s.M, s.bad, s.scored)
    if key in _memo:
        return _memo[key]
    cells, rg0, rows = _scan_inputs(s)
    data = _data(s.M)
    o = O.CRP(data, DP_alpha=[-1, -1], param_beta=list(SCAN_PAR['pb']),
        FN_error=SCAN_PAR['FN'], FP_error=SCAN_PAR['FP'])
    ll = o._rg_get_ll(cells[1:-1], rows[:2])
    seed = _scan_seed(s)
    np.random.seed(seed)
    rg, prob = reference_rg_scan(ll, o.DP_a, rg0, True)
    labels = np.concatenate([[0], rg, [1]])
    n1 = np.stack([(data[cells][labels == g] == 1).sum(0) for g in (0, 1)])
    n0 = np.stack([(data[cells][labels == g] == 0).sum(0) for g in (0, 1)])
    if s.G == 3:
        n1 = np.vstack([n1, n1.sum(0, keepdims=True)])
        n0 = np.vstack([n0, n0.sum(0, keepdims=True)])
    n1, n0 = n1.astype(np.int32), n0.astype(np.int32)
    draws = _lib.mh_draws(s.G, s.M, 3)      # from behind the scan
    position = np.random.random()
    new = probs = None
    if s.bad is None:
        probe = P.CRP.__new__(P.CRP)
        probe.param_proposal_sd = np.array(SCAN_PAR['sd'])
        probe.p, probe.q = SCAN_PAR['pb']
        probe.beta_prior_uniform = False
        probe.FP, probe.FN = SCAN_PAR['FP'], SCAN_PAR['FN']
        scored = s.scored
        new, A, _, _ = probe._mh_math(rows, probe.param_proposal_sd[draws[0]],
            draws[1], draws[2], n1, n0, scored, None)
        probs = np.cumsum(A, axis=1)[:, -1] if scored else None
    rg_again, margins = _margins(ll, o.DP_a, rg0, seed)
    assert np.array_equal(rg_again, rg)
    _memo[key] = Scan(cells, rg0, rows, rg, prob, margins, n1, n0, draws, new,
        probs, position)
    return _memo[key]


@pytest.mark.parametrize('s', SCAN_CASES, ids=_scan_id)
def test_a_scan_case_is_off_the_knife_edge(s):
    """reference 2 alone: every pick of the NumPy scan has |c0 / c1 - u| >
    1e-9, both sides are populated afterwards where the view allows, and the
    batch behind a status-1 row is handed back by the host library too."""
    ref = _scan_reference(s)
    assert ref.margins.shape == (s.n - 2,) and (ref.margins > EDGE_PICK).all()
    if s.n > 3:
        assert 0 < ref.rg.sum() < s.n - 2
    pl = scan_plan(s.G, s.M, s.scored, s.knobs)
    assert pl.fused == (not s.scored and s.M not in (170, 255))
    if s.knobs.get('BNPC_MH_AHEAD') == '2':
        assert pl[2:] == ((1, 1) if pl.fused else (0, 0))
    assert scan_plan(2, 256, False, _AHEAD2) == ScanPlan(True, 512, 1, 1) \
        and 2 * 256 == MH_SCREEN_MIN
    assert scan_plan(3, 683, False) == ScanPlan(True, 2049, 1, 1)
    assert scan_plan(3, 682, False) == ScanPlan(True, 2046, 0, 0)
    assert scan_plan(3, 683, False, {'BNPC_MH_AHEAD': '3'})[2:] == (1, 0)
    if s.bad is not None:
        table = P._native_kernels()
        if table is None:
            pytest.skip('native kernel table not available')
        np.random.seed(1)
        status = _lib.mh_batch(table, ref.rows, ref.n1, ref.n0,
            np.array(SCAN_PAR['sd']), O.TMIN, O.TMAX, SCAN_PAR['FP'],
            SCAN_PAR['FN'], .25, .25, False, False)[0]
        assert status == 1


# ------------------------------------------------------------ the device side
class _Dev:
    """one context per data set, made on first use"""

    def __init__(self):
        self.ctxs = {}

    def ctx(self, M, variant='two'):
        if (M, variant) not in self.ctxs:
            self.ctxs[M, variant] = _lib.Context(data=_data(M, variant))
        return self.ctxs[M, variant]

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


def _stream():
    kind, key, pos, has_gauss, cached = np.random.get_state()
    return key.copy(), int(pos), int(has_gauss), float(cached)


def _same_stream(a, b):
    return np.array_equal(a[0], b[0]) and a[1:] == b[1:]


Dev = collections.namedtuple('Dev', 'snap done screened ahead native')


def _device_move(c, ctx, monkeypatch):
    """The case's move through P.CRP on `ctx`, a spy on _lib.sm_move beside
    it (what it returned - None: handed back -, the stream and the model
    around the call).  The caller has set the knobs."""
    m = _model(P, c, ctx)
    calls = []
    real = _lib.sm_move

    def counters():
        return (ctx.mh_screen_stats()[0],) + tuple(ctx.mh_ahead_stats())

    def spy(*args, **kw):
        before = (_stream(), args[6].copy(), args[7].copy(), counters())
        out = real(*args, **kw)
        calls.append((out, before, (_stream(), args[6].copy(),
            args[7].copy(), counters())))
        return out
    try:
        with monkeypatch.context() as mp:
            mp.setattr(_lib, 'sm_move', spy)
            _start(c)
            res, kind = _do(m, c)
        snap = _snap(m, res, kind)
    finally:
        m._ctx = None           # (the context is the caller's)
    assert len(calls) == 1, 'the move did not go to bnpc_sm_move'
    done, before, after = calls[0]
    if done is None:
        assert _same_stream(before[0], after[0]), \
            'a handed-back move moved the stream or the cached Gaussian'
        assert np.array_equal(before[1], after[1]) \
            and np.array_equal(before[2].view(np.int32),
                after[2].view(np.int32)), 'a handed-back move wrote'
    # (the counters around the native call alone: the walk behind a
    # hand-back runs scans of its own)
    grown = tuple(a - b for a, b in zip(after[3], before[3]))
    return Dev(snap, done, grown[0], grown[1:],
        getattr(m, '_native_moves', 0))


def _check_move(c, got):
    """a device move against the oracle and the plan"""
    want, rec = _oracle(c)
    what = _case_id(c)
    _same_snap(got.snap, want, what)
    n = len(rec['cells'])
    pl = _plan(c, n, 'merge' if want.kind else 'split')
    assert describe(pl) == describe(_plan(c, kind='merge' if want.kind
        else 'split')), what
    assert got.native == pl.native, (what, 'native moves', got.native)
    assert got.screened == pl.screened, (what, describe(pl), 'screened grew '
        f'by {got.screened}, the plan says {pl.screened}')
    assert got.ahead == (pl.begun, pl.taken, pl.rows), (what, describe(pl),
        got.ahead)
    if pl.handback:
        assert got.done is None, what
        return
    assert got.done is not None, (what, 'handed back')
    accepted, cl_i, cl_j, moved, n_cells, log_A = got.done
    assert n_cells == n and accepted == (want.res == [1, 0]), what
    terms = rec['terms']
    assert len(terms) == 4
    A = terms[0] + terms[1] + terms[2] + terms[3]
    bound = RTOL * max(abs(t) for t in terms)
    print(f'{what}: log_A {log_A!r} oracle {A!r} terms {terms} bound {bound}')
    assert abs(log_A - A) <= bound, (what, log_A, A, terms)


_DEVICE_CASES = [c for c in CASES if c.group not in 'EJ']


@pytest.mark.gpu
@pytest.mark.parametrize('c', _DEVICE_CASES, ids=_case_id)
def test_a_move_equals_the_oracles(c, dev, monkeypatch):
    """groups A - D, F, G: see the module docstring and the case's id"""
    ctx = dev.ctx(c.M, c.variant)
    with _knobs(monkeypatch, ctx, c.knobs):
        _check_move(c, _device_move(c, ctx, monkeypatch))


_GOOD_BEHIND = _c('E', 'split', 'lump', 66, 171, 2, 'accepted')


@pytest.mark.gpu
@pytest.mark.parametrize('c', [c for c in CASES if c.group == 'E'],
    ids=_case_id)
def test_a_handed_back_move_leaves_no_trace(c, dev, monkeypatch):
    """Group E: _lib.sm_move returns None with the stream, the cached
    Gaussian, the assignment and the parameters where they were (asserted
    around the call), the binding's walk that follows equals the oracle's
    move - and its own walk without the native call (BNPC_NATIVE_MOVES=0)
    ends at the same stream position -, and a good move behind it on the same
    context is right."""
    ctx = dev.ctx(c.M, c.variant)
    with _knobs(monkeypatch, ctx, c.knobs):
        got = _device_move(c, ctx, monkeypatch)
        _check_move(c, got)
        assert got.done is None
    with _knobs(monkeypatch, ctx, {'BNPC_NATIVE_MOVES': '0'}):
        m = _model(P, c, ctx)
        try:
            _start(c)
            res, kind = _do(m, c)
            walk = _snap(m, res, kind)
        finally:
            m._ctx = None
        assert getattr(m, '_native_moves', 0) == 0
        _same_snap(walk, got.snap, 'the step-by-step walk')
    behind = _GOOD_BEHIND._replace(M=c.M)
    with _knobs(monkeypatch, ctx, {}):
        _check_move(behind, _device_move(behind, ctx, monkeypatch))


@pytest.mark.gpu
def test_one_context_through_a_history_of_moves(monkeypatch):
    """Group H: eight moves on one context - large, 3 cells, across a block
    edge, a hand-back, fused after unfused - take the pinned block and the
    view through growth and reuse; each equals the same move on a fresh
    context and the oracle's."""
    M = HISTORY[0].M
    ctx = _lib.Context(data=_data(M))
    try:
        for c in HISTORY:
            with _knobs(monkeypatch, ctx, c.knobs):
                used = _device_move(c, ctx, monkeypatch)
            _check_move(c, used)
            fresh_ctx = _lib.Context(data=_data(M))
            try:
                with _knobs(monkeypatch, fresh_ctx, c.knobs):
                    fresh = _device_move(c, fresh_ctx, monkeypatch)
            finally:
                fresh_ctx.close()
            _check_move(c, fresh)
            _same_snap(used.snap, fresh.snap, _case_id(c))
            assert (used.done is None) == (fresh.done is None)
            if used.done is not None:
                assert used.done == fresh.done, _case_id(c)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_a_direct_call_on_a_row_strided_slice(dev, monkeypatch):
    """Group F: _lib.sm_move with `parameters` a row-strided slice of a wider
    array (param_stride > M): the oracle's move, and the columns beyond M
    untouched."""
    table = P._native_kernels()
    if table is None:
        pytest.skip('native kernel table not available')
    for c in (_c('F', 'split', 'lump', 66, 171, 1, 'accepted'),
            _c('F', 'merge', 'halves', 66, 171, 1, 'accepted')):
        want, rec = _oracle(c)
        ctx = dev.ctx(c.M)
        m = _model(P, c)
        wide = np.full((N_CELLS, c.M + 13), np.float32(-3.5), np.float32)
        wide[:, :c.M] = m.parameters
        params = wide[:, :c.M]
        assert params.strides[0] // 4 == c.M + 13
        ids = np.array(list(m.cells_per_cluster), dtype=np.int64)
        sizes = np.array(list(m.cells_per_cluster.values()), dtype=np.int64)
        with _knobs(monkeypatch, ctx, {}):
            _start(c)
            done = _lib.sm_move(ctx, table, 0 if c.kind == 'split' else 1,
                c.scan_no, ids, sizes, m.assignment, params, m.DP_a,
                m.param_proposal_sd, m.FP, m.FN, m.p, m.q,
                m.beta_prior_uniform, P.TMIN, P.TMAX, m._beta_mix_const[0],
                P.VIEW_MOVE)
            peek = np.random.random()
        assert done is not None and done[0] and done[4] == len(rec['cells'])
        assert (wide[:, c.M:] == np.float32(-3.5)).all()
        assert np.array_equal(m.assignment, want.assignment)
        live = [i for i, _ in want.items]
        assert np.array_equal(np.ascontiguousarray(params[live])
            .view(np.int32), want.rows)
        assert peek == want.peek
        if c.kind == 'split':
            assert dict(want.items)[done[2]] == done[3]


# ----------------------------------------------------------- I: one scan alone
@pytest.mark.gpu
@pytest.mark.parametrize('s', SCAN_CASES, ids=_scan_id)
def test_one_scan_alone(s, dev, monkeypatch):
    """Group I: _lib.rg_scan_step against reference 2 - rg_assignment, the
    n1 / n0 rows (the third the sum of the first two), the new theta bits,
    the scan and batch log-probabilities (1e-9 against the reference), the
    stream position.  Status 1: the scan and the counts are done and right,
    the three draw arrays come back whole, the stream stands behind all of
    them."""
    table = P._native_kernels()
    if table is None:
        pytest.skip('native kernel table not available')
    ref = _scan_reference(s)
    ctx = dev.ctx(s.M)
    scored = s.scored
    pl = scan_plan(s.G, s.M, scored, s.knobs)
    dp = O.CRP(_data(s.M), DP_alpha=[-1, -1]).DP_a
    with _knobs(monkeypatch, ctx, s.knobs):
        ctx.view_set(P.VIEW_MOVE, ref.cells)
        rg = ref.rg0.copy()
        _, sd_idx, U, u, _ = _lib._mh_buffers(s.G, s.M)
        sd_idx[...] = -1
        U[...] = np.nan
        u[...] = np.nan
        screened = ctx.mh_screen_stats()[0]
        ahead = ctx.mh_ahead_stats()
        np.random.seed(_scan_seed(s))
        status, new, n1, n0, draws, scan_prob, probs = _lib.rg_scan_step(
            ctx, table, P.VIEW_MOVE, s.n, rg, dp, ref.rows,
            np.array(SCAN_PAR['sd']), P.TMIN, P.TMAX, SCAN_PAR['FP'],
            SCAN_PAR['FN'], SCAN_PAR['pb'][0], SCAN_PAR['pb'][1], False,
            trans_prob=scored)
        draws = tuple(x.copy() for x in draws)
        position = np.random.random()
        grown = ctx.mh_screen_stats()[0] - screened
        ahead = tuple(a - b for a, b in zip(ctx.mh_ahead_stats(), ahead))
    assert status == (0 if s.bad is None else 1)
    assert np.array_equal(rg, ref.rg)
    assert n1.dtype == ref.n1.dtype and np.array_equal(n1, ref.n1)
    assert np.array_equal(n0, ref.n0)
    if s.G == 3:
        assert np.array_equal(n1[2], n1[0] + n1[1]) \
            and np.array_equal(n0[2], n0[0] + n0[1])
    assert position == ref.position, 'stream position'
    # (unfused, the batch behind the counts is still screened from 512 on)
    assert grown == (s.G * s.M if not scored and s.G * s.M >= MH_SCREEN_MIN
        else 0)
    assert ahead == (pl.begun, pl.taken, s.G * pl.taken), (ahead, pl)
    if status == 0:
        assert np.array_equal(new.view(np.int32), ref.new.view(np.int32)), \
            np.argwhere(new.view(np.int32) != ref.new.view(np.int32))[:4]
    if status != 0 or s.G * s.M < MH_SCREEN_MIN or scored:
        # (a screened batch that ends well keeps its draws in the pinned block)
        for g, w, name in zip(draws, ref.draws, ('sd_idx', 'U', 'u')):
            assert g.dtype == w.dtype and np.array_equal(g, w), name
    if scored:
        print(f'{_scan_id(s)}: scan {scan_prob!r} reference {ref.prob!r}, '
            f'batch {probs} reference {ref.probs}')
        assert abs(scan_prob - ref.prob) <= RTOL * abs(ref.prob)
        np.testing.assert_allclose(probs, ref.probs, rtol=RTOL, atol=0)
    else:
        assert scan_prob == 0.0


# --------------------------------------------- J: a move beside an issued tile
@pytest.mark.gpu
@pytest.mark.parametrize('c', [c for c in CASES if c.group == 'J'],
    ids=_case_id)
def test_a_move_beside_an_issued_tile(c, monkeypatch):
    """Group J: a tile issued on another view slot and left uncollected; the
    move runs unfused beside it (the plan with tile=True), equals the
    oracle's, and the tile collected afterwards is intact."""
    rng = np.random.RandomState(c.M)
    theta = np.clip(rng.uniform(size=(40, c.M)), 1e-5, 1 - 1e-5) \
        .astype(np.float32)
    ctx = _lib.Context(data=_data(c.M))
    try:
        ctx.theta_put(0, theta)
        rows = rng.permutation(40)[:23]
        cells = rng.permutation(N_CELLS)[:150]
        ctx.view_set(3, cells)
        want = ctx.ll_rows_pinned(3, rows, 0.01, 0.2, rows.size).copy()
        with _knobs(monkeypatch, ctx, c.knobs):
            ctx.ll_rows_issue(3, rows, 0.01, 0.2, rows.size, 0)
            got = _device_move(c, ctx, monkeypatch)
            tile = ctx.ll_rows_wait(0, cells.size, rows.size).copy()
        assert np.array_equal(tile, want), 'the tile beside the move'
        _check_move(c, got)
        assert describe(_plan(c)) == 'unfused'
    finally:
        ctx.close()
