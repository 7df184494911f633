"""The tile pipeline of a tiled Gibbs sweep at every slot, growth and lane
edge: bnpc_view_set_slot, bnpc_theta_put, bnpc_ll_rows_issue[_hint],
bnpc_ll_rows_wait[_hint], bnpc_ll_rows_pinned and the side lane (SideLane,
ensure_lanes) - three streams, four slots, two device result buffers chosen by
the parity of the issue count, five pinned buffers per slot, eight buffers
that grow by free-and-reallocate.

The scenarios are DATA: lists of steps (put, set a slot's view, issue - hinted
or not -, wait, a call in between, an expected refusal) that one runner plays
on a context.  Every tile of a scenario has its own cells, rows, K, ld and
error rates, and the store rows it does not select hold other valid
parameters: a result from the wrong slot or device buffer, or made with
another tile's rows or priors, or with row k instead of row rows[k], is finite
and wrong.

  * CPU half (not marked gpu): every scenario runs through
    tests/fake_device.FakeContext, where the matrices must EQUAL the
    strict-order reference (oracle.seqsum.table_sums over NumPy tables of the
    store as of the issue) and the hints must pass _check_wide_hints; and every
    scenario asserts from its own inputs alone that it reaches the edge it
    names (bytes against the modelled capacity of the same parity, n against
    the room of bnpc_view_set_slot, K against the K before, the parity each
    slot sees).
  * device half (-m gpu): the same scenarios on a context of their own.  A
    waited tile is held to the strict-order reference with rtol = atol = 1e-12
    (the bound of tests/test_ll_launch_forms.py for device-built tables - the
    only tolerance of this file) and, after the pipeline has drained, must be
    bit for bit ll_theta(view, store_as_of_issue[rows], FP, FN) on the same
    cells, with Context.last_launch() asserted to name the same form and chunk
    count for both.

Groups: A rows under every sums form and both table builders; B slots against
parities; C growth with tiles in flight (tile_out and the slot's pinned
result, the K-sized buffers, the view's masks, the store); D hinted and
unhinted tiles on one slot; E calls between issue and wait (side lane, the
tiles' stream, refusals, a parameter batch); F a row rewritten under a tile.

Thresholds read from the sources (a retune fails the scenario that aims at it,
with a message that says to re-aim it): TABLES_FLAT_MAX and the slack of
ensure() from bnpc_ctx.h; the `4 * n` and `16384` of bnpc_view_set_slot's room
and the slack of ensure_host() from bnpc_context.cpp; the `need + need / 2` of
bnpc_theta_put from bnpc_kernels.hip; TILE_SLOTS from bnpc_amd._lib.
"""
import collections
import os
import re

import numpy as np
import pytest

from bnpc_amd import _lib
from oracle import seqsum as S
from fake_device import FakeContext
import test_host_logic as H
import test_ll_launch_forms as L
import test_mh_batch_routes as R

TILE_SLOTS = _lib.TILE_SLOTS
RE_AIM = ('the sources changed - re-aim the scenarios of '
    'tests/test_tile_pipeline.py at the new value instead of dropping them')


# ------------------------------------------- constants, read from the sources
def _squeezed(name):
    return re.sub(r'\s+', ' ', R._source(name))


def _read_constants():
    ctx_h, context, kernels = (_squeezed(f) for f in
        ('bnpc_ctx.h', 'bnpc_context.cpp', 'bnpc_kernels.hip'))
    c = {}
    m = re.search(r'#define TABLES_FLAT_MAX \((\d+) << (\d+)\)', ctx_h)
    assert m, 'TABLES_FLAT_MAX: ' + RE_AIM
    c['flat_max'] = int(m.group(1)) << int(m.group(2))
    m = re.search(r'int64_t room = std::max<int64_t>\((\d+) \* n, (\d+)\); '
        r'room = std::min<int64_t>\(std::max<int64_t>\(room, n\), '
        r'std::max\(c->N, n\)\);', context)
    assert m, "bnpc_view_set_slot's room: " + RE_AIM
    c['room_factor'], c['room_min'] = int(m.group(1)), int(m.group(2))
    m = re.search(r'size_t cap = bytes \+ bytes / (\d+) \+ (\d+);', ctx_h)
    assert m, 'ensure(): ' + RE_AIM
    c['dev_slack'] = (int(m.group(1)), int(m.group(2)))
    m = re.search(r'pinned_alloc\(p, cap, bytes \+ bytes / (\d+) \+ (\d+)\)',
        context)
    assert m, 'ensure_host(): ' + RE_AIM
    c['pin_slack'] = (int(m.group(1)), int(m.group(2)))
    m = re.search(r'ensure\(bigger, need \+ need / (\d+)\)', kernels)
    assert m, 'bnpc_theta_put: ' + RE_AIM
    c['store_extra'] = int(m.group(1))
    assert 'const int par = (int)(c->tile_seq & 1);' in kernels, \
        'the parity of an issue: ' + RE_AIM
    assert re.search(r'#define BNPC_TILE_SLOTS\s+(\d+)',
        open(os.path.join(R.ROOT, 'include', 'bnpc_hip.h')).read()) \
        .group(1) == str(TILE_SLOTS)
    return c


CONST = _read_constants()


def room(n, N):
    """view slots bnpc_view_set_slot makes room for at a view's first tile"""
    r = max(CONST['room_factor'] * n, CONST['room_min'])
    return min(max(r, n), max(N, n))


class Cap:
    """A buffer that grows by free-and-reallocate (ensure / ensure_host)."""

    def __init__(self, slack):
        self.div, self.add = CONST[slack]
        self.cap = 0

    def need(self, nbytes):
        """True if this request reallocates"""
        if nbytes <= self.cap:
            return False
        self.cap = nbytes + nbytes // self.div + self.add
        return True


class StoreCap:
    """The resident store's capacity under bnpc_theta_put."""

    def __init__(self):
        self.buf = Cap('dev_slack')

    def need(self, nbytes):
        if nbytes <= self.buf.cap:
            return False
        self.buf.cap = 0
        return self.buf.need(nbytes + nbytes // CONST['store_extra'])


# --------------------------------------------------------------- the inputs
MATS = {
    'm900x130': lambda: H.synth(31, 900, 130, 6, 0.15),     # the hint test's
    'm20000x40': lambda: H.synth(41, 20000, 40, 6, 0.15),
    'm20000x8': lambda: H.synth(43, 20000, 8, 4, 0.15),
    'm640x256': lambda: R._data(256),
}
_memo = {}


def matrix(name):
    if name not in _memo:
        _memo[name] = MATS[name]()
    return _memo[name]


def params(rng, rows, M):
    return np.clip(rng.uniform(size=(rows, M)), 1e-5, 1 - 1e-5) \
        .astype(np.float32)


def tables(theta, fp, fn):
    """host_tables of tests/test_ll_launch_forms.py under a tile's own rates
    (test_tables_are_the_siblings pins them to each other)"""
    t64 = theta.astype(np.float64)
    om64 = (1 - theta).astype(np.float64)
    return (np.log(t64 * (1 - fn) + om64 * fp),
        np.log(t64 * fn + om64 * (1 - fp)))


def pick_rows(rng, K, pool):
    """K store ids out of `pool`, in no order; from K = 3 on one id serves
    two columns; an id above K where the pool has one"""
    pool = np.asarray(pool, dtype=np.int64)
    assert pool.size >= K
    rows = rng.permutation(pool)[:K]
    if K >= 3:
        rows[K // 2] = rows[0]
    if rows.max() < K <= pool.max():
        rows[-1] = pool.max()
    return rows


Tile = collections.namedtuple('Tile', 'name view cells rows ld fp fn prior')


class Maker:
    """The tiles of one scenario: no two share cells, rows, ld or rates."""

    def __init__(self, mat, seed, store_rows):
        self.mat = mat
        self.N, self.M = matrix(mat).shape
        self.rng = np.random.RandomState(seed)
        self.store = params(self.rng, store_rows, self.M)
        self.count = 0

    def tile(self, n, K, view, hinted=False, pool=None, must=()):
        i = self.count
        self.count += 1
        rng = self.rng
        if view == 0:
            cells = np.arange(self.N)
        elif i % 2:
            cells = rng.randint(0, self.N, n)           # with repeats
        else:
            cells = rng.permutation(self.N)[:n] if n <= self.N \
                else rng.randint(0, self.N, n)
        if pool is None:
            pool = np.arange(self.store.shape[0])
        rows = pick_rows(rng, K, pool)
        for at, r in enumerate(must):
            rows[-1 - at] = r
        prior = None
        if hinted:
            prior = -rng.uniform(0, 9, size=K)
            if K > 2:
                prior[2] = prior[0]
        return Tile(f't{i}', view, cells, rows, K + (0, 3, 16)[i % 3],
            0.004 + 0.003 * i, 0.05 + 0.011 * i, prior)


class Scenario:
    def __init__(self, name, mat, steps, aim, note):
        self.name, self.mat, self.steps, self.aim, self.note = \
            name, mat, steps, aim, note


def go(tile, slot):
    """view and issue of a tile on a slot"""
    if tile.view == 0:
        return [('issue', tile, slot)]
    return [('view', tile, slot), ('issue', tile, slot)]


# ---------------------------------------------------- the host-side trace
def trace(scn):
    """What the steps do to the pipeline's bookkeeping, from the inputs
    alone: one dict per step that matters."""
    N, M = matrix(scn.mat).shape
    events, pending, seq, store_rows = [], {}, 0, 0
    for step in scn.steps:
        op = step[0]
        if op == 'put':
            _, row0, theta = step
            events.append(dict(op='put', row0=row0, rows=len(theta),
                before=store_rows, pending=dict(pending),
                bytes=(row0 + len(theta)) * M * 4))
            store_rows = max(store_rows, row0 + len(theta))
        elif op == 'view':
            _, t, slot = step
            assert slot not in pending
            events.append(dict(op='view', tile=t, slot=slot, view=t.view,
                n=t.cells.size, pending=dict(pending)))
        elif op == 'issue':
            _, t, slot = step
            assert slot not in pending and t.rows.max() < store_rows
            n = N if t.view == 0 else t.cells.size
            events.append(dict(op='issue', i=seq, par=seq & 1, slot=slot,
                tile=t, n=n, K=t.rows.size, bytes=n * t.ld * 8,
                hinted=t.prior is not None, pending=dict(pending)))
            pending[slot] = t
            seq += 1
        elif op == 'wait':
            t = pending.pop(step[1])
            events.append(dict(op='wait', slot=step[1], tile=t,
                pending=dict(pending)))
    assert not pending, 'a scenario drains its pipeline'
    return events


def issues(events):
    return [e for e in events if e['op'] == 'issue']


# ------------------------------------------------------------ the scenarios
def _b1():
    mk = Maker('m900x130', 101, 607)
    ns = (64, 1, 63, 65, 600, 333, 64, 128, 577, 100, 200, 65, 63, 1, 400, 64)
    Ks = (1, 300, 2, 40, 7, 64, 65, 9, 150, 3, 33, 17, 255, 8, 5, 12)
    tiles = [mk.tile(n, K, 0 if i == 9 else 1, hinted=i % 2 == 0)
        for i, (n, K) in enumerate(zip(ns, Ks))]
    steps = [('put', 0, mk.store)]
    nxt = iter(range(4, 16))

    def on(i, slot):            # a slot's tiles use view slot + 1
        if tiles[i].view != 0:
            tiles[i] = tiles[i]._replace(view=slot + 1)
        return go(tiles[i], slot)
    for s in range(4):
        steps += on(s, s)
    for order in ((0, 1, 2, 3), (3, 2, 1, 0), (1, 2, 0, 3)):
        for s in order:         # FIFO, LIFO, middle first; reissued at once
            steps += [('wait', s, 'hint')] + on(next(nxt), s)
    steps += [('wait', s, 'plain') for s in (2, 0, 3, 1)]

    def aim(ev):
        iss = issues(ev)
        assert len(iss) == 16
        assert max(len(e['pending']) for e in iss) == TILE_SLOTS - 1, \
            'all four slots in flight'
        for s in range(TILE_SLOTS):
            assert {e['par'] for e in iss if e['slot'] == s} == {0, 1}, s
        waits = [e['slot'] for e in ev if e['op'] == 'wait']
        assert waits[:12] == [0, 1, 2, 3, 3, 2, 1, 0, 1, 2, 0, 3]
        sizes = {e['n'] for e in iss}
        assert {1, 63, 64, 65, 600} <= sizes and 900 in sizes
        assert {e['K'] for e in iss} >= {1, 300}
    return Scenario('B1-four-slots-fifo-lifo-middle', 'm900x130', steps, aim,
        'four slots in flight, waited in three orders, each slot under '
        'both parities')


def _b2():
    mk = Maker('m900x130', 102, 200)
    steps = [('put', 0, mk.store)]
    Ks = (5, 77, 1, 130, 9, 64, 33, 2, 100)
    ns = (65, 300, 64, 63, 600, 1, 129, 500, 64)
    for i in range(9):
        s = i % 3
        if i >= 3:
            steps.append(('wait', s, 'plain' if i % 2 else 'hint'))
        steps += go(mk.tile(ns[i], Ks[i], s + 1, hinted=i % 2 == 0), s)
    steps += [('wait', s, 'hint') for s in (0, 1, 2)]

    def aim(ev):
        iss = issues(ev)
        assert [e['i'] for e in iss] == list(range(9))
        for s in range(3):
            pars = [e['par'] for e in iss if e['slot'] == s]
            assert len(pars) == 3 and set(pars) == {0, 1}, (s, pars)
        assert all(len(e['pending']) == 2 for e in iss[2:])
    return Scenario('B2-nine-issues-three-slots', 'm900x130', steps, aim,
        'an odd number of slots: every slot is written under both parities')


def _b3():
    mk = Maker('m900x130', 103, 300)
    steps = [('put', 0, mk.store)]
    Ks = (3, 120, 1, 64, 17, 250, 8, 65, 2, 40)
    ns = (600, 64, 65, 1, 333, 100, 63, 450, 128, 64)
    for i in range(10):
        steps += go(mk.tile(ns[i], Ks[i], 3, hinted=i % 3 == 0), 2)
        steps.append(('wait', 2, 'hint'))

    def aim(ev):
        iss = issues(ev)
        assert [e['par'] for e in iss] == [0, 1] * 5
        assert all(not e['pending'] and e['slot'] == 2 for e in iss)
    return Scenario('B3-one-slot-alone', 'm900x130', steps, aim,
        'one slot alternates between the two device buffers')


def _b4():
    mk = Maker('m20000x8', 104, 500)
    warm = [mk.tile(0, K, 0, hinted=K % 2 == 0) for K in (210, 20, 205, 9)]
    t = [mk.tile(0, K, 0) for K in (200, 5, 200, 6)]
    steps = [('put', 0, mk.store)]
    for tiles in (warm, t):
        for s in range(4):
            steps += go(tiles[s], s)
        steps += [('wait', s, 'hint') for s in range(4)]

    def aim(ev):
        iss = issues(ev)
        assert [e['par'] for e in iss] == [0, 1, 0, 1] * 2
        assert [len(e['pending']) for e in iss] == [0, 1, 2, 3] * 2
        # the second round reallocates nothing (a reallocation synchronises
        # the device): its issues are queued back to back, and the copy of
        # its first tile, tens of megabytes, is still running when the sums
        # of the next two are queued
        caps = dict(out=[Cap('dev_slack'), Cap('dev_slack')],
            row_idx=[Cap('dev_slack')],
            pin=[Cap('pin_slack') for _ in range(TILE_SLOTS)],
            rows_pin=[Cap('pin_slack') for _ in range(TILE_SLOTS)])
        for i, e in enumerate(iss):
            grew = [caps['out'][e['par']].need(e['bytes']),
                caps['pin'][e['slot']].need(e['bytes']),
                caps['row_idx'][0].need(e['K'] * 8),
                caps['rows_pin'][e['slot']].need(e['K'] * 8)]
            assert i < 4 or not (any(grew) or e['hinted']), (i, grew, RE_AIM)
        assert iss[4]['bytes'] >= 16 << 20 and iss[6]['bytes'] >= 16 << 20
        assert iss[5]['bytes'] * 4 < iss[4]['bytes']
    return Scenario('B4-long-copies-back-to-back', 'm20000x8', steps, aim,
        'the sums of a tile wait for the copy that last read their device '
        'buffer, and only for that one')


def _c_out():
    mk = Maker('m900x130', 111, 1300)
    t = [mk.tile(64, 5, 1), mk.tile(300, 150, 2), mk.tile(600, 300, 3),
        mk.tile(200, 1250, 1)]
    steps = [('put', 0, mk.store)] + go(t[0], 0) + go(t[1], 1) + go(t[2], 2) \
        + [('wait', 0, 'plain')] + go(t[3], 0) \
        + [('wait', 2, 'plain'), ('wait', 1, 'plain'), ('wait', 0, 'plain')]

    def aim(ev):
        iss = issues(ev)
        out = [Cap('dev_slack'), Cap('dev_slack')]
        pin = [Cap('pin_slack') for _ in range(TILE_SLOTS)]
        grew = []
        for e in iss:
            grew.append((out[e['par']].need(e['bytes']),
                pin[e['slot']].need(e['bytes'])))
        for i in (2, 3):
            assert iss[i]['bytes'] >= 4 * iss[i - 2]['bytes'], RE_AIM
            assert grew[i][0], f'tile_out[{i & 1}] does not grow: ' + RE_AIM
            assert iss[i - 1]['slot'] in iss[i]['pending'], \
                'the tile in between is waited for too early'
        assert grew[3][1] and iss[3]['slot'] == iss[0]['slot'], \
            "the slot's pinned result does not grow: " + RE_AIM
    return Scenario('C-tile-out-grows-in-flight', 'm900x130', steps, aim,
        'tile_out[par] and a slot pinned result grow while the other '
        "parity's tile is pending")


def _c_k():
    mk = Maker('m900x130', 112, 1100)
    t = [mk.tile(64, 3, 1, True), mk.tile(65, 40, 2, True),
        mk.tile(63, 700, 3, True), mk.tile(100, 1000, 1, True)]
    steps = [('put', 0, mk.store)] + go(t[0], 0) + go(t[1], 1) + go(t[2], 2) \
        + [('wait', 0, 'hint')] + go(t[3], 0) \
        + [('wait', s, 'hint') for s in (1, 2, 0)]

    def aim(ev):
        iss = issues(ev)
        assert [e['K'] for e in iss] == [3, 40, 700, 1000]
        assert [e['par'] for e in iss] == [0, 1, 0, 1]
        assert all(e['hinted'] for e in iss)
        row_idx = Cap('dev_slack')
        prior_dev = [Cap('dev_slack'), Cap('dev_slack')]
        rows_pin = [Cap('pin_slack') for _ in range(TILE_SLOTS)]
        prior_pin = [Cap('pin_slack') for _ in range(TILE_SLOTS)]
        for i, e in enumerate(iss):
            b = e['K'] * 8
            g = (row_idx.need(b), prior_dev[e['par']].need(b),
                rows_pin[e['slot']].need(b), prior_pin[e['slot']].need(b))
            assert g[0], f'row_idx does not grow at issue {i}: ' + RE_AIM
            if i >= 2:
                assert g[1], f'tile_prior_dev does not grow at {i}: ' + RE_AIM
                assert e['pending'], 'nothing in flight'
            if i == 3:
                assert g[2] and g[3], \
                    'tile_rows / tile_prior of slot 0 do not grow: ' + RE_AIM
    return Scenario('C-K-sized-buffers-grow', 'm900x130', steps, aim,
        'row_idx, tile_rows, tile_prior and tile_prior_dev grow with K under '
        'pending tiles')


def _c_masks():
    mk = Maker('m20000x40', 113, 60)
    first = mk.tile(64, 7, 1, True)
    other = mk.tile(300, 40, 2)
    big = mk.tile(17001, 5, 1, True)
    small = mk.tile(70, 9, 1, True)
    steps = [('put', 0, mk.store)] + go(first, 0) + [('wait', 0, 'hint')] \
        + go(other, 1) + go(big, 0) + [('wait', 0, 'hint')] + go(small, 0) \
        + [('wait', 0, 'hint'), ('wait', 1, 'plain')]

    def aim(ev):
        views = [e for e in ev if e['op'] == 'view' and e['view'] == 1]
        assert [e['n'] for e in views] == [64, 17001, 70]
        N = matrix('m20000x40').shape[0]
        assert room(64, N) == CONST['room_min'] < N, RE_AIM
        assert views[1]['n'] > room(views[0]['n'], N), \
            "the large tile fits the room of the view's first: " + RE_AIM
        assert 1 in views[1]['pending'] and 1 in views[2]['pending']
        assert all(e['slot'] == 0 for e in views)
    return Scenario('C-view-masks-grow-then-shrink', 'm20000x40', steps, aim,
        "a view's masks grow past the room taken at its first tile while "
        'another slot is pending; a 70-cell tile follows on it')


def _c_store():
    mk = Maker('m900x130', 114, 700)
    old = np.arange(300)
    t = [mk.tile(600, 200, 1, pool=old), mk.tile(333, 64, 2, True, pool=old),
        mk.tile(65, 290, 3, pool=old)]
    after = mk.tile(128, 120, 4, True, must=(5, 699))
    steps = [('put', 0, mk.store[:300])] + go(t[0], 0) + go(t[1], 1) \
        + go(t[2], 2) + [('put', 300, mk.store[300:])] \
        + [('wait', s, 'hint') for s in (0, 1, 2)] + go(after, 3) \
        + [('wait', 3, 'hint')]

    def aim(ev):
        puts = [e for e in ev if e['op'] == 'put']
        cap = StoreCap()
        assert cap.need(puts[0]['bytes'])
        assert cap.need(puts[1]['bytes']), \
            'the second put fits the store: ' + RE_AIM
        assert puts[1]['row0'] == puts[1]['before'] == 300 \
            and puts[1]['row0'] + puts[1]['rows'] >= 2 * puts[1]['before']
        assert len(puts[1]['pending']) == 3
        assert all(p.rows.max() < 300 for p in puts[1]['pending'].values())
        assert after.rows.min() < 300 <= after.rows.max()
    return Scenario('C-store-grows-under-three-tiles', 'm900x130', steps, aim,
        'bnpc_theta_put moves the store while three tiles that read it are '
        'queued')


def _d():
    mk = Maker('m900x130', 121, 300)
    a, b, c = mk.tile(300, 200, 2, True), mk.tile(100, 50, 2), \
        mk.tile(400, 260, 2, True)
    d, e = mk.tile(90, 30, 2, True), mk.tile(80, 20, 2)
    steps = [('put', 0, mk.store)]
    for t, how in ((a, 'hint'), (b, 'hint'), (c, 'hint'), (d, 'plain'),
            (e, 'hint')):
        steps += go(t, 1) + [('wait', 1, how)]

    def aim(ev):
        iss = issues(ev)
        assert [e['hinted'] for e in iss] == [True, False, True, True, False]
        assert [e['n'] for e in iss][:3] == [300, 100, 400]
        assert {e['slot'] for e in iss} == {1}
    return Scenario('D-hinted-and-unhinted-on-one-slot', 'm900x130', steps,
        aim,
        'tile_hinted is per issue; records of a smaller tile in a buffer '
        'sized by a larger one')


def _f():
    mk = Maker('m900x130', 141, 200)
    keep = np.delete(np.arange(200), 77)
    a = mk.tile(500, 120, 1, True, pool=keep, must=(77,))
    b = mk.tile(333, 60, 2, pool=keep)
    fresh = params(np.random.RandomState(9), 1, 130)
    c = mk.tile(200, 33, 3, pool=keep, must=(77,))
    steps = [('put', 0, mk.store)] + go(a, 0) + go(b, 1) \
        + [('put', 77, fresh), ('wait', 1, 'plain'), ('wait', 0, 'hint')] \
        + go(c, 2) + [('wait', 2, 'plain')]

    def aim(ev):
        put = [e for e in ev if e['op'] == 'put'][1]
        assert set(put['pending']) == {0, 1}
        assert (a.rows == 77).sum() == 1 and not (b.rows == 77).any()
        assert (c.rows == 77).sum() == 1
    return Scenario('F-a-row-rewritten-under-a-tile', 'm900x130', steps, aim,
        'the reborn-id case of FakeContext._poison_in_flight: one column of '
        'one tile is open, everything else exact')


# ---- E: calls between issue and wait
def _form(ctx):
    last = getattr(ctx, 'last_launch', None)
    return last() if last else None


def _e():
    mk = Maker('m900x130', 131, 320)
    data = matrix('m900x130')
    N, M = data.shape
    rng = np.random.RandomState(132)
    pool = np.arange(319)                       # row 319: read by no tile
    a = mk.tile(600, 300, 1, True, pool=pool)
    b = mk.tile(577, 250, 2, pool=pool)
    cells5 = rng.permutation(N)[:333]
    th1, th40 = params(rng, 1, M), params(rng, 40, M)
    labels = rng.randint(-1, 3, cells5.size)
    ids = np.array([7, 2, 4], dtype=np.int64)
    assign = ids[rng.randint(0, 3, N)]
    thG = params(rng, 3, M)
    rows_p = pick_rows(rng, 33, pool)
    L1, L0 = tables(params(rng, 4, M), 0.02, 0.3)
    cells_a = rng.permutation(N)[:500]
    cells_b = rng.randint(0, N, 1200)

    def theta_on(view, theta):
        def f(ctx):
            return ctx.ll_theta(view, theta, L.FP, L.FN), _form(ctx)
        return f

    def ll_tables(ctx):
        got = ctx.ll_tables(5, L1, L0)
        want = S.table_sums(data[cells5], L1, L0)
        assert np.array_equal(got, want), L._first_difference(got, want)
        return (got,)

    def view_then(view, cells):
        def f(ctx):
            ctx.view_set(view, cells)
            return ctx.ll_theta(view, th40, L.FP, L.FN), _form(ctx)
        return f

    def pinned_again(ctx):
        got = ctx.ll_theta_pinned(5, th40, L.FP, L.FN, 43)[:, :40].copy()
        pinned = _form(ctx)
        want = ctx.ll_theta(5, th40, L.FP, L.FN)
        assert pinned == _form(ctx)
        assert np.array_equal(got, want), L._first_difference(got, want)
        return ()

    calls = [
        ('ll_theta K=1', theta_on(5, th1)),
        ('ll_theta K=40', theta_on(5, th40)),
        ('view_counts', lambda ctx: ctx.view_counts(5, labels, 3)),
        ('colcounts_by_label',
            lambda ctx: ctx.colcounts_by_label(assign, ids)),
        ('ll_total', lambda ctx: (ctx.ll_total(thG, [.01, .02], [.2, .1]),)),
        ('ll_rows_pinned', lambda ctx: (ctx.ll_rows_pinned(5, rows_p, .03,
            .15, 36)[:, :33].copy(), _form(ctx))),
        ('ll_tables', ll_tables),
        ('view_set n <= N', view_then(3, cells_a)),
        ('view_set n > N', view_then(4, cells_b)),
    ]
    bad_rows = np.array([0, 320])
    slots = TILE_SLOTS
    refusals = [
        (lambda ctx: ctx.ll_theta_pinned(5, th40, L.FP, L.FN, 40),
            'not available while an issued tile is in flight', False),
        (lambda ctx: ctx.ll_theta_pinned_top2(5, th40, L.FP, L.FN, 40,
            np.zeros(40)),
            'not available while an issued tile is in flight', False),
        (lambda ctx: ctx.ll_theta_pinned_top2(5, th40, L.FP, L.FN, 40,
            np.zeros(40), wait=False),
            'not available while an issued tile is in flight', False),
        (lambda ctx: ctx.ll_rows_issue(1, a.rows, a.fp, a.fn, a.ld, 0),
            'unconsumed tile', True),
        (lambda ctx: ctx.view_set_slot(1, a.cells, 0), 'unconsumed tile',
            True),
        (lambda ctx: ctx.ll_rows_issue(5, bad_rows, .01, .2, 2, 1),
            'row is not in the resident parameter store', True),
        (lambda ctx: ctx.ll_rows_wait(1, 333, 2), 'no tile was issued', True),
        (lambda ctx: ctx.ll_rows_issue(5, rows_p, .01, .2, 33, slots),
            'slot out of range', True),
        (lambda ctx: ctx.view_set_slot(3, np.zeros(0, np.int64), 1),
            'empty cell list', False),
        (lambda ctx: ctx.view_set_slot(3, np.array([0, N]), 1),
            'cell index out of range', False),
    ]
    steps = [('put', 0, mk.store),
        ('call', None, lambda ctx: ctx.view_set(5, cells5) and ())]
    steps += [('call', key, f) for key, f in calls]
    steps += go(a, 0) + go(b, 2)
    steps += [('call', key, f) for key, f in calls[:3]]
    steps.append(('put', 319, params(rng, 1, M)))
    steps += [('call', key, f) for key, f in calls[3:]]
    steps += [('refuse',) + r for r in refusals]
    steps += [('wait', 2, 'plain'), ('wait', 0, 'hint'),
        ('call', None, pinned_again)]

    def aim(ev):
        put = [e for e in ev if e['op'] == 'put'][1]
        assert set(put['pending']) == {0, 2} and put['row0'] == 319
        assert max(a.rows.max(), b.rows.max(), rows_p.max()) < 319
        assert cells_a.size <= N < cells_b.size
        assert bad_rows.max() == mk.store.shape[0]
    return Scenario('E-calls-between-issue-and-wait', 'm900x130', steps, aim,
        'side-lane calls, calls queued on the stream of the tiles and '
        'refusals with two tiles pending')


SCENARIOS = [f() for f in (_b1, _b2, _b3, _b4, _c_out, _c_k, _c_masks,
    _c_store, _d, _e, _f)]
_ids = [s.name for s in SCENARIOS]


# ---------------------------------------------------------------- the runner
class _Rec:
    def __init__(self, tile, snap, form):
        self.tile, self.snap, self.form = tile, snap, form
        self.open = np.zeros(tile.rows.size, dtype=bool)
        self.mat = self.hint = None


def _same(got, want, what):
    if isinstance(want, np.ndarray):
        R._same(got, want, what)
    else:
        assert got == want, (what, got, want)


def _check_tile(rec, data, device):
    """a waited tile against the strict-order reference"""
    t = rec.tile
    cells = np.arange(data.shape[0]) if t.view == 0 else t.cells
    want = S.table_sums(data[cells], *tables(rec.snap, t.fp, t.fn))
    keep = ~rec.open
    got = rec.mat
    assert got.shape == want.shape, (t.name, got.shape, want.shape)
    if device:
        np.testing.assert_allclose(got[:, keep], want[:, keep], rtol=1e-12,
            atol=1e-12, err_msg=t.name)
    else:
        assert np.array_equal(got[:, keep], want[:, keep]), (t.name,
            L._first_difference(got[:, keep], want[:, keep]))
    if rec.hint is not None and keep.all():
        L._check_wide_hints(got, rec.hint, t.prior, t.name)


def run(scn, ctx, device):
    """Play a scenario's steps on a context: every waited tile against the
    strict-order reference at its wait; on the device, once the pipeline has
    drained, bit for bit against ll_theta under the same form; the calls made
    more than once give the same bits every time."""
    data = matrix(scn.mat)
    N, M = data.shape
    store = np.zeros((0, M), np.float32)
    pending, done, calls = {}, [], {}
    for step in scn.steps:
        op = step[0]
        if op == 'put':
            _, row0, theta = step
            ctx.theta_put(row0, theta)
            end = row0 + len(theta)
            if end > len(store):
                store = np.concatenate([store,
                    np.zeros((end - len(store), M), np.float32)])
            store[row0:end] = theta
            for rec in pending.values():
                rec.open |= (rec.tile.rows >= row0) & (rec.tile.rows < end)
        elif op == 'view':
            _, t, slot = step
            assert ctx.view_set_slot(t.view, t.cells, slot) == t.cells.size
        elif op == 'issue':
            _, t, slot = step
            snap = store[t.rows].copy()
            if t.prior is None:
                ctx.ll_rows_issue(t.view, t.rows, t.fp, t.fn, t.ld, slot)
            else:
                ctx.ll_rows_issue_hint(t.view, t.rows, t.fp, t.fn, t.ld, slot,
                    t.prior)
            pending[slot] = _Rec(t, snap, _form(ctx) if device else None)
        elif op == 'wait':
            _, slot, how = step
            rec = pending.pop(slot)
            t = rec.tile
            n = N if t.view == 0 else t.cells.size
            if how == 'hint':
                mat, hint = ctx.ll_rows_wait_hint(slot, n, t.ld)
                assert (hint is None) == (t.prior is None), (t.name,
                    'hints of an unhinted tile' if t.prior is None
                    else 'no hints')
                rec.hint = None if hint is None else hint.copy()
            else:
                mat = ctx.ll_rows_wait(slot, n, t.ld)
            assert mat.shape == (n, t.ld)
            rec.mat = mat[:, :t.rows.size].copy()
            _check_tile(rec, data, device)
            done.append(rec)
        elif op == 'call':
            _, key, f = step
            got = f(ctx)
            if key is not None:
                calls.setdefault(key, []).append(got)
        elif op == 'refuse':
            _, f, message, on_fake = step
            if device:
                with pytest.raises(RuntimeError, match=message):
                    f(ctx)
            elif on_fake:
                with pytest.raises((AssertionError, KeyError, IndexError)):
                    f(ctx)
        else:
            raise AssertionError(op)
    assert not pending
    for key, results in calls.items():
        assert len(results) >= 2, key
        for again in results[1:]:
            assert len(again) == len(results[0])
            for g, w in zip(again, results[0]):
                _same(g, w, f'{key}: with tiles in flight against alone')
    if device:
        for rec in done:
            t = rec.tile
            view = 0
            if t.view != 0:
                view = 6
                ctx.view_set(view, t.cells)
            want = ctx.ll_theta(view, rec.snap, t.fp, t.fn)
            assert _form(ctx) == rec.form, (t.name, _form(ctx), rec.form)
            keep = ~rec.open
            assert np.array_equal(rec.mat[:, keep], want[:, keep]), (t.name,
                rec.form, L._first_difference(rec.mat[:, keep],
                want[:, keep]))
    return done


# ------------------------------------------------------------- the CPU half
def test_tables_are_the_siblings():
    theta = params(np.random.RandomState(3), 5, 41)
    for got, want in zip(tables(theta, L.FP, L.FN), L.host_tables(theta)):
        assert np.array_equal(got, want)


@pytest.mark.parametrize('scn', SCENARIOS, ids=_ids)
def test_scenario_reaches_its_edge(scn):
    """From the inputs alone: the edge the scenario names, and rows that
    tell rows[k] from k (ids above K, out of order, one id for two columns);
    no two tiles share their cells, rows, ld or rates."""
    ev = trace(scn)
    scn.aim(ev)
    tiles = [e['tile'] for e in issues(ev)]
    assert any(t.rows.max() >= t.rows.size for t in tiles)
    assert any(np.any(np.diff(t.rows) < 0) for t in tiles)
    assert any(np.unique(t.rows).size < t.rows.size for t in tiles)
    assert {t.ld - t.rows.size for t in tiles} <= {0, 3, 16}
    if len(tiles) >= 3:
        assert {t.ld - t.rows.size for t in tiles} == {0, 3, 16}
    assert len({(t.fp, t.fn) for t in tiles}) == len(tiles)
    for i, t in enumerate(tiles):
        assert 0 < t.fp < 1 and 0 < t.fn < 1
        for u in tiles[:i]:
            assert not (t.cells.size == u.cells.size and t.view != 0
                and np.array_equal(t.cells, u.cells)), (t.name, u.name)
            assert not np.array_equal(t.rows, u.rows), (t.name, u.name)


@pytest.mark.parametrize('scn', SCENARIOS, ids=_ids)
def test_scenario_on_the_cpu_stand_in(scn):
    """FakeContext computes the calls with the oracle's strict-order sums:
    the scenario and its expectations hold with no device."""
    ctx = FakeContext(data=matrix(scn.mat))
    done = run(scn, ctx, device=False)
    assert len(done) == len(issues(trace(scn)))
    if scn.name.startswith('F-'):
        assert ctx.poisoned == 1 and sum(r.open.sum() for r in done) == 1
        bad = [r for r in done if r.open.any()][0]
        assert np.isnan(bad.mat[:, bad.open]).all()
    else:
        assert not getattr(ctx, 'poisoned', 0)


# ---- group A on the CPU: the cases and the builder threshold
def _mt(M):
    """bnpc_create: table rows per group, M rounded up to 8"""
    assert 'c->Mt = (int)((M + 7) / 8 * 8);' \
        in _squeezed('bnpc_context.cpp'), RE_AIM
    return (M + 7) // 8 * 8


def _a_cases():
    small = [c for c in L.CASES if c.entry == 'theta' and c.K <= 210
        and L.MATS[c.mat][0] * L.MATS[c.mat][1]
            <= L.MATS['m5000x1000'][0] * L.MATS['m5000x1000'][1]]
    Mt = _mt(L.MATS['m4100x1003'][1])
    K_over = CONST['flat_max'] // Mt + 1
    while (K_over + 7) // 8 * 8 * Mt <= CONST['flat_max'] or K_over % 8 == 0:
        K_over += 1
    K_under = (CONST['flat_max'] // (8 * Mt)) * 8 - 3
    extra = [
        L.Case('m4100x1003', (601, 11), K_over, 'theta', {}, None, None,
            'k_tables_theta', 'rows through the non-flat builder'),
        L.Case('m4100x1003', (601, 11), K_under, 'theta', {}, None, None,
            'k_tables_theta_flat', 'just below it at the same shape'),
    ]
    return small, extra


A_SMALL, A_EXTRA = _a_cases()
A_CASES = A_SMALL + A_EXTRA
_seen_forms = {}


def _kw_of(name):
    if name.startswith('k_ll8'):
        return 8
    m = re.match(r'k_ll<(\d)>', name)
    assert m, f'{name!r}: the cluster tile of this form is not known here'
    return int(m.group(1))


def _flat(case, name):
    """whether the flat builder makes the tables of this case under the
    form `name` (launch_ll, bnpc_kernels.hip)"""
    KW = _kw_of(name)
    G = (case.K + KW - 1) // KW
    return G * KW * _mt(L.MATS[case.mat][1]) <= CONST['flat_max']


def test_group_a_cases_are_where_they_say():
    assert len(A_SMALL) == 9 and any(c.view and c.view[0]
        > L.MATS[c.mat][0] for c in A_SMALL), \
        'the cases of tests/test_ll_launch_forms.py changed: ' + RE_AIM
    over, under = A_EXTRA
    assert over.K % 8 and under.K % 8 and under.K < over.K
    assert 'G * KW * (int64_t)c->Mt <= TABLES_FLAT_MAX' \
        in _squeezed('bnpc_kernels.hip'), RE_AIM
    # (with the 8-wide tile every split launch runs; the device test asserts
    # the same for the tile last_launch reports)
    assert not _flat(over, 'k_ll8_asm') and _flat(under, 'k_ll8_asm')
    for c in A_SMALL:
        assert (c.builder == 'k_tables_theta_flat') == _flat(c, c.form), c


# ------------------------------------------------------------ the device half
def _clean_knobs(monkeypatch):
    for k in set(L.KNOBS) | set(R.KNOBS):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize('scn', SCENARIOS, ids=_ids)
def test_scenario_on_the_device(scn, monkeypatch):
    """groups B - F: see the module docstring and the scenario's note"""
    _clean_knobs(monkeypatch)
    scn.aim(trace(scn))
    ctx = _lib.Context(data=matrix(scn.mat))
    try:
        done = run(scn, ctx, device=True)
        print(f'\n[tiles] {scn.name}: {len(done)} tiles; forms '
            f'{sorted({r.form[0] for r in done})}')
    finally:
        ctx.close()


@pytest.mark.gpu
def test_parameter_batch_with_tiles_in_flight(monkeypatch):
    """Group E: bnpc_mh_batch_dev (the screen on the side lane) and
    bnpc_label_counts_and_batch (not fused while a tile is pending) at a shape
    where the screen applies, with two tiles pending: the plain host batch
    bit for bit, and both tiles exact afterwards."""
    _clean_knobs(monkeypatch)
    table = R._table()
    M, G = 256, 3
    assert G * M >= R.MH_SCREEN_MIN
    inp = R._inputs(M, G)
    host, draws, _ = R._reference(table, M, G, R.PAR, False)
    mk = Maker('m640x256', 151, 120)
    a, b = mk.tile(600, 100, 1, True), mk.tile(500, 64, 2)
    seed = R._seed(G, M)

    def batch(route):
        def f(ctx):
            R._poison_scratch(G, M)
            if route == 'label':
                c1, c0 = np.full_like(inp.n1, -7), np.full_like(inp.n0, -7)
                got = R._batch(table, inp.old, c1, c0, R.PAR, seed,
                    label=(inp.assign, inp.ids), ctx=ctx)
            else:
                c1, c0 = ctx.colcounts_by_label(inp.assign, inp.ids)
                got = R._batch(table, inp.old, inp.n1, inp.n0, R.PAR, seed,
                    ctx=ctx)
            R._same(c1, inp.n1, f'{route}: n1')
            R._same(c0, inp.n0, f'{route}: n0')
            assert got.status == host.status == 0
            assert got.position == host.position, 'stream position'
            R._same(got.new, host.new, f'{route}: new')
            R._same(got.declined, host.declined, f'{route}: declined')
            R._same(got.prior, host.prior, f'{route}: prior')
            return ()
        return f
    steps = [('put', 0, mk.store)] + go(a, 0) + go(b, 3) \
        + [('call', None, batch('dev')), ('call', None, batch('label')),
        ('wait', 3, 'plain'), ('wait', 0, 'hint')]
    scn = Scenario('E-parameter-batch', 'm640x256', steps, None, '')
    assert len(issues(trace(scn))) == 2
    ctx = _lib.Context(data=matrix(scn.mat))
    try:
        run(scn, ctx, device=True)
    finally:
        ctx.close()


# ---- group A: rows under every form
@pytest.fixture(scope='module')
def mats():
    assert S._LIB is not None, \
        'oracle/_build/liboracle_seqsum.so missing: run make -C oracle'
    m = L._Mats()
    m.store_cap = {}
    yield m
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize('case', A_CASES, ids=L._case_id)
def test_rows_under_every_form(case, mats, monkeypatch):
    """Group A: ll_rows_pinned and a tile issued on slot 1 give the bits of
    ll_theta on the gathered rows under the same form - the whole output -
    and hold 1e-12 against the strict-order reference; the store is filled in
    two puts, the second past its capacity."""
    data, ctx = mats.matrix(case.mat)
    N, M = data.shape
    K = case.K
    cells = np.arange(N) if case.view is None \
        else np.random.RandomState(case.view[1]).randint(0, N, case.view[0])
    n = cells.size
    # the store: at least 2 K + 7 rows, and past what this context holds
    cap = mats.store_cap.setdefault(case.mat, StoreCap())
    cap.need((K + 3) * M * 4)
    rows_total = max(2 * K + 7, cap.buf.cap // (M * 4) + 2)
    rng = np.random.RandomState(1000 + K)
    store = params(rng, rows_total, M)
    ctx.theta_put(0, store[:K + 3])
    assert cap.need(rows_total * M * 4), 'the second put does not grow'
    ctx.theta_put(K + 3, store[K + 3:])
    rows = pick_rows(rng, K, np.arange(rows_total))
    theta = store[rows]
    ld = K + (0, 3, 16)[K % 3]

    view = 0
    if case.view is not None:
        view = 1
        ctx.view_set(view, cells)
    L._set_knobs(monkeypatch, ctx, case.knobs)
    want_bits = ctx.ll_theta(view, theta, L.FP, L.FN)
    if case.form is not None:
        L._assert_form(ctx, case, 'll_theta on the gathered rows')
    form = ctx.last_launch()
    _seen_forms[L._case_id(case)] = form[0]
    flat = _flat(case, form[0])
    assert flat == (case.builder == 'k_tables_theta_flat'), (
        f'{L._case_id(case)} ran {form[0]!r}: G * KW * Mt is on the other '
        f'side of TABLES_FLAT_MAX = {CONST["flat_max"]} - ' + RE_AIM)
    print(f'\n[rows] {L._case_id(case)}: {form[0]!r}, {form[2]} chunk(s), '
        f'{"flat" if flat else "non-flat"} builder, store {rows_total} rows')

    got = ctx.ll_rows_pinned(view, rows, L.FP, L.FN, ld)[:, :K].copy()
    assert ctx.last_launch() == form, ('ll_rows_pinned', ctx.last_launch())
    assert np.array_equal(got, want_bits), ('ll_rows_pinned',
        L._first_difference(got, want_bits))

    tile_view = 0
    if case.view is not None:
        tile_view = 2
        ctx.view_set_slot(tile_view, cells, 1)
    prior = -rng.uniform(0, 9, size=K)
    ctx.ll_rows_issue_hint(tile_view, rows, L.FP, L.FN, ld, 1, prior)
    assert ctx.last_launch() == form, ('issued tile', ctx.last_launch())
    mat, hint = ctx.ll_rows_wait_hint(1, n, ld)
    mat = mat[:, :K].copy()
    assert np.array_equal(mat, want_bits), ('issued tile',
        L._first_difference(mat, want_bits))
    L._check_wide_hints(mat, hint.copy(), prior, L._case_id(case))

    want = S.table_sums(data[cells], *L.host_tables(theta))
    np.testing.assert_allclose(want_bits, want, rtol=1e-12, atol=1e-12)
    L._set_knobs(monkeypatch, ctx, {})


@pytest.mark.gpu
def test_rows_cases_cover_the_forms_between_them():
    """after the parametrised cases: the forms last_launch reported include
    every form the chosen cases of tests/test_ll_launch_forms.py name"""
    missing = [L._case_id(c) for c in A_CASES if L._case_id(c)
        not in _seen_forms]
    assert not missing, f'run the whole file: {missing} did not run'
    assert {c.form for c in A_SMALL} <= set(_seen_forms.values()), \
        sorted(_seen_forms.values())
