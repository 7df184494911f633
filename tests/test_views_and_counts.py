"""The layer under every sum: the matrix packed into {ones, zeros} bit planes
(bnpc_create, bnpc_create_codes, bnpc_create_planes: bnpc_context.cpp), the
lane masks a view gathers from them (k_gather_transpose behind bnpc_view_set)
and the per-segment column counts (k_colcounts behind colcounts_device,
k_counts_masks behind counts_from_masks: bnpc_kernels.hip), each launch edge
reached on purpose.

Everything here is integers and bits: nothing has a tolerance.

A view is read back BIT FOR BIT by `view_bits`: ll_tables with K = 2 W
clusters (W = ceil(M / 64)) over power-of-two tables - for the ones plane
L1[k][m] = 2 ** (m - 32 k) for 32 k <= m < 32 k + 32, else 0, and L0 = 0; for
the zeros plane the roles are swapped.  Every sum is an integer below 2 ** 32,
exact in float64 in any order, and its bits are the plane's.  A mismatch names
the slot, the mutation and the plane.

House pattern: every group has a `*_cases()` builder that needs no device; an
unmarked test plays every case through tests/fake_device.FakeContext, asserts
the expected values there and, from the inputs alone with the driver's
arithmetic restated (`view_route`, `chunking`, `member_route`, `masks_lds`,
`label_route`), that the case reaches the edge it names; the `gpu` tests play
the same cases on a _lib.Context.  test_the_thresholds_are_the_sources reads
the restated thresholds out of the sources: when one is retuned it fails and
the cases are re-aimed, not dropped.

Groups: A the matrix to the identity view by the three creation routes, with
their refusals; B gathered views (sizes round the 64-slot block, repeats, the
routes a cell list travels, every view at once, refusals, shrink and grow, two
views back to back); C k_colcounts over cell lists (the 32-cell chunk, the
4-wide loop at every remainder, zero-fill, the second launch past 65 535
chunks, colcounts_by_label on that route); D k_counts_masks (blocks against
waves, the LDS floor, segments against CM_SEG, labels -1, the in-place limit
of the membership words, the G bounds).

Deliberately out of scope, because other files own them: the deferred-result
route of the counts (test_mh_batch_routes.py), view_set with a tile in flight
(test_tile_pipeline.py) and views past 57 344 cells (test_large_views.py).
"""
import collections
import contextlib
import functools
import os
import re

import numpy as np
import pytest

from bnpc_amd import _lib
from bnpc_amd.bitplanes import BitPlanes
from fake_device import FakeContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'bnpc_amd', 'csrc')

# what the route functions restate (test_the_thresholds_are_the_sources)
ZC_IN_MAX = 256 << 10       # bytes read in place from the pinned arena
CH = 32                     # cells of a k_colcounts chunk
MAXY = 65535                # chunks of one k_colcounts launch
CM_SEG = 8                  # segments of a k_counts_masks workgroup
CM_RANGE_MAX = 896          # blocks of one LDS range of membership words
RED_BYTES = 16384           # k_counts_masks' reduction floor of dynamic LDS
MAX_VIEWS = 7
G_MAX = 4096                # segments bnpc_view_counts takes
MASK_COUNTS_MAX = 64        # clusters colcounts_by_label counts from masks

KNOBS = ('BNPC_ZERO_COPY', 'BNPC_MASK_COUNTS_MAX')


def _source(name, folder=CSRC):
    with open(os.path.join(folder, name)) as f:
        return f.read()


def test_the_thresholds_are_the_sources():
    """Every threshold the cases are aimed at, read out of the sources: a
    retuned one fails HERE, and the cases are then re-aimed at the edges
    their names carry - do not drop them."""
    ctx_h = _source('bnpc_ctx.h')
    kernels = _source('bnpc_kernels.hip')
    context = _source('bnpc_context.cpp')
    api = _source('bnpc_hip.h', os.path.join(ROOT, 'include'))
    msg = 're-aim the cases of this file, do not drop them'
    assert re.search(r'#define ZC_IN_MAX \(\(int64_t\)(\d+) << (\d+)\)',
        ctx_h).groups() == ('256', '10') and ZC_IN_MAX == 256 << 10, msg
    body = re.search(r'static int colcounts_device\(.*?\n}\n', kernels,
        re.S).group(0)
    assert re.search(r'const int64_t CH = (\d+);', body).group(1) \
        == str(CH), msg
    assert re.search(r'const size_t maxy = (\d+);', body).group(1) \
        == str(MAXY), msg
    assert '(const Chunk *)c->chunks.p + off' in body, msg
    assert 'hipMemsetAsync(cnt.p, 0, cnt_bytes, c->stream)' in body, msg
    assert re.search(r'#define CM_SEG (\d+)', kernels).group(1) \
        == str(CM_SEG), msg
    assert re.search(r'#define CM_RANGE_MAX (\d+)', kernels).group(1) \
        == str(CM_RANGE_MAX), msg
    red = re.search(r'const size_t red_bytes = (.+?);', kernels).group(1)
    assert red == '4 * 2 * CM_SEG * 64 * sizeof(int)' \
        and 4 * 2 * CM_SEG * 64 * 4 == RED_BYTES, msg
    squeezed = re.sub(r'\s+', ' ', kernels + context)
    for line in (
            # k_counts_masks: the 4 waves take every 4th block
            'for (long long b = wave; b < nb; b += 4) {',
            'size_t lds = (size_t)range * CM_SEG * sizeof(unsigned long '
            'long);',
            'if (lds < red_bytes) lds = red_bytes;',
            'if (c->tun.zero_copy && (int64_t)mem_bytes <= ZC_IN_MAX) {',
            f'ARGCHK(G > 0 && G <= {G_MAX}, "G out of range");',
            'if (K <= c->tun.mask_counts_max && c->views[0].nblk <= '
            'CM_RANGE_MAX) {',
            # k_gather_transpose: 4 row words per workgroup
            'const int w = blockIdx.y * 4 + (threadIdx.x >> 6);',
            'dim3 grid((unsigned)v.nblk, (unsigned)((c->W + 3) / 4));',
            # bnpc_view_set: its own pinned list, else the arena, else a copy
            'if (c->view_cells_pin && n <= c->N && !c->any_tile_pending()) {',
            'if (!c->tun.zero_copy || (int64_t)bytes > ZC_IN_MAX) return '
            'nullptr;',
            'ARGCHK(view >= 1 && view < BNPC_MAX_VIEWS, "view out of '
            'range");'):
        assert line in squeezed, f'{line!r}: {msg}'
    assert re.search(r'#define BNPC_MAX_VIEWS (\d+)', api).group(1) \
        == str(MAX_VIEWS) and _lib.MAX_VIEWS == MAX_VIEWS, msg
    assert re.search(r'int mask_counts_max = (\d+);', ctx_h).group(1) \
        == str(MASK_COUNTS_MAX), msg


# ------------------------------------------------- the driver's arithmetic
def view_route(N, n, zero_copy=1):
    """bnpc_view_set (no tile in flight): how the cell list reaches the
    gather kernel."""
    if n == 0:
        return 'empty'
    if n <= N:
        return 'pinned'         # the context's own pinned list of N entries
    if zero_copy and 8 * n <= ZC_IN_MAX:
        return 'arena'          # read in place from the pinned arena
    return 'copied'             # through a device buffer


def chunking(sizes):
    """colcounts_device: [(begin, end, segment)] of one call."""
    out, b0 = [], 0
    for g, size in enumerate(sizes):
        for b in range(b0, b0 + size, CH):
            out.append((b, min(b0 + size, b + CH), g))
        b0 += size
    return out


def blocks(n):
    return (n + 63) // 64


def masks_lds(n):
    """counts_from_masks: (bytes of dynamic LDS, which term sets them)."""
    words = min(blocks(n), CM_RANGE_MAX) * CM_SEG * 8
    return (RED_BYTES, 'floor') if words < RED_BYTES else (words, 'words')


def member_route(G, n, zero_copy=1):
    """counts_from_masks: where the membership words are built."""
    if zero_copy and G * blocks(n) * 8 <= ZC_IN_MAX:
        return 'arena'
    return 'heap'


def label_route(K, N, mask_counts_max=MASK_COUNTS_MAX):
    if K <= mask_counts_max and blocks(N) <= CM_RANGE_MAX:
        return 'masks'
    return 'cells'


# ------------------------------------------------------------ the matrices
SPECIAL_FROM = 31       # the smallest M that holds the four special columns


@functools.lru_cache(maxsize=None)
def matrix(N, M, seed=0):
    """N x M float64 of 0 | 1 | NaN; from M = 31 on with an all-ones, an
    all-zeros and an all-missing column and one set only in the last cell
    (the last mutation: the top bit of the last word in use)."""
    rng = np.random.RandomState(1000 * N + M + seed)
    data = (rng.random_sample((N, M)) < 0.4).astype(np.float64)
    data[rng.random_sample((N, M)) < 0.25] = np.nan
    if M >= SPECIAL_FROM:
        data[:, 0] = 1
        data[:, M // 2] = 0
        data[:, M - 2] = np.nan
        data[:, M - 1] = np.nan
        data[N - 1, M - 1] = 1
    data.setflags(write=False)
    return data


def as_codes(data, seed=0):
    """int8 codes of `data` with about half of the ones written as 2."""
    rng = np.random.RandomState(seed)
    codes = np.where(np.isnan(data), 3, data).astype(np.int8)
    codes[(codes == 1) & (rng.random_sample(codes.shape) < 0.5)] = 2
    return codes


def power_tables(M):
    K = 2 * ((M + 63) // 64)
    T = np.zeros((K, M))
    for k in range(K):
        m = np.arange(32 * k, min(32 * k + 32, M))
        T[k, m] = 2.0 ** (m - 32 * k)
    return T


def view_bits(ctx, view):
    """(ones, zeros): the view's two planes as boolean n x M arrays, read
    through ll_tables over power-of-two tables - one launch per plane."""
    M = ctx.M
    T = power_tables(M)
    Z = np.zeros_like(T)
    n, K = ctx.view_size(view), T.shape[0]
    planes = []
    for L1, L0 in ((T, Z), (Z, T)):
        sums = np.array(ctx.ll_tables(view, L1, L0), dtype=np.float64)
        assert sums.shape == (n, K)
        assert np.array_equal(sums, np.floor(sums)) and (sums >= 0).all() \
            and (sums < 2.0 ** 32).all(), 'the sums are not 32-bit integers'
        words = sums.astype(np.uint64)
        bits = ((words[:, :, None] >> np.arange(32, dtype=np.uint64)) & 1) \
            .astype(bool).reshape(n, 32 * K)
        assert not bits[:, M:].any()
        planes.append(bits[:, :M])
    return planes


def check_view(ctx, view, data, cells, what=''):
    cells = np.asarray(cells, dtype=np.int64)
    assert ctx.view_size(view) == cells.size, what
    got = view_bits(ctx, view)
    sub = data[cells]
    for plane, bits, value in (('ones', got[0], 1), ('zeros', got[1], 0)):
        bad = np.argwhere(bits != (sub == value))
        assert bad.size == 0, (f'{what}: view {view}, {plane} plane: '
            f'{len(bad)} wrong bits, the first at slot {bad[0][0]} (cell '
            f'{cells[bad[0][0]]}), mutation {bad[0][1]}')


def want_counts(data, segments):
    G, M = len(segments), data.shape[1]
    n1 = np.zeros((G, M), dtype=int)
    n0 = np.zeros((G, M), dtype=int)
    for g, seg in enumerate(segments):
        sub = data[np.asarray(seg, dtype=np.int64)]
        n1[g] = (sub == 1).sum(0)
        n0[g] = (sub == 0).sum(0)
    return n1, n0


def check_counts(got, want, what=''):
    for name, g, w in zip(('n1', 'n0'), got, want):
        assert g.dtype == np.int32 and g.shape == w.shape, (what, name)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (f'{what}: {name}: {len(bad)} wrong counts, '
            f'the first at segment {bad[0][0]}, mutation {bad[0][1]}: '
            f'{g[tuple(bad[0])]} for {w[tuple(bad[0])]}')


@contextlib.contextmanager
def _knobs(monkeypatch, ctx, knobs):
    with monkeypatch.context() as mp:
        for k in KNOBS:
            mp.delenv(k, raising=False)
        for k, v in knobs.items():
            mp.setenv(k, str(v))
        ctx.reload_options()
        try:
            yield
        finally:
            mp.undo()
            ctx.reload_options()


@contextlib.contextmanager
def closing(ctx):
    try:
        yield ctx
    finally:
        ctx.close()


# ===================================================== A: matrix -> view 0
def creation_cases():
    """(N, M): every N of {1, 63, 64, 65, 129} and every M of {1, 31, 32, 33,
    63, 64, 65, 255, 256, 257, 513}."""
    return [(1, 1), (63, 31), (64, 32), (65, 33), (129, 63), (129, 64),
        (1, 65), (63, 255), (64, 256), (65, 257), (129, 513), (1, 513)]


def test_creation_cases_reach_their_edges():
    cases = creation_cases()
    assert {n for n, _ in cases} == {1, 63, 64, 65, 129}
    assert {m for _, m in cases} == {1, 31, 32, 33, 63, 64, 65, 255, 256,
        257, 513}
    words = {(m + 63) // 64 for _, m in cases}
    assert words == {1, 2, 4, 5, 9}
    # k_gather_transpose: 4 row words per workgroup, (W + 3) / 4 grid rows
    assert {(W, -W % 4) for W in words} == {(1, 3), (2, 2), (4, 0), (5, 3),
        (9, 3)}
    assert {(W + 3) // 4 for W in words} == {1, 2, 3}
    for N, M in cases:
        if M < SPECIAL_FROM:
            continue
        data = matrix(N, M)
        cols = [data[:, m] for m in range(M)]
        assert any((c == 1).all() for c in cols)
        assert any((c == 0).all() for c in cols)
        assert any(np.isnan(c).all() for c in cols)
        assert np.isnan(data[:-1, M - 1]).all() and data[-1, M - 1] == 1
        assert (as_codes(data) == 2).any() or N * M < 8


def play_creation(Ctx, N, M):
    data = matrix(N, M)
    codes = as_codes(data)
    want = ((data == 1).sum(1), (data == 0).sum(1))
    for route, kw in (('data', {'data': data.copy()}),
            ('codes', {'codes': codes}),
            ('planes', {'data': BitPlanes.from_data(data)})):
        with closing(Ctx(**kw)) as ctx:
            assert (ctx.N, ctx.M) == (N, M)
            check_view(ctx, 0, data, np.arange(N), f'{route} {N}x{M}')
            n1, n0 = ctx.cell_counts()
            assert np.array_equal(n1, want[0]) \
                and np.array_equal(n0, want[1]), route


def refusal_cases():
    """name -> the arguments of a creation that must be refused."""
    good = matrix(3, 65)
    both = BitPlanes.from_data(good).planes.copy()
    both[1, 0, 0] |= np.uint64(1 << 5)
    both[1, 0, 1] |= np.uint64(1 << 5)
    past = BitPlanes.from_data(good).planes.copy()
    past[2, 1, 1] |= np.uint64(1 << 1)          # mutation 65 of M = 65

    def codes_with(v):
        codes = as_codes(good)
        codes[2, 64] = v
        return codes

    def data_with(v):
        data = good.copy()
        data[0, 64] = v
        return data
    return {
        'planes with a bit in both words': {'data': BitPlanes(both, 65)},
        'planes with a bit past M': {'data': BitPlanes(past, 65)},
        'code 4': {'codes': codes_with(4)},
        'code -1': {'codes': codes_with(-1)},
        'float 0.5': {'data': data_with(0.5)},
        'float inf': {'data': data_with(np.inf)},
        'N = 0, data': {'data': np.empty((0, 65))},
        'N = 0, codes': {'codes': np.empty((0, 65), dtype=np.int8)},
        'M = 0, data': {'data': np.empty((3, 0))},
        'M = 0, codes': {'codes': np.empty((3, 0), dtype=np.int8)}}


def play_refusals(Ctx):
    good = matrix(3, 65)
    for name, kw in refusal_cases().items():
        with pytest.raises(RuntimeError):
            Ctx(**kw)
            pytest.fail(f'{name}: not refused')
        # ... and the next creation is none the worse for it
        with closing(Ctx(data=good.copy())) as ctx:
            check_view(ctx, 0, good, np.arange(3), f'after {name}')


def test_creation_on_the_host():
    for N, M in creation_cases():
        play_creation(FakeContext, N, M)
    play_refusals(FakeContext)


@pytest.mark.gpu
@pytest.mark.parametrize('N,M', creation_cases())
def test_creation_routes_agree_bit_for_bit(N, M):
    play_creation(_lib.Context, N, M)


@pytest.mark.gpu
def test_creation_refusals():
    play_refusals(_lib.Context)


# ======================================================= B: gathered views
ViewCase = collections.namedtuple('ViewCase', 'name cells route zero_copy')
VIEW_SHAPES = ((200, 257), (130, 64), (130, 256))


def view_cases(N):
    rng = np.random.RandomState(N)
    out = []
    for n in (0, 1, 63, 64, 65, 127, 128, 129):
        out.append(ViewCase(f'n={n}', rng.randint(0, N, n),
            'pinned' if n else 'empty', 1))
    out.append(ViewCase('one cell 70 times', np.full(70, N - 1), 'pinned', 1))
    out.append(ViewCase('reversed', np.arange(N)[::-1], 'pinned', 1))
    out.append(ViewCase('permutation', rng.permutation(N), 'pinned', 1))
    out.append(ViewCase('2N+1, in place', rng.randint(0, N, 2 * N + 1),
        'arena', 1))
    out.append(ViewCase('2N+1, copied', rng.randint(0, N, 2 * N + 1),
        'copied', 0))
    return out


def limit_view_cases():
    """On a 100 x 70 context: lists at the in-place limit of the arena."""
    rng = np.random.RandomState(5)
    n = ZC_IN_MAX // 8
    return [ViewCase('ZC_IN_MAX / 8', rng.randint(0, 100, n), 'arena', 1),
        ViewCase('ZC_IN_MAX / 8 + 1', rng.randint(0, 100, n + 1), 'copied',
            1)]


def test_view_cases_reach_their_routes():
    for N, _ in VIEW_SHAPES:
        cases = view_cases(N)
        assert {c.cells.size for c in cases} >= {0, 1, 63, 64, 65, 127, 128,
            129, 70, N, 2 * N + 1}
        for c in cases:
            assert view_route(N, c.cells.size, c.zero_copy) == c.route, c.name
        assert {c.route for c in cases} == {'empty', 'pinned', 'arena',
            'copied'}
    lo, hi = limit_view_cases()
    assert lo.cells.size * 8 == ZC_IN_MAX and hi.cells.size == \
        lo.cells.size + 1
    for c in (lo, hi):
        assert view_route(100, c.cells.size, c.zero_copy) == c.route


def play_views(Ctx, monkeypatch, N, M, cases):
    data = matrix(N, M)
    with closing(Ctx(data=data.copy())) as ctx:
        for i, c in enumerate(cases):
            view = 1 + i % (MAX_VIEWS - 1)
            with _knobs(monkeypatch, ctx, {'BNPC_ZERO_COPY': c.zero_copy}):
                assert ctx.view_set(view, c.cells) == c.cells.size
                check_view(ctx, view, data, c.cells, c.name)
        check_view(ctx, 0, data, np.arange(N), 'identity, afterwards')


def play_view_slots(Ctx):
    """Every view holds its own list at once; refusals leave a view as it
    was; one view shrinks and grows."""
    N, M = 130, 64
    data = matrix(N, M)
    rng = np.random.RandomState(11)
    lists = {v: rng.randint(0, N, n) for v, n in
        zip(range(1, MAX_VIEWS), (1, 63, 64, 65, 129, 70))}
    assert len(lists) == MAX_VIEWS - 1
    with closing(Ctx(data=data.copy())) as ctx:
        for v, cells in lists.items():
            ctx.view_set(v, cells)
        for v, cells in lists.items():
            check_view(ctx, v, data, cells, f'view {v} of all at once')
        for view in (0, MAX_VIEWS, -1):
            with pytest.raises(RuntimeError):
                ctx.view_set(view, [0, 1])
        for bad in (N, -1):
            cells = lists[3].copy()
            cells[-1] = bad
            with pytest.raises(RuntimeError):
                ctx.view_set(3, cells)
            check_view(ctx, 3, data, lists[3], f'view 3 after a list with '
                f'{bad}')
        check_view(ctx, 0, data, np.arange(N), 'identity after refusals')
        for n in (129, 65, 1, 128):
            cells = rng.randint(0, N, n)
            ctx.view_set(2, cells)
            check_view(ctx, 2, data, cells, f'view 2 resized to {n}')
        for v in (1, 4, 6):
            check_view(ctx, v, data, lists[v], f'view {v}, untouched')


def play_back_to_back(Ctx):
    """Two views set with nothing between them, each a full permutation (the
    second list is written into the pinned buffer the first gather reads:
    this catches the loss of its event guard only when the timing falls that
    way, and costs nothing)."""
    N, M = 20000, 65
    data = matrix(N, M)
    rng = np.random.RandomState(3)
    p1, p2 = rng.permutation(N), rng.permutation(N)
    assert view_route(N, N) == 'pinned'
    with closing(Ctx(data=data.copy())) as ctx:
        ctx.view_set(1, p1)
        ctx.view_set(2, p2)
        check_view(ctx, 1, data, p1, 'first of two back to back')
        check_view(ctx, 2, data, p2, 'second of two back to back')


def test_views_on_the_host(monkeypatch):
    for N, M in VIEW_SHAPES:
        play_views(FakeContext, monkeypatch, N, M, view_cases(N))
    play_views(FakeContext, monkeypatch, 100, 70, limit_view_cases())
    play_view_slots(FakeContext)
    play_back_to_back(FakeContext)


@pytest.mark.gpu
@pytest.mark.parametrize('N,M', VIEW_SHAPES)
def test_views_gather_every_list(monkeypatch, N, M):
    play_views(_lib.Context, monkeypatch, N, M, view_cases(N))


@pytest.mark.gpu
def test_views_at_the_in_place_limit(monkeypatch):
    play_views(_lib.Context, monkeypatch, 100, 70, limit_view_cases())


@pytest.mark.gpu
def test_view_slots_refusals_and_resizing():
    play_view_slots(_lib.Context)


@pytest.mark.gpu
def test_two_views_back_to_back():
    play_back_to_back(_lib.Context)


# ============================================ C: k_colcounts (cell lists)
SEG_SIZES = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 97)
COUNT_MS = (1, 255, 256, 257, 513)


def segment_calls(N=70):
    """name -> the segments of one call: the sizes 0 .. 97 with the empty
    segment first, in the middle and last; cells drawn with repetition."""
    rng = np.random.RandomState(17)

    def draw(sizes):
        return [rng.randint(0, N, s) for s in sizes]
    half = len(SEG_SIZES) // 2
    return {'empty first': draw((0,) + SEG_SIZES),
        'empty in the middle': draw(SEG_SIZES[:half] + (0,)
            + SEG_SIZES[half:]),
        'empty last': draw(SEG_SIZES + (0,)),
        'G = 14': draw((0,) + SEG_SIZES + (0,)),
        'G = 1': draw((5,))}


@functools.lru_cache(maxsize=None)
def second_launch_case():
    """(data, segments, expected counts) of a call of more than 65 535
    chunks on a 70 x 3 context."""
    data = matrix(70, 3)
    rng = np.random.RandomState(23)
    sizes = [1] * (MAXY - 1) + [100] + [1] * 2
    cells = rng.randint(0, 70, sum(sizes))
    segments = np.split(cells, np.cumsum(sizes)[:-1])
    return data, segments, want_counts(data, segments)


def test_segment_cases_reach_their_edges():
    calls = segment_calls()
    for name, at in (('empty first', 0), ('empty in the middle', 6),
            ('empty last', 12)):
        sizes = [len(s) for s in calls[name]]
        assert sizes[at] == 0 and sorted(sizes) == [0] + list(SEG_SIZES)
        lengths = [e - b for b, e, _ in chunking(sizes)]
        # the 32-cell chunk edge: a whole chunk alone, and with 1 more cell
        assert sizes.count(CH) == 1 and sizes.count(CH + 1) == 1
        assert max(lengths) == CH
        # the 4-wide loop: no trip, whole trips only, every remainder
        assert {n % 4 for n in lengths} == {0, 1, 2, 3}
        assert {1, 2, 3, 4, 5, 31, 32} <= set(lengths)
    assert len(calls['G = 14']) == 14 and len(calls['G = 1']) == 1
    # a cell twice in a segment, a cell in two segments
    segs = calls['empty first']
    assert any(np.unique(s).size < s.size for s in segs)
    assert np.intersect1d(segs[-1], segs[-2]).size
    # the second launch: the 100-cell segment's chunks lie on both sides
    _, segments, _ = second_launch_case()
    chunks = chunking([len(s) for s in segments])
    assert len(chunks) == MAXY + 5 == 65540
    big = [i for i, (_, _, g) in enumerate(chunks) if g == MAXY - 1]
    assert big == [MAXY - 1, MAXY, MAXY + 1, MAXY + 2]
    assert [chunks[i][1] - chunks[i][0] for i in big] == [32, 32, 32, 4]


def play_segments(Ctx, M):
    data = matrix(70, M)
    calls = segment_calls()
    with closing(Ctx(data=data.copy())) as ctx:
        n1, n0 = ctx.colcounts([])
        assert n1.shape == n0.shape == (0, M)
        for name in ('empty first', 'empty in the middle', 'empty last'):
            want = want_counts(data, calls[name])
            check_counts(ctx.colcounts(calls[name]), want, name)
            # zero-fill per call: the same call again, the same integers
            check_counts(ctx.colcounts(calls[name]), want, name + ', again')
        for name in ('G = 14', 'G = 1'):
            check_counts(ctx.colcounts(calls[name]),
                want_counts(data, calls[name]), name)


def play_second_launch(Ctx):
    data, segments, want = second_launch_case()
    with closing(Ctx(data=data.copy())) as ctx:
        check_counts(ctx.colcounts(segments), want, 'second launch')


def label_cases(N=70):
    """name -> (assignment, ids) for colcounts_by_label."""
    rng = np.random.RandomState(29)
    sparse = np.array([40, 7, 1000, 3])
    return {'K = 1': (np.full(N, 5), np.array([5])),
        'K = N': (rng.permutation(N) * 3, rng.permutation(N) * 3),
        'sparse ids, one unused': (sparse[rng.choice([0, 1, 3], N)], sparse)}


def label_refusals(N=70):
    ok = np.arange(N) % 3
    out = {'duplicate id': (ok, [0, 1, 2, 1]),
        'negative id': (ok, [0, 1, 2, -4]),
        'assignment outside ids': (ok, [0, 1]),
        'assignment above every id': (ok + 1, [0, 1, 2]),
        'K = 0': (ok, [])}
    return out


def check_by_label(ctx, data, assignment, ids, what):
    segments = [np.flatnonzero(assignment == i) for i in ids]
    check_counts(ctx.colcounts_by_label(assignment, ids),
        want_counts(data, segments), what)


def play_labels(Ctx, monkeypatch):
    N, M = 70, 257
    data = matrix(N, M)
    with closing(Ctx(data=data.copy())) as ctx, \
            _knobs(monkeypatch, ctx, {'BNPC_MASK_COUNTS_MAX': 0}):
        for name, (assignment, ids) in label_cases().items():
            assert label_route(len(ids), N, 0) == 'cells'
            check_by_label(ctx, data, assignment, ids, name)
        name, (assignment, ids) = 'sparse ids, one unused', \
            label_cases()['sparse ids, one unused']
        n1, n0 = ctx.colcounts_by_label(assignment, ids)
        assert not n1[2].any() and not n0[2].any()
        for bad, (a, i) in label_refusals().items():
            with pytest.raises(RuntimeError):
                ctx.colcounts_by_label(a, i)
                pytest.fail(f'{bad}: not refused')
            check_by_label(ctx, data, assignment, ids, f'after {bad}')


def test_counts_over_cell_lists_on_the_host(monkeypatch):
    for M in COUNT_MS:
        play_segments(FakeContext, M)
    play_second_launch(FakeContext)
    play_labels(FakeContext, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize('M', COUNT_MS)
def test_colcounts_chunks_and_zero_fill(M):
    play_segments(_lib.Context, M)


@pytest.mark.gpu
def test_colcounts_second_launch():
    play_second_launch(_lib.Context)


@pytest.mark.gpu
def test_colcounts_by_label_over_cell_lists(monkeypatch):
    play_labels(_lib.Context, monkeypatch)


# ================================================== D: k_counts_masks
MASK_N = 300
MASK_MS = (1, 63, 64, 65, 129)
MASK_VIEWS = (1, 64, 65, 192, 193, 256, 257, 320)
MASK_GS = (1, 7, 8, 9, 16, 17)
FLOOR_VIEWS = (16320, 16384, 16385)


def draw_labels(rng, n, G):
    """n labels of -1 .. G - 1, every one of them where n allows."""
    labels = rng.randint(-1, G, n)
    head = rng.permutation(np.arange(-1, G))[:n]
    labels[:head.size] = head
    return labels


def view_count_segments(cells, labels, G):
    return [cells[labels == g] for g in range(G)]


def check_view_counts(ctx, data, view, cells, labels, G, what):
    check_counts(ctx.view_counts(view, labels, G),
        want_counts(data, view_count_segments(cells, labels, G)), what)


def test_mask_cases_reach_their_edges():
    # 1 .. 5 blocks against the 4 waves of a workgroup
    assert sorted({blocks(n) for n in MASK_VIEWS}) == [1, 2, 3, 4, 5]
    assert {n % 64 for n in MASK_VIEWS} >= {0, 1}
    # workgroups of 8 segments: one partly filled, one full, a second one
    # holding 1 segment, two full, a third holding 1
    assert [(-(-G // CM_SEG), G % CM_SEG) for G in MASK_GS] == [(1, 1),
        (1, 7), (1, 0), (2, 1), (2, 0), (3, 1)]
    # either side of the LDS floor
    assert [blocks(n) for n in FLOOR_VIEWS] == [255, 256, 257]
    assert [masks_lds(n) for n in FLOOR_VIEWS] == [(RED_BYTES, 'floor'),
        (RED_BYTES, 'words'), (RED_BYTES + 64, 'words')]
    assert all(view_route(MASK_N, n) == 'arena' for n in FLOOR_VIEWS)
    # the membership words at the in-place limit
    assert 512 * blocks(4096) * 8 == ZC_IN_MAX
    assert member_route(512, 4096) == 'arena'
    assert member_route(513, 4096) == 'heap'
    assert member_route(512, 4096, zero_copy=0) == 'heap'
    assert label_route(64, MASK_N) == 'masks'
    assert label_route(65, MASK_N) == 'cells'
    assert label_route(64, MASK_N, 0) == 'cells'


def play_mask_counts(Ctx, monkeypatch, M):
    data = matrix(MASK_N, M)
    rng = np.random.RandomState(31 + M)
    with closing(Ctx(data=data.copy())) as ctx:
        for zero_copy in (1, 0):
            with _knobs(monkeypatch, ctx, {'BNPC_ZERO_COPY': zero_copy}):
                for n in MASK_VIEWS:
                    cells = rng.randint(0, MASK_N, n)
                    ctx.view_set(1, cells)
                    for G in MASK_GS:
                        check_view_counts(ctx, data, 1, cells,
                            draw_labels(rng, n, G), G,
                            f'n={n} G={G} zero_copy={zero_copy}')
                # the identity view, too
                check_view_counts(ctx, data, 0, np.arange(MASK_N),
                    draw_labels(rng, MASK_N, 9), 9, 'identity view')


def play_mask_edges(Ctx, monkeypatch):
    M = 65
    data = matrix(MASK_N, M)
    rng = np.random.RandomState(37)
    with closing(Ctx(data=data.copy())) as ctx:
        # an empty view: zeros of shape (G, M)
        n1, n0 = ctx.view_counts(3, np.zeros(0, dtype=np.int64), 5)
        assert n1.shape == n0.shape == (5, M) and n1.dtype == np.int32
        assert not n1.any() and not n0.any()
        for zero_copy in (1, 0):
            with _knobs(monkeypatch, ctx, {'BNPC_ZERO_COPY': zero_copy}):
                for n in FLOOR_VIEWS:
                    cells = rng.randint(0, MASK_N, n)
                    ctx.view_set(1, cells)
                    check_view_counts(ctx, data, 1, cells,
                        draw_labels(rng, n, 9), 9,
                        f'{blocks(n)} blocks, zero_copy={zero_copy}')
                # G = 17 fills the buffers; then no slot belongs anywhere
                cells = rng.randint(0, MASK_N, 257)
                ctx.view_set(2, cells)
                check_view_counts(ctx, data, 2, cells,
                    draw_labels(rng, 257, 17), 17, 'G = 17')
                n1, n0 = ctx.view_counts(2, np.full(257, -1), 17)
                assert n1.shape == n0.shape == (17, M)
                assert not n1.any() and not n0.any(), 'labels all -1'
                # the membership words at the in-place limit and past it
                cells = rng.randint(0, MASK_N, 4096)
                ctx.view_set(4, cells)
                for G in (512, 513):
                    check_view_counts(ctx, data, 4, cells,
                        draw_labels(rng, 4096, G), G,
                        f'G={G}: words {member_route(G, 4096, zero_copy)}')
        # the bounds of G, and a label equal to G
        cells = rng.randint(0, MASK_N, 65)
        ctx.view_set(5, cells)
        labels = draw_labels(rng, 65, 7)
        check_view_counts(ctx, data, 5, cells, rng.randint(-1, G_MAX, 65),
            G_MAX, f'G = {G_MAX}')
        with pytest.raises(RuntimeError, match='out of range'):
            ctx.view_counts(5, labels, G_MAX + 1)
        check_view_counts(ctx, data, 5, cells, labels, 7, 'after G too large')
        bad = labels.copy()
        bad[64] = 7
        with pytest.raises(RuntimeError, match='out of range'):
            ctx.view_counts(5, bad, 7)
        check_view_counts(ctx, data, 5, cells, labels, 7,
            'after a label equal to G')


def play_label_limit(Ctx, monkeypatch):
    """colcounts_by_label either side of BNPC_MASK_COUNTS_MAX: the masks and
    the cell lists give the same integers."""
    M = 129
    data = matrix(MASK_N, M)
    rng = np.random.RandomState(41)
    with closing(Ctx(data=data.copy())) as ctx:
        for K in (MASK_COUNTS_MAX, MASK_COUNTS_MAX + 1):
            ids = rng.permutation(2 * K)[:K]
            assignment = ids[draw_labels(rng, MASK_N, K).clip(0)]
            got = {}
            for limit in (None, 0):
                knobs = {} if limit is None else \
                    {'BNPC_MASK_COUNTS_MAX': limit}
                with _knobs(monkeypatch, ctx, knobs):
                    got[limit] = ctx.colcounts_by_label(assignment, ids)
                    check_by_label(ctx, data, assignment, ids,
                        f'K={K}, limit {limit}')
            check_counts(got[None], got[0], f'K={K}: masks against cells')


def test_counts_from_masks_on_the_host(monkeypatch):
    for M in MASK_MS:
        play_mask_counts(FakeContext, monkeypatch, M)
    play_mask_edges(FakeContext, monkeypatch)
    play_label_limit(FakeContext, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize('M', MASK_MS)
def test_view_counts_blocks_against_waves(monkeypatch, M):
    play_mask_counts(_lib.Context, monkeypatch, M)


@pytest.mark.gpu
def test_view_counts_floor_limit_and_bounds(monkeypatch):
    play_mask_edges(_lib.Context, monkeypatch)


@pytest.mark.gpu
def test_colcounts_by_label_either_side_of_the_mask_limit(monkeypatch):
    play_label_limit(_lib.Context, monkeypatch)
