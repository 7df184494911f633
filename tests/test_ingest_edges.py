"""The host side of the packed matrix at its edges: the packer and unpacker of
the bit planes (bnpc_pack_codes, bnpc_unpack_codes) against a NumPy packer
written here, and the three readers of the text format - io.load_codes_native
(bnpc_parse_matrix), io.load_data and bitplanes.load_matrix - against
pandas.read_csv, the reader the reference's loader rests on.  CPU only;
everything is compared exactly.

Group E: N and M each in {1, 63, 64, 65, 129}; the input contiguous, as a
transposed view (the 64 x 64 tile path of the packer) and as a strided slice;
bits past M, code 2, bad codes by name on both paths; unpacking with no list,
repeats, an index out of range and an empty list.

Group F: every case declares its separator, header row and index column and
hands them to read_csv itself (3 -> NaN, 2 -> 1); that io._sniff_layout finds
the declared layout is asserted apart.  The three readers, in both
orientations, first run and cached run, give the pandas matrix - or, where
read_csv refuses the file, all three refuse it.  What an all-missing row is
matters: it is a cell (transposed: a mutation) the chain then carries, and the
bit-plane cache is written from the native scan, so the readers must agree on
it with each other and with the reference.
"""
import collections
import os

import numpy as np
import pytest

from bnpc_amd import bitplanes as B
from bnpc_amd import io as bio

SIZES = (1, 63, 64, 65, 129)


# ======================================================== E: pack / unpack
def np_pack(codes):
    """(N, M) codes 0 | 1 | 2 | 3 -> (N, W, 2) uint64 {ones, zeros}."""
    codes = np.asarray(codes)
    N, M = codes.shape
    W = (M + 63) // 64
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    planes = np.zeros((N, W, 2), dtype=np.uint64)
    for p, hit in enumerate(((codes == 1) | (codes == 2), codes == 0)):
        bits = np.zeros((N, W * 64), dtype=np.uint64)
        bits[:, :M] = hit
        planes[:, :, p] = (bits.reshape(N, W, 64) * weights).sum(axis=2,
            dtype=np.uint64)
    return planes


def codes_of(N, M):
    rng = np.random.RandomState(100 * N + M)
    return rng.choice([0, 1, 2, 3], size=(N, M), p=[.4, .3, .1, .2]) \
        .astype(np.int8)


def layouts(codes):
    """name -> an array equal to `codes` with its own strides."""
    N, M = codes.shape
    big = np.random.RandomState(1).choice([0, 1, 2, 3],
        size=(2 * N, 3 * M)).astype(np.int8)
    big[::2, ::3] = codes
    return {'contiguous': np.ascontiguousarray(codes),
        'transposed': np.ascontiguousarray(codes.T).T,
        'strided': big[::2, ::3]}


def takes_tile_path(arr):
    """bnpc_pack_codes: row_stride == 1 && col_stride != 1"""
    return arr.strides[0] == 1 and arr.strides[1] != 1


def test_numpy_packer_on_a_case_worked_by_hand():
    codes = np.full((2, 65), 3, dtype=np.int8)
    codes[0, 0], codes[0, 63], codes[0, 64], codes[1, 1] = 1, 0, 2, 0
    planes = np_pack(codes)
    assert planes.shape == (2, 2, 2)
    assert planes[0].tolist() == [[1, 1 << 63], [1, 0]]
    assert planes[1].tolist() == [[0, 2], [0, 0]]


@pytest.mark.parametrize('N', SIZES)
@pytest.mark.parametrize('M', SIZES)
def test_pack_and_unpack_against_numpy(N, M):
    codes = codes_of(N, M)
    want = np_pack(codes)
    assert (codes == 2).any() or N * M < 8
    tail = M - 64 * ((M - 1) // 64)
    for name, arr in layouts(codes).items():
        assert np.array_equal(arr, codes)
        if name == 'transposed':
            # (the stride of an axis of length 1 is NumPy's to choose)
            assert takes_tile_path(arr) or 1 in (N, M)
        else:
            assert not takes_tile_path(arr)
        got = B.BitPlanes.from_codes(arr)
        assert got.shape == (N, M) and got.planes.shape == want.shape
        assert np.array_equal(got.planes, want), name
        # bits past M are clear, no bit stands in both planes
        if tail < 64:
            assert not (got.planes[:, -1, :] >> np.uint64(tail)).any(), name
        assert not (got.planes[:, :, 0] & got.planes[:, :, 1]).any()
    # ... and back: 2 has become 1
    back = np.where(codes == 2, 1, codes)
    planes = B.BitPlanes(want, M)
    assert np.array_equal(planes.codes(), back)
    rng = np.random.RandomState(N + M)
    cells = rng.randint(0, N, 2 * N + 3)            # with repeats
    got = planes.codes(cells)
    assert got.dtype == np.int8 and np.array_equal(got, back[cells])
    assert planes.codes(np.zeros(0, dtype=np.int64)).shape == (0, M)
    for bad in (N, -1):
        with pytest.raises(RuntimeError, match='out of range'):
            planes.codes(np.array([0, bad]))


@pytest.mark.parametrize('N,M', [(1, 1), (65, 129), (129, 65), (64, 64)])
def test_a_bad_code_is_refused_by_name_on_both_paths(N, M):
    for i, m in {(0, 0), (N - 1, M - 1), (N // 2, M - 1), (N - 1, M // 2)}:
        for v in (4, -1, 127):
            codes = codes_of(N, M)
            codes[i, m] = v
            for name, arr in layouts(codes).items():
                with pytest.raises(RuntimeError,
                        match=rf'codes\[{i},{m}\] = {v} is not'):
                    B.BitPlanes.from_codes(arr)
                    pytest.fail(f'{name}: not refused')


# ==================================================== F: the text scanner
Case = collections.namedtuple('Case', 'name text sep header index')
T = '\t'


def _table(sep, header, index, eol='\n', final=True, as_float=False):
    rng = np.random.RandomState(7)
    mat = rng.choice([0, 1, 2, 3], size=(7, 5), p=[.4, .3, .1, .2])
    fmt = (lambda v: f'{float(v):.1f}') if as_float else str
    lines = []
    if header:
        lines.append(sep.join((['id'] if index else [])
            + [f'c{j}' for j in range(mat.shape[1])]))
    for i, r in enumerate(mat):
        lines.append(sep.join(([f'm{i}'] if index else [])
            + [fmt(v) for v in r]))
    return eol.join(lines) + (eol if final else '')


def scanner_cases():
    out = [
        # the three disagreements this file was written for
        Case('tab file, last line a lone tab', '0\t1\n1\t0\n\t\n', T, 0, 0),
        Case('empty line inside the body', '0\t1\n\n1\t0\n', T, 0, 0),
        Case('comma file, last line a lone tab', '0,1\n1,0\n\t\n', ',', 0, 0)]
    for sep, tag in ((' ', 'space'), (T, 'tab'), (',', 'comma')):
        for header, index in ((0, 0), (1, 0), (1, 1)):
            for eol, final in (('\n', True), ('\r\n', True), ('\n', False),
                    ('\r\n', False)):
                out.append(Case(f'{tag} table, header {header}, index {index}'
                    f', {eol!r}, final newline {final}',
                    _table(sep, header, index, eol, final), sep, header,
                    index))
        out.append(Case(f'{tag} table of floats',
            _table(sep, 1, 1, as_float=True), sep, 1, 1))
    out += [
        # trailing lines: empty, spaces only, separators
        Case('trailing empty lines', '0,1\n1,0\n\n\n', ',', 0, 0),
        Case('trailing empty lines, CRLF', '0 1\r\n1 0\r\n\r\n', ' ', 0, 0),
        Case('trailing line of spaces, comma', '0,1\n1,0\n   \n', ',', 0, 0),
        Case('trailing line of spaces, tab', '0\t1\n1\t0\n   \n', T, 0, 0),
        Case('trailing line of spaces, no newline', '0,1\n1,0\n  ', ',', 0,
            0),
        Case('trailing line of separators, comma', '0,1\n1,0\n,\n', ',', 0,
            0),
        Case('trailing line of one separator, space', '0 1\n1 0\n \n', ' ',
            0, 0),
        Case('trailing line of too many separators, space',
            '0 1\n1 0\n   \n', ' ', 0, 0),
        Case('trailing line of separators under names',
            'id\ta\tb\nr0\t0\t1\nr1\t1\t0\n\t\t\n', T, 1, 1),
        # blank lines inside
        Case('empty line inside, CRLF', '0,1\r\n\r\n1,0\r\n', ',', 0, 0),
        Case('empty line inside, space', '0 1\n\n1 0\n', ' ', 0, 0),
        Case('empty line inside, one column', '0\n1\n\n1\n', ' ', 0, 0),
        Case('empty line inside under names',
            'id\ta\tb\r\nr0\t0\t1\r\n\r\nr1\t1\t0\r\n', T, 1, 1),
        Case('line of spaces inside, comma', '0,1\n  \n1,0\n', ',', 0, 0),
        Case('line of a tab inside, space', '0 1\n\t\n1 0\n', ' ', 0, 0),
        Case('line of separators inside', '0,1\n,\n1,0\n', ',', 0, 0),
        Case('empty line after the header', 'a,b\n\n0,1\n1,0\n', ',', 1, 0),
        Case('empty first line', '\n0,1\n1,0\n', ',', 0, 0),
        Case('blank lines before the header', '\n  \nid\ta\tb\nr0\t0\t1\n', T,
            1, 1),
        # ragged rows
        Case('short rows, comma', '0,1,1\n1\n1,0\n', ',', 0, 0),
        Case('short rows, tab', '0\t1\t1\n1\n1\t0\n', T, 0, 0),
        Case('short rows under names', 'id,a,b\nr0,0,1\nr1,1\nr2\n', ',', 1,
            1),
        Case('a longer row later', '0,1\n1,0,1\n', ',', 0, 0),
        Case('a longer row later under names', 'id,a,b\nr0,0,1\nr1,1,0,1\n',
            ',', 1, 1),
        Case('a header of column names only', 'a,b\nr0,0,1\nr1,1,0\n', ',',
            1, 1),
        Case('a header of column names only, a longer row later',
            'a,b\nr0,0,1\nr1,1,0,1\n', ',', 1, 1),
        # spellings and fields
        Case('spellings', '1,1.0,2.0\n3.0,1e0,01\n0.0,00,0e0\n', ',', 0, 0),
        Case('empty fields, comma', '1,,0\n,1,\n0,0,1\n', ',', 0, 0),
        Case('empty fields, tab', '1\t\t0\n\t1\t\n0\t0\t1\n', T, 0, 0),
        Case('a doubled space', '0  1\n1  0\n', ' ', 0, 0),
        Case('spaces round the fields, comma', '0,1,1,1\n 1,0 ,1, 0 \n', ',',
            0, 0),
        Case('spaces round the fields, tab',
            '0\t1\t1\t1\n 1\t0 \t1\t 0 \n', T, 0, 0),
        Case('a trailing space, space', '0 1 \n1 0 \n', ' ', 0, 0),
        Case('a leading space, space', ' 0 1\n 1 0\n', ' ', 0, 0),
        # the scanner's token buffer held 63 characters
        Case('a number of 63 characters', '1,1.' + '0' * 61 + '\n0,1\n', ',',
            0, 0),
        Case('a number of 64 characters', '1,1.' + '0' * 62 + '\n0,1\n', ',',
            0, 0),
        Case('a number of 72 characters', '1,' + '0' * 71 + '1\n0,3\n', ',',
            0, 0),
        Case('a number of 72 characters, last in the file',
            '1\t0\n0\t2.' + '0' * 70, T, 0, 0),
        Case('no number', '0,1\n1,x\n', ',', 0, 0)]
    assert len({c.name for c in out}) == len(out)
    return out


def read_with_pandas(path, case):
    pd = pytest.importorskip('pandas')
    df = pd.read_csv(path, sep=case.sep, header=0 if case.header else None,
        index_col=0 if case.index else None)
    mat = df.to_numpy(dtype=np.float64).copy()
    mat[mat == 3] = np.nan
    mat[mat == 2] = 1
    if mat.size == 0:
        raise ValueError('no data')
    return mat


def test_the_cases_cover_what_they_are_meant_to():
    cases = scanner_cases()
    assert {c.sep for c in cases} == {' ', T, ','}
    assert {(c.header, c.index) for c in cases} == {(0, 0), (1, 0), (1, 1)}
    text = [c.text for c in cases]
    assert any('\r\n' in t for t in text)
    assert any(not t.endswith('\n') for t in text)
    for token in ('1.0', '2.0', '3.0', '1e0', '01'):
        assert any(token in t for t in text)
    assert any(len(tok) >= 64 for t in text for ln in t.split('\n')
        for tok in ln.replace(T, ',').split(','))


@pytest.mark.parametrize('case', scanner_cases(), ids=lambda c: c.name)
def test_sniffed_layout_is_the_declared_one(case):
    head = bio._sniff_head(case.text.split('\n'), case.name)
    assert bio._sniff_layout(head) == (case.sep, bool(case.header),
        bool(case.index))


@pytest.mark.parametrize('case', scanner_cases(), ids=lambda c: c.name)
def test_three_readers_against_read_csv(case, tmp_path):
    pd = pytest.importorskip('pandas')
    path = str(tmp_path / 'matrix.txt')
    with open(path, 'wb') as f:
        f.write(case.text.encode())
    side = path + B.SUFFIX
    readers = {
        'load_codes_native': lambda t: bio.codes_to_data(
            bio.load_codes_native(path, transpose=t)),
        'load_data': lambda t: bio.load_data(path, transpose=t),
        'load_matrix, first run': lambda t: np.asarray(
            B.load_matrix(path, transpose=t)),
        'load_matrix, cached run': lambda t: np.asarray(
            B.load_matrix(path, transpose=t))}
    try:
        want = read_with_pandas(path, case)
    except (pd.errors.ParserError, ValueError):
        want = None
    for transpose in (True, False):
        if os.path.exists(side):
            os.remove(side)
        for name, read in readers.items():
            if want is None:
                with pytest.raises((RuntimeError, ValueError)):
                    read(transpose)
                    pytest.fail(f'{name}: read_csv refuses this file')
                assert not os.path.exists(side)
                continue
            got = read(transpose)
            ref = want.T if transpose else want
            assert got.shape == ref.shape, (name, transpose, got, ref)
            assert np.array_equal(got, ref, equal_nan=True), (name,
                transpose, got, ref)
            if name == 'load_matrix, cached run':
                assert isinstance(B.load_matrix(path,
                    transpose=transpose).planes, np.memmap)


def test_the_golden_example_loads_as_before(golden_dir):
    path = os.path.join(golden_dir, 'example_data.csv')
    data = bio.load_data(path)
    assert data.shape == (100, 100) and np.isnan(data).sum() == 948
    assert (data == 1).sum() == 2445 and (data == 0).sum() == 6607
    assert np.array_equal(bio.codes_to_data(bio.load_codes_native(path)),
        data, equal_nan=True)
    assert np.array_equal(np.asarray(B.load_matrix(path, cache=False)), data,
        equal_nan=True)
    want = read_with_pandas(path, Case('golden', None, ' ', 0, 0))
    assert np.array_equal(data, want.T, equal_nan=True)
