"""GPU: the single-pass exclusive scan and the ordered index list of
bsa_scan.hip on their own, through their test entries (bsa_scan_excl,
bsa_flagged_list), against numpy.  Both are integer-exact, so
every comparison is np.array_equal with a numpy result, never with another run
of the device code.

The scan is a decoupled look-back over tiles: a tile's wave 0 reads the status
words of its 64 nearest predecessors per round and steps 64 tiles back while
none of them holds an inclusive prefix yet.  The sizes below are written in
the two tile sizes, so that the tile count -- and with it the window
arithmetic a size pins -- is visible:

  tiles <= 64       the window reaches tile 0 (lanes past it count as inclusive 0)
  tiles == 65       the last tile's first window is exactly tiles 63 .. 0
  tiles >= 66       a second round exists (top -= 64); >= 130: a third

Which predecessors are already inclusive when a tile looks back is the
hardware's choice and no test can pin it; a tile that finds an inclusive
prefix early takes fewer rounds than its distance allows.

The state a context carries from scan to scan (ticket base, epoch in the
status words, the status words of earlier and larger launches) is covered by
one fixed sequence of sizes on one context, alone and with a detect between
the scans.  The status buffer is allocated in units of 2 MiB (262144 words), so
after the first scan of a context it grows only above 262143 tiles: no size a
test can afford reaches that reset; the sequence covers the first-use reset
and every reuse under a new epoch."""
import ctypes

import numpy as np
import pytest

from bluesky_amd import _lib, statebased
from tests import util
from tests.test_gpu_k2_paths import HPZ, RPZ, TLA, fresh, oracle0, traffic

pytestmark = pytest.mark.gpu

# scan_excl's `small` rule (bsa_scan.hip): n <= 2^19 words run k_scan_excl<512, 4>, tiles of T words;
# larger n run k_scan_excl<1024, 8>, tiles of U words
T = 2048
U = 8192
SMALL_MAX = 1 << 19
WINDOW = 64     # predecessor tiles per look-back round

ONE_TILE_AND_EDGES = ['1', '2', '63', '64', '65', '511', '512', '2047', '2048', '2049', '2*T', '2*T+1']
SMALL_ROUNDS = ['64*T', '64*T+1', '65*T+1', '128*T+1', '129*T+7', '2**19']
BIG = ['2**19+1', '65*U+1', '129*U+5']
SEQUENCE = ['2049', '65*T+1', '5', '129*T+7', '2**19+1', '64', '129*U+5', '4097']


def size(expr):
    return int(eval(expr, {'T': T, 'U': U}))


def tile_words(n):
    return T if n <= SMALL_MAX else U


def tiles(n):
    return -(-n // tile_words(n))


def scan_ref(x):
    """The exclusive sum in 64 bits, cut to 32 (the leading zero as uint64: numpy joins an int list
    and a uint64 array as float64)."""
    s = np.concatenate((np.zeros(1, np.uint64), np.cumsum(x.astype(np.uint64))[:-1])) & np.uint64(0xffffffff)
    return s.astype(np.uint32)


def check_scan(c, x, what):
    got = c.scan_excl(x)
    exp = scan_ref(x)
    assert got.dtype == np.uint32 and got.shape == exp.shape, what
    if not np.array_equal(got, exp):
        i = int(np.flatnonzero(got != exp)[0])
        pytest.fail('%s, n = %d: first difference at index %d (tile %d of %d-word tiles, tile %d of %d-word '
                    'tiles): got %d, expected %d; %d words differ'
                    % (what, len(x), i, i // T, T, i // U, U, got[i], exp[i], int((got != exp).sum())))


def single_one_positions(n):
    """Index 0, the last index of a tile and the first of the next (the first and the last tile
    edge inside n), and n - 1."""
    t = tile_words(n)
    last_edge = (n - 1) // t * t
    return sorted({p for p in (0, t - 1, t, last_edge - 1, last_edge, n - 1) if 0 <= p < n})


def scan_inputs(n, seed):
    rng = np.random.default_rng(seed)
    yield 'zeros', np.zeros(n, np.uint32)
    yield 'ones', np.ones(n, np.uint32)
    for p in single_one_positions(n):
        x = np.zeros(n, np.uint32)
        x[p] = 1
        yield 'single 1 at %d' % p, x
    # sums that wrap 32 bits many times: the inclusive status words carry wrapped values
    yield 'random words', rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    yield 'random counts 0..8', rng.integers(0, 9, n).astype(np.uint32)


def test_sizes_pin_the_paths_they_name():
    """The arithmetic the size lists rest on."""
    assert all(tiles(size(e)) == 1 for e in ONE_TILE_AND_EDGES[:9])
    assert [tiles(size(e)) for e in ONE_TILE_AND_EDGES[9:]] == [2, 2, 3]
    assert all(size(e) <= SMALL_MAX for e in SMALL_ROUNDS) and all(size(e) > SMALL_MAX for e in BIG)
    # the last tile has tiles - 1 predecessors: 63 (one window, past tile 0), 64 (one window exactly), then 2, 3 rounds
    assert [tiles(size(e)) for e in SMALL_ROUNDS] == [WINDOW, WINDOW + 1, WINDOW + 2, 2 * WINDOW + 1, 2 * WINDOW + 2, 256]
    assert [tiles(size(e)) for e in BIG] == [WINDOW + 1, WINDOW + 2, 2 * WINDOW + 2]
    assert size('129*U+5') * 4 < 4.5e6    # the largest transfer, bytes
    assert single_one_positions(2 * T + 1) == [0, T - 1, T, 2 * T - 1, 2 * T]
    assert single_one_positions(64) == [0, 63] and single_one_positions(1) == [0]
    # the list scans its wave counts and one zero word: T words at 64 (T - 1) flags, T + 1 at one more
    assert [(n + 63) // 64 + 1 for n in (64 * (T - 1), 64 * (T - 1) + 1)] == [T, T + 1]


@pytest.mark.parametrize('expr', ONE_TILE_AND_EDGES + SMALL_ROUNDS + BIG)
def test_scan_matches_numpy(expr):
    """Every input at one size, on a context of its own: the first call finds the scan state
    unallocated, the later ones reuse its status words under new epochs."""
    n = size(expr)
    c = _lib.Context(0)
    try:
        for what, x in scan_inputs(n, seed=n):
            check_scan(c, x, '%s, %s' % (expr, what))
    finally:
        c.close()


def sequence_input(k, n):
    return np.random.default_rng(1000 + k).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def test_scan_state_across_calls():
    """SEQUENCE on one context: status words written by an earlier, larger launch are read under a
    new epoch, and both kernels alternate on one ticket counter."""
    c = _lib.Context(0)
    try:
        for k, expr in enumerate(SEQUENCE):
            check_scan(c, sequence_input(k, size(expr)), 'call %d, %s' % (k, expr))
    finally:
        c.close()


def test_scan_state_shared_with_a_detect():
    """The same sequence with the product's own scan between the calls: a detect at bucket width 0
    (clique case h, 65 pairs per row: scan + scatter) draws tickets and epochs from the same
    context, and its pair list stays the oracle's."""
    t, exp = traffic('h'), oracle0('h')
    with fresh(0) as c:
        for k, expr in enumerate(SEQUENCE):
            check_scan(c, sequence_input(k, size(expr)), 'call %d, %s' % (k, expr))
            got = statebased.detect_indices(t, t, RPZ, HPZ, TLA, ctx=c)
            util.assert_detect_equal(got, exp, RPZ, TLA)
        check_scan(c, sequence_input(99, size('65*T+1')), 'after the last detect')


def test_scan_entry_edges():
    c = _lib.Context(0)
    try:
        assert c.scan_excl(np.zeros(0, np.uint32)).shape == (0,)
        assert c.lib.bsa_scan_excl(c.h, 0, None, None) == 0
        one = np.ones(1, np.uint32)
        for n, a, b, msg in ((-1, one, one, 'bad n'), ((1 << 31), one, one, 'bad n'), (1, None, one, 'NULL'),
                             (1, one, None, 'NULL')):
            st = c.lib.bsa_scan_excl(c.h, n, _lib.ptr(a, _lib._c_u32p), _lib.ptr(b, _lib._c_u32p))
            assert st != 0 and msg in c.lib.bsa_last_error(c.h).decode(), (n, msg)
        check_scan(c, np.arange(5, dtype=np.uint32), 'after the refused calls')
    finally:
        c.close()


# ---------------------------------------------------------------- ordered index list
# 131008 = 64 * (T - 1): T - 1 wave counts and the zero word, one scan tile; one more aircraft: two tiles
LIST_SIZES = [1, 63, 64, 65, 127, 128, 255, 256, 257, 4095, 4096, 4097, 64 * (T - 1), 64 * (T - 1) + 1, 200003]
XA_EXIT, XA_TAXI = 2, 4     # bsa::exparea::kExit, kTaxi (bsa_exparea_math.h); bit 1 is kInside


def list_ref(flag, id2h, mask):
    return np.flatnonzero((flag[id2h] if id2h is not None else flag) & mask)


def check_list(c, flag, id2h, mask, what):
    exp = list_ref(flag, id2h, mask)
    got = c.flagged_list(flag, id2h=id2h, mask=mask)
    assert len(got) == len(exp), '%s: count %d, expected %d' % (what, len(got), len(exp))
    if not np.array_equal(got, exp):
        i = int(np.flatnonzero(got != exp)[0])
        pytest.fail('%s: first difference at position %d of %d: got %d, expected %d' % (what, i, len(exp), got[i], exp[i]))
    assert np.all(np.diff(got) > 0), '%s: not ascending' % what
    return exp


def patterns(n):
    rng = np.random.default_rng(7 * n + 1)
    yield 'none', np.zeros(n, bool)
    yield 'all', np.ones(n, bool)
    yield 'only 0', np.arange(n) == 0
    yield 'only n-1', np.arange(n) == n - 1
    w = (n - 1) // 64 * 64 or 64     # the last wave edge inside n (the first one when n <= 64)
    yield 'lanes %d and %d' % (w - 1, w), np.isin(np.arange(n), (w - 1, w))
    yield 'alternating', np.arange(n) % 2 == 1
    yield 'random 1 %', rng.random(n) < 0.01
    yield 'random 50 %', rng.random(n) < 0.5


def id2h_cases(n):
    return (('direct', None), ('identity', np.arange(n, dtype=np.uint32)),
            ('permutation', np.random.default_rng(n).permutation(n).astype(np.uint32)))


@pytest.mark.parametrize('n', LIST_SIZES)
def test_flagged_list_matches_numpy(n):
    """Every flag pattern directly, through the identity and through a permutation (the identity
    and the direct list are both np.flatnonzero(flag), hence equal)."""
    c = _lib.Context(0)
    try:
        for what, f in patterns(n):
            flag = f.astype(np.uint8)
            for how, id2h in id2h_cases(n):
                check_list(c, flag, id2h, 1, 'n = %d, %s, %s' % (n, what, how))
    finally:
        c.close()


@pytest.mark.parametrize('n', LIST_SIZES)
def test_flagged_list_masks(n):
    """Flag bytes that carry several bits: only the mask's bits count.  The experiment area's two
    lists are taken back to back on one context, from the same arrays and the same workspace."""
    rng = np.random.default_rng(3 * n + 2)
    flag = rng.integers(0, 256, n).astype(np.uint8)
    flag[rng.random(n) < 0.25] = 0xFE
    flag[n - 1] = 0xFE
    c = _lib.Context(0)
    try:
        for how, id2h in id2h_cases(n):
            what = 'n = %d, %s' % (n, how)
            listed = check_list(c, flag, id2h, 1, what + ', mask 1')
            src = flag[id2h] if id2h is not None else flag
            assert (src == 0xFE).any() and not (src[listed] == 0xFE).any()
            check_list(c, flag, id2h, 0x06, what + ', mask 0x06')
            check_list(c, flag, id2h, XA_EXIT, what + ', exit')
            check_list(c, flag, id2h, XA_TAXI, what + ', taxi')
            check_list(c, flag, id2h, XA_EXIT, what + ', exit after taxi')
    finally:
        c.close()


@pytest.mark.parametrize('n', [65, 4097, 64 * (T - 1) + 1])
def test_flagged_list_capacity(n):
    flag = (np.random.default_rng(n).random(n) < 0.5).astype(np.uint8)
    exp = np.flatnonzero(flag)
    assert len(exp) > 1
    c = _lib.Context(0)
    try:
        assert np.array_equal(c.flagged_list(flag, cap=len(exp)), exp)
        with pytest.raises(_lib.AccelError, match=r'%d flagged, room for %d' % (len(exp), len(exp) - 1)) as e:
            c.flagged_list(flag, cap=len(exp) - 1)
        assert e.value.count == len(exp)
        assert np.array_equal(c.flagged_list(flag, cap=len(exp)), exp)     # the context is usable after the refusal
    finally:
        c.close()


def test_flagged_list_entry_edges():
    c = _lib.Context(0)
    try:
        assert c.flagged_list(np.zeros(0, np.uint8)).shape == (0,)
        assert c.flagged_list(np.zeros(0, np.uint8), id2h=np.zeros(0, np.uint32), cap=0).shape == (0,)
        with pytest.raises(_lib.AccelError, match=r'id2h\[2\] = 3 of 3'):
            c.flagged_list(np.ones(3, np.uint8), id2h=np.array([0, 1, 3], np.uint32))
        with pytest.raises(_lib.AccelError, match='NULL flags'):
            c.check(c.lib.bsa_flagged_list(c.h, 1, None, None, 1, 1, None, ctypes.byref(ctypes.c_int64())),
                    'bsa_flagged_list')
        assert c.lib.bsa_flagged_list(c.h, 1, None, None, 1, 1, None, None) != 0
        check_list(c, np.ones(3, np.uint8), None, 1, 'after the refused calls')
    finally:
        c.close()
