"""CPU: fms.append_routes, the host's copy of the route table after a create with
guidance on (bsa_sim_create_with appends the new rows and rebases their offsets)."""
import numpy as np
import pytest

from bluesky_amd import fms


def table(counts, seed):
    rng = np.random.default_rng(seed)
    cnt = np.array(counts, dtype=np.int32)
    off = (np.cumsum(cnt) - cnt).astype(np.int32)
    return rng.normal(size=(int(cnt.sum()), 8)), off, cnt


def routes_of(rows, off, cnt):
    return [rows[o:o + c] for o, c in zip(off, cnt)]


def test_offsets_are_rebased_and_every_route_keeps_its_rows():
    rows, off, cnt = table([4, 1, 3], 1)
    nrows, noff, ncnt = table([2, 5], 2)
    keep = [a.copy() for a in (rows, off, cnt, nrows, noff, ncnt)]
    r, o, c = fms.append_routes(rows, off, cnt, nrows, noff, ncnt)
    assert r.shape == (15, 8) and r.dtype == np.float64 and o.dtype == np.int32 and c.dtype == np.int32
    assert np.array_equal(o, [0, 4, 5, 8, 10]) and np.array_equal(c, [4, 1, 3, 2, 5])
    for got, exp in zip(routes_of(r, o, c), routes_of(rows, off, cnt) + routes_of(nrows, noff, ncnt)):
        assert np.array_equal(got, exp)
    for a, b in zip((rows, off, cnt, nrows, noff, ncnt), keep):     # the inputs stay as they are
        assert np.array_equal(a, b)


def test_offsets_need_not_be_packed():
    """A table with holes (deleted aircraft's rows) and routes out of order: the rebase is by the
    old table's row count, not by the rows in use."""
    rows = np.arange(80.).reshape(10, 8)
    off, cnt = np.array([6, 0], np.int32), np.array([2, 3], np.int32)     # rows 3-5 and 8-9 are holes
    nrows = -np.arange(24.).reshape(3, 8)
    r, o, c = fms.append_routes(rows, off, cnt, nrows, [1, 0], [2, 1])
    assert np.array_equal(o, [6, 0, 11, 10]) and np.array_equal(c, [2, 3, 2, 1])
    assert np.array_equal(r[:10], rows) and np.array_equal(r[10:], nrows)


def test_empty_routes():
    rows, off, cnt = table([0, 3, 0], 3)
    nrows, noff, ncnt = table([0, 0, 2, 0], 4)
    r, o, c = fms.append_routes(rows, off, cnt, nrows, noff, ncnt)
    assert np.array_equal(c, [0, 3, 0, 0, 0, 2, 0]) and np.array_equal(o, [0, 0, 3, 3, 3, 3, 5])
    assert np.array_equal(r[o[5]:o[5] + 2], nrows)
    # new aircraft without a single waypoint
    r, o, c = fms.append_routes(rows, off, cnt, np.zeros((0, 8)), [0, 0], [0, 0])
    assert np.array_equal(r, rows) and np.array_equal(o, [0, 0, 3, 3, 3]) and not c[3:].any()


def test_empty_old_table():
    nrows, noff, ncnt = table([2, 4], 5)
    r, o, c = fms.append_routes(np.zeros((0, 8)), [], [], nrows, noff, ncnt)
    assert np.array_equal(r, nrows) and np.array_equal(o, noff) and np.array_equal(c, ncnt)
    r, o, c = fms.append_routes(np.zeros((0, 8)), [0], [0], nrows, noff, ncnt)      # one aircraft, no route
    assert np.array_equal(r, nrows) and np.array_equal(o, [0, 0, 2]) and np.array_equal(c, [0, 2, 4])


def test_twice_equals_once():
    a, b, c = table([3, 2], 6), table([1], 7), table([4, 0], 8)
    step = fms.append_routes(*fms.append_routes(*a, *b), *c)
    bc = fms.append_routes(*b, *c)
    once = fms.append_routes(*a, *bc)
    for x, y in zip(step, once):
        assert np.array_equal(x, y)


def test_refusals():
    rows, off, cnt = table([3, 2], 9)
    with pytest.raises(ValueError):
        fms.append_routes(rows, off, cnt, np.zeros((2, 8)), [0], [3])       # a new route past its rows
    with pytest.raises(ValueError):
        fms.append_routes(rows, off, cnt, np.zeros((2, 8)), [-1], [1])
    with pytest.raises(ValueError):
        fms.append_routes(rows[:4], off, cnt, np.zeros((2, 8)), [0], [2])   # an old one past its rows
    with pytest.raises(ValueError):
        fms.append_routes(rows, off, cnt[:1], np.zeros((2, 8)), [0], [2])   # offsets and counts differ in length
