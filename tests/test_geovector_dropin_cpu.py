"""CPU: bluesky_amd.geovector's bookkeeping (defgeovec / delgeovec / query / reset) against the
sequence tools/make_golden_geovec.py recorded from plugins/geovector.py:133-209 -- return values,
messages and the list after every call -- and ``table()``'s rows."""
import os

import numpy as np
import pytest

from bluesky_amd import _lib, geovector
from tests import geovec_np, util


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(os.path.join(util.GOLDEN, 'geovec_apply.npz')))


def unflatten(area, val, none, lo, hi):
    return [[str(area[r])] + [None if none[r, q] else float(val[r, q]) for q in range(6)] for r in range(lo, hi)]


def test_bookkeeping_sequence_matches_the_reference(golden):
    g = golden
    geovector.reset()
    assert geovector.geovecs == []
    seen = set()
    for k, op in enumerate(str(x) for x in g['bk_op']):
        area = str(g['bk_area'][k])
        if op == 'def':
            args = [None if g['bk_arg_none'][k, q] else float(g['bk_arg'][k, q]) for q in range(6)]
            r = geovector.defgeovec(area, *args)
        else:
            r = geovector.delgeovec(area)
        exp = True if (g['bk_ok'][k] and str(g['bk_msg'][k]) == '') else (bool(g['bk_ok'][k]), str(g['bk_msg'][k]))
        assert r == exp and type(r) is type(exp), (k, op, area, r, exp)
        off = g['bk_list_off']
        assert geovector.geovecs == unflatten(g['bk_list_area'], g['bk_list_limits'], g['bk_list_none'], off[k], off[k + 1]), k
        seen.add((op, r if r is True else r[0]))
    assert seen == {('def', True), ('def', False), ('del', True), ('del', False)}
    assert len(geovector.geovecs) > 0
    geovector.reset()
    assert geovector.geovecs == []


def test_defgeovec_without_arguments():
    geovector.reset()
    assert geovector.defgeovec() == (False, 'We need an area')
    assert geovector.delgeovec('X') == (False, 'No geovector found for X')


def test_table_sets_given_by_python_truth(golden):
    names = ['BOX', 'CIRC', 'POLY']
    gv = [['CIRC', 100., None, None, None, None, None],          # gsmin alone
          ['NOSUCH', 100., 200., 10., 20., -1., 1.],             # unknown area: skipped
          ['BOX', None, 200., 0., 90., -3., 0.],                 # trkmin = 0: no track limit; vsmax = 0: off
          ['POLY', 0, 0., 350., 10., None, 2.5],                 # zero speeds are off; a wrap-around track interval
          ['BOX', None, None, 20., None, None, -2.]]             # one track bound alone is no limit
    rows, kept = geovector.table(gv, names)
    assert kept == [0, 2, 3, 4]
    assert [r[0] for r in rows] == [1, 0, 2, 0]
    assert [r[1] for r in rows] == [_lib.GEOVEC_GSMIN, _lib.GEOVEC_GSMAX | _lib.GEOVEC_VSMIN,
                                    _lib.GEOVEC_TRK | _lib.GEOVEC_VSMAX, _lib.GEOVEC_VSMAX]
    assert rows[1][2:] == (0., 200., 0., 0., -3., 0.)            # the track pair is stored only when it is on
    assert rows[2][2:] == (0., 0., 350., 10., 0., 2.5)
    tab, m = _lib.geovec_rows(rows)
    assert m == 4 and tab[2].trkmin == 350. and tab[2].given == rows[2][1] and tab[3].vsmax == -2.
    assert _lib.geovec_rows(tab)[0] is tab
    assert geovector.table([], names) == ([], [])


def test_table_of_every_golden_list_has_no_given_zero(golden):
    """What bsa_geovec_apply refuses (a given bound of exactly 0) never comes out of table()."""
    lists, areas = geovec_np.load_lists(golden), geovec_np.load_areas(golden)
    fields = [(_lib.GEOVEC_GSMIN, 2), (_lib.GEOVEC_GSMAX, 3), (_lib.GEOVEC_TRK, 4), (_lib.GEOVEC_TRK, 5),
              (_lib.GEOVEC_VSMIN, 6), (_lib.GEOVEC_VSMAX, 7)]
    for name, gv in lists.items():
        rows, kept = geovector.table(gv, list(areas))
        assert len(rows) == sum(v[0] in areas for v in gv), name
        for r in rows:
            assert all(r[col] != 0.0 for bit, col in fields if r[1] & bit), (name, r)
            assert all(r[col] == 0.0 for bit, col in fields if not r[1] & bit), (name, r)
    rows, _ = geovector.table(lists['zero_is_off'], list(areas))
    assert rows[0][1] == _lib.GEOVEC_GSMAX | _lib.GEOVEC_VSMIN


def test_struct_layout_matches_the_header():
    import ctypes
    assert ctypes.sizeof(_lib.Geovec) == 56 and _lib.Geovec.gsmin.offset == 8 and _lib.Geovec.vsmax.offset == 48
