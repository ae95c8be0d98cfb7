"""CPU: tests/exparea_np.py (the numpy restatement of plugins/area.py's Area.update and its delete
sequence) bitwise against the reference's goldens, and the drop-in ``bluesky_amd.exparea.Area``'s
``create / update / set_area / set_taxi`` surface with the restatement in place of the device call."""
import os
import types

import numpy as np
import pytest

from bluesky_amd import areafilter, exparea
from tests import exparea_np, util


@pytest.fixture(scope='module')
def upd():
    return dict(np.load(os.path.join(util.GOLDEN, 'exparea_update.npz')))


@pytest.fixture(scope='module')
def flight():
    return dict(np.load(os.path.join(util.GOLDEN, 'exparea_flight64.npz')))


def case_of(upd, name):
    """(inputs, state before, area, swtaxi, active, expected) of one recorded update."""
    n = name.split('_')[0]
    inp = {k: upd['%s_%s' % (n, k)] for k in ('gs', 'vs', 'alt', 'lat', 'lon', 'thrust')}
    st = {k: upd['%s_%s' % (n, k)] for k in exparea_np.ARRAYS}
    a = str(upd[name + '_area'])
    area = None if a == '' else (str(upd['area_%s_type' % a]), upd['area_%s_coords' % a], float(upd['area_%s_levels' % a][0]),
                                 float(upd['area_%s_levels' % a][1]))
    swtaxi, active = (bool(x) for x in upd[name + '_flags'])
    exp = {k: upd['%s_out_%s' % (name, k)] for k in exparea_np.ARRAYS}
    exp.update(delidx=upd[name + '_delidx'], delidxalt=upd[name + '_delidxalt'])
    return inp, st, area, swtaxi, active, exp


def test_update_matches_the_reference_bitwise(upd):
    both = 0
    for name in [str(x) for x in upd['names']]:
        inp, st, area, swtaxi, active, exp = case_of(upd, name)
        got, d1, d2 = exparea_np.update(st, dt=float(upd['dt']), area=area, active=active, swtaxi=swtaxi,
                                        swtaxialt=float(upd['swtaxialt']), **inp)
        assert np.array_equal(d1, exp['delidx']) and np.array_equal(d2, exp['delidxalt']), name
        for k in exparea_np.ARRAYS:
            assert np.array_equal(got[k], exp[k], equal_nan=True), (name, k)
            num = ~np.isnan(np.asarray(exp[k], dtype=np.float64))
            assert np.asarray(got[k])[num].tobytes() == np.asarray(exp[k])[num].tobytes(), (name, k)
        both += len(set(d1) & set(d2)) > 0
    assert both >= 4
    assert np.isnan(upd['n63_box_out_work'][9]) and 7 in upd['n63_box_delidx']          # NaN thrust; NaN position exits
    assert 11 in upd['n63_circle_delidxalt'] and 12 not in upd['n63_circle_delidxalt']  # exactly at swtaxialt, either side
    assert len(upd['n63_early_delidx']) == 0 and np.array_equal(upd['n63_early_out_distance2D'], upd['n63_distance2D'])


def test_delete_sequence_keeps_the_stale_indices(flight):
    """The recorded flight's survivors follow from the two lists of every update applied as the reference
    applies them: delidxalt taken before the first delete, used after it."""
    ids = [str(x) for x in flight['ids']]
    off, offa, stale = flight['ev_off'], flight['ev_offalt'], 0
    for q in range(len(flight['ev_step'])):
        d1, d2 = flight['ev_delidx'][off[q]:off[q + 1]], flight['ev_delidxalt'][offa[q]:offa[q + 1]]
        left = exparea_np.delete_sequence(len(ids), d1, d2)
        naive = np.delete(np.arange(len(ids)), np.union1d(d1, d2).astype(np.int64))
        stale += not np.array_equal(left, naive)
        ids = [ids[k] for k in left]
    assert ids == [str(x) for x in flight['survivors']] and stale >= 1
    assert list(exparea_np.delete_sequence(5, [1], [4])) == [0, 2, 3, 4]        # 4 is past the shrunk table: dropped
    assert list(exparea_np.delete_sequence(5, [1], [3])) == [0, 2, 3]           # stale: the old 4 goes, not the old 3


class Traf:
    def __init__(self, n):
        z = np.zeros(n)
        self.id = ['AC%d' % k for k in range(n)]
        self.gs, self.vs, self.tas, self.hdg = np.full(n, 100.), z.copy(), np.full(n, 100.), z.copy()
        self.lat, self.lon, self.alt = np.full(n, 52.0), np.linspace(3.0, 5.0, n), np.full(n, 3000.)
        self.perf = types.SimpleNamespace(thrust=np.full(n, 1e4))
        self.asas = types.SimpleNamespace(active=np.zeros(n, dtype=bool))
        self.pilot = types.SimpleNamespace(alt=z.copy(), tas=z.copy(), vs=z.copy(), hdg=z.copy())
        self.deleted = []

    def delete(self, idx):
        self.deleted.append(list(np.atleast_1d(idx)))
        for obj in (self, self.perf, self.asas, self.pilot):
            for k, v in list(vars(obj).items()):
                if isinstance(v, np.ndarray):
                    setattr(obj, k, np.delete(v, idx))
        gone = set(int(k) for k in np.atleast_1d(idx))
        self.id = [x for k, x in enumerate(self.id) if k not in gone]


def np_evaluate(**a):
    st = {k: a[k] for k in exparea_np.ARRAYS}
    new, d1, d2 = exparea_np.update(st, a['gs'], a['vs'], a['alt'], a['lat'], a['lon'], a['thrust'], a['dt'], a['area'],
                                    a['active'], a['swtaxi'], a['swtaxialt'])
    return dict(new, delidx=d1, delidxalt=d2)


def test_dropin_surface():
    areafilter.reset()
    traf, rows, now = Traf(5), [], [7.0]
    a = exparea.Area(traf, logger=lambda *cols: rows.append(cols), clock=lambda: now[0], evaluate=np_evaluate)
    a.create(5)
    assert list(a.create_time) == [7.0] * 5 and np.array_equal(a.oldalt, traf.alt) and not a.inside.any()
    a.update()                                                 # swtaxi and not active: nothing happens
    assert not a.distance2D.any()
    assert a.set_area('NOPE')[0] is False and a.set_area(1.0, 2.0)[0] is False
    assert a.set_area()[1].startswith('Area is currently OFF')
    ok, msg = a.set_area(51.0, 3.4, 53.0, 4.6, 5000., 1000.)   # the box form, with top and bottom
    assert ok and a.name == 'DELAREA' and a.active and areafilter.hasArea('DELAREA')
    assert areafilter.areas['DELAREA'][2:] == (5000., 1000.)
    a.update()
    assert list(a.inside) == [False, True, True, True, False] and rows == []
    assert np.array_equal(a.distance2D, np.full(5, 50.)) and np.array_equal(a.work, np.full(5, 1e4 * 0.5 * 100.))
    traf.lon[1] = 9.0                                          # aircraft 1 leaves
    a.set_taxi(False, 2000.)
    assert a.swtaxi is False and a.swtaxialt == 2000.
    traf.alt[4] = 1500.                                        # aircraft 4 sinks through 2000 m: stale index 4 is dropped
    now[0] = 9.5
    a.update()
    assert len(rows) == 1 and len(rows[0]) == 17 and list(rows[0][0]) == ['AC1'] and list(rows[0][2]) == [2.5]
    assert traf.deleted == [[1], []] and traf.id == ['AC0', 'AC2', 'AC3', 'AC4'] and len(a.inside) == 4
    areafilter.defineArea('SECT', 'CIRCLE', [52., 4., 50.])
    assert a.set_area('SECT')[0] and a.name == 'SECT'
    assert a.set_area('OFF')[0] and a.name is None and not a.active and not areafilter.hasArea('SECT')
    areafilter.reset()
