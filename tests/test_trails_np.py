"""CPU: tests/trails_np.py against the reference's recorded Trails results (trails_update.npz,
trails_flight64.npz), and the drop-in's host-only methods against the recorded reference results."""
import os
import types

import numpy as np
import pytest

from bluesky_amd import trails
from tests import trails_np, util

NS = (1, 63, 64, 65, 257)
CASES = ('mixed', 'none', 'all', 'inactive')


@pytest.fixture(scope='module')
def upd():
    return dict(np.load(os.path.join(util.GOLDEN, 'trails_update.npz')))


@pytest.fixture(scope='module')
def flight():
    return dict(np.load(os.path.join(util.GOLDEN, 'trails_flight64.npz')))


def case_of(g, n, case, gui='qtgl'):
    """(lat, lon, the arrays before, active, the arrays after, the segments) of a recorded update."""
    base, name = 'n%d_%s_' % (n, case), 'n%d_%s_%s_' % (n, case, gui)
    st = {k: g[base + k] for k in trails_np.ARRAYS}
    return (g[base + 'lat'], g[base + 'lon'], st, case != 'inactive', {k: g[name + 'out_' + k] for k in trails_np.ARRAYS},
            {k: g[name + 'seg_' + k] for k in ('idx',) + trails_np.SEGMENT})


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b)) and \
        a[~np.isnan(a)].tobytes() == b[~np.isnan(b)].tobytes()


def colours(col):
    return np.array([[-1, -1, -1] if isinstance(c, str) else np.asarray(c) for c in col], dtype=np.int64).reshape(-1, 3)


@pytest.mark.parametrize('n', NS)
def test_restatement_equals_the_update_golden(upd, n):
    for case in CASES:
        for gui in ('qtgl', 'pygame'):
            lat, lon, st, active, exp, seg = case_of(upd, n, case, gui)
            got, gseg = trails_np.update(st, lat, lon, float(upd['t']), float(upd['dt']), active)
            for k in trails_np.ARRAYS:
                assert same(got[k], exp[k]), (case, gui, k)
            assert np.array_equal(gseg['idx'], seg['idx'])
            for k in trails_np.SEGMENT:
                assert same(gseg[k], seg[k]), (case, gui, k)
    if n >= 63:                                           # the edge aircraft did what the file's description says
        idx = set(case_of(upd, n, 'mixed')[5]['idx'])
        assert 3 not in idx and 4 in idx and 5 not in idx and 6 in idx and {63, 64, n - 1} & set(range(n)) <= idx


def replay(g):
    """The flight's trail side replayed by the restatement on the recorded segment ends; yields per emitting step."""
    ev = {k: g['ev_' + k] for k in ('idx',) + trails_np.SEGMENT}
    off = g['ev_off']
    for q, step in enumerate(g['ev_step']):
        yield int(step), float(g['ev_t'][q]), {k: v[off[q]:off[q + 1]] for k, v in ev.items()}


def test_restatement_equals_the_flight_golden(flight):
    """The emitting steps follow from the clock alone: simt accumulated in fp64, lasttim set by the last inactive
    update or the last emission, created aircraft at lasttim 0.  Replayed here without positions."""
    g = flight
    simdt, dt = float(g['simdt']), float(g['dt'])
    on, create, delete, off, on2 = [int(x) for x in g['commands']]
    n, simt, active = 64, 0.0, False
    lasttim = np.zeros(n)
    want = {s: (t, seg) for s, t, seg in replay(g)}
    seen = []
    for step in range(int(g['nsteps'])):
        active = True if step in (on, on2) else False if step == off else active
        if step == create:
            lasttim = np.append(lasttim, np.zeros(3))
        if step == delete:
            lasttim = np.delete(lasttim, g['deleted'])
        z = np.zeros(len(lasttim))
        st, seg = trails_np.update(dict(lastlat=z, lastlon=z, lasttim=lasttim), z, z, simt, dt, active)
        lasttim = st['lasttim']
        if len(seg['idx']):
            t, exp = want[step + 1]
            assert t == simt and np.array_equal(seg['idx'], exp['idx']) and same(seg['time'], exp['time']), step
            seen.append(step + 1)
        simt += simdt
    assert seen == [int(x) for x in g['ev_step']] and simt == float(g['final_simt'])
    assert same(lasttim, g['final_lasttim'])
    zs = g['zero_starts']
    assert len(zs) == 2 and set(zs[:, 0]) == {create + 1} and list(zs[:, 1]) == [64, 65]


def test_capacity_bound_covers_the_flight(flight):
    g = flight
    off = g['ev_off']
    steps = g['ev_step']
    for k in (1, 7, 50, 400):
        for s0 in range(0, 400, 13):
            inside = (steps > s0) & (steps <= s0 + k)
            emitted = sum(off[q + 1] - off[q] for q in np.flatnonzero(inside))
            assert emitted <= trails_np.bound(67, k, float(g['simdt']), float(g['dt'])), (k, s0)


# ---------------------------------------------------------------- the drop-in's host-only methods
def dropin(upd, gui='pygame'):
    lat, lon = upd['n65_mixed_lat'], upd['n65_mixed_lon']
    traf = types.SimpleNamespace(lat=lat.copy(), lon=lon.copy(), id=['AC%03d' % k for k in range(65)])
    return trails.Trails(traf, float(upd['dt']), gui_type=gui)


def test_dropin_host_methods_equal_the_reference(upd):
    tr = dropin(upd)
    rets = [tr.setTrails(), tr.setTrails(True), tr.setTrails(), tr.setTrails(True, 5.0)]
    tr.create(65)
    assert tr.accolor[:64] == [''] * 64 and np.array_equal(tr.accolor[64], tr.defcolor)
    assert not tr.lastlat[:64].any() and tr.lastlat[64] == tr.traf.lat[64] and not tr.lasttim.any()
    for k in trails_np.ARRAYS:
        setattr(tr, k, upd['n65_mixed_' + k].copy())
    rets += [tr.setTrails(3, 'RED'), tr.setTrails(3, 'GREEN'), tr.setTrails(3)]
    tr.dt = float(upd['dt'])
    t = float(upd['t'])
    # the update itself is the device's (tests/test_gpu_trails.py): here its recorded result is taken in
    seg = {k: upd['n65_mixed_pygame_seg_' + k] for k in ('idx',) + trails_np.SEGMENT}
    tr.acid = tr.traf.id
    tr._take(seg, t)
    assert same(colours(tr.col), upd['host_col'])
    with pytest.raises(AttributeError):
        trails.Trails(tr.traf).buffer()                   # the reference's quirk: no bgacid before clearbg()
    tr.clearbg()
    tr.buffer()
    for k in trails_np.SEGMENT:
        assert same(getattr(tr, 'bg' + k), upd['host_bg' + k]), k
    assert same(colours(tr.bgcol), upd['host_bgcol'])
    assert [len(getattr(tr, k)) for k in trails_np.SEGMENT + ('col',)] == list(upd['host_fg_len'])
    st = {k: upd['n65_mixed_pygame_out_' + k] for k in trails_np.ARRAYS}
    _, seg2 = trails_np.update(st, tr.traf.lat, tr.traf.lon, t + 20.0, tr.dt, True)
    tr._take(seg2, t + 20.0)
    assert same(tr.fcol, upd['host_fcol2']) and same(tr.time, upd['host_time2'])
    rets.append(tr.setTrails(False))
    tr.lasttim = st['lasttim']
    assert [len(tr.lastlat), len(tr.lastlon), len(tr.lasttim), len(tr.lat0), len(tr.bglat0), len(tr.newlat0),
            int(tr.active)] == list(upd['host_after_off'])
    assert tr.dt == float(upd['host_dt'])
    assert [repr(r) for r in rets] == [str(x) for x in upd['host_returns']]
    tr.reset()
    assert len(tr.lasttim) == 0 and tr.accolor == [] and not tr.active


@pytest.mark.parametrize('n', NS)
def test_dropin_fcol_and_lists_on_recorded_results(upd, n):
    """Both GUI paths: the recorded segments taken into the drop-in's lists as the reference filled its own."""
    for case in CASES[:3]:
        lat, lon, st, active, exp, seg = case_of(upd, n, case, 'pygame')
        traf = types.SimpleNamespace(lat=lat, lon=lon, id=[])
        tr = trails.Trails(traf, float(upd['dt']), gui_type='pygame')
        tr.accolor = [tr.colorList[('BLUE', 'RED', 'YELLOW', 'CYAN')[k % 4]] for k in range(n)]
        for k in trails_np.SEGMENT:
            setattr(tr, k, upd['prior_' + k].copy())
        tr.col = [tr.defcolor] * 3
        tr._take(seg, float(upd['t']))
        assert same(tr.fcol, upd['n%d_%s_pygame_fcol' % (n, case)]) and same(colours(tr.col), upd['n%d_%s_pygame_col' % (n, case)])
        assert same(tr.lat0[3:], seg['lat0']) and same(tr.time[3:], seg['time']) and tr.newlat0 == []
        q = trails.Trails(traf, float(upd['dt']))
        q.accolor = tr.accolor
        q._take(seg, float(upd['t']))
        assert same(np.array(q.newlat0, dtype=np.float64), seg['lat0']) and same(np.array(q.newlon1, dtype=np.float64), seg['lon1'])
        assert len(q.lat0) == 0 and len(q.col) == len(seg['idx'])
