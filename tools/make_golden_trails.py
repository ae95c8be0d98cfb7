#!/usr/bin/env python3
"""Capture tests/golden/trails_update.npz and trails_flight64.npz from the REFERENCE's own ``Trails``
class (traffic/trails.py; build container only).

``bs.traf`` is a stand-in with ``lat`` / ``lon`` / ``id``, ``bs.gui_type`` is set per case ('qtgl' or
'pygame').  Only data is written.  tests/trails_np.py is asserted bitwise equal to the reference on every
case here.

trails_update: single ``update(t)`` calls at n = 1, 63, 64, 65, 257 on both GUI paths -- 'mixed' (from
n = 63 on: aircraft 3 with t - lasttim exactly dt, not emitted; aircraft 4 one ulp above, emitted;
aircraft 5 with a NaN lasttim, never emitted; aircraft 6 emitting with a NaN lat, copied as a NaN;
emitting aircraft at 63, 64 and n - 1), 'none' (nobody emits), 'all' (everybody does) and 'inactive'.
The pygame cases start from three earlier segments, so ``fcol`` covers old and new entries.  Also the
host-only methods' results: the ``setTrails`` returns, ``buffer`` and the ``clear*`` family.

trails_flight64: the closed loop (``run_flight``).

Usage:  python tools/make_golden_trails.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                     # noqa: E402  (numpy shims, sys.path: reference + repo)

import bluesky as bs                                         # noqa: E402
from bluesky.traffic.trails import Trails as RefTrails       # noqa: E402
from tests import trails_np                                  # noqa: E402

OUT = os.path.join(mg.REPO, 'tests', 'golden')
SEED = 20261021
T, DT = 100.0, 10.0
NOCOL = np.array([-1, -1, -1])


def ref_trails(gui, traf, dt=10.):
    bs.gui_type, bs.traf = gui, traf
    return RefTrails(dt)


def colours(col):
    """A col list as an (m, 3) int array; the '' of an aircraft created before the last of its batch as -1."""
    return np.array([NOCOL if isinstance(c, str) else np.asarray(c) for c in col], dtype=np.int64).reshape(-1, 3)


def inputs(rng, n, case):
    lat, lon = rng.uniform(-60., 60., n), rng.uniform(-179., 179., n)
    st = dict(lastlat=lat + rng.uniform(-0.1, 0.1, n), lastlon=lon + rng.uniform(-0.1, 0.1, n),
              lasttim=rng.uniform(T - 2 * DT, T, n))
    if case == 'none':
        st['lasttim'] = np.full(n, T)
    elif case == 'all':
        st['lasttim'] = np.zeros(n)
    elif n >= 63:
        st['lasttim'][3] = T - DT                                  # exactly dt: not emitted
        st['lasttim'][4] = np.nextafter(T - DT, -np.inf)           # one ulp above: emitted
        st['lasttim'][5] = np.nan                                  # never emitted
        st['lasttim'][6], lat[6] = 0.0, np.nan                     # emits a NaN
        for k in (63, 64, n - 1):
            if k < n:
                st['lasttim'][k] = 0.0
        assert T - st['lasttim'][3] == DT and T - st['lasttim'][4] > DT
    else:
        st['lasttim'][0] = 0.0
    return lat, lon, st


def run_update():
    rng = np.random.default_rng(SEED)
    out, names = dict(t=T, dt=DT), []
    prior = dict(lat0=np.array([1., 2., 3.]), lon0=np.array([4., 5., 6.]), lat1=np.array([1.5, 2.5, 3.5]),
                 lon1=np.array([4.5, 5.5, 6.5]), time=np.array([T - 100., T - 30., T - 5.]))
    out.update({'prior_' + k: v for k, v in prior.items()})
    for n in (1, 63, 64, 65, 257):
        for case in ('mixed', 'none', 'all', 'inactive'):
            lat, lon, st0 = inputs(rng, n, case)
            for gui in ('qtgl', 'pygame'):
                traf = types.SimpleNamespace(lat=lat.copy(), lon=lon.copy(), id=['AC%03d' % k for k in range(n)])
                tr = ref_trails(gui, traf, DT)
                tr.active = case != 'inactive'
                for k in trails_np.ARRAYS:
                    setattr(tr, k, st0[k].copy())
                tr.accolor = [tr.colorList[('BLUE', 'RED', 'YELLOW', 'CYAN')[k % 4]] for k in range(n)]
                if gui == 'pygame':
                    for k, v in prior.items():
                        setattr(tr, k, v.copy())
                    tr.col = [tr.defcolor] * 3
                with np.errstate(invalid='ignore'):
                    tr.update(T)
                st1, seg = trails_np.update(st0, lat, lon, T, DT, tr.active)
                for k in trails_np.ARRAYS:
                    assert np.array_equal(np.asarray(getattr(tr, k)), st1[k], equal_nan=True), (n, case, gui, k)
                m = len(seg['idx'])
                if gui == 'qtgl':
                    got = {k: np.array(getattr(tr, 'new' + k), dtype=np.float64) for k in ('lat0', 'lon0', 'lat1', 'lon1')}
                else:
                    got = {k: getattr(tr, k)[3:] for k in trails_np.SEGMENT}
                    assert np.array_equal(colours(tr.col)[3:], colours([tr.accolor[i] for i in seg['idx']]))
                for k, v in got.items():
                    assert len(v) == m and np.array_equal(v, seg[k], equal_nan=True), (n, case, gui, k)
                name = 'n%d_%s_%s' % (n, case, gui)
                out.update({name + '_out_' + k: st1[k] for k in trails_np.ARRAYS})
                out.update({name + '_seg_' + k: v for k, v in seg.items()})
                if gui == 'pygame':
                    out[name + '_col'] = colours(tr.col)
                    out[name + '_fcol'] = np.asarray(tr.fcol)
                    if tr.active:
                        assert np.array_equal(tr.fcol, trails_np.fcol(T, tr.time))
                names.append(name)
            out.update({'n%d_%s_lat' % (n, case): lat, 'n%d_%s_lon' % (n, case): lon})
            out.update({'n%d_%s_%s' % (n, case, k): v for k, v in st0.items()})
            print('trails_update n%-3d %-8s segments %3d' % (n, case, len(seg['idx'])))
    # the host-only methods on a pygame object holding the n = 65 'mixed' result
    lat, lon = out['n65_mixed_lat'], out['n65_mixed_lon']
    traf = types.SimpleNamespace(lat=lat.copy(), lon=lon.copy(), id=['AC%03d' % k for k in range(65)])
    tr = ref_trails('pygame', traf, DT)
    rets = [tr.setTrails(), tr.setTrails(True), tr.setTrails(), tr.setTrails(True, 5.0)]
    tr.create(65)
    for k in trails_np.ARRAYS:
        setattr(tr, k, out['n65_mixed_' + k].copy())
    rets += [tr.setTrails(3, 'RED'), tr.setTrails(3, 'GREEN'), tr.setTrails(3)]
    tr.dt = DT
    with np.errstate(invalid='ignore'):
        tr.update(T)
    out['host_col'] = colours(tr.col)
    tr.clearbg()
    tr.buffer()
    out.update({'host_bg' + k: getattr(tr, 'bg' + k) for k in trails_np.SEGMENT})
    out['host_bgcol'] = colours(tr.bgcol)
    out['host_fg_len'] = np.array([len(getattr(tr, k)) for k in trails_np.SEGMENT + ('col',)])
    with np.errstate(invalid='ignore'):
        tr.update(T + 20.0)
    out['host_fcol2'] = np.asarray(tr.fcol)
    out['host_time2'] = np.asarray(tr.time)
    rets.append(tr.setTrails(False))
    out['host_after_off'] = np.array([len(tr.lastlat), len(tr.lastlon), len(tr.lasttim), len(tr.lat0), len(tr.bglat0),
                                      len(tr.newlat0), int(tr.active)])
    out['host_dt'] = tr.dt
    out['host_returns'] = np.array([repr(r) for r in rets])
    out['names'] = np.array(names)
    path = os.path.join(OUT, 'trails_update.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1000000
    print('trails_update.npz %d bytes' % os.path.getsize(path))


FLIGHT_STEPS, SIMDT, TRAIL_DT = 400, 0.1, 1.0
ON_AT, CREATE_AT, DELETE_AT, OFF_AT, ON2_AT = 25, 150, 230, 330, 345       # commands typed before the step of that number
DELETED = np.array([5, 65])                                                  # one of the first 64, one created


def run_flight(gui, seed=91):
    """trails_flight64: 64 aircraft, simdt 0.1, Pilot.APorASAS -> UpdateAirSpeed / GroundSpeed / Position with the
    reference's own methods and constant autopilot targets, then ``trails.update(simt)`` with the simt the step
    started at; ``simt += simdt`` after it.  Trails are inactive for the first 25 steps, then TRAIL ON with dt 1.0;
    3 aircraft are created before step 150 (Traffic.create's appends on the stand-ins, then ``Trails.create(3)``:
    the first two start at (0, 0, 0)); aircraft 5 and 65 are deleted before step 230; TRAIL OFF before step 330
    and ON again before step 345."""
    from bluesky.traffic.pilot import Pilot
    rng = np.random.default_rng(seed)
    n = 64
    hdg = rng.uniform(0., 360., n)
    tas = rng.uniform(140., 240., n)
    lat, lon = rng.uniform(51., 53., n), rng.uniform(3., 5., n)
    alt = rng.uniform(3000 * 0.3048, 20000 * 0.3048, n)

    def state(lat, lon, alt, tas, hdg, ap_tas):
        m = len(lat)
        return {k: np.array(v, dtype=np.float64) for k, v in dict(
            lat=lat, lon=lon, alt=alt, tas=tas, hdg=hdg, vs=np.zeros(m), gs=tas.copy(), trk=hdg.copy(),
            gseast=tas * np.sin(np.radians(hdg)), gsnorth=tas * np.cos(np.radians(hdg)), ap_trk=hdg.copy(), ap_tas=ap_tas,
            ap_alt=alt.copy(), ap_vs=np.full(m, 1500. * 0.3048 / 60.), selalt=alt.copy(), bank=np.full(m, np.radians(25.)),
            eps=np.full(m, 0.01), accel=np.full(m, 0.5), asas_alt=alt.copy()).items()}

    init = state(lat, lon, alt, tas, hdg, tas + rng.choice([0.0, 15.0, -10.0], n))
    new = state(rng.uniform(51., 53., 3), rng.uniform(3., 5., 3), rng.uniform(2000., 6000., 3), rng.uniform(140., 240., 3),
                rng.uniform(0., 360., 3), rng.uniform(140., 240., 3))

    def stand_ins(s):
        traf = {k: s[k].copy() for k in ('lat', 'lon', 'alt', 'tas', 'hdg', 'vs', 'gs', 'trk', 'bank', 'eps')}
        ap = dict(trk=s['ap_trk'].copy(), tas=s['ap_tas'].copy(), alt=s['ap_alt'].copy(), vs=s['ap_vs'].copy())
        asas = dict(active=np.zeros(len(s['lat']), dtype=bool), trk=s['hdg'].copy(), tas=s['tas'].copy(), alt=s['alt'].copy(),
                    vs=np.zeros(len(s['lat'])))
        return traf, ap, asas

    t0, a0, s0 = stand_ins(init)
    traf = types.SimpleNamespace(**t0)
    traf.id = ['AC%02d' % k for k in range(n)]
    traf.ntraf = n
    traf.ap, traf.asas = types.SimpleNamespace(**a0), types.SimpleNamespace(**s0)
    traf.pilot = Pilot.__new__(Pilot)
    traf.wind = mg.WindSim()
    hold = dict(acc=np.full(n, 0.5))
    traf.perf = types.SimpleNamespace(acceleration=lambda: hold['acc'])
    tr = ref_trails(gui, traf, 10.)
    tr.create(n)                                                     # (as the children of Traffic.create would have been)
    tr.lastlat, tr.lastlon = traf.lat.copy(), traf.lon.copy()
    st = {k: np.array(getattr(tr, k)) for k in trails_np.ARRAYS}

    def every_array():
        for obj in (traf, traf.ap, traf.asas, traf.pilot):
            for name, v in list(vars(obj).items()):
                if isinstance(v, np.ndarray) and v.shape[:1] == (traf.ntraf,):
                    yield obj, name, v

    def create():
        t1, a1, s1 = stand_ins(new)
        for obj, name, v in list(every_array()):
            src = t1 if obj is traf else a1 if obj is traf.ap else s1 if obj is traf.asas else {}
            setattr(obj, name, np.append(v, src.get(name, np.zeros(3, dtype=v.dtype))))
        hold['acc'] = np.append(hold['acc'], new['accel'])
        traf.id += ['NEW%d' % k for k in range(3)]
        traf.ntraf += 3
        tr.create(3)

    def delete(idx):
        for obj, name, v in list(every_array()):
            setattr(obj, name, np.delete(v, idx))
        hold['acc'] = np.delete(hold['acc'], idx)
        traf.id = [x for k, x in enumerate(traf.id) if k not in set(int(q) for q in idx)]
        traf.ntraf -= len(idx)
        tr.delete(idx)

    simt, active, dt = 0.0, False, 10.
    events, snaps = [], {}

    def snapshot(tag):
        if gui == 'pygame':
            snaps.update({'%s_%s' % (tag, k): np.array(getattr(tr, k)) for k in trails_np.SEGMENT + ('fcol',)})
            snaps[tag + '_col'] = colours(tr.col)
        else:
            snaps.update({'%s_new%s' % (tag, k): np.array(getattr(tr, 'new' + k), dtype=np.float64)
                          for k in ('lat0', 'lon0', 'lat1', 'lon1')})

    saved = getattr(bs, 'traf', None)
    try:
        with np.errstate(all='ignore'):
            for step in range(FLIGHT_STEPS):
                if step in (ON_AT, ON2_AT):
                    assert tr.setTrails(True, TRAIL_DT) is True
                    active, dt = True, TRAIL_DT
                if step == OFF_AT:
                    snapshot('before_off')
                    assert tr.setTrails(False) is True
                    active = False
                if step == CREATE_AT:
                    create()
                    st = trails_np.create(st, traf.lat, traf.lon, 3)
                if step == DELETE_AT:
                    delete(DELETED)
                    st = trails_np.delete(st, DELETED)
                Pilot.APorASAS(traf.pilot)
                mg.RefTraffic.UpdateAirSpeed(traf, SIMDT, simt)
                mg.RefTraffic.UpdateGroundSpeed(traf, SIMDT)
                mg.RefTraffic.UpdatePosition(traf, SIMDT)
                before = len(tr.newlat0) if gui == 'qtgl' else len(tr.lat0)
                tr.update(simt)
                st, seg = trails_np.update(st, traf.lat, traf.lon, simt, dt, active)
                for k in trails_np.ARRAYS:
                    assert np.array_equal(np.asarray(getattr(tr, k)), st[k], equal_nan=True), (step, k)
                src = {k: (np.array(getattr(tr, 'new' + k)) if gui == 'qtgl' else getattr(tr, k))[before:]
                       for k in ('lat0', 'lon0', 'lat1', 'lon1')}
                for k, v in src.items():
                    assert np.array_equal(v, seg[k]), (step, k)
                if len(seg['idx']):
                    events.append(dict(step=step + 1, t=simt, **seg))
                simt += SIMDT
    finally:
        bs.traf = saved
    snapshot('final')
    steps = [e['step'] for e in events]
    print('trails_flight64 (%s): %d segments in %d emitting steps: %s' % (gui, sum(len(e['idx']) for e in events), len(steps), steps))
    zero_starts = [(e['step'], int(i)) for e in events for i, a, b in zip(e['idx'], e['lat0'], e['lon0']) if a == 0.0 and b == 0.0]
    assert len(zero_starts) == 2, zero_starts
    out = {'init_' + k: v for k, v in init.items()}
    out.update({'new_' + k: v for k, v in new.items()})
    out.update(simdt=SIMDT, dt=TRAIL_DT, nsteps=FLIGHT_STEPS, commands=np.array([ON_AT, CREATE_AT, DELETE_AT, OFF_AT, ON2_AT]),
               deleted=DELETED, ev_step=np.array(steps), ev_t=np.array([e['t'] for e in events]),
               ev_off=np.cumsum([0] + [len(e['idx']) for e in events]), final_simt=simt,
               zero_starts=np.array(zero_starts), numpy_version=np.array(np.__version__))
    for k in ('idx',) + trails_np.SEGMENT:
        out['ev_' + k] = np.concatenate([e[k] for e in events])
    out.update({'final_' + k: np.asarray(getattr(tr, k)) for k in trails_np.ARRAYS})
    out.update({'final_traf_' + k: getattr(traf, k) for k in ('lat', 'lon')})
    return out, snaps


if __name__ == '__main__':
    run_update()
    out, snaps = run_flight('qtgl')
    out2, snaps2 = run_flight('pygame')
    for k in out:                                                   # the GUI path changes where segments go, not which
        assert np.asarray(out[k]).tobytes() == np.asarray(out2[k]).tobytes(), k
    out.update({'qtgl_' + k: v for k, v in snaps.items()})
    out.update({'pygame_' + k: v for k, v in snaps2.items()})
    path = os.path.join(OUT, 'trails_flight64.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1000000
    print('trails_flight64.npz %d bytes' % os.path.getsize(path))
