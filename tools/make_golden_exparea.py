#!/usr/bin/env python3
"""Capture tests/golden/exparea_update.npz and exparea_flight64.npz from the REFERENCE's own ``Area``
class (plugins/area.py; build container only).

``datalog.defineLogger`` is replaced by a recorder that keeps the logger's arguments, the module's
``traf`` / ``sim`` by stand-ins, ``areafilter.areas`` is filled with the reference's own shape objects
(``defineArea`` needs ``bs.scr``).  Only data is written.  tests/exparea_np.py is asserted bitwise
equal to the reference on every case here.

exparea_update: single ``update()`` calls at n = 1, 63, 64, 65, 257 for a BOX with top and bottom, a
CIRCLE, a POLY, ``name`` None (with ``active`` False and ``swtaxi`` False) and the early return
(``swtaxi`` True, ``active`` False); ``swtaxi`` both ways.  From n = 63 on the inputs hold an altitude
exactly at ``swtaxialt`` on either side of the crossing (oldalt == swtaxialt: deleted; alt ==
swtaxialt: not), a NaN position (aircraft 7: inside nothing, so it exits if it was inside), a NaN
thrust (aircraft 9: its work is NaN) and aircraft that are at once an exit and a taxi delete.  The
capture ASSERTS that no point lies within 1e-9 (relative) of the circle's rim or 1e-9 deg of a box
face or polygon edge, so a last-bit difference of a device ``cos`` cannot flip a flag.

exparea_flight64: the closed loop (``run_flight``).

Usage:  python tools/make_golden_exparea.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                     # noqa: E402  (numpy shims, sys.path: reference + repo)
import make_golden_area as mga                               # noqa: E402  (seg_dist, ref_object)

import bluesky as bs                                         # noqa: E402
from bluesky.tools import areafilter as ref_af               # noqa: E402
from tests import exparea_np                                 # noqa: E402

OUT = os.path.join(mg.REPO, 'tests', 'golden')
FT = 0.3048
SEED = 20261020
CLAT, CLON = 52.0, 4.0
TAXIALT = 1500 * FT
MARGIN = 1e-9


class Recorder:
    def __init__(self):
        self.rows = []

    def log(self, *args):
        self.rows.append([np.array(a) for a in args])

    def start(self):
        pass

    def reset(self):
        pass


def load_ref_area():
    """plugins/area.py as a module whose ``datalog.defineLogger`` hands out Recorders."""
    spec = importlib.util.spec_from_file_location('ref_area_plugin', os.path.join(mg.REF, 'plugins', 'area.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.datalog = types.SimpleNamespace(defineLogger=lambda name, header: Recorder())
    mod.settings.performance_model = 'openap'
    return mod


AREAS = {
    'box': ('BOX', np.array([52.3, 4.5, 51.7, 3.5]), 9000 * FT, 1000 * FT),          # corners swapped, top and bottom
    'circle': ('CIRCLE', np.array([52.05, 3.95, 18.0]), 1e9, -1e9),
    'poly': ('POLY', np.array([51.6, 3.4, 52.4, 3.6, 52.5, 4.4, 52.0, 4.7, 51.5, 4.3]), 12000 * FT, 0.0),
}


def margins_ok(area, lat, lon):
    typ, co = area[0], area[1]
    ok = np.isfinite(lat) & np.isfinite(lon)
    la, lo = lat[ok], lon[ok]
    if typ == 'BOX':
        m = min(np.abs(la - co[0]).min(), np.abs(la - co[2]).min(), np.abs(lo - co[1]).min(), np.abs(lo - co[3]).min())
        return m > MARGIN
    if typ == 'CIRCLE':
        from tests import area_np
        d = area_np.kwikdist(co[0], co[1], la, lo)
        return (np.abs(d - co[2]) > MARGIN * co[2]).all()
    v = co.reshape(-1, 2)
    m = min(mga.seg_dist(la, lo, v[k][0], v[k][1], v[(k + 1) % len(v)][0], v[(k + 1) % len(v)][1]).min() for k in range(len(v)))
    return m > MARGIN


def inputs(rng, n):
    lat = rng.uniform(CLAT - 0.7, CLAT + 0.7, n)
    lon = rng.uniform(CLON - 0.9, CLON + 0.9, n)
    alt = rng.uniform(200 * FT, 11000 * FT, n)
    gs = rng.uniform(60., 260., n)
    vs = rng.choice([0.0, 7.62, -7.62, -12.5, 2.0], n)
    thrust = rng.uniform(2e4, 2e5, n)
    st = dict(distance2D=rng.uniform(0., 5e5, n), distance3D=rng.uniform(0., 5e5, n), work=rng.uniform(0., 1e11, n),
              oldalt=alt + rng.choice([0.0, 40.0, -40.0, 400.0], n), inside=rng.random(n) < 0.6)
    if n >= 63:
        lat[7] = np.nan                                   # a NaN position: inside nothing
        st['inside'][7] = True
        thrust[9] = np.nan
        st['oldalt'][11], alt[11] = TAXIALT, TAXIALT - 0.25            # oldalt exactly at swtaxialt: deleted
        st['oldalt'][12], alt[12] = TAXIALT + 0.25, TAXIALT            # alt exactly at swtaxialt: not
        st['oldalt'][13], alt[13] = TAXIALT - 0.25, TAXIALT - 0.5      # already below
        for k in (20, 21, n - 1):                         # at once an exit and a taxi delete: far outside, sinking through
            lat[k], lon[k] = CLAT + 3.0, CLON - 3.0
            st['inside'][k] = True
            st['oldalt'][k], alt[k] = TAXIALT + 3.0, TAXIALT - 3.0
    else:
        st['inside'][0] = True
        lat[0], lon[0] = CLAT + 3.0, CLON
        st['oldalt'][0], alt[0] = TAXIALT + 3.0, TAXIALT - 3.0
    return dict(gs=gs, vs=vs, alt=alt, lat=lat, lon=lon, thrust=thrust), st


CASES = (('box', 'box', True, True), ('circle', 'circle', False, True), ('poly', 'poly', False, True),
         ('boxoff', 'box', False, True), ('none', None, False, False), ('early', 'box', True, False))


def run_update():
    mod = load_ref_area()
    rng = np.random.default_rng(SEED)
    out, names = {}, []
    for key, a in AREAS.items():
        out.update({'area_%s_type' % key: np.array(a[0]), 'area_%s_coords' % key: a[1],
                    'area_%s_levels' % key: np.array([a[2], a[3]])})
        ref_af.areas[key] = mga.ref_object(key, *a)
    seen_both = False
    for n in (1, 63, 64, 65, 257):
        inp, st0 = inputs(rng, n)
        for a in AREAS.values():
            assert margins_ok(a, inp['lat'], inp['lon']), 'a point within the margin: change the seed'
        out.update({'n%d_%s' % (n, k): v for k, v in inp.items()})
        out.update({'n%d_%s' % (n, k): v for k, v in st0.items()})
        for case, aname, swtaxi, active in CASES:
            area = mod.Area()
            area.name, area.active, area.swtaxi, area.swtaxialt, area.dt = aname, active, swtaxi, TAXIALT, 0.5
            for k in exparea_np.ARRAYS:
                setattr(area, k, np.array(st0[k]))
            area.create_time = np.zeros(n)
            deleted = []
            traf = types.SimpleNamespace(id=['AC%03d' % k for k in range(n)], tas=inp['gs'], hdg=np.zeros(n),
                                         perf=types.SimpleNamespace(thrust=inp['thrust']),
                                         asas=types.SimpleNamespace(active=np.zeros(n, dtype=bool)),
                                         pilot=types.SimpleNamespace(alt=np.zeros(n), tas=np.zeros(n), vs=np.zeros(n), hdg=np.zeros(n)),
                                         delete=lambda idx: deleted.append(np.array(idx, dtype=np.int64)), **inp)
            mod.traf, mod.sim = traf, types.SimpleNamespace(simt=100.0)
            with np.errstate(all='ignore'):
                area.update()
            logged = area.logger.rows
            delidx = np.array([int(x[2:]) for x in logged[0][0]], dtype=np.int64) if logged else np.zeros(0, dtype=np.int64)
            rest = deleted
            if len(delidx):                               # traf.delete(delidx) first, then traf.delete(list(delidxalt))
                assert np.array_equal(deleted[0], delidx)
                rest = deleted[1:]
            delidxalt = rest[0] if rest else np.zeros(0, dtype=np.int64)
            st1, d1, d2 = exparea_np.update(st0, dt=0.5, area=AREAS.get(aname), active=active, swtaxi=swtaxi,
                                            swtaxialt=TAXIALT, **inp)
            assert np.array_equal(d1, delidx) and np.array_equal(d2, delidxalt), (n, case)
            for k in exparea_np.ARRAYS:
                assert np.array_equal(np.asarray(getattr(area, k)), st1[k], equal_nan=True), (n, case, k)
            seen_both = seen_both or len(set(d1) & set(d2)) > 0
            name = 'n%d_%s' % (n, case)
            out.update({name + '_out_' + k: st1[k] for k in exparea_np.ARRAYS})
            out.update({name + '_delidx': delidx, name + '_delidxalt': delidxalt,
                        name + '_flags': np.array([swtaxi, active]), name + '_area': np.array(aname or '')})
            names.append(name)
            print('exparea_update %-12s exits %3d taxi %3d' % (name, len(delidx), len(delidxalt)))
    assert seen_both
    out.update(names=np.array(names), swtaxialt=TAXIALT, dt=0.5)
    path = os.path.join(OUT, 'exparea_update.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1000000
    print('exparea_update.npz %d bytes' % os.path.getsize(path))


FLIGHT_STEPS, SIMDT, AREA_DT = 384, 0.0625, 0.5
FLIGHT_BOX = ('BOX', np.array([51.9, 3.85, 52.1, 4.15]), 30000 * FT, 1000 * FT)


def run_flight(seed=83):
    """exparea_flight64: 64 aircraft, simdt 0.0625, Pilot.APorASAS -> UpdateAirSpeed / GroundSpeed / Position with
    the reference's own methods and constant autopilot targets (no turns; some accelerate, some descend), and the
    reference's Area on a BOX, TAXI OFF (swtaxi False), dt 0.5: ``update()`` after every 8th step with ``sim.simt``
    that step's time before its increment.  ``traf.delete`` is np.delete on every array of the stand-ins and on the
    Area's own (TrafficArrays.delete).  Aircraft start just inside a face flying outwards, at staggered distances,
    so the exits are spread over the run; descenders start just above swtaxialt."""
    from bluesky.traffic.pilot import Pilot
    mod = load_ref_area()
    rng = np.random.default_rng(seed)
    n = 64
    every = int(AREA_DT / SIMDT)
    c = FLIGHT_BOX[1]
    hdg = rng.choice([0., 90., 180., 270.], n)
    tas = rng.uniform(140., 240., n)
    dist = rng.uniform(150., 4500., n)                              # metres inside the face the aircraft flies to
    lat, lon = rng.uniform(c[0] + 0.06, c[2] - 0.06, n), rng.uniform(c[1] + 0.09, c[3] - 0.09, n)
    mlat, mlon = 111194.9, 111194.9 * np.cos(np.radians(CLAT))
    lat = np.where(hdg == 0., c[2] - dist / mlat, np.where(hdg == 180., c[0] + dist / mlat, lat))
    lon = np.where(hdg == 90., c[3] - dist / mlon, np.where(hdg == 270., c[1] + dist / mlon, lon))
    alt = rng.uniform(3000 * FT, 20000 * FT, n)
    outside = np.arange(n) % 9 == 4                                  # never seen inside: never an exit
    lat[outside] += 1.0
    slow = np.arange(n) % 7 == 3                                     # stay inside to the end
    dist_far = slow & ~outside
    lat[dist_far], lon[dist_far] = CLAT, CLON
    desc = np.arange(n) % 5 == 2                                     # sink through swtaxialt
    alt[desc] = TAXIALT + rng.uniform(2., 90., desc.sum())
    ap_alt = np.where(desc, 500 * FT, alt)
    ap_tas = tas + rng.choice([0.0, 15.0, -10.0], n)
    init = dict(lat=lat, lon=lon, alt=alt, tas=tas, hdg=hdg, vs=np.zeros(n), gs=tas.copy(), trk=hdg.copy(),
                gseast=tas * np.sin(np.radians(hdg)), gsnorth=tas * np.cos(np.radians(hdg)), ap_trk=hdg.copy(), ap_tas=ap_tas,
                ap_alt=ap_alt, ap_vs=np.full(n, 1500. * FT / 60.), selalt=ap_alt.copy(), bank=np.full(n, np.radians(25.)),
                eps=np.full(n, 0.01), accel=np.full(n, 0.5), asas_alt=alt.copy())
    init = {k: np.array(v, dtype=np.float64) for k, v in init.items()}
    thrust = np.zeros(n)                                             # no OpenAP forces in this loop: work stays 0
    traf = types.SimpleNamespace(**{k: init[k].copy() for k in ('lat', 'lon', 'alt', 'tas', 'hdg', 'vs', 'gs', 'trk', 'bank', 'eps')})
    traf.id = ['AC%02d' % k for k in range(n)]
    traf.ntraf = n
    traf.ap = types.SimpleNamespace(trk=init['ap_trk'].copy(), tas=init['ap_tas'].copy(), alt=init['ap_alt'].copy(), vs=init['ap_vs'].copy())
    traf.asas = types.SimpleNamespace(active=np.zeros(n, dtype=bool), trk=hdg.copy(), tas=tas.copy(), alt=alt.copy(), vs=np.zeros(n))
    traf.pilot = Pilot.__new__(Pilot)
    traf.wind = mg.WindSim()
    hold = dict(acc=np.full(n, 0.5))
    traf.perf = types.SimpleNamespace(acceleration=lambda: hold['acc'], thrust=thrust.copy())
    ref_af.areas['EXP'] = mga.ref_object('EXP', *FLIGHT_BOX)
    area = mod.Area()
    area.name, area.active, area.swtaxi, area.swtaxialt, area.dt = 'EXP', True, False, TAXIALT, AREA_DT
    sim = types.SimpleNamespace(simt=0.0)
    mod.traf, mod.sim = traf, sim
    for k in exparea_np.ARRAYS + ('create_time',):                   # Area.create for every aircraft at simt 0
        setattr(area, k, np.zeros(n, dtype=bool) if k == 'inside' else np.zeros(n))
    area.oldalt = traf.alt.copy()
    calls = []

    def delete(idx):
        calls.append(np.array(idx, dtype=np.int64))
        for obj in (traf, traf.ap, traf.asas, traf.perf, traf.pilot, area):
            for name, v in list(vars(obj).items()):
                if isinstance(v, np.ndarray) and v.shape[:1] == (traf.ntraf,):
                    setattr(obj, name, np.delete(v, idx))
        hold['acc'] = np.delete(hold['acc'], idx)
        gone = set(int(k) for k in np.atleast_1d(idx))
        traf.id = [x for k, x in enumerate(traf.id) if k not in gone]
        traf.ntraf = len(traf.lat)

    traf.delete = delete
    saved = getattr(bs, 'traf', None)
    bs.traf = traf
    events, both, stale = [], 0, 0
    st = {k: getattr(area, k).copy() for k in exparea_np.ARRAYS}
    try:
        with np.errstate(all='ignore'):
            for step in range(FLIGHT_STEPS):
                Pilot.APorASAS(traf.pilot)
                mg.RefTraffic.UpdateAirSpeed(traf, SIMDT, sim.simt)
                mg.RefTraffic.UpdateGroundSpeed(traf, SIMDT)
                mg.RefTraffic.UpdatePosition(traf, SIMDT)
                if (step + 1) % every == 0:
                    ids, ntraf = list(traf.id), traf.ntraf
                    del calls[:]
                    nrows = len(area.logger.rows)
                    st, d1, d2 = exparea_np.update(st, traf.gs, traf.vs, traf.alt, traf.lat, traf.lon, traf.perf.thrust, AREA_DT,
                                                   FLIGHT_BOX, True, False, TAXIALT)
                    assert margins_ok(FLIGHT_BOX, traf.lat, traf.lon), 'a point within the margin: change the seed'
                    area.update()
                    left = exparea_np.delete_sequence(ntraf, d1, d2)
                    assert [ids[k] for k in left] == traf.id, step
                    st = {k: np.array(v)[left] for k, v in st.items()}
                    for k in exparea_np.ARRAYS:
                        assert np.array_equal(st[k], getattr(area, k)), (step, k)
                    assert (len(area.logger.rows) > nrows) == (len(d1) > 0)
                    if len(d1) or len(d2):
                        events.append(dict(step=step + 1, simt=sim.simt, delidx=d1, delidxalt=d2,
                                           row=area.logger.rows[-1] if len(d1) else None))
                        both += bool(len(d1) and len(d2))
                        stale += bool(len(d1) and len(d2) and d2.max() >= d1.min())
                sim.simt += SIMDT
    finally:
        bs.traf = saved
    nexit = sum(len(e['delidx']) for e in events)
    assert nexit >= 12 and both >= 1 and stale >= 1 and len(set(e['step'] for e in events)) >= 8, (nexit, both, stale)
    out = {'init_' + k: v for k, v in init.items()}
    out.update(thrust=thrust, simdt=SIMDT, dt=AREA_DT, every=every, nsteps=FLIGHT_STEPS, swtaxialt=TAXIALT,
               area_type=np.array(FLIGHT_BOX[0]), area_coords=FLIGHT_BOX[1], area_levels=np.array(FLIGHT_BOX[2:]),
               ids=np.array(['AC%02d' % k for k in range(n)]), survivors=np.array(traf.id),
               ev_step=np.array([e['step'] for e in events]), ev_simt=np.array([e['simt'] for e in events]),
               ev_off=np.cumsum([0] + [len(e['delidx']) for e in events]),
               ev_offalt=np.cumsum([0] + [len(e['delidxalt']) for e in events]),
               ev_delidx=np.concatenate([e['delidx'] for e in events]).astype(np.int64),
               ev_delidxalt=np.concatenate([e['delidxalt'] for e in events]).astype(np.int64),
               numpy_version=np.array(np.__version__))
    for q, name in enumerate(exparea_np.LOG_COLUMNS):                # the logger's arguments, concatenated over the events
        col = [e['row'][q] for e in events if e['row'] is not None]
        out['log_' + name] = np.concatenate(col)
    for k in ('lat', 'lon', 'alt', 'tas', 'hdg', 'vs'):
        out['final_' + k] = getattr(traf, k)
    out.update({'final_' + k: getattr(area, k) for k in exparea_np.ARRAYS + ('create_time',)})
    path = os.path.join(OUT, 'exparea_flight64.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1000000
    print('exparea_flight64.npz: %d exits over %d updates (%d with both lists, %d with a stale index), %d left, %d bytes'
          % (nexit, len(events), both, stale, traf.ntraf, os.path.getsize(path)))


if __name__ == '__main__':
    run_update()
    for seed in range(83, 123):                                      # the first seed whose run has every wanted event
        try:
            run_flight(seed)
            break
        except (AssertionError, IndexError) as e:          # (IndexError: a stale index past the shrunk table, the reference raises)
            print('seed %d: %s' % (seed, e))
    else:
        raise SystemExit('no seed gave a flight with every wanted event')
