#!/usr/bin/env python3
"""Capture tests/golden/adsb_update.npz and adsb_flight64.npz from the REFERENCE's own ``ADSB`` class
(traffic/adsbmodel.py; build container only).

``bs.traf`` is a stand-in with the seven arrays the model reads.  Only data is written.  tests/adsb_np.py is asserted
bitwise equal to the reference on every case here.  The unit normals the reference consumed are recovered by
re-seeding numpy and drawing the same three values with scale 1 (as ``make_golden.run_turb`` does).

adsb_update: single ``update(time)`` calls at n = 1, 63, 64, 65, 257, noise off / on, trunctime 0 / 5.  From n = 63 on
the hand-made rows are: 3 with lastupdate + trunctime exactly ``time`` (not updated), 4 one ulp below (updated), 8 one
ulp above (not updated), 5 with a NaN lastupdate (never updated), 6 more than two periods behind (advances by one
period only), 7 due with a NaN ``traf.lat`` (copied as NaN).  Case ``zero``: time 0, every lastupdate 0, trunctime 0 --
nobody updates.  Also ``create(3)`` on a non-empty object with the uniforms it drew, and ``SetNoise``'s resets.

adsb_flight64: the closed loop (``run_flight``), once with noise off and once with noise on.

Usage:  python tools/make_golden_adsb.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                     # noqa: E402  (numpy shims, sys.path: reference + repo)

import bluesky as bs                                         # noqa: E402
from bluesky.traffic.adsbmodel import ADSB as RefADSB        # noqa: E402
from tests import adsb_np                                    # noqa: E402

OUT = os.path.join(mg.REPO, 'tests', 'golden')
SEED = 20261022
T = 100.0
EDGE = dict(on=3, below=4, nan=5, behind=6, nanlat=7, above=8)


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        a[~np.isnan(a)].tobytes() == b[~np.isnan(b)].tobytes()


def ref_adsb(traf, st, noise, trunctime):
    bs.traf = traf
    ad = RefADSB()
    ad.SetNoise(noise)
    ad.trunctime = trunctime
    for k in adsb_np.ARRAYS:
        setattr(ad, k, np.array(st[k]))
    return ad


def drawn_update(ad, time, seed):
    """``ad.update(time)`` under a fixed numpy seed; returns the three unit normals it consumed (noise on)."""
    np.random.seed(seed)
    with np.errstate(invalid='ignore'):
        ad.update(time)
    if not ad.transnoise:
        return np.zeros(3)
    np.random.seed(seed)
    z = np.array([np.random.normal(0, 1, 1)[0] for _ in range(3)])
    np.random.seed(seed)                                     # the scaled draws follow from the unit ones, bitwise
    for q in range(3):
        s = ad.transerror[0 if q < 2 else 1]
        assert np.random.normal(0, s, 1)[0] == 0.0 + s * z[q]
    return z


def inputs(rng, n, trunctime):
    traf = {k: v for k, v in zip(adsb_np.FIELDS, (
        rng.uniform(-60., 60., n), rng.uniform(-179., 179., n), rng.uniform(1000., 11000., n), rng.uniform(0., 360., n),
        rng.uniform(120., 250., n), rng.uniform(120., 250., n), rng.uniform(-10., 10., n)))}
    st = {k: traf[k] + rng.uniform(-0.5, 0.5, n) for k in adsb_np.FIELDS}
    st['lastupdate'] = T - trunctime + rng.uniform(-3., 3., n)          # about half are due
    if n >= 63:
        lu = st['lastupdate']
        lu[EDGE['on']] = T - trunctime
        lu[EDGE['below']] = np.nextafter(T - trunctime, -np.inf)
        lu[EDGE['above']] = np.nextafter(T - trunctime, np.inf)
        lu[EDGE['nan']] = np.nan
        lu[EDGE['behind']] = T - 2 * trunctime - 1.0
        lu[EDGE['nanlat']], traf['lat'][EDGE['nanlat']] = T - trunctime - 1.0, np.nan
        for k in (63, 64, n - 1):                                        # a due aircraft each side of a wave's end
            if k < n:
                lu[k] = T - trunctime - 2.0
        assert lu[EDGE['on']] + trunctime == T and lu[EDGE['below']] + trunctime < T < lu[EDGE['above']] + trunctime
    else:
        st['lastupdate'][0] = T - trunctime - 1.0                        # the single aircraft is due
    return traf, st


def run_update():
    rng = np.random.default_rng(SEED)
    out, names = dict(time=T), []
    for n in (1, 63, 64, 65, 257):
        for noise in (False, True):
            for trunctime in (0, 5):
                traf, st0 = inputs(rng, n, trunctime)
                ad = ref_adsb(types.SimpleNamespace(**{k: v.copy() for k, v in traf.items()}), st0, noise, trunctime)
                z = drawn_update(ad, T, SEED + len(names))
                got = adsb_np.update(st0, traf, T, trunctime, noise, ad.transerror, z)
                for k in adsb_np.ARRAYS:
                    assert same(getattr(ad, k), got[k]), (n, noise, trunctime, k)
                name = 'n%d_noise%d_trunc%d' % (n, noise, trunctime)
                up = adsb_np.due(st0['lastupdate'], trunctime, T)
                if n >= 63:
                    s = set(up)
                    assert {EDGE['below'], EDGE['behind'], EDGE['nanlat']} <= s and \
                        not {EDGE['on'], EDGE['above'], EDGE['nan']} & s
                    assert got['lastupdate'][EDGE['behind']] == T - trunctime - 1.0 and np.isnan(got['lat'][EDGE['nanlat']])
                out.update({name + '_traf_' + k: v for k, v in traf.items()})
                out.update({name + '_in_' + k: v for k, v in st0.items()})
                out.update({name + '_out_' + k: np.asarray(getattr(ad, k)) for k in adsb_np.ARRAYS})
                out[name + '_z'] = z
                out[name + '_trunctime'] = np.float64(trunctime)
                names.append(name)
                print('adsb_update %-22s due %3d of %3d' % (name, len(up), n))
    # time 0 with all zeros: nobody updates
    traf, st0 = inputs(rng, 64, 0)
    st0['lastupdate'] = np.zeros(64)
    ad = ref_adsb(types.SimpleNamespace(**{k: v.copy() for k, v in traf.items()}), st0, True, 0)
    z = drawn_update(ad, 0.0, SEED + 100)
    for k in adsb_np.ARRAYS:
        assert same(getattr(ad, k), st0[k]) and same(adsb_np.update(st0, traf, 0.0, 0, True, ad.transerror, z)[k], st0[k])
    out.update({'zero_traf_' + k: v for k, v in traf.items()})
    out.update({'zero_in_' + k: v for k, v in st0.items()})
    out['zero_z'] = z
    # create(3) on a non-empty object (Traffic.create appended to traf first), trunctime 5
    traf, st0 = inputs(rng, 65, 5)
    more = inputs(rng, 3, 5)[0]
    traf3 = {k: np.append(traf[k], more[k]) for k in adsb_np.FIELDS}
    ad = ref_adsb(types.SimpleNamespace(**{k: v.copy() for k, v in traf3.items()}), st0, True, 5)
    np.random.seed(SEED + 200)
    ad.create(3)
    np.random.seed(SEED + 200)
    u = np.random.rand(3)
    got = adsb_np.create(st0, traf3, 3, 5, u)
    for k in adsb_np.ARRAYS:
        assert same(getattr(ad, k), got[k]), ('create', k)
    assert not got['vs'][-3:].any() and (got['lastupdate'][-3:] < 0).all()
    out.update({'create_traf_' + k: v for k, v in traf3.items()})
    out.update({'create_in_' + k: v for k, v in st0.items()})
    out.update({'create_out_' + k: np.asarray(getattr(ad, k)) for k in adsb_np.ARRAYS})
    out.update(create_u=u, create_trunctime=np.float64(5))
    # SetNoise's resets
    ad.transerror, ad.trunctime = [1.0, 2.0], 7
    rows = []
    for flag in (True, False):
        ad.SetNoise(flag)
        rows.append([float(ad.transnoise), float(ad.truncated), ad.transerror[0], ad.transerror[1], float(ad.trunctime)])
        assert (ad.transnoise, ad.truncated, ad.transerror, ad.trunctime) == adsb_np.set_noise(flag)
    out['setnoise'] = np.array(rows)
    out['names'] = np.array(names)
    path = os.path.join(OUT, 'adsb_update.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1000000
    print('adsb_update.npz %d bytes' % os.path.getsize(path))


FLIGHT_CALLS, SIMDT, TRUNC = 40, 1.0, 5


def run_flight(noise, seed=92):
    """adsb_flight64: 64 aircraft, simdt 1.0, trunctime 5, lastupdate staggered over one period as ``create`` leaves it.
    Per call, in Traffic.update's order: ``adsb.update(simt)`` on the state the previous step left, then
    Pilot.APorASAS -> UpdateAirSpeed / GroundSpeed / Position with the reference's own methods and constant autopilot
    targets; ``simt += simdt``.  The object's own arrays carry over from call to call."""
    from bluesky.traffic.pilot import Pilot
    rng = np.random.default_rng(seed)
    n = 64
    hdg, tas = rng.uniform(0., 360., n), rng.uniform(140., 240., n)
    lat, lon = rng.uniform(51., 53., n), rng.uniform(3., 5., n)
    alt = rng.uniform(3000 * 0.3048, 20000 * 0.3048, n)
    traf = types.SimpleNamespace(lat=lat, lon=lon, alt=alt, tas=tas.copy(), hdg=hdg.copy(), vs=np.zeros(n), gs=tas.copy(),
                                 trk=hdg.copy(), bank=np.full(n, np.radians(25.)), eps=np.full(n, 0.01))
    traf.ntraf = n
    traf.ap = types.SimpleNamespace(trk=hdg + rng.choice([0., 20., -35.], n), tas=tas + rng.choice([0., 15., -10.], n),
                                    alt=alt + rng.choice([0., 600., -900.], n), vs=np.full(n, 1500. * 0.3048 / 60.))
    traf.asas = types.SimpleNamespace(active=np.zeros(n, dtype=bool), trk=hdg.copy(), tas=tas.copy(), alt=alt.copy(),
                                      vs=np.zeros(n))
    traf.pilot = Pilot.__new__(Pilot)
    traf.wind = mg.WindSim()
    traf.perf = types.SimpleNamespace(acceleration=lambda: np.full(n, 0.5))
    st = {k: np.array(getattr(traf, k)) for k in adsb_np.FIELDS}
    st['vs'] = np.zeros(n)
    st['lastupdate'] = -TRUNC * rng.random(n)
    st0 = {k: v.copy() for k, v in st.items()}
    saved = getattr(bs, 'traf', None)
    hist = {k: [] for k in adsb_np.ARRAYS}
    seen = {k: [] for k in adsb_np.FIELDS}
    zs, ts, ndue = [], [], []
    try:
        ad = ref_adsb(traf, st, noise, TRUNC)
        simt = 0.0
        with np.errstate(all='ignore'):
            for call in range(FLIGHT_CALLS):
                now = {k: np.array(getattr(traf, k)) for k in adsb_np.FIELDS}
                ndue.append(len(adsb_np.due(st['lastupdate'], TRUNC, simt)))
                z = drawn_update(ad, simt, SEED + 1000 + call)
                st = adsb_np.update(st, now, simt, TRUNC, noise, ad.transerror, z)
                for k in adsb_np.ARRAYS:
                    assert same(getattr(ad, k), st[k]), (call, k)
                    hist[k].append(st[k])
                for k in adsb_np.FIELDS:
                    seen[k].append(now[k])
                zs.append(z)
                ts.append(simt)
                Pilot.APorASAS(traf.pilot)
                mg.RefTraffic.UpdateAirSpeed(traf, SIMDT, simt)
                mg.RefTraffic.UpdateGroundSpeed(traf, SIMDT)
                mg.RefTraffic.UpdatePosition(traf, SIMDT)
                simt += SIMDT
    finally:
        bs.traf = saved
    print('adsb_flight64 noise %d: due per call %s' % (noise, ndue))
    assert 0 < min(ndue[1:]) and max(ndue) < n and sum(ndue) > 4 * n
    out = dict(z=np.array(zs), **{'hist_' + k: np.array(v) for k, v in hist.items()})
    common = dict(t=np.array(ts), ndue=np.array(ndue), **{'traf_' + k: np.array(v) for k, v in seen.items()})
    common.update({'init_' + k: v for k, v in st0.items()})
    return out, common


if __name__ == '__main__':
    run_update()
    off, common = run_flight(False)
    on, common2 = run_flight(True)
    for k in common:                                                # the picture feeds nothing back into the traffic
        assert np.asarray(common[k]).tobytes() == np.asarray(common2[k]).tobytes(), k
    out = dict(common, simdt=SIMDT, trunctime=np.float64(TRUNC), transerror=np.array(adsb_np.TRANSERROR), ncalls=FLIGHT_CALLS,
               numpy_version=np.array(np.__version__))
    out.update({'off_' + k: v for k, v in off.items() if k != 'z'})
    out.update({'on_' + k: v for k, v in on.items()})
    path = os.path.join(OUT, 'adsb_flight64.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1000000
    print('adsb_flight64.npz %d bytes' % os.path.getsize(path))
