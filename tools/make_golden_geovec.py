#!/usr/bin/env python3
"""Capture tests/golden/geovec_apply.npz from the REFERENCE geovector plugin (build container only).

Imports plugins/geovector.py itself, points its ``traf`` at a fake traffic object, puts the
reference's own ``Box`` / ``Circle`` / ``Poly`` / ``Line`` objects straight into
``areafilter.areas`` (``defineArea`` needs ``bs.scr``), defines several geovector lists with
``defgeovec`` and runs ``applygeovec`` on 1000 aircraft around 52 N 4 E.  Stores the shapes, the
traffic, every list as ``defgeovec`` left it (``None`` as NaN plus a mask) and the four arrays
after each list -- arrays only.  The numpy restatement tests/geovec_np.py is asserted bitwise equal
on all four arrays at capture.  A ``defgeovec`` / ``delgeovec`` / query sequence is recorded with
the reference's return values and the list after every call.

The first 64 aircraft hold the exact-border rows (trk == a track bound, vs == a V/S bound, selspd
== the clamp value: each triggers nothing) and NaN lat / alt / vs / trk rows.  For the random
aircraft the capture ASSERTS the margins that make the device comparison exact: none within 1e-6
relative of a casmin / casmax, none within 1e-9 deg of a track bound or 1e-9 m/s of a V/S bound,
and the area margins of tools/make_golden_area.py; every limit of the six-limit list changes at
least 20 aircraft and leaves at least 20 inside aircraft alone.  If an assertion fires, change the
seed, not the margin.

Usage:  python tools/make_golden_geovec.py
"""
import os
import sys
import types

import numpy as np

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT = os.path.join(REPO, 'tests', 'golden', 'geovec_apply.npz')
AREAS = os.path.join(REPO, 'tests', 'golden', 'area_shapes.npz')

# numpy-2 shims for the 2019 reference
np.mat = np.asmatrix
np.int = int
np.float = float
np.object = object
np.str = str
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REF, 'plugins'))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from bluesky.tools import areafilter as ref_area      # noqa: E402
from bluesky.tools.aero import vtas2cas as ref_cas    # noqa: E402
from bluesky.tools.misc import degto180 as ref_180    # noqa: E402
import geovector as ref                               # noqa: E402  (plugins/geovector.py)
from tests import area_np, geovec_np                  # noqa: E402
from make_golden_area import ref_object, seg_dist     # noqa: E402

FT = 0.3048
SEED = 20261020
N, NSPECIAL = 1000, 64
MARGIN = 1e-9
MARGIN_CAS = 1e-6
USED = ('BOXSWAP', 'CIRC', 'C', 'SEAM', 'LINE')     # of area_shapes.npz (SEAM: kAreaChunk + 1 vertices)
BOX_ALL = ('BOXSWAP', 210., 150., 100., 200., 5., -5.)   # speed and V/S given max first: defgeovec swaps them

# name -> the defgeovec calls that build the list
LISTS = [
    ('box_all', [BOX_ALL]),
    ('circle_wrap', [('CIRC', None, None, 350., 30., None, None)]),
    ('gsmax_only', [('BOXSWAP', None, 120., None, None, None, None)]),
    ('vsmin_negative', [('CIRC', None, None, None, None, -3., None)]),
    ('overlap_ab', [('BOXSWAP', 150., 210., None, None, None, None), ('CIRC', 100., 140., None, None, None, None)]),
    ('overlap_ba', [('CIRC', 100., 140., None, None, None, None), ('BOXSWAP', 150., 210., None, None, None, None)]),
    ('zero_is_off', [('BOXSWAP', None, 160., 0., 90., -4., 0.)]),
    ('line_and_missing', [('LINE', 100., 120., 10., 20., -1., 1.), ('NOSUCH', 100., 120., 10., 20., -1., 1.)]),
    ('poly_seam', [('SEAM', 130., None, 200., 300., None, 2.)]),
    ('three_areas', [('C', None, 170., 45., 135., None, None), ('SEAM', 120., None, None, None, -6., 6.),
                     ('CIRC', None, 150., 300., 60., None, 4.)]),
]


def fake_traf(st):
    t = types.SimpleNamespace(ntraf=len(st['lat']), ap=types.SimpleNamespace(trk=st['ap_trk'].copy()))
    for k in ('lat', 'lon', 'alt', 'trk', 'vs', 'selspd', 'selvs', 'selalt'):
        setattr(t, k, st[k].copy())
    return t


def define(calls):
    ref.reset()
    for c in calls:
        assert ref.defgeovec(*c) is True, c
    return [list(v) for v in ref.geovecs]


def flatten(lists):
    """[[area, six limits]] lists -> offsets, areas, limits (None as NaN), None mask"""
    off, area, lim = [0], [], []
    for rows in lists:
        for r in rows:
            area.append(r[0])
            lim.append(r[1:])
        off.append(len(area))
    none = np.array([[x is None for x in r] for r in lim], dtype=bool).reshape(-1, 6)
    val = np.array([[np.nan if x is None else float(x) for x in r] for r in lim], dtype=np.float64).reshape(-1, 6)
    return np.array(off, dtype=np.int64), np.array(area if area else [''], dtype=str)[:len(area)], val, none


def main():
    ga = dict(np.load(AREAS))
    all_names = [str(x) for x in ga['names']]
    shapes_all = area_np.load_shapes(ga)
    shapes = [shapes_all[all_names.index(k)] for k in USED]
    ref_area.areas.clear()
    for name, (typ, co, top, bottom) in zip(USED, shapes):
        ref_area.areas[name] = ref_object(name, area_np.TYPE_NAMES[typ], co, top, bottom)
    areas = dict(zip(USED, area_np.named(shapes)))

    rng = np.random.RandomState(SEED)
    st = dict(lat=rng.uniform(51.0, 53.0, N), lon=rng.uniform(2.5, 5.5, N), alt=rng.uniform(0.0, 42000 * FT, N),
              trk=rng.uniform(0.0, 360.0, N), vs=rng.normal(0.0, 6.0, N), selspd=rng.uniform(60.0, 230.0, N),
              selvs=rng.normal(0.0, 4.0, N))
    st['ap_trk'] = (st['trk'] + rng.normal(0.0, 5.0, N)) % 360.0
    st['selalt'] = st['alt'] + rng.choice([0.0, 600.0, -900.0], N)

    # the special rows: inside BOXSWAP, CIRC and SEAM alike, harmless for every limit but the one they sit on
    k = np.arange(NSPECIAL)
    st['lat'][k], st['lon'][k], st['alt'][k] = 52.0, 4.0, 25000 * FT
    st['trk'][k], st['vs'][k], st['selspd'][k] = 150.0, 0.0, 100.0
    gsmin, gsmax, trkmin, trkmax, vsmin, vsmax = 150., 210., 100., 200., -5., 5.    # BOX_ALL as defgeovec stores it
    casmin = ref_cas(np.ones(1) * gsmin, st['alt'][:1])[0]
    casmax = ref_cas(np.ones(1) * gsmax, st['alt'][:1])[0]
    assert casmin < 140.0 < casmax
    st['selspd'][k] = 140.0
    special = {0: ('trk', trkmin), 1: ('trk', trkmax), 2: ('vs', vsmin), 3: ('vs', vsmax), 4: ('selspd', casmin),
               5: ('selspd', casmax), 6: ('trk', 350.0), 7: ('trk', 30.0), 8: ('lat', np.nan), 9: ('alt', np.nan),
               10: ('vs', np.nan), 11: ('trk', np.nan), 12: ('lon', np.nan), 13: ('vs', -3.0)}
    for row, (field, value) in special.items():
        st[field][row] = value
    # ... and neighbours just outside each border, which do trigger: one ulp for V/S and speed, 1e-9 deg for the
    # track (degto180 adds 180 first, which swallows anything below half an ulp of 180)
    st['trk'][14], st['trk'][15] = trkmin - 1e-9, trkmax + 1e-9
    st['vs'][16], st['vs'][17] = np.nextafter(vsmin, -10.0), np.nextafter(vsmax, 10.0)
    st['selspd'][18], st['selspd'][19] = np.nextafter(casmin, 0.0), np.nextafter(casmax, 1000.0)

    # ---- margins of the random aircraft
    rnd = slice(NSPECIAL, N)
    lat, lon, alt = st['lat'][rnd], st['lon'][rnd], st['alt'][rnd]
    m_edge = m_face = m_rim = m_level = np.inf
    for name, (typ, co, top, bottom) in zip(USED, shapes):
        tn = area_np.TYPE_NAMES[typ]
        if tn != 'LINE':
            m_level = min(m_level, np.abs(alt - top).min(), np.abs(alt - bottom).min())
        if tn == 'BOX':
            m_face = min(m_face, np.abs(lat - co[0]).min(), np.abs(lat - co[2]).min(), np.abs(lon - co[1]).min(),
                         np.abs(lon - co[3]).min())
        elif tn == 'CIRCLE':
            d = ref_area.kwikdist(co[0], co[1], lat, lon)
            m_rim = min(m_rim, (np.abs(d - co[2]) / co[2]).min())
        elif tn == 'POLY':
            v = co.reshape(-1, 2)
            for q in range(len(v)):
                m_edge = min(m_edge, seg_dist(lat, lon, v[q - 1, 0], v[q - 1, 1], v[q, 0], v[q, 1]).min())
    assert m_edge >= MARGIN and m_face >= MARGIN and m_rim >= MARGIN and m_level >= MARGIN, \
        'area margins (%g %g %g %g): change SEED' % (m_edge, m_face, m_rim, m_level)

    lists = [(name, define(calls)) for name, calls in LISTS]
    m_cas = m_trk = m_vs = np.inf
    for name, rows in lists:
        for area, a, b, c, d, e, f in rows:
            for g in (a, b):
                if g:
                    cas = ref_cas(np.ones(N - NSPECIAL) * g, alt)
                    m_cas = min(m_cas, (np.abs(st['selspd'][rnd] - cas) / cas).min())
            if c and d:
                for g in (c, d):
                    m_trk = min(m_trk, np.abs(ref_180(st['trk'][rnd] - g)).min())
            for g in (e, f):
                if g:
                    m_vs = min(m_vs, np.abs(st['vs'][rnd] - g).min())
    assert m_cas >= MARGIN_CAS, 'a random selspd within %g relative of a clamp value (%g): change SEED' % (MARGIN_CAS, m_cas)
    assert m_trk >= MARGIN, 'a random track within %g deg of a bound (%g): change SEED' % (MARGIN, m_trk)
    assert m_vs >= MARGIN, 'a random V/S within %g m/s of a bound (%g): change SEED' % (MARGIN, m_vs)

    # ---- every limit of the six-limit list acts on >= 20 aircraft and leaves >= 20 inside ones alone
    inside = ref_area.checkInside('BOXSWAP', st['lat'], st['lon'], st['alt'])
    cmin, cmax = ref_cas(np.ones(N) * gsmin, st['alt']), ref_cas(np.ones(N) * gsmax, st['alt'])
    with np.errstate(invalid='ignore'):
        acts = dict(gsmin=st['selspd'] < cmin, gsmax=st['selspd'] > cmax, trkmin=ref_180(st['trk'] - trkmin) < 0,
                    trkmax=ref_180(st['trk'] - trkmax) > 0, vsmin=st['vs'] < vsmin, vsmax=st['vs'] > vsmax)
    for lim, m in acts.items():
        assert (inside & m).sum() >= 20 and (inside & ~m).sum() >= 20, \
            '%s: acts on %d, leaves %d inside: change SEED' % (lim, (inside & m).sum(), (inside & ~m).sum())

    # ---- the reference's applygeovec, list by list, and the restatement
    out = {k: np.zeros((len(lists), N)) for k in geovec_np.TARGETS}
    counts = np.zeros((len(lists), 4), dtype=np.uint64)
    for q, (name, rows) in enumerate(lists):
        ref.geovecs = [list(r) for r in rows]
        t = fake_traf(st)
        ref.traf = t
        with np.errstate(invalid='ignore'):
            ref.applygeovec()
        got = dict(selspd=t.selspd, ap_trk=t.ap.trk, selvs=t.selvs, selalt=t.selalt)
        for f in ('lat', 'lon', 'alt', 'trk', 'vs'):
            assert np.array_equal(getattr(t, f), st[f], equal_nan=True), f     # traffic state is never written
        mine = geovec_np.apply(rows, areas, st)
        for f in geovec_np.TARGETS:
            assert np.array_equal(mine[f].view(np.uint64), got[f].view(np.uint64)), (name, f)
            out[f][q] = got[f]
        counts[q], masks = geovec_np.changed(st, got)
        quiet = {'box_all': [0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12], 'circle_wrap': [6, 7, 8, 9, 11, 12],
                 'vsmin_negative': [8, 9, 10, 12, 13]}.get(name, [8, 9, 12])
        for f, m in masks.items():
            assert not m[quiet].any(), (name, f, np.flatnonzero(m[quiet]))     # on a border, or NaN: nothing triggers
        print('%-17s %d geovectors  changed selspd %4d  ap_trk %4d  selvs %4d  selalt %4d' % ((name, len(rows)) + tuple(counts[q])))
    names = [n for n, _ in lists]
    ab, ba = names.index('overlap_ab'), names.index('overlap_ba')
    assert not np.array_equal(out['selspd'][ab], out['selspd'][ba]), 'the two orders must differ'
    assert counts[names.index('line_and_missing')].sum() == 0
    z = names.index('zero_is_off')
    assert counts[z][1] == 0 and counts[z][0] > 0 and counts[z][2] > 0     # no track limit; gsmax and vsmin act
    assert (out['selvs'][z] <= st['selvs'].max()).all() and not (out['selvs'][z] == 0.0).any()
    box = names.index('box_all')
    assert out['ap_trk'][box][14] == trkmin and out['ap_trk'][box][15] == trkmax
    assert out['selvs'][box][16] == vsmin and out['selvs'][box][17] == vsmax
    assert out['selspd'][box][18] == casmin and out['selspd'][box][19] == casmax

    # ---- the bookkeeping sequence: op, area, limits -> ok, message, the list after it
    seq = [('def', 'A1', (100., 200., None, None, None, None)), ('def', 'B2', (None, None, 350., 10., None, None)),
           ('def', 'a1', (250., 150., None, None, 4., -4.)),           # replaces A1 (upper-case compare), swaps both
           ('def', 'A1', (None,) * 6), ('def', 'a1', (None,) * 6),     # queries, matched upper-case
           ('def', 'C3', (None,) * 6),                                 # ... and one that finds nothing
           ('def', '', (100., None, None, None, None, None)),         # no area
           ('def', 'C3', (None, None, 0., 90., None, None)),           # trkmin 0: no limit at all, so a query
           ('def', 'C3', (None, 120., 0., 90., None, 0.)),             # kept as given: the zeros stay in the list
           ('def', 'D4', (None, None, 20., 10., 5., None)),            # the track pair is not swapped
           ('del', 'b2', None), ('del', 'B2', None), ('del', 'NOPE', None), ('def', 'D4', (None,) * 6)]
    ref.reset()
    bk_ok, bk_msg, bk_lists = [], [], []
    for op, area, lim in seq:
        r = ref.defgeovec(area, *lim) if op == 'def' else ref.delgeovec(area)
        ok, msg = (r, '') if isinstance(r, bool) else r
        bk_ok.append(bool(ok))
        bk_msg.append(msg)
        bk_lists.append([list(v) for v in ref.geovecs])
    assert bk_ok.count(False) >= 4 and any(' uses ' in m for m in bk_msg)
    bl_off, bl_area, bl_val, bl_none = flatten(bk_lists)
    arg_val = np.array([[np.nan if (lim is None or x is None) else x for x in (lim or (None,) * 6)] for _, _, lim in seq])
    arg_none = np.array([[lim is None or x is None for x in (lim or (None,) * 6)] for _, _, lim in seq])

    l_off, l_area, l_val, l_none = flatten([rows for _, rows in lists])
    off = np.concatenate(([0], np.cumsum([len(s[1]) for s in shapes])))
    np.savez_compressed(
        OUT, names=np.array(USED), types=np.array([s[0] for s in shapes], dtype=np.int32),
        coords=np.concatenate([s[1] for s in shapes]), coord_off=off.astype(np.int64),
        top=np.array([s[2] for s in shapes]), bottom=np.array([s[3] for s in shapes]),
        list_names=np.array(names), list_off=l_off, gv_area=l_area, gv_limits=l_val, gv_none=l_none,
        changed=counts, nspecial=np.int64(NSPECIAL), special_rows=np.array(sorted(special), dtype=np.int64),
        margins=np.array([m_edge, m_face, m_rim, m_level, m_cas, m_trk, m_vs]), seed=np.int64(SEED),
        bk_op=np.array([s[0] for s in seq]), bk_area=np.array([s[1] for s in seq]), bk_arg=arg_val, bk_arg_none=arg_none,
        bk_ok=np.array(bk_ok), bk_msg=np.array(bk_msg), bk_list_off=bl_off, bk_list_area=bl_area,
        bk_list_limits=bl_val, bk_list_none=bl_none,
        **{k: st[k] for k in st}, **{'out_' + k: out[k] for k in out})
    print('margins: edge %.3g face %.3g rim %.3g level %.3g cas %.3g rel, trk %.3g deg, vs %.3g m/s'
          % (m_edge, m_face, m_rim, m_level, m_cas, m_trk, m_vs))
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
