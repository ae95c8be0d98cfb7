"""numpy restatement of the experiment area plugin (plugins/area.py:107-175): ``update`` is
``Area.update`` up to the two index lists, ``delete_sequence`` the two ``traf.delete`` calls that
follow, ``pilot_columns`` the four pilot columns of the log from what the resident step keeps.
Pinned bitwise against the reference's own class by tools/make_golden_exparea.py at capture and by
tests/test_exparea_np.py against the goldens."""
import numpy as np

from tests import area_np

FT = 0.3048
ARRAYS = ('distance2D', 'distance3D', 'work', 'oldalt', 'inside')
LOG_COLUMNS = ('id', 'create_time', 'flight_time', 'distance2D', 'distance3D', 'work', 'lat', 'lon', 'alt', 'tas', 'vs',
               'hdg', 'asas_active', 'pilot_alt', 'pilot_tas', 'pilot_vs', 'pilot_hdg')


def inside_of(area, lat, lon, alt):
    """areafilter.checkInside for ``area`` = (type, coordinates, top, bottom) or None (name None)."""
    if area is None:
        return np.zeros(len(lat), dtype=bool)
    typ = area_np.TYPE_NAMES.index('POLY' if str(area[0])[:4] == 'POLY' else str(area[0]))
    return area_np.inside(typ, area[1], area[2], area[3], lat, lon, alt)


def update(st, gs, vs, alt, lat, lon, thrust, dt, area, active=True, swtaxi=True, swtaxialt=1500 * FT):
    """One Area.update on ``st`` (dict of ARRAYS): (new st, delidx, delidxalt).  thrust None: work stays."""
    st = {k: np.array(st[k]) for k in ARRAYS}
    none = np.zeros(0, dtype=np.int64)
    if swtaxi and not active:                                                  # area.py:115
        return st, none, none
    with np.errstate(all='ignore'):
        resultantspd = np.sqrt(gs * gs + vs * vs)
        st['distance2D'] = st['distance2D'] + dt * gs
        st['distance3D'] = st['distance3D'] + dt * resultantspd
        if thrust is not None:
            st['work'] = st['work'] + (thrust * dt * resultantspd)
        if not swtaxi:
            delidxalt = np.where((st['oldalt'] >= swtaxialt) * (alt < swtaxialt))[0]
            st['oldalt'] = np.array(alt)
        else:
            delidxalt = none
        inside = inside_of(area, lat, lon, alt)
    delidx = np.where(np.array(st['inside']) * (np.array(inside) == False))[0]  # noqa: E712
    st['inside'] = inside
    return st, delidx, delidxalt


def delete_sequence(n, delidx, delidxalt):
    """The surviving original indices after ``traf.delete(delidx)`` and then ``traf.delete(list(delidxalt))``
    with delidxalt computed BEFORE the first delete (area.py:170-175): its indices are stale once the first
    delete removed anything.  An index past the shrunk table is dropped (the reference raises there)."""
    left = np.delete(np.arange(n), np.asarray(delidx, dtype=np.int64))
    second = np.array([k for k in np.asarray(delidxalt, dtype=np.int64) if k < len(left)], dtype=np.int64)
    return np.delete(left, second)


def pilot_columns(rec):
    """pilot.alt / tas / vs / hdg of Pilot.APorASAS without wind (pilot.py:37-48, 63) from a record of
    ``bsa_sim_exparea_poll`` (dict over _lib.EXPAREA_RECORD)."""
    act = np.asarray(rec['active']) != 0
    return dict(pilot_alt=np.where(act, rec['asas_alt'], rec['ap_alt']), pilot_tas=np.where(act, rec['asas_tas'], rec['ap_tas']),
                pilot_vs=np.abs(np.where(act, rec['asas_vs'], rec['ap_vs'])),
                pilot_hdg=np.where(act, rec['asas_trk'], rec['ap_trk']) % 360.)
