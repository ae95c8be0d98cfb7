"""numpy restatement of the waypoint recovery ``ASAS.ResumeNav`` starts for an
ownship whose resopair it drops (asas.py:459-465): ``Route.findact``
(route.py:1043-1079) and ``Route.direct`` (route.py:635-688) with the whole of
``Autopilot.ComputeVNAV`` (autopilot.py:207-304), over plain arrays and the
route table of ``bluesky_amd.fms.route_table``, expression by expression in
the reference's operation order.

TEST INFRASTRUCTURE ONLY: the expected values of the device kernels
(bsa_fms_recover, k_sim_recover).  tools/make_golden.py asserts it bitwise
equal to the reference's own ``Route`` / ``Autopilot`` objects when it captures
tests/golden/fms_recover2000.npz and (composed, tests/recover_cases.py) fms_recover_flight.npz.

Unlike the tick (tests/fms_np.py), ``ComputeVNAV``'s writes of ``ap.alt`` and
``actwp.vs`` are restated: ``direct`` runs after ``ap.update``, and
``Pilot.APorASAS`` of the same step reads ``ap.alt``.  ``wpdirfrom`` is derived
from the table's ``nextqdr`` column (``calcfp``, route.py:1005-1012).
"""
import numpy as np

try:
    from . import fms_np
except ImportError:          # imported as a top-level module
    import fms_np

NM, FT, G0, STEEPNESS = fms_np.NM, fms_np.FT, fms_np.G0, fms_np.STEEPNESS
R_LAT, R_LON, R_ALT, R_SPD, R_XTOALT, R_TOALT, R_FLYBY, R_NEXTQDR = range(8)

TRAFFIC = ('lat', 'lon', 'alt', 'tas', 'gs', 'trk', 'bank')          # read only
# everything a recovery may change
OUTPUTS = ('actwp_lat', 'actwp_lon', 'actwp_nextaltco', 'actwp_xtoalt', 'actwp_spd', 'actwp_vs', 'actwp_turndist',
           'actwp_flyby', 'dist2vs', 'selspd', 'ap_alt', 'swlnav', 'swvnav', 'iactwp')
# what it reads or writes of the FMS: direct sets neither next_qdr nor (outside ComputeVNAV) nextaltco
UNTOUCHED = ('actwp_next_qdr', 'vnavvs', 'swvnavvs', 'selvs', 'apvsdef', 'abco', 'belco', 'ap_trk', 'ap_tas', 'ap_vs',
             'selalt')


def wpdirfrom(route, i):
    """``Route.wpdirfrom[i]`` from the table's nextqdr column."""
    nwp = len(route)
    if i + 1 < nwp:
        return route[i, R_NEXTQDR]
    return route[nwp - 2, R_NEXTQDR] if nwp > 1 else 0.


def findact(s, i, route, m=None, info=None):
    """route.py:1043-1079 for aircraft i with its rows ``route``."""
    nwp = len(route)
    if nwp <= 0:
        return -1
    elif nwp == 1:
        return 0
    coslat = np.cos(np.deg2rad(s['lat'][i]))             # traffic.py:482
    dy = (route[:, R_LAT] - s['lat'][i])
    dx = (route[:, R_LON] - s['lon'][i]) * coslat
    dist2 = dx * dx + dy * dy
    near = int(np.argmin(dist2))
    iwpnear = max(int(s['iactwp'][i]), near)
    if m is not None:
        others = np.delete(dist2, near)
        m.add(others, np.full(len(others), dist2[near]), rows=np.full(len(others), i))
    if info is not None:
        info['argmin'] = near
        info['turntest'] = 0                              # 0 none, 1 does not advance, 2 advances
    if iwpnear + 1 < nwp:
        qdr = np.degrees(np.arctan2(dx[iwpnear], dy[iwpnear]))
        delhdg = abs(fms_np.degto180(s['trk'][i] - qdr))
        tas, bank = s['tas'][i], s['bank'][i]
        with np.errstate(divide='ignore', invalid='ignore'):
            time_turn = max(0.01, tas) * np.radians(delhdg) / (G0 * np.tan(bank))
            time_straight = np.sqrt(dist2[iwpnear]) * 60. * NM / max(0.01, tas)
        if m is not None:
            m.add(time_turn, time_straight, rows=[i])
        if info is not None:
            info['turntest'] = 2 if time_turn > time_straight else 1
            info['time_turn'] = float(time_turn)
        if time_turn > time_straight:
            iwpnear += 1
    return iwpnear


def compute_vnav(s, i, toalt, xtoalt, m=None, info=None):
    """autopilot.py:207-304 for aircraft i, whole (``ap.alt`` and ``actwp.vs``
    included).  ``info['vnav']``: 1 toalt < 0, 2 VNAV off, 3 descent, 6 urgent
    descent, 4 climb, 5 level."""
    if toalt < 0 or not s['swvnav'][i]:
        s['dist2vs'][i] = -999.
        if info is not None:
            info['vnav'] = 1 if toalt < 0 else 2
        return
    alt, gs, tas = s['alt'][i], s['gs'][i], s['tas'][i]
    coslat = np.cos(np.deg2rad(s['lat'][i]))
    if m is not None:
        m.add([alt, alt], [toalt + 10. * FT, toalt - 10. * FT], rows=[i, i])
    if alt > toalt + 10. * FT:
        s['actwp_nextaltco'][i] = min(alt, toalt + xtoalt * STEEPNESS)
        s['actwp_xtoalt'][i] = xtoalt
        s['dist2vs'][i] = s['actwp_turndist'][i] + np.abs(alt - s['actwp_nextaltco'][i]) / STEEPNESS
        dy = (s['actwp_lat'][i] - s['lat'][i])
        dx = (s['actwp_lon'][i] - s['lon'][i]) * coslat
        legdist = 60. * NM * np.sqrt(dx * dx + dy * dy)
        if m is not None:
            m.add(legdist, s['dist2vs'][i], rows=[i])
        if legdist < s['dist2vs'][i]:
            s['ap_alt'][i] = s['actwp_nextaltco'][i]
            t2go = max(0.1, legdist + xtoalt) / max(0.01, gs)
            s['actwp_vs'][i] = (s['actwp_nextaltco'][i] - alt) / t2go
        else:
            s['actwp_vs'][i] = -STEEPNESS * (gs + (gs < 0.2 * tas) * tas)
        if info is not None:
            info['vnav'] = 6 if legdist < s['dist2vs'][i] else 3
    elif alt < toalt - 10. * FT:
        s['actwp_nextaltco'][i] = toalt
        s['actwp_xtoalt'][i] = xtoalt
        s['ap_alt'][i] = s['actwp_nextaltco'][i]
        s['dist2vs'][i] = 99999. * NM
        dy = (s['actwp_lat'][i] - s['lat'][i])
        dx = (s['actwp_lon'][i] - s['lon'][i]) * coslat
        legdist = 60. * NM * np.sqrt(dx * dx + dy * dy)
        t2go = max(0.1, legdist + xtoalt) / max(0.01, gs)
        s['actwp_vs'][i] = np.maximum(STEEPNESS * gs, (s['actwp_nextaltco'][i] - alt) / t2go)
        if info is not None:
            info['vnav'] = 4
    else:
        s['dist2vs'][i] = -999.
        if info is not None:
            info['vnav'] = 5


def direct(s, i, route, wpidx, m=None, info=None):
    """route.py:635-688 for aircraft i to its waypoint ``wpidx`` (the reference
    looks it up by name and takes the first match: the same index for a route
    with unique names)."""
    row = route[wpidx]
    s['iactwp'][i] = wpidx
    s['actwp_lat'][i] = row[R_LAT]
    s['actwp_lon'][i] = row[R_LON]
    s['actwp_flyby'][i] = row[R_FLYBY]
    compute_vnav(s, i, row[R_TOALT], row[R_XTOALT], m, info)
    wpspd, wpalt = row[R_SPD], row[R_ALT]
    if wpspd > 0.:
        if wpalt < 0.0:
            alt = s['alt'][i]
        else:
            alt = wpalt
        if wpspd < 2.0:
            cas = fms_np.mach2cas(float(wpspd), alt)
        else:
            cas = wpspd
        s['actwp_spd'][i] = cas
        if s['swvnav'][i]:
            s['selspd'][i] = cas
    else:
        s['actwp_spd'][i] = -999.
    with np.errstate(invalid='ignore', divide='ignore'):
        qdr, _ = fms_np.qdrdist(s['lat'][i], s['lon'][i], s['actwp_lat'][i], s['actwp_lon'][i])
    tas = s['tas'][i]
    turnrad = tas * tas / np.tan(np.radians(25.)) / G0 / NM
    dq = abs(fms_np.degto180(qdr - wpdirfrom(route, wpidx)))
    s['actwp_turndist'][i] = (s['actwp_flyby'][i] > 0.5) * turnrad * abs(np.tan(0.5 * np.radians(max(5., dq))))
    s['swlnav'][i] = True


def recover(state, rows, off, nwp, count, margins=None, info=None):
    """``findact`` + ``direct`` applied ``count[i]`` times in sequence to every
    aircraft i (once per resopair ResumeNav dropped for it in one call).
    ``state``: dict of the TRAFFIC arrays and the FMS arrays of fms_np; returns a
    new dict (inputs are not modified).  ``info``: a list that receives one dict
    per application (aircraft ``i``, application ``q``, iactwp ``before`` / ``after``,
    ``argmin``, ``turntest``, ``vnav``)."""
    s = {k: np.array(v) for k, v in state.items()}
    for k in fms_np.FLAGS:
        if k in s:
            s[k] = s[k].astype(bool)
    for i in np.flatnonzero(np.asarray(count) > 0):
        route = rows[off[i]:off[i] + nwp[i]]
        for q in range(int(count[i])):
            rec = None if info is None else dict(i=int(i), q=q, before=int(s['iactwp'][i]), vnav=0)
            iw = findact(s, i, route, margins, rec)
            if iw != -1:
                direct(s, i, route, iw, margins, rec)
            if rec is not None:
                rec['after'] = int(s['iactwp'][i])
                info.append(rec)
            if iw == -1:
                break
    return s


def near_threshold(state, rows, off, nwp, count, rel=1e-9):
    """Mask of the aircraft for which a discontinuous comparison of this recovery
    (the argmin's runner-up, time_turn > time_straight, alt vs toalt +- 10 ft,
    legdist < dist2vs) lies within ``rel`` relative of equality (min(alt, limit)
    and max(5, dq) are continuous)."""
    m = fms_np._Margins(len(state['lat']), rel)
    recover(state, rows, off, nwp, count, margins=m)
    return m.near
