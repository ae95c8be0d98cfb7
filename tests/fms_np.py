"""numpy restatement of ``Autopilot.update`` (bluesky/traffic/autopilot.py:59-304)
over plain arrays and the route table of ``bluesky_amd.fms.route_table``, with
``ActiveWaypoint.Reached`` / ``calcturn`` (activewpdata.py:31-65), ``geo.qdrdist``
(geo.py:57-107), ``Route.getnextwp`` (route.py:778-800) and the scalar
``cas2mach`` / ``mach2cas`` (aero.py:178-239, 339-368), expression by
expression in the reference's operation order.

TEST INFRASTRUCTURE ONLY: the expected values of the device kernel
(bsa_fms_update).  tools/make_golden.py asserts it bitwise equal to the
reference's own ``Autopilot.update`` when it captures
tests/golden/fms_update2000.npz.

``ComputeVNAV`` writes ``ap.alt[i]`` and ``actwp.vs[i]``; the continuous part
overwrites both arrays whole in the same tick (autopilot.py:171, 182), so
those writes are never seen and are not restated.
"""
import math

import numpy as np

NM = 1852.
FT = 0.3048
G0 = 9.80665
RGAS = 287.05287
P0 = 101325.
RHO0 = 1.225
TSTRAT = 216.65
GAMMA = 1.40
STEEPNESS = 3000. * FT / (10. * NM)       # autopilot.py:21
FMS_DT = 1.01                             # autopilot.py:18

TRAFFIC = ('lat', 'lon', 'alt', 'tas', 'gs', 'trk', 'ax', 'bank')       # read only
ACTWP = ('actwp_lat', 'actwp_lon', 'actwp_nextaltco', 'actwp_xtoalt', 'actwp_spd', 'actwp_vs',
         'actwp_turndist', 'actwp_flyby', 'actwp_next_qdr')
REALS = ACTWP + ('dist2vs', 'vnavvs', 'swvnavvs', 'selspd', 'selvs', 'apvsdef')
FLAGS = ('swlnav', 'swvnav', 'abco', 'belco')
TARGETS = ('ap_trk', 'ap_tas', 'ap_alt', 'ap_vs', 'selalt')
# everything a tick may change (selvs / apvsdef / abco / belco are inputs only)
OUTPUTS = ACTWP + ('dist2vs', 'vnavvs', 'swvnavvs', 'selspd', 'swlnav', 'swvnav', 'iactwp') + TARGETS
# route-table columns
R_LAT, R_LON, R_ALT, R_SPD, R_XTOALT, R_TOALT, R_FLYBY, R_NEXTQDR = range(8)


def ticks(simt, t0):
    """autopilot.py:61: does the FMS part run at simt, given the last tick's t0?"""
    return t0 + FMS_DT < simt or simt < t0 or simt < FMS_DT


def rwgs84(latd):
    lat = np.radians(latd)
    a = 6378137.0
    b = 6356752.314245
    coslat = np.cos(lat)
    sinlat = np.sin(lat)
    an = a * a * coslat
    bn = b * b * sinlat
    ad = a * coslat
    bd = b * sinlat
    return np.sqrt((an * an + bn * bn) / (ad * ad + bd * bd))


def qdrdist(latd1, lond1, latd2, lond2):
    """geo.py:57-107: qdr [deg], dist [nm]."""
    res1 = rwgs84(0.5 * (latd1 + latd2))
    a = 6378137.0
    r1 = rwgs84(latd1)
    r2 = rwgs84(latd2)
    res2 = 0.5 * (abs(latd1) * (r1 + a) + abs(latd2) * (r2 + a)) / (abs(latd1) + abs(latd2))
    sw = (latd1 * latd2 >= 0.)
    r = sw * res1 + (1 - sw) * res2
    lat1 = np.radians(latd1)
    lon1 = np.radians(lond1)
    lat2 = np.radians(latd2)
    lon2 = np.radians(lond2)
    sin1 = np.sin(0.5 * (lat2 - lat1))
    sin2 = np.sin(0.5 * (lon2 - lon1))
    coslat1 = np.cos(lat1)
    coslat2 = np.cos(lat2)
    root = sin1 * sin1 + coslat1 * coslat2 * sin2 * sin2
    d = 2.0 * r * np.arctan2(np.sqrt(root), np.sqrt(1.0 - root))
    qdr = np.degrees(np.arctan2(np.sin(lon2 - lon1) * coslat2,
                                coslat1 * np.sin(lat2) - np.sin(lat1) * coslat2 * np.cos(lon2 - lon1)))
    return qdr, d / NM


def degto180(angle):
    return (angle + 180.) % 360 - 180.


def calcturn(tas, bank, wpqdr, next_wpqdr):
    """activewpdata.py:57-65."""
    turnrad = tas * tas / (np.maximum(0.01, np.tan(bank)) * G0)
    turndist = np.abs(turnrad * np.tan(np.radians(0.5 * np.abs(degto180(wpqdr % 360. - next_wpqdr % 360.)))))
    return turndist, turnrad


# ---- scalar aero (aero.py:178-239, 304-368): the layer table, not vatmos
_H0 = [0.0, 11000., 20000., 32000., 47000., 51000., 71000., 86852.]
_P0 = [101325., 22631.7009099, 5474.71768857, 867.974468302, 110.898214043, 66.939, 3.9564]
_T0 = [288.15, 216.65, 216.65, 228.65, 270.65, 270.65, 214.65]
_A = [-0.0065, 0, 0.001, 0.0028, 0, -0.0028, -0.002]


def atmos(h):
    h = max(0.0, min(float(h), _H0[-1]))
    i = 0
    while h > _H0[i + 1] and i < len(_H0) - 2:
        i = i + 1
    if _A[i] == 0:
        T = _T0[i]
        p = _P0[i] * math.exp(-G0 / (RGAS * T) * (h - _H0[i]))
        rho = p / (RGAS * T)
    else:
        T = _T0[i] + _A[i] * (h - _H0[i])
        p = _P0[i] * ((T / _T0[i])**(-G0 / (_A[i] * RGAS)))
        rho = p / (RGAS * T)
    return p, rho, T


def vsound(h):
    return math.sqrt(GAMMA * RGAS * atmos(h)[2])


def cas2tas(cas, h):
    p, rho, T = atmos(h)
    qdyn = P0 * ((1. + RHO0 * cas * cas / (7. * P0))**3.5 - 1.)
    tas = math.sqrt(7. * p / rho * ((1. + qdyn / p)**(2. / 7.) - 1.))
    return -1 * tas if cas < 0 else tas


def tas2cas(tas, h):
    p, rho, T = atmos(h)
    qdyn = p * ((1. + rho * tas * tas / (7. * p))**3.5 - 1.)
    cas = math.sqrt(7. * P0 / RHO0 * ((qdyn / P0 + 1.)**(2. / 7.) - 1.))
    return -1 * cas if tas < 0 else cas


def cas2mach(cas, h):
    return cas2tas(cas, h) / vsound(h)


def mach2cas(M, h):
    return tas2cas(M * vsound(h), h)


# ---- vectorised aero (aero.py:62-172)
def vatmos(h):
    T = np.maximum(288.15 - 0.0065 * h, TSTRAT)
    rhotrop = 1.225 * (T / 288.15)**4.256848030018761
    dhstrat = np.maximum(0., h - 11000.)
    rho = rhotrop * np.exp(-dhstrat / 6341.552161)
    p = rho * RGAS * T
    return p, rho, T


def vmach2tas(M, h):
    T = np.maximum(288.15 - 0.0065 * h, TSTRAT)
    return M * np.sqrt(GAMMA * RGAS * T)


def vcas2tas(cas, h):
    p, rho, T = vatmos(h)
    qdyn = P0 * ((1. + RHO0 * cas * cas / (7. * P0))**3.5 - 1.)
    tas = np.sqrt(7. * p / rho * ((1. + qdyn / p)**(2. / 7.) - 1.))
    return np.where(cas < 0, -1 * tas, tas)


def vcasormach2tas(spd, h):
    return np.where(np.abs(spd) < 1, vmach2tas(spd, h), vcas2tas(spd, h))


class _Margins:
    """Collects the operand pairs of every discontinuous comparison per aircraft."""

    def __init__(self, n, rel=1e-9):
        self.near = np.zeros(n, dtype=bool)
        self.rel = rel

    def add(self, a, b, rows=None):
        a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
        with np.errstate(invalid='ignore'):
            hit = np.abs(a - b) <= self.rel * np.maximum(np.abs(a), np.abs(b))
        hit = hit & np.isfinite(a) & np.isfinite(b) & ~((a == 0) & (b == 0))
        if rows is None:
            self.near |= hit
        else:
            np.logical_or.at(self.near, np.asarray(rows), hit)


def _compute_vnav(s, i, toalt, xtoalt, coslat, m, info=None):
    """autopilot.py:207-304 for aircraft i (what survives the tick: nextaltco,
    xtoalt, dist2vs)."""
    if toalt < 0 or not s['swvnav'][i]:
        s['dist2vs'][i] = -999.
        if info is not None:
            info['vnav'][i] = 1 if toalt < 0 else 2
        return
    alt = s['alt'][i]
    if info is not None:
        info['vnav'][i] = 3 if alt > toalt + 10. * FT else (4 if alt < toalt - 10. * FT else 5)
    if m is not None:
        m.add([alt, alt], [toalt + 10. * FT, toalt - 10. * FT], rows=[i, i])
    if alt > toalt + 10. * FT:
        s['actwp_nextaltco'][i] = min(alt, toalt + xtoalt * STEEPNESS)
        s['actwp_xtoalt'][i] = xtoalt
        s['dist2vs'][i] = s['actwp_turndist'][i] + np.abs(alt - s['actwp_nextaltco'][i]) / STEEPNESS
        dy = (s['actwp_lat'][i] - s['lat'][i])
        dx = (s['actwp_lon'][i] - s['lon'][i]) * coslat[i]
        legdist = 60. * NM * np.sqrt(dx * dx + dy * dy)
        if m is not None:
            m.add(legdist, s['dist2vs'][i], rows=[i])       # (the branch only picks values nobody sees)
        if info is not None and legdist < s['dist2vs'][i]:
            info['vnav'][i] = 6                             # the urgent descent
    elif alt < toalt - 10. * FT:
        s['actwp_nextaltco'][i] = toalt
        s['actwp_xtoalt'][i] = xtoalt
        s['dist2vs'][i] = 99999. * NM
    else:
        s['dist2vs'][i] = -999.


def update(state, rows, off, nwp, tick=True, margins=None, info=None):
    """One ``Autopilot.update`` call.  ``state``: dict of the TRAFFIC, REALS,
    FLAGS, TARGETS arrays and ``iactwp``; returns a new dict (inputs are not
    modified).  ``tick`` False: only autopilot.py:203.  ``info``: a dict that
    receives the ``reached`` mask, which arm reached it and ComputeVNAV's path."""
    s = {k: np.array(v) for k, v in state.items()}
    for k in FLAGS:
        s[k] = s[k].astype(bool)
    n = len(s['lat'])
    m = margins
    if tick:
        lat, lon, alt, tas, gs = s['lat'], s['lon'], s['alt'], s['tas'], s['gs']
        coslat = np.cos(np.deg2rad(lat))                      # traffic.py:482
        with np.errstate(invalid='ignore', divide='ignore'):
            qdr, distinnm = qdrdist(lat, lon, s['actwp_lat'], s['actwp_lon'])
            dist = distinnm * NM
            # ---- ActiveWaypoint.Reached (activewpdata.py:31-54)
            next_qdr = np.where(s['actwp_next_qdr'] < -900., qdr, s['actwp_next_qdr'])
            s['actwp_turndist'], turnrad = s['actwp_flyby'] * calcturn(tas, s['bank'], qdr, next_qdr)
            dtrk = np.abs(degto180(s['trk'] % 360. - qdr % 360.))
            away = dtrk > 90.
            proxfact = 1.01
            incircle = dist < turnrad * proxfact
            circling = away * incircle
            bydist = dist < s['actwp_turndist']
            reached = np.where(s['swlnav'] * (bydist + circling))[0]
        if m is not None:
            m.add(dist, s['actwp_turndist'])
            m.add(dist, turnrad * proxfact)
            m.add(dtrk, 90.)
        if info is not None:
            info['reached'] = np.zeros(n, dtype=bool)
            info['reached'][reached] = True
            info['bydist'] = bydist & s['swlnav']
            info['circling'] = circling & s['swlnav']
            info['vnav'] = np.zeros(n, dtype=int)   # ComputeVNAV's path: 1 toalt < 0, 2 VNAV off, 3 / 6 descent
            #                                         (6: urgent), 4 climb, 5 level
        for i in reached:
            oldspd = s['actwp_spd'][i]
            # ---- Route.getnextwp (route.py:778-800) on the table
            lnavon = s['iactwp'][i] + 1 < nwp[i]
            if lnavon:
                s['iactwp'][i] += 1
            row = rows[off[i] + s['iactwp'][i]]
            wlat, wlon, walt, spd = row[R_LAT], row[R_LON], row[R_ALT], row[R_SPD]
            s['actwp_xtoalt'][i], toalt = row[R_XTOALT], row[R_TOALT]
            flyby, s['actwp_next_qdr'][i] = row[R_FLYBY], row[R_NEXTQDR]
            s['swlnav'][i] = s['swlnav'][i] and lnavon
            s['swvnav'][i] = s['swvnav'][i] and s['swlnav'][i]
            s['actwp_lat'][i] = wlat
            s['actwp_lon'][i] = wlon
            s['actwp_flyby'][i] = int(flyby)
            if walt >= -0.01:
                s['actwp_nextaltco'][i] = walt
            if spd > -990. and s['swlnav'][i] and s['swvnav'][i]:
                if s['abco'][i] and spd > 1.0:
                    s['actwp_spd'][i] = cas2mach(float(spd), alt[i])
                elif s['belco'][i] and 0. < spd <= 1.0:
                    s['actwp_spd'][i] = mach2cas(float(spd), alt[i])
                else:
                    s['actwp_spd'][i] = spd
            else:
                s['actwp_spd'][i] = -999.
            if s['swvnav'][i] and oldspd > 0.0:
                s['selspd'][i] = oldspd
            with np.errstate(invalid='ignore', divide='ignore'):
                qdr[i], _ = qdrdist(lat[i], lon[i], s['actwp_lat'][i], s['actwp_lon'][i])
                if s['actwp_next_qdr'][i] < -900.:
                    local_next_qdr = qdr[i]
                else:
                    local_next_qdr = s['actwp_next_qdr'][i]
                s['actwp_turndist'][i], _ = calcturn(tas[i], s['bank'][i], qdr[i], local_next_qdr)
            _compute_vnav(s, i, toalt, s['actwp_xtoalt'][i], coslat, m, info)
        # ---- continuous guidance (autopilot.py:147-199)
        with np.errstate(invalid='ignore', divide='ignore'):
            dy = (s['actwp_lat'] - lat)
            dx = (s['actwp_lon'] - lon) * coslat
            dist2wp = 60. * NM * np.sqrt(dx * dx + dy * dy)
            startdescent = (dist2wp < s['dist2vs']) + (s['actwp_nextaltco'] > alt)
            swvnavvs = s['swvnav'] * np.where(s['swlnav'], startdescent,
                                              dist <= np.maximum(185.2, s['actwp_turndist']))
            t2go2alt = np.maximum(0., (dist2wp + s['actwp_xtoalt'] - s['actwp_turndist'])) / np.maximum(0.5, gs)
            s['actwp_vs'] = np.maximum(STEEPNESS * gs, np.abs((s['actwp_nextaltco'] - alt)) / np.maximum(1.0, t2go2alt))
            s['vnavvs'] = np.where(swvnavvs, s['actwp_vs'], s['vnavvs'])
            selvs = np.where(abs(s['selvs']) > 0.1, s['selvs'], s['apvsdef'])
            s['ap_vs'] = np.where(swvnavvs, s['vnavvs'], selvs)
            s['ap_alt'] = np.where(swvnavvs, s['actwp_nextaltco'], s['selalt'])
            s['selalt'] = np.where(swvnavvs, s['actwp_nextaltco'], s['selalt'])
            s['ap_trk'] = np.where(s['swlnav'], qdr, s['ap_trk'])
            nexttas = vcasormach2tas(s['actwp_spd'], alt)
            tasdiff = nexttas - tas
            dtspdchg = np.abs(tasdiff) / np.maximum(0.01, np.abs(s['ax']))
            dxspdchg = 0.5 * np.sign(tasdiff) * np.abs(s['ax']) * dtspdchg * dtspdchg + tas * dtspdchg
            usespdcon = (dist2wp < dxspdchg) * (s['actwp_spd'] > -990.) * s['swvnav']
            s['selspd'] = np.where(usespdcon, s['actwp_spd'], s['selspd'])
        s['swvnavvs'] = swvnavvs.astype(np.float64)
        if m is not None:
            m.add(dist2wp, s['dist2vs'])
            m.add(dist2wp, dxspdchg)
            m.add(dist, np.maximum(185.2, s['actwp_turndist']))
            m.add(np.abs(s['actwp_spd']), 1.0)
        if info is not None:
            info['usespdcon'] = np.asarray(usespdcon, dtype=bool)
            info['startdescent'] = np.asarray(startdescent, dtype=bool)
    with np.errstate(invalid='ignore', divide='ignore'):
        if m is not None:
            m.add(np.abs(s['selspd']), 1.0)
        s['ap_tas'] = vcasormach2tas(s['selspd'], s['alt'])         # autopilot.py:203
    return s


def near_threshold(state, rows, off, nwp, tick=True, rel=1e-9):
    """Mask of the aircraft for which a discontinuous comparison of this update
    (dist < turndist, dist < turnrad 1.01, |dtrk| > 90, dist2wp < dist2vs,
    dist2wp < dxspdchg, legdist < dist2vs, alt vs toalt +- 10 ft, |spd| < 1, and
    dist <= max(185.2, turndist)) lies within ``rel`` (1e-9) relative of equality."""
    m = _Margins(len(state['lat']), rel)
    update(state, rows, off, nwp, tick=tick, margins=m)
    return m.near
