"""Autopilot LNAV / VNAV guidance on the device: the route table and the
standalone ``Autopilot.update`` call (bsa_fms_update).

A route table holds every aircraft's waypoints as rows of 8 doubles
(``lat, lon, alt, spd, xtoalt, toalt, flyby, nextqdr``); aircraft k owns rows
``off[k] .. off[k] + n[k]`` and flies to its row ``iactwp[k]``.  ``xtoalt`` /
``toalt`` are the route's own ``wpxtoalt`` / ``wptoalt`` after
``Route.calcfp`` (route.py:983-1041); ``nextqdr`` is what ``Route.getnextqdr``
(route.py:1101-1109) returns with that waypoint active.  Both are host work,
done once per route with numpy; the device only looks rows up.
"""
import numpy as np

from . import _lib

NM = 1852.
COLS = ('lat', 'lon', 'alt', 'spd', 'xtoalt', 'toalt', 'flyby', 'nextqdr')
WP_DEST = 3      # Route.dest (route.py)
WP_RUNWAY = 5    # Route.runway: its landing logic pushes stack commands, not modelled

TRAFFIC = _lib.FMS_TRAFFIC
REALS = _lib.FMS_REALS
FLAGS = _lib.FMS_FLAGS
TARGETS = _lib.FMS_TARGETS


def _rwgs84(latd):
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
    """geo.qdrdist (geo.py:57-107), in its operation order: qdr [deg], dist [nm]."""
    res1 = _rwgs84(0.5 * (latd1 + latd2))
    a = 6378137.0
    r1 = _rwgs84(latd1)
    r2 = _rwgs84(latd2)
    with np.errstate(invalid='ignore', divide='ignore'):
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


def flight_plan(wplat, wplon, wpalt, wptype):
    """``(wpxtoalt, wptoalt)`` as ``Route.calcfp`` (route.py:983-1041) leaves
    them, for a route given without them: per waypoint, the next altitude
    constraint at or after it and the distance [m] from the waypoint to it."""
    nwp = len(wplat)
    distto = [0.] * nwp
    for i in range(nwp - 1):
        distto[i + 1] = float(qdrdist(np.float64(wplat[i]), np.float64(wplon[i]),
                                      np.float64(wplat[i + 1]), np.float64(wplon[i + 1]))[1])
    wptoalt, wpxtoalt = [-999.] * nwp, [1.] * nwp
    toalt, xtoalt = -999., 0.
    for i in range(nwp - 1, -1, -1):
        if wptype[i] == WP_DEST:
            toalt, xtoalt = 0., 0.
        elif wpalt[i] >= 0:
            toalt, xtoalt = wpalt[i], 0.
        elif i != nwp - 1:
            xtoalt += distto[i + 1] * NM
        else:
            xtoalt = 0.0
        wptoalt[i], wpxtoalt[i] = toalt, xtoalt
    return wpxtoalt, wptoalt


def route_table(routes, swlnav=None):
    """``(rows, off, n, iactwp)`` for a list of routes: objects with the
    reference ``Route``'s fields ``wplat wplon wpalt wpspd wpflyby wptype
    iactwp nwp`` and, after ``calcfp()``, ``wpxtoalt wptoalt`` (computed here by
    ``flight_plan`` where a route lacks them).  ``rows``: float64 [sum(n), 8].
    Runway waypoints, an active waypoint outside its route and (with ``swlnav``
    given) LNAV on an empty route raise ValueError."""
    rows, off, cnt, act = [], [], [], []
    for k, r in enumerate(routes):
        nwp = len(r.wplat)
        if getattr(r, 'nwp', nwp) != nwp:
            raise ValueError('route %d: nwp %d but %d waypoints' % (k, r.nwp, nwp))
        for f in ('wplon', 'wpalt', 'wpspd', 'wpflyby', 'wptype'):
            if len(getattr(r, f)) != nwp:
                raise ValueError('route %d: %s has %d entries, wplat %d' % (k, f, len(getattr(r, f)), nwp))
        if any(t == WP_RUNWAY for t in r.wptype):
            raise ValueError('route %d: runway waypoints (type %d) are not supported' % (k, WP_RUNWAY))
        off.append(len(rows))
        cnt.append(nwp)
        if nwp == 0:
            if swlnav is not None and swlnav[k]:
                raise ValueError('route %d is empty but LNAV is on' % k)
            act.append(-1)
            continue
        if not 0 <= r.iactwp < nwp:
            raise ValueError('route %d: active waypoint %d outside [0, %d)' % (k, r.iactwp, nwp))
        act.append(int(r.iactwp))
        if getattr(r, 'wpxtoalt', None) is not None and len(r.wpxtoalt) == nwp and len(r.wptoalt) == nwp:
            xtoalt, toalt = r.wpxtoalt, r.wptoalt
        else:
            xtoalt, toalt = flight_plan(r.wplat, r.wplon, r.wpalt, r.wptype)
        lat = np.array(r.wplat, dtype=np.float64)
        lon = np.array(r.wplon, dtype=np.float64)
        nextqdr = np.full(nwp, -999.)
        if nwp > 1:
            nextqdr[:-1] = qdrdist(lat[:-1], lon[:-1], lat[1:], lon[1:])[0]
        for i in range(nwp):
            rows.append((lat[i], lon[i], r.wpalt[i], r.wpspd[i], xtoalt[i], toalt[i],
                         1.0 if r.wpflyby[i] else 0.0, nextqdr[i]))
    rows = np.array(rows, dtype=np.float64).reshape(-1, len(COLS))
    return rows, np.array(off, dtype=np.int32), np.array(cnt, dtype=np.int32), np.array(act, dtype=np.int32)


def from_bluesky(traf, unique_names=False):
    """``(rows, off, n, state)`` of a BlueSky ``Traffic`` object: its routes
    (``traf.ap.route``) as a table, and the state dict ``update`` takes --
    the traffic arrays, ``traf.actwp``, ``traf.ap`` and ``traf.swlnav / swvnav /
    selspd / selvs / apvsdef / abco / belco / selalt``.  ``unique_names``: raise
    ValueError for a route that holds a waypoint name twice -- ``Route.direct``
    looks its waypoint up by name and takes the first match, the device's
    waypoint recovery (``recover``, ``ResidentSim.set_recovery``) goes to the
    index ``findact`` found, and the two agree only for unique names."""
    if unique_names:
        for k, r in enumerate(traf.ap.route):
            names = [str(x).upper().strip() for x in getattr(r, 'wpname', [])]
            if len(set(names)) != len(names):
                twice = sorted(set(x for x in names if names.count(x) > 1))
                raise ValueError('route %d holds the waypoint name %s more than once' % (k, ', '.join(twice)))
    swlnav = np.asarray(traf.swlnav).astype(bool)
    rows, off, cnt, act = route_table(traf.ap.route, swlnav)
    w, ap = traf.actwp, traf.ap
    st = {k: np.array(getattr(traf, k), dtype=np.float64) for k in TRAFFIC}
    st.update(actwp_lat=w.lat, actwp_lon=w.lon, actwp_nextaltco=w.nextaltco, actwp_xtoalt=w.xtoalt,
              actwp_spd=w.spd, actwp_vs=w.vs, actwp_turndist=w.turndist, actwp_flyby=w.flyby,
              actwp_next_qdr=w.next_qdr, dist2vs=ap.dist2vs, vnavvs=ap.vnavvs, swvnavvs=ap.swvnavvs,
              selspd=traf.selspd, selvs=traf.selvs, apvsdef=traf.apvsdef,
              ap_trk=ap.trk, ap_tas=ap.tas, ap_alt=ap.alt, ap_vs=ap.vs, selalt=traf.selalt)
    st = {k: np.array(v, dtype=np.float64) for k, v in st.items()}
    st.update(swlnav=swlnav, swvnav=np.asarray(traf.swvnav).astype(bool),
              abco=np.asarray(traf.abco).astype(bool), belco=np.asarray(traf.belco).astype(bool), iactwp=act)
    return rows, off, cnt, st


def synthetic_routes(state, seed=0, nwp=4, leg=(3000., 9000.), first=(200., 12000.)):
    """Generated routes for a synthetic traffic set (``resident.initial_state``):
    ``nwp`` waypoints per aircraft roughly ahead of it, the first ``first`` metres
    away, legs of ``leg`` metres with turns, mixed altitude / speed constraints and
    fly-over waypoints.  Returns ``(rows, off, n, fms_state)`` for
    ``ResidentSim.set_fms``: every aircraft flies to its first waypoint, LNAV on,
    VNAV on for most."""
    import types
    rng = np.random.default_rng(seed)
    m = len(state['lat'])
    routes = []
    for k in range(m):
        la, lo, brg = float(state['lat'][k]), float(state['lon'][k]), float(state['trk'][k])
        wplat, wplon = [], []
        for i in range(nwp):
            d = rng.uniform(*(first if i == 0 else leg))
            brg = (brg + rng.choice([0., 25., -40., 85., -120.])) % 360.   # (not 90: |dtrk| > 90 is a threshold)
            la = la + np.degrees(d * np.cos(np.radians(brg)) / 6371000.)
            lo = lo + np.degrees(d * np.sin(np.radians(brg)) / 6371000. / np.cos(np.radians(la)))
            wplat.append(float(la))
            wplon.append(float(lo))
        alt = float(state['alt'][k])
        wpalt = [float(rng.choice([-999., alt, alt - 600., alt + 500.])) for _ in range(nwp)]
        wpspd = [float(rng.choice([-999., 130., 0.7])) for _ in range(nwp)]
        routes.append(types.SimpleNamespace(wplat=wplat, wplon=wplon, wpalt=wpalt, wpspd=wpspd,
                                            wpflyby=[bool(rng.random() < 0.8) for _ in range(nwp)],
                                            wptype=[0] * nwp, iactwp=0, nwp=nwp))
    rows, off, cnt, act = route_table(routes)
    r0 = rows[off]
    st = dict(actwp_lat=r0[:, 0].copy(), actwp_lon=r0[:, 1].copy(), actwp_nextaltco=np.array(state['alt'], dtype=np.float64),
              actwp_xtoalt=r0[:, 4].copy(), actwp_spd=np.full(m, -999.), actwp_vs=np.zeros(m),
              actwp_turndist=np.ones(m), actwp_flyby=r0[:, 6].copy(), actwp_next_qdr=r0[:, 7].copy(),
              dist2vs=np.full(m, -999.), vnavvs=np.zeros(m), swvnavvs=np.zeros(m),
              selspd=np.array(state['tas'], dtype=np.float64) * 0.8, selvs=np.zeros(m), apvsdef=np.full(m, 1500. * 0.3048 / 60.),
              swlnav=np.ones(m, dtype=bool), swvnav=rng.random(m) < 0.75, abco=np.zeros(m, dtype=bool),
              belco=np.ones(m, dtype=bool), iactwp=act)
    return rows, off, cnt, st


def append_routes(rows, off, n, new_rows, new_off, new_n):
    """The route table after ``ResidentSim.create(..., fms=(new_rows, new_off, new_n, state))``,
    as the device keeps it: ``new_rows`` behind ``rows``, ``new_off`` rebased by ``len(rows)``.
    Returns ``(rows, off, n)`` for the old aircraft followed by the new ones; the inputs stay
    as they are.  Pure numpy: the host's own copy of the table."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, len(COLS))
    new_rows = np.asarray(new_rows, dtype=np.float64).reshape(-1, len(COLS))
    off, n, new_off, new_n = (np.asarray(a, dtype=np.int32).ravel() for a in (off, n, new_off, new_n))
    if len(off) != len(n) or len(new_off) != len(new_n):
        raise ValueError('append_routes: one offset and one count per aircraft')
    for o, c, r in ((off, n, rows), (new_off, new_n, new_rows)):
        if len(o) and ((o < 0).any() or (c < 0).any() or (o.astype(np.int64) + c).max() > len(r)):
            raise ValueError('append_routes: a route lies outside its table')
    return (np.concatenate([rows, new_rows]), np.concatenate([off, new_off + np.int32(len(rows))]),
            np.concatenate([n, new_n]))


FMS_DT = 1.01    # Autopilot.dt (autopilot.py:18)


def tick_schedule(simt, simdt, nsteps, t0=-999.):
    """Which of the next ``nsteps`` steps run the FMS part of ``Autopilot.update``
    (autopilot.py:61-62: ``t0 + dt < simt or simt < t0 or simt < dt``, then ``t0 =
    simt``), for a sim loop that accumulates ``simt += simdt`` (simulation.py:119).
    ``simt``: the time of the first of these steps.  Returns (bool [nsteps], the
    simt of the step after them, t0 after them)."""
    simt, t0 = float(simt), float(t0)
    out = np.zeros(nsteps, dtype=bool)
    for k in range(nsteps):
        if t0 + FMS_DT < simt or simt < t0 or simt < FMS_DT:
            t0 = simt
            out[k] = True
        simt += simdt
    return out, simt, t0


def update(rows, off, n, state, ctx=None):
    """One ``Autopilot.update`` call with a forced FMS tick on the device
    (bsa_fms_update) for the aircraft of ``state`` (dict of the TRAFFIC, REALS,
    FLAGS, TARGETS arrays and ``iactwp``).  Returns the FMS state after the
    call: dict of REALS, FLAGS, TARGETS and ``iactwp``; the inputs stay as they are."""
    ctx = ctx or _lib.default_context()
    return ctx.fms_update(rows, off, n, state)


def recover(rows, off, n, state, count, ctx=None):
    """Waypoint recovery on the device (bsa_fms_recover): what ``ASAS.ResumeNav``
    does for an ownship whose resopair it drops (asas.py:459-465),
    ``Route.findact`` + ``Route.direct``, applied ``count[k]`` times in sequence to
    aircraft k (once per dropped pair).  ``state`` as ``update`` takes it (``ax``
    and the targets other than ``ap_alt`` are not needed).  Returns the FMS state
    after the call: dict of REALS, FLAGS, ``ap_alt`` and ``iactwp``; the inputs stay
    as they are.  ``direct`` goes to the waypoint's index: the reference's lookup
    by name for routes with unique names (``from_bluesky(unique_names=True)``)."""
    ctx = ctx or _lib.default_context()
    return ctx.fms_recover(rows, off, n, state, count)


# ---- route edits (ADDWPT / DELWPT / DIRECT; bsa_route_edit)
INSERT, OVERWRITE, DELETE, DIRECT = _lib.ROUTE_INSERT, _lib.ROUTE_OVERWRITE, _lib.ROUTE_DELETE, _lib.ROUTE_DIRECT
WP_ORIG, WP_CALC = 2, 4
RouteEditRefused = _lib.RouteEditRefused


def record(aircraft, op, pos, lat=0., lon=0., alt=-999., spd=-999., flyby=True, wptype=0, bump_active=False):
    """One edit record (a dict ``_lib.route_records`` takes)."""
    return dict(aircraft=int(aircraft), op=int(op), pos=int(pos), flyby=int(bool(flyby)), wptype=int(wptype),
                bump_active=int(bool(bump_active)), lat=float(lat), lon=float(lon), alt=float(alt), spd=float(spd))


def edit(rows, off, n, state, records, wptype=None, ctx=None):
    """A batch of edit records on the device, standalone (bsa_route_edit): returns
    ``(rows, off, n, wptype, fms_state)``, the new table compacted in aircraft order
    and the FMS state after the batch; the inputs stay as they are.  ``state`` as
    ``recover`` takes it.  A refused batch raises ``RouteEditRefused`` (``.code``)."""
    ctx = ctx or _lib.default_context()
    return ctx.route_edit(rows, off, n, state, records, wptype)


class RouteNames:
    """The host's side of a route edit: the waypoint names (and types) of every
    aircraft's route, and the reference's lookups on them.  ``addwpt`` / ``delwpt``
    / ``direct`` take ``Route.addwpt`` / ``delwpt`` / ``direct``'s arguments with the
    position already resolved (the nav database is the host's) and return edit
    records for ``edit`` / ``ResidentSim.edit_routes``; each also applies the edit to
    the names, so the next call sees the route this one leaves.  ``create`` /
    ``delete`` mirror ``ResidentSim.create`` / ``delete``."""

    def __init__(self, names, types=None):
        self.names = [[str(x).upper().strip() for x in r] for r in names]
        self.types = [[0] * len(r) for r in names] if types is None else [[int(t) for t in r] for r in types]
        if [len(r) for r in self.names] != [len(r) for r in self.types]:
            raise ValueError('one waypoint type per name')

    def create(self, names, types=None):
        new = RouteNames(names, types)
        self.names += new.names
        self.types += new.types

    def delete(self, idx):
        gone = set(int(i) for i in np.unique(np.asarray(idx, dtype=np.int64).ravel()))
        self.names = [r for k, r in enumerate(self.names) if k not in gone]
        self.types = [r for k, r in enumerate(self.types) if k not in gone]

    @staticmethod
    def available_name(data, name, len_=2):
        """Route.get_available_name: ``name``, or ``name`` + the first free number."""
        appi, out = 0, name
        fmt = '{:0' + str(len_) + 'd}'
        while data.count(out) > 0:
            appi += 1
            out = name + fmt.format(appi)
        return out

    def addwpt(self, iac, name, wptype, lat, lon, alt=-999., spd=-999., afterwp="", beforewp="", flyby=True):
        """route.py:537-594 for a waypoint the nav database found (``lat, lon``: its
        position).  ORIG / DEST (route.py:498-535 updates no ``next_qdr``), runway and
        calculated waypoints are refused."""
        if wptype in (WP_ORIG, WP_DEST, WP_CALC, WP_RUNWAY):
            raise ValueError('addwpt: waypoint type %d is not supported on the device' % wptype)
        names, types = self.names[iac], self.types[iac]
        name = name.upper().strip()
        newname = self.available_name(names, name, 3) if wptype == 0 else self.available_name(names, name)
        aftwp, bfwp = afterwp.upper().strip(), beforewp.upper().strip()
        bump = False
        if (afterwp and names.count(aftwp) > 0) or (beforewp and names.count(bfwp) > 0):
            pos = names.index(aftwp) + 1 if afterwp else names.index(bfwp)
            bump = bool(afterwp)
        elif len(names) > 0 and types[-1] == WP_DEST:
            pos = len(names) - 1
        else:
            pos = len(names)
        names.insert(pos, newname)
        types.insert(pos, int(wptype))
        return [record(iac, INSERT, pos, lat, lon, alt, spd, flyby, wptype, bump)]

    def delwpt(self, iac, name):
        """route.py:808-838: the LAST waypoint of that name; ``*``: every waypoint."""
        names, types = self.names[iac], self.types[iac]
        if name == '*':
            out = [record(iac, DELETE, 0) for _ in names]
            del names[:], types[:]
            return out
        idx = -1
        i = len(names)
        while idx == -1 and i > 0:
            i -= 1
            if names[i].upper() == name.upper():
                idx = i
        if idx == -1:
            raise ValueError('delwpt: waypoint %s not found' % name)
        del names[idx], types[idx]
        return [record(iac, DELETE, idx)]

    def direct(self, iac, name):
        """route.py:635-640: the FIRST waypoint of that name."""
        name = name.upper().strip()
        if name == '' or self.names[iac].count(name) == 0:
            raise ValueError('direct: waypoint %s not found' % name)
        return [record(iac, DIRECT, self.names[iac].index(name))]
