"""numpy restatement of the reference's Trails (traffic/trails.py) for what the device computes: one
``update(t)``, ``create(n)`` and ``delete(idx)`` on the three per-aircraft arrays, and the segments an update
emits.  tools/make_golden_trails.py asserts it bitwise equal to the reference's own class on every recorded
case; the GPU tests then use it on read-back state.  There is no arithmetic on positions: every number of a
segment is a copy, the only computed value is ``t - lasttim``."""
import numpy as np

ARRAYS = ('lastlat', 'lastlon', 'lasttim')
SEGMENT = ('lat0', 'lon0', 'lat1', 'lon1', 'time')


def empty():
    return dict(idx=np.zeros(0, dtype=np.int64), **{k: np.zeros(0) for k in SEGMENT})


def update(st, lat, lon, t, dt, active=True):
    """One Trails.update(t): (the arrays after it, the segments in emission order with the emitting ``idx``)."""
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    if not active:
        return dict(lastlat=lat.copy(), lastlon=lon.copy(), lasttim=np.full(len(lat), float(t))), empty()
    with np.errstate(invalid='ignore'):
        idx = np.where(t - np.asarray(st['lasttim']) > dt)[0]          # strict; a NaN delta selects nothing
    seg = dict(idx=idx.astype(np.int64), lat0=np.array(st['lastlat'])[idx], lon0=np.array(st['lastlon'])[idx],
               lat1=lat[idx], lon1=lon[idx], time=np.full(len(idx), float(t)))
    out = {k: np.array(st[k], dtype=np.float64) for k in ARRAYS}
    out['lastlat'][idx], out['lastlon'][idx], out['lasttim'][idx] = lat[idx], lon[idx], t
    return out, seg


def create(st, lat, lon, n=1):
    """Trails.create(n) after Traffic.create appended n aircraft (``lat`` / ``lon``: traf's, already n longer):
    TrafficArrays' default 0.0 for all n, then only the LAST gets its position; lasttim stays 0."""
    out = {k: np.append(np.asarray(st[k], dtype=np.float64), np.zeros(n)) for k in ARRAYS}
    out['lastlat'][-1], out['lastlon'][-1] = lat[-1], lon[-1]
    return out


def delete(st, idx):
    return {k: np.delete(st[k], idx) for k in ARRAYS}


def fcol(t, time, tcol0=60.0):
    return 1. - np.minimum(tcol0, np.abs(t - np.asarray(time))) / tcol0


def concat(segs):
    """Several updates' segments as one stream."""
    segs = list(segs)
    if not segs:
        return empty()
    return {k: np.concatenate([s[k] for s in segs]) for k in ('idx',) + SEGMENT}


def bound(n, k, simdt, dt):
    """The most segments k steps can emit (bsa_sim_step's capacity rule)."""
    return n * min(k, int(np.floor(k * simdt / dt)) + 1)
