"""numpy restatement of the reference's ADS-B model (traffic/adsbmodel.py) for what the device computes: one
``update(time)``, ``create(n)`` and ``delete(idx)`` on ``lastupdate`` and the seven picture arrays, with the unit
normals handed in, and the build-defined draws (bluesky_amd/csrc/bsa_adsb_math.h: tests/turb_np.py's Philox, streams
1 and 2).  tools/make_golden_adsb.py asserts it bitwise equal to the reference's own class on every recorded case."""
import numpy as np

from tests import turb_np

FT = 0.3048
FIELDS = ('lat', 'lon', 'alt', 'trk', 'tas', 'gs', 'vs')
ARRAYS = ('lastupdate',) + FIELDS
TRANSERROR = (1e-4, 100 * FT)
STREAM_UPDATE, STREAM_CREATE = 1, 2


def due(lastupdate, trunctime, time):
    """adsbmodel.py:45: the indices that update -- strict, false for a NaN."""
    with np.errstate(invalid='ignore'):
        return np.where(np.asarray(lastupdate) + trunctime < time)[0]


def update(st, traf, time, trunctime=0, noise=False, transerror=TRANSERROR, z=None):
    """One ADSB.update(time) (adsbmodel.py:44-59): the arrays after it.  ``z``: the unit normals of lat, lon, alt --
    three values (the reference's single shared draw per quantity) or (3, n), one row of draws per aircraft.
    np.random.normal(0, s) is 0 + s * z."""
    up = due(st['lastupdate'], trunctime, time)
    out = {k: np.array(st[k], dtype=np.float64) for k in ARRAYS}
    for k in FIELDS:
        out[k][up] = np.asarray(traf[k], dtype=np.float64)[up]
    if noise:
        z = np.asarray(z, dtype=np.float64)
        for q, k in enumerate(('lat', 'lon', 'alt')):
            e = 0.0 + transerror[0 if q < 2 else 1] * (z[q] if z.ndim == 1 else z[q][up])
            with np.errstate(invalid='ignore'):
                out[k][up] = np.asarray(traf[k], dtype=np.float64)[up] + e
    out['lastupdate'][up] = out['lastupdate'][up] + trunctime
    return out


def create(st, traf, n, trunctime, u):
    """ADSB.create(n) after Traffic.create appended n aircraft (``traf``'s arrays are already n longer): lastupdate =
    -trunctime * u (``u``: the n uniforms), the picture from the state, vs at the append's 0."""
    out = {k: np.append(np.asarray(st[k], dtype=np.float64), np.zeros(n)) for k in ARRAYS}
    out['lastupdate'][-n:] = -trunctime * np.asarray(u)
    for k in FIELDS[:-1]:
        out[k][-n:] = np.asarray(traf[k])[-n:]
    return out


def delete(st, idx):
    return {k: np.delete(st[k], idx) for k in ARRAYS}


def set_noise(n):
    """SetNoise(n) (adsbmodel.py:27-31): transnoise, truncated, transerror, trunctime."""
    return n, n, [1e-4, 100 * FT], 0


def raw_words(n, seed=0, call=0, first_index=0, stream=STREAM_UPDATE):
    """(n, 4) uint64: the block of counter {index, call, stream, 0}, key {seed, 0} per index."""
    out = np.empty((n, 4), dtype=np.uint64)
    for i in range(n):
        out[i] = turb_np.philox4x64_10((first_index + i, call, stream, 0), (seed, 0))
    return out


def draws(n, seed=0, call=0, first_index=0):
    """(n, 3) unit normals (lat, lon, alt) of the update stream; the shared draw is row 0 of ``draws(1, seed, call)``."""
    return turb_np.normals(raw_words(n, seed, call, first_index, STREAM_UPDATE))


def create_uniforms(n, seed=0, call=0, first_index=0):
    """(n,) create's uniforms: word 0 of the create stream's block."""
    return turb_np.uniforms(raw_words(n, seed, call, first_index, STREAM_CREATE))[:, 0]


class ArrayTree:
    """A stand-in for the reference's TrafficArrays parent (what ``Traffic`` is to ``traf.adsb``): the named
    per-aircraft arrays and a list of children that ``create_children``, ``delete`` and ``reset`` walk -- the only
    way ``Traffic.create / delete / reset`` reach the ADS-B object."""

    def __init__(self, names=FIELDS):
        self.parent, self.children, self.names = None, [], tuple(names)
        for k in self.names:
            setattr(self, k, np.array([]))

    @property
    def ntraf(self):
        return len(getattr(self, self.names[0]))

    def create(self, n=1, **values):
        """Traffic.create: the own arrays grow by n (0.0 unless given), then the children's."""
        for k in self.names:
            setattr(self, k, np.append(getattr(self, k), np.asarray(values.get(k, np.zeros(n)), dtype=np.float64)))
        self.create_children(n)

    def create_children(self, n=1):
        for child in self.children:
            child.create(n)
            child.create_children(n)

    def delete(self, idx):
        for child in self.children:
            child.delete(idx)
        for k in self.names:
            setattr(self, k, np.delete(getattr(self, k), idx))

    def reset(self):
        for child in self.children:
            child.reset()
        for k in self.names:
            setattr(self, k, np.array([]))
