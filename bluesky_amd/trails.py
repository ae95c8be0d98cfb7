"""Aircraft trails with the reference's surface (traffic/trails.py), computed on the device.

``Trails`` has no ``bs.traf``: the traffic object (anything with ``lat`` / ``lon`` / ``id``) goes to the
constructor.  Standalone, ``update(t)`` is one ``bsa_trails_update``.  Attached to a ``ResidentSim``
(``attach(sim)``) the sim's own stage runs ``Trails.update`` inside every step; ``update`` is then a
no-op and ``collect()`` drains the device's segments into the same lists the reference fills: ``new*``
on the QtGL path, ``lat0 .. / time / col`` (and ``fcol``, recomputed) on the pygame path.  The host-only
methods (``setTrails``, ``buffer``, the ``clear*`` family, ``changeTrailColor``, ``reset``) keep the
reference's return values, texts and quirks.
"""
import numpy as np

from . import _lib


def _none():
    return np.array([])


class Trails:
    def __init__(self, traf=None, dttrail=10., gui_type='qtgl', ctx=None):
        self.traf, self.sim, self._ctx = traf, None, ctx
        self.active = False
        self.dt = dttrail
        self.pygame = gui_type == 'pygame'
        self.tcol0 = 60.
        self.colorList = {'BLUE': np.array([0, 0, 255]), 'CYAN': np.array([0, 255, 255]),
                          'RED': np.array([255, 0, 0]), 'YELLOW': np.array([255, 255, 0])}
        self.defcolor = self.colorList['CYAN']
        self.lat0, self.lon0, self.lat1, self.lon1, self.time = _none(), _none(), _none(), _none(), _none()
        self.col, self.fcol = [], _none()
        self.bglat0, self.bglon0, self.bglat1, self.bglon1, self.bgtime = _none(), _none(), _none(), _none(), _none()
        self.bgcol = []                                  # (no bgacid yet: the reference's buffer() before clearbg() raises)
        self.accolor = []
        self.lastlat, self.lastlon, self.lasttim = _none(), _none(), _none()
        self.clearnew()

    # ------------------------------------------------------------ per-aircraft arrays
    def create(self, n=1):
        """After the traffic object grew by ``n``: 0.0 / '' for all of them, then only the LAST new
        aircraft gets its position and the default colour."""
        self.accolor.extend([''] * n)
        for k in ('lastlat', 'lastlon', 'lasttim'):
            setattr(self, k, np.append(getattr(self, k), [0.0] * n))
        self.accolor[-1] = self.defcolor
        self.lastlat[-1] = self.traf.lat[-1]
        self.lastlon[-1] = self.traf.lon[-1]

    def delete(self, idx):
        if self.sim is not None:                         # the undrained segments name the indices (and colours) of now;
            self.collect()                               # the arrays are the sim's, which its own delete shrinks
        else:
            for k in ('lastlat', 'lastlon', 'lasttim'):
                setattr(self, k, np.delete(getattr(self, k), idx))
        for i in (reversed(idx) if isinstance(idx, np.ndarray) else [idx]):
            del self.accolor[i]

    # ------------------------------------------------------------ the update
    def attach(self, sim, **kw):
        """Let ``sim`` (a ResidentSim) run the update inside its steps: ``sim.set_trails`` with this object's
        ``active`` / ``dt`` and ``kw`` (simt, lasttim, max_segments)."""
        self.sim = sim
        sim.set_trails(True, self.active, self.dt, **kw)

    def update(self, t):
        if self.sim is not None:
            return
        self.acid = self.traf.id
        if not self.active:
            self.lastlat = self.traf.lat
            self.lastlon = self.traf.lon
            self.lasttim[:] = t
            return
        ctx = self._ctx or _lib.default_context()
        r = ctx.trails_update(self.traf.lat, self.traf.lon, self.lastlat, self.lastlon, self.lasttim, t, self.dt)
        self.lastlat, self.lastlon, self.lasttim = r['lastlat'], r['lastlon'], r['lasttim']
        self._take(r, t)

    def collect(self, t=None):
        """Attached: drain the sim's segments into the lists; ``t`` (default: the ``t`` of the last step's
        update) dates ``fcol``.  Returns the number of segments taken."""
        r = self.sim.ctx.sim_trails_drain(last=True)
        self.lastlat, self.lastlon = r['lastlat'], r['lastlon']
        if t is None:
            t = self.sim.ctx.sim_read_trails(arrays=False)['last_t']
        self._take(r, t)
        return len(r['idx'])

    def _take(self, r, t):
        if len(r['idx']):
            if isinstance(self.col, np.ndarray):
                self.col = self.col.tolist()
            self.col.extend(self.accolor[i] for i in r['idx'])
        if self.pygame:
            for k in ('lat0', 'lon0', 'lat1', 'lon1', 'time'):
                setattr(self, k, np.concatenate((getattr(self, k), r[k])))
        else:
            for k in ('lat0', 'lon0', 'lat1', 'lon1'):
                getattr(self, 'new' + k).extend(r[k].tolist())
        self.fcol = 1. - np.minimum(self.tcol0, np.abs(t - self.time)) / self.tcol0

    # ------------------------------------------------------------ host-only
    def buffer(self):
        for k in ('lat0', 'lon0', 'lat1', 'lon1', 'time'):
            setattr(self, 'bg' + k, np.append(getattr(self, 'bg' + k), getattr(self, k)))
        if isinstance(self.bgcol, np.ndarray):
            self.bgcol = self.bgcol.tolist()
        if isinstance(self.col, np.ndarray):
            self.col = self.col.tolist()
        self.bgcol = self.bgcol + self.col
        self.bgacid = self.bgacid + self.acid
        self.clearfg()

    def clearnew(self):
        self.newlat0, self.newlon0, self.newlat1, self.newlon1 = [], [], [], []

    def clearfg(self):
        self.lat0, self.lon0, self.lat1, self.lon1, self.time = _none(), _none(), _none(), _none(), _none()
        self.col = _none()

    def clearbg(self):
        self.bglat0, self.bglon0, self.bglat1, self.bglon1, self.bgtime = _none(), _none(), _none(), _none(), _none()
        self.bgacid = []

    def clear(self):
        self.lastlon, self.lastlat = _none(), _none()
        self.clearfg()
        self.clearbg()
        self.clearnew()

    def setTrails(self, *args):
        if len(args) == 0:
            return True, 'TRAIL ON/OFF, [dt] / TRAIL acid color\n' + ('TRAILS ARE ON' if self.active else 'TRAILS ARE OFF')
        if type(args[0]) == bool:
            self.active = args[0]
            if len(args) > 1:
                self.dt = args[1]
            if not self.active:
                self.clear()
            if self.sim is not None:
                self.sim.set_trails(True, self.active, self.dt)
        else:
            if len(args) < 2 or args[1] not in ['BLUE', 'RED', 'YELLOW']:
                return False, 'Set aircraft trail color with: TRAIL acid BLUE/RED/YELLOW'
            self.changeTrailColor(args[1], args[0])
        return True

    def changeTrailColor(self, color, idx):
        self.accolor[idx] = self.colorList[color]

    def reset(self):
        self.accolor = []
        self.lastlat, self.lastlon, self.lasttim = _none(), _none(), _none()
        self.clear()
        self.active = False
