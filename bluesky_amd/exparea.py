"""The experiment area (the reference's AREA plugin, plugins/area.py:85-220) on the device: a
drop-in ``Area`` with the reference's surface -- ``create``, ``update``, ``set_area``, ``set_taxi``
and ``active / dt / name / swtaxi / swtaxialt / inside / oldalt / distance2D / distance3D / work /
create_time`` -- without its ``bs`` globals and without ``bs.scr``: the traffic object, the clock
and the logger are handed to the constructor.  The logger is any callable, or an object with
``log(*columns)``; it receives the reference's 17 columns in the reference's order.

On host arrays ``update`` evaluates through ``bsa_exparea_update``.  Inside a resident run the
same object goes to ``run``: the arrays live in the sim (``ResidentSim.set_exparea``), the pass is
the step's last stage, and a step with an exit or a taxi delete stops the batch.

The reference's properties, kept: ``inside`` starts all False, so an aircraft must be seen inside
once before it can exit; ``delidxalt`` is computed before ``traf.delete(delidx)`` and applied after
it, so its indices are stale once the first delete removed anything (an index past the shrunk
table is dropped here; the reference raises); ``update`` returns at once while ``swtaxi and not
active``; the accumulators use the nominal ``dt``, whatever time passed.
"""
import numpy as np

from . import _lib, areafilter, conditional

ft = 0.3048
LOG_COLUMNS = ('id', 'create_time', 'flight_time', 'distance2D', 'distance3D', 'work', 'lat', 'lon', 'alt', 'tas', 'vs',
               'hdg', 'asas_active', 'pilot_alt', 'pilot_tas', 'pilot_vs', 'pilot_hdg')


class Area:
    def __init__(self, traf=None, logger=None, clock=None, ctx=None, evaluate=None):
        """``traf``: what the reference reads from ``bs.traf`` (``id gs vs alt lat lon tas hdg``,
        ``perf.thrust``, ``asas.active``, ``pilot.alt / tas / vs / hdg``, ``delete``).  ``clock()``:
        ``sim.simt``.  ``evaluate(**arrays) -> dict`` replaces the device call (tests without a device)."""
        self.traf, self.ctx, self.evaluate = traf, ctx, evaluate
        self.clock = clock if clock is not None else (lambda: 0.0)
        self.logger = logger
        self.active = False
        self.dt = 0.5
        self.name = None
        self.swtaxi = True
        self.swtaxialt = 1500.
        self.inside = np.array([], dtype=bool)
        self.oldalt = np.array([])
        self.distance2D = np.array([])
        self.distance3D = np.array([])
        self.work = np.array([])
        self.create_time = np.array([])
        self.sim = None          # a ResidentSim once attached (run)
        self.ids = None          # ... and its callsigns by aircraft index

    # ---------------------------------------------------------------- the reference's surface
    def create(self, n=1):
        self.inside = np.append(self.inside, np.zeros(n, dtype=bool))
        for k in ('oldalt', 'distance2D', 'distance3D', 'work', 'create_time'):
            setattr(self, k, np.append(getattr(self, k), np.zeros(n)))
        self.create_time[-n:] = self.clock()
        self.oldalt[-n:] = np.asarray(self.traf.alt)[-n:]

    def delete(self, idx):
        """TrafficArrays.delete on this object's arrays."""
        for k in ('inside', 'oldalt', 'distance2D', 'distance3D', 'work', 'create_time'):
            setattr(self, k, np.delete(getattr(self, k), idx))

    def log(self, *columns):
        if self.logger is None:
            return
        (self.logger.log if hasattr(self.logger, 'log') else self.logger)(*columns)

    def update(self):
        if self.swtaxi and not self.active:
            return
        traf = self.traf
        args = dict(gs=traf.gs, vs=traf.vs, alt=traf.alt, lat=traf.lat, lon=traf.lon, thrust=traf.perf.thrust,
                    distance2D=self.distance2D, distance3D=self.distance3D, work=self.work, oldalt=self.oldalt,
                    inside=self.inside, dt=self.dt, area=areafilter.areas.get(self.name) if self.name is not None else None,
                    active=self.active, swtaxi=self.swtaxi, swtaxialt=self.swtaxialt)
        r = self.evaluate(**args) if self.evaluate is not None else (self.ctx or _lib.default_context()).exparea_update(**args)
        for k in ('distance2D', 'distance3D', 'work', 'oldalt', 'inside'):
            setattr(self, k, np.array(r[k]))
        delidx, delidxalt = r['delidx'], r['delidxalt']
        if len(delidx) > 0:
            simt = self.clock()
            self.log(np.array(traf.id)[delidx], self.create_time[delidx], simt - self.create_time[delidx],
                     self.distance2D[delidx], self.distance3D[delidx], self.work[delidx],
                     traf.lat[delidx], traf.lon[delidx], traf.alt[delidx], traf.tas[delidx], traf.vs[delidx],
                     traf.hdg[delidx], traf.asas.active[delidx], traf.pilot.alt[delidx], traf.pilot.tas[delidx],
                     traf.pilot.vs[delidx], traf.pilot.hdg[delidx])
            self._delete(np.array(delidx))
        if len(delidxalt) > 0:
            self._delete([int(k) for k in delidxalt if k < len(self.inside)])

    def _delete(self, idx):
        n = len(self.inside)
        self.traf.delete(idx)
        if len(self.inside) == n:       # (a traffic stand-in without the reference's child registry)
            self.delete(idx)

    def set_area(self, *args):
        if not args:
            return True, "Area is currently " + ("ON" if self.active else "OFF") + \
                         "\nCurrent Area name is: " + str(self.name)
        if isinstance(args[0], str) and len(args) == 1:
            if areafilter.hasArea(args[0]):
                self.name = args[0]
                self.active = True
                self._logger('start')
                self._push(areas=True)
                return True, "Area is set to " + str(self.name)
            if args[0] == 'OFF' or args[0] == 'OF':
                areafilter.deleteArea(self.name)
                self._logger('reset')
                self.active = False
                self.name = None
                self._push(areas=True)
                return True, "Area is switched OFF"
            return False, "Shapename unknown. " + \
                "Please create shapename first or shapename is misspelled!"
        if isinstance(args[0], (float, int)) and 4 <= len(args) <= 6:
            self.active = True
            self.name = 'DELAREA'
            areafilter.defineArea(self.name, 'BOX', args[:4], *args[4:])
            self._logger('start')
            self._push(areas=True)
            return True, "Area is ON. Area name is: " + str(self.name)
        return False, "Incorrect arguments" + \
                      "\nAREA Shapename/OFF or\n Area lat,lon,lat,lon,[top,bottom]"

    def set_taxi(self, flag, alt=1500 * ft):
        self.swtaxi = flag
        self.swtaxialt = alt
        self._push()

    def _logger(self, what):
        f = getattr(self.logger, what, None)
        if callable(f):
            f()

    # ---------------------------------------------------------------- inside a resident run
    def attach(self, sim, ids=None, simdt=None, simt=0.0):
        """The arrays move into ``sim`` (as after ``Area.create`` for every aircraft at ``simt``) and the
        pass becomes the step's last stage, every ``max(dt, simdt) / simdt`` steps."""
        self.sim, self.simt = sim, float(simt)
        self.simdt = float(simdt if simdt is not None else sim.params.simdt)
        self.ids = list(ids) if ids is not None else ['AC%d' % k for k in range(sim.ctx.n)]
        if len(self.ids) != sim.ctx.n:
            raise ValueError('attach: one id per aircraft')
        self._push(areas=True)

    def every(self):
        return max(1, int(round(max(self.dt, self.simdt) / self.simdt)))

    def _push(self, areas=False):
        if self.sim is None:
            return
        if areas and self.name is not None:
            self.sim.set_areas(dict(areafilter.areas))
        self.sim.set_exparea(self.name, dt=self.dt, every=self.every(), simt=self.simt, taxi=self.swtaxi,
                             taxialt=self.swtaxialt, active=self.active)


def run(sim, area, nsteps, cond=None, execute=None, batch=None):
    """Advance ``sim`` (a ``ResidentSim`` ``area`` is attached to) by ``nsteps`` in batches (of ``batch``
    steps, default all at once).  A step with an exit or a taxi delete ends its batch; then, as the plugin does:
    poll, log the 17 columns of the exited aircraft in the reference's order, ``delete(delidx)``,
    ``delete(list(delidxalt))`` with the indices taken BEFORE the first delete (those past the shrunk
    table dropped), and step on.  The deletion time is ``simt`` of the stopping step before its increment
    (simulation.py:107-119: traf.update, plugin.update, simt += simdt).

    With ``cond`` (a ``conditional.Condition``) and ``execute`` the conditions run too.  The order is the
    reference's Simulation.step: the commands a step's ``cond.update()`` stacked are processed at the START
    of the next step (stack.process, simulation.py:104), after this step's plugin update -- so the area's
    deletes (with their ``delac``) come first, then the fired commands are executed.

    Returns (events, stops): ``events`` a list of dicts (step, simt, ids, delidx, delidxalt, deleted_ids,
    columns: the 17 log columns by LOG_COLUMNS), ``stops`` the conditions' (step, fired, commands)."""
    if area.sim is not sim:
        raise ValueError('run: area.attach(sim, ...) first')
    if cond is not None:
        sim.set_conditions(cond)
    events, stops, done, last = [], [], 0, area.simt
    while done < nsteps:
        ran = sim.step(min(nsteps - done, batch or nsteps))
        done += ran
        for _ in range(ran):
            last, area.simt = area.simt, area.simt + area.simdt
        sim.ctx.sim_exparea_simt(area.simt)
        stop = conditional.take_stop(sim, cond) if cond is not None else None   # (before any delete)
        if stop is not None:
            stops.append(stop)
        ev = sim.exparea_events()
        delidx, delidxalt = ev['delidx'], ev['delidxalt']
        if len(delidx) or len(delidxalt):
            rec = ev['records']
            act = rec['active'] != 0
            cols = dict(id=np.array(area.ids)[delidx], create_time=rec['create_time'], flight_time=last - rec['create_time'],
                        distance2D=rec['distance2D'], distance3D=rec['distance3D'], work=rec['work'], lat=rec['lat'],
                        lon=rec['lon'], alt=rec['alt'], tas=rec['tas'], vs=rec['vs'], hdg=rec['hdg'], asas_active=act,
                        # Pilot.APorASAS's select without wind (pilot.py:37-48, 63) for these few rows
                        pilot_alt=np.where(act, rec['asas_alt'], rec['ap_alt']),
                        pilot_tas=np.where(act, rec['asas_tas'], rec['ap_tas']),
                        pilot_vs=np.abs(np.where(act, rec['asas_vs'], rec['ap_vs'])),
                        pilot_hdg=np.where(act, rec['asas_trk'], rec['ap_trk']) % 360.)
            if len(delidx):
                area.log(*[cols[k] for k in LOG_COLUMNS])
            gone = []
            for lst in (delidx, [int(k) for k in delidxalt]):
                lst = [int(k) for k in lst if k < sim.ctx.n]
                if len(lst) == 0:
                    continue
                gone += [area.ids[k] for k in sorted(set(lst))]
                sim.delete(lst)
                dead = set(lst)
                area.ids = [x for k, x in enumerate(area.ids) if k not in dead]
            events.append(dict(step=ev['step'], simt=last, delidx=delidx, delidxalt=delidxalt, deleted_ids=gone, columns=cols))
        if stop is not None:
            conditional.execute_stop(sim, cond, stop[2], execute)
    if cond is not None and cond.ncond:
        cond.lastdif = sim.read_conditions()['lastdif']
    return events, stops
