"""GPU-resident synthetic sim step over libbsaccel's bsa_sim_*.

State lives in HBM across steps; the host only launches.  One step:
CD + MVP every ``cd_every`` steps (asas.update, asas.py:473-504, with
``asas.active = inconf`` standing in for ResumeNav, or with ``resume_nav`` the
device-side resopairs bookkeeping + ResumeNav), then Pilot.APorASAS
(no wind, constant wind or a 2-D field) fused with the kinematic update
(traffic.py:397-409).  State is kept on the device in home order (the spatial
order of the initial traffic); arrays cross the API in aircraft-index order.
With several ranks (one process per GPU) each rank owns a contiguous,
spatially compact range of home rows; before each CD it receives, over RCCL,
only the column tiles its rows can reach (the halo exchange).
"""
import numpy as np

from . import _lib, dist

FT = 0.3048
KTS = 0.514444
NM = 1852.0
FPM = FT / 60.


def initial_state(traf):
    """Sim state of a freshly created synthetic traffic set (no wind).

    Mirrors Traffic.create (traffic.py:192-312) for what the step reads:
    tas = gs, hdg = trk, gs components, AP targets = the initial values,
    ``ap.vs = 1500 fpm`` (traffic.py:289), ``selalt = alt``, bank 25 deg,
    eps 0.01 (traffic.py:290-308), OpenAP airborne acceleration 0.5 m/s^2
    (perfoap.py:271-280), ``asas.alt = alt`` (asas.py:405-409).
    """
    n = traf.ntraf
    tas = np.array(traf.gs, dtype=np.float64)
    hdg = np.array(traf.trk, dtype=np.float64)
    return dict(lat=np.array(traf.lat, dtype=np.float64), lon=np.array(traf.lon, dtype=np.float64),
                alt=np.array(traf.alt, dtype=np.float64), tas=tas, hdg=hdg,
                vs=np.array(traf.vs, dtype=np.float64), gs=tas.copy(), trk=hdg.copy(),
                gseast=tas * np.sin(np.radians(hdg)), gsnorth=tas * np.cos(np.radians(hdg)),
                ap_trk=hdg.copy(), ap_tas=tas.copy(), ap_alt=np.array(traf.alt, dtype=np.float64),
                ap_vs=np.full(n, 1500. * FPM), selalt=np.array(traf.alt, dtype=np.float64),
                bank=np.full(n, np.radians(25.)), eps=np.full(n, 0.01), accel=np.full(n, 0.5),
                asas_alt=np.array(traf.alt, dtype=np.float64))


def params(simdt=0.05, rpz=5.0 * NM, hpz=1000.0 * FT, tla=300.0, cd_every=1, reso=True, mar=1.05,
           swresohoriz=True, swresospd=False, swresohdg=False, swresovert=False, swprio=False,
           priocode='FF1', wind=None, resume_nav=False, windfield=False, windfield3d=False, turbulence=None):
    """bsa_sim_params; ASAS defaults of asas.py:81-112 with asas_mar from data/default.cfg.
    ``wind=(vnorth, veast)`` [m/s]: constant wind (winddim 1); ``windfield=True``: the
    2-D field handed to ``ResidentSim(windfield=...)`` (winddim 2); ``windfield3d=True``: the
    3-D field handed to ``ResidentSim(windfield3d=...)`` (winddim 3).  ``resume_nav``: ASAS.update's
    resopairs bookkeeping and ResumeNav's asas.active (asas.py:409-504) instead of
    ``active = inconf``.  ``turbulence``: dict(on, sd, seed) for ``ResidentSim.set_turbulence``, which
    ``ResidentSim`` applies right after its init (kept beside the C struct, not in it)."""
    mvp = _lib.MvpParams(Rm=rpz * mar, dhm=hpz * mar, dtlookahead=tla, vmin=200.0 * NM / 3600.,
                         vmax=500.0 * NM / 3600., vsmin=-3000. / 60. * FT, vsmax=3000. / 60. * FT,
                         swresohoriz=int(swresohoriz), swresospd=int(swresospd),
                         swresohdg=int(swresohdg), swresovert=int(swresovert), swprio=int(swprio),
                         priocode=_lib.PRIO_CODES.get(priocode, 0), swnoreso=0, swresooff=0)
    wn, we = (0.0, 0.0) if wind is None else (float(wind[0]), float(wind[1]))
    if turbulence is not None and not set(turbulence) <= {'on', 'sd', 'seed'}:
        raise ValueError('turbulence: dict(on=, sd=, seed=)')
    p = _lib.SimParams(simdt=simdt, rpz=rpz, hpz=hpz, tla=tla, cd_every=int(cd_every),
                          reso=int(bool(reso)), mvp=mvp,
                          winddim=3 if windfield3d else (2 if windfield else (0 if wind is None else 1)),
                          resume_nav=int(bool(resume_nav)),
                          windnorth=wn, windeast=we)
    p.turbulence = None if turbulence is None else dict(turbulence)
    return p


class ResidentSim:
    """Device-resident traffic; ``rank``/``world`` > 1 shards the rows over GPUs."""

    def __init__(self, state, p, ctx=None, rank=0, world=1, windfield=None, limits=None, group=None,
                 windfield3d=None):
        """``windfield``: dict(lat, lon, vnorth, veast) of the 2-D field's points
        (Windfield.lat / lon / vnorth[0, :] / veast[0, :]) for ``winddim`` 2.
        ``windfield3d``: dict(lat, lon, vnorth, veast, altstep) of the 3-D field
        (Windfield.lat / lon, vnorth / veast of shape (nalt, nvec), altstep [m])
        for ``winddim`` 3: Windfield.getdata's altitude branch (windfield.py:181-202)
        per aircraft; every rank uploads it on its own context.
        ``limits``: per-aircraft OpenAP envelope dict(hmax, vmin, vmax, vsmin,
        vsmax, axmax) for Pilot.applylimits (pilot.py:65-68), or None.
        ``group``: an in-process ``_lib.Group`` to join as ``rank`` instead of
        an RCCL communicator (several ranks in one process, one thread each)."""
        self.ctx = ctx or _lib.default_context()
        self.rank, self.world = rank, world
        if group is not None:
            if getattr(self.ctx, 'comm_rank_world', None) != (rank, group.nranks):
                self.ctx.comm_init_group(group, rank)
        elif world > 1:
            dist.init_comm(self.ctx, rank, world)
        if windfield is not None:
            self.ctx.set_windfield(windfield['lat'], windfield['lon'], windfield['vnorth'],
                                   windfield['veast'])
        if windfield3d is not None:
            self.set_windfield3d(**windfield3d)
        self.ctx.sim_init(state, p)
        if limits is not None:
            self.ctx.sim_set_limits(limits)
        self.params = p
        if getattr(p, 'turbulence', None) is not None:
            self.set_turbulence(**p.turbulence)

    def step(self, nsteps=1):
        """Advance ``nsteps`` in one batch; returns the steps run -- fewer when a condition
        of ``set_conditions`` fired: the batch ends after that step (``conditions()``)."""
        return self.ctx.sim_step(nsteps)

    def set_conditions(self, cond=None, idx=(), condtype=(), target=(), lastdif=()):
        """Conditional commands (ATALT / ATSPD; conditional.py:25-49) as the last stage of
        every step (bsa_sim_set_conditions): ``cond`` is a ``bluesky_amd.conditional.Condition``
        (kept: ``delete`` applies ``delac`` to it as well), or pass the arrays ``idx`` (aircraft
        index), ``condtype`` (0 altitude, 1 speed), ``target``, ``lastdif``.  A step in which a
        condition fires completes, then the batch stops: ``step`` returns early, ``conditions()``
        names the fired ones, and the caller executes their commands before stepping on
        (``bluesky_amd.conditional.run`` is that loop).  None / empty switches it off.
        One rank only."""
        self._cond = cond
        if cond is not None:
            idx, condtype, target, lastdif = cond.arrays() if cond.ncond else ((), (), (), ())
        self.ctx.sim_set_conditions(idx, condtype, target, lastdif)

    def conditions(self):
        """(indices of the conditions that fired at the last stop, ascending, as rows of the
        table before this call; the step count at which they fired) -- bsa_sim_cond_poll.  The
        fired conditions then leave the device table (delcondition); without a stop since
        the last call the list is empty."""
        return self.ctx.sim_cond_poll()

    def read_conditions(self):
        """dict of idx, condtype, target, lastdif of the live conditions (bsa_sim_read_conditions)."""
        return self.ctx.sim_read_conditions()

    def set_params(self, p):
        """New parameters for the running sim (bsa_sim_set_params; e.g. ZONER / DTLOOK)."""
        self.ctx.sim_set_params(p)
        self.params = p

    def set_windfield3d(self, lat=None, lon=None, vnorth=None, veast=None, altstep=None):
        """Replace the 3-D wind field between steps (a weather reload; bsa_set_windfield3d).
        The steps that follow read the new field; no kept detect state is dropped (the
        field is no detect input).  Sharded: every rank calls it."""
        self.ctx.set_windfield3d(lat, lon, vnorth, veast, altstep)

    def set_turbulence(self, on=True, sd=(0, 0.1, 0.1), seed=0):
        """Turbulence.Woosh (turbulence.py:24-46) as the last stage of every step
        (bsa_sim_set_turbulence): position noise with standard deviations ``sd`` [m/s] along
        the flight direction, the wing direction and the vertical, scaled by sqrt(simdt);
        ``sd`` is clamped like ``SetStandards`` (at least 1e-6).  The draws are build-defined
        (``bluesky_amd.turbulence.draws``): a function of ``seed``, the call number
        (``turb_call``) and the aircraft's current index only, so a run repeats bitwise
        whatever the batching or the rank count.  While on, every detect makes its records
        from the perturbed state.  ``on=False`` keeps ``sd`` / ``seed`` but
        runs nothing.  Sharded: every rank calls it alike."""
        self.ctx.sim_set_turbulence(on, sd, seed)

    def turb_call(self, set_to=None):
        """The call number of the next step's draws (0 at init, + 1 per step while
        turbulence is on); ``set_to`` continues another sim's stream."""
        return self.ctx.sim_turb_call(set_to)

    def halo_stats(self):
        """Halo exchange of the sharded step (bsa_sim_halo_stats): rx / tx bytes per CD
        call, tiles received at the last CD call, capacity regrowths."""
        return self.ctx.sim_halo_stats()

    def update(self, **arrays):
        """Overwrite state arrays (host simulator changed the traffic between
        steps) keeping the ASAS bookkeeping (bsa_sim_update)."""
        self.ctx.sim_update(**arrays)

    def set_perf(self, table=None, type_idx=None):
        """OpenAP.update's flight phase, phase-dependent envelope and
        acceleration in every step (bsa_sim_set_perf; bluesky_amd.perf builds
        ``table`` / ``type_idx``); None switches it off."""
        self.ctx.sim_set_perf(table, type_idx)

    def read_perf(self):
        """(flight phase of the last step, traf.ax) of this rank's rows."""
        return self.ctx.sim_read_perf()

    def set_forces(self, ftable=None, mass=None):
        """The drag / thrust / fuel-flow half of OpenAP.update in every step, and
        the fuel burnt per aircraft (bsa_sim_set_forces; needs ``set_perf``;
        bluesky_amd.perf.force_table builds ``ftable`` / ``mass``); None switches it off."""
        self.ctx.sim_set_forces(ftable, mass)

    def read_forces(self):
        """dict of cd0, drag, thrustratio, thrust, fuelflow, bank of the last step
        and fuel_used [kg] so far, of this rank's rows."""
        return self.ctx.sim_read_forces()

    def set_fms(self, rows=None, off=None, n=None, state=None, simt=0.0, t0=-999.):
        """Autopilot.update (LNAV / VNAV guidance, waypoint switching) at the start
        of every step, so the aircraft follow their routes inside a batch
        (bsa_sim_set_fms; ``rows, off, n, state`` from ``bluesky_amd.fms.route_table`` /
        ``from_bluesky``; ``simt``: the sim time of the next step, ``t0``: Autopilot.t0).
        None switches it off."""
        self.ctx.sim_set_fms(rows, off, n, state, simt, t0)

    def set_recovery(self, on=True):
        """Waypoint recovery after ResumeNav inside the step (bsa_sim_set_recovery):
        with ``resume_nav`` on, every CD call sends each ownship whose resopair it
        drops back to its route with ``Route.findact`` + ``Route.direct``
        (asas.py:459-465), once per dropped pair, before the step's pilot reads
        ``ap.alt``.  Needs ``set_fms`` (refused without it; ``set_fms(None)``
        switches it off) and does nothing with ``resume_nav`` off.  Limit: the
        reference's ``direct`` looks the waypoint up by NAME and takes the first
        match; the device goes to the index ``findact`` found, which is the same
        only for routes whose waypoint names are unique
        (``fms.from_bluesky(traf, unique_names=True)`` checks that)."""
        self.ctx.sim_set_recovery(on)

    def read_dropcount(self):
        """Resopairs ResumeNav dropped per ownship in the last CD call, this rank's
        rows (bsa_sim_read_dropcount)."""
        return self.ctx.sim_read_dropcount()

    def read_fms(self):
        """dict of the FMS state, ``iactwp``, the autopilot targets of this rank's
        rows, and ``simt``, ``t0``, ``ticks`` (bsa_sim_read_fms)."""
        return self.ctx.sim_read_fms()

    def edit_routes(self, records):
        """A batch of route edit records (``fms.RouteNames.addwpt`` / ``delwpt`` /
        ``direct``, ``fms.record``) on the sim's own route table, between batches of steps
        (bsa_sim_route_edit): ADDWPT / DELWPT / DIRECT without reading the
        table back.  The FMS clock, the tick count and every kept detect state stay.  A
        refused batch raises ``fms.RouteEditRefused`` and changes nothing.  One rank only."""
        self.ctx.sim_route_edit(records)

    def read_routes(self):
        """``(rows, off, n, wptype)``: the route table in aircraft order, compacted, as
        ``set_fms`` takes it (bsa_sim_read_routes)."""
        return self.ctx.sim_read_routes()

    def route_stats(self):
        """dict of the table's ``live`` and ``dead`` rows, the rows ``written`` by the last
        ``edit_routes`` and the ``compactions`` since ``set_fms`` (bsa_sim_route_stats)."""
        return self.ctx.sim_route_stats()

    def create(self, state, ids=None, *, limits=None, perf=None, mass=None, fms=None):
        """Append aircraft (Traffic.create; ``state`` as ``initial_state`` returns,
        m long each): indices n..n+m-1 (bsa_sim_create; collective with several ranks).
        ``ids``: their callsigns, when ``set_sectors`` was given ids.
        While the envelope, OpenAP or the guidance run, plain ``create`` is refused; hand in
        the new aircraft's part of every such stage (bsa_sim_create_with), m
        long each: ``limits`` (the dict ``ResidentSim(limits=...)`` takes), ``perf`` (their
        ``type_idx``, rows of ``set_perf``'s table), ``mass`` (``set_forces``), ``fms`` =
        ``(rows, off, n, state)`` as ``fms.route_table`` / ``fms.from_bluesky`` /
        ``fms.synthetic_routes`` return it for the new aircraft alone.  A part for a stage that
        is off, a missing one, a type outside the table or a route outside ``rows`` is refused
        and changes nothing.  The others keep everything -- fuel burnt, the FMS clock and tick
        count; the new ones start as after ``set_perf`` / ``set_forces``.  With guidance on:
        one rank only."""
        extra = {k: v for k, v in (('limits', limits), ('type_idx', perf), ('mass', mass), ('fms', fms)) if v is not None}
        if getattr(self, 'ids', None) is not None:
            if ids is None or len(ids) != len(state['lat']):
                raise ValueError('create: one id per new aircraft (set_sectors was given ids)')
        self.ctx.sim_create(state, extra or None)
        if getattr(self, 'ids', None) is not None:   # (after the call: a refused create changes nothing)
            self.ids = self.ids + list(ids)

    def delete(self, idx):
        """Remove aircraft ``idx`` (Traffic.delete: the rest shift down in order),
        keeping the callsign-keyed ASAS bookkeeping of the others (bsa_sim_delete).
        With sectors on, those that were inside a sector are reported as ``left`` by
        the next ``sectors()``."""
        d = np.unique(np.asarray(idx, dtype=np.int64).ravel())
        self.ctx.sim_delete(d)
        if getattr(self, '_cond', None) is not None:   # Traffic.delete: cond.delac(idx), idx sorted (traffic.py:370-377)
            self._cond.delac(d)
            # the reference's sequential delac can leave a condition of the last aircraft pointing past the
            # new n (it would raise at the next update there); the device table drops it, so does the drop-in
            past = np.where(np.asarray(self._cond.idx) >= self.ctx.n)[0]
            if len(past):
                self._cond.delcondition(past)
        if getattr(self, '_sect_names', None):
            pos, words = self.ctx.sim_sectors_deleted()
            ids = getattr(self, 'ids', None)
            for q, w in zip(pos, words):
                who = ids[d[q]] if ids is not None else int(d[q])
                self._sect_gone.append((who, int(w)))
        if getattr(self, 'ids', None) is not None:
            gone = set(int(x) for x in d)
            self.ids = [x for k, x in enumerate(self.ids) if k not in gone]

    def set_areas(self, areas):
        """The sim's area table (bsa_sim_set_areas): ``areas`` maps a name to ``(type, coordinates,
        top, bottom)`` -- ``bluesky_amd.areafilter.areas`` is such a dict.  Forgets the sectors.
        Sharded: every rank calls it alike."""
        self._area_names = list(areas)
        self._sect_names, self._sect_gone = [], []
        self.ctx.sim_set_areas([areas[k] for k in self._area_names])

    def set_sectors(self, names, every=1, ids=None):
        """Sector occupancy inside the step (plugins/sectorcount.py:53-96; bsa_sim_set_sectors):
        the areas ``names`` (at most 64, of ``set_areas``) are tested every ``every`` steps --
        ``every = max(1, round(update_interval / simdt))`` -- after the step's last stage; the
        masks are seeded at the current state, as SECTORCOUNT ADD does.  ``ids``: the callsigns
        by aircraft index; ``sectors()`` then lists callsigns, and ``create`` wants the new
        ones.  ``names = []`` switches it off.  Sharded: every rank calls it alike."""
        tab = getattr(self, '_area_names', [])
        missing = [k for k in names if k not in tab]
        if missing:
            raise ValueError('set_sectors: no area %r (set_areas)' % (missing[0],))
        if ids is not None and len(ids) != self.ctx.n:
            raise ValueError('set_sectors: one id per aircraft')
        self.ctx.sim_set_sectors([tab.index(k) for k in names], every)
        self._sect_names, self._sect_gone = list(names), []
        self._sect_gone_total = np.zeros(len(names), dtype=np.int64)
        self.ids = None if ids is None else list(ids)

    def sectors(self, masks=False):
        """The LAST sector update of this rank's rows (bsa_sim_sectors_poll): per sector name a dict
        of ``count``, ``arrived`` and ``left`` (aircraft indices, ascending; callsigns, sorted, with
        ids), ``arrived_total`` / ``left_total`` over every update since ``set_sectors`` (also those
        inside a batch) and ``step``, the step count of that update (0: the seeding pass).  Aircraft
        deleted since the last call that were inside are listed in ``left_deleted`` (their
        index when deleted, or callsign), count in ``left_total`` and, with ids, are part of
        ``left`` -- once.  ``masks``: also ``inside`` / ``inside_before``, bool per row of
        ``row_ids()``.  Several ranks: ``dist.merge_sectors`` sums the ranks' answers."""
        names = getattr(self, '_sect_names', None)
        if not names:
            raise ValueError('sectors: set_sectors first')
        r = self.ctx.sim_sectors_poll(masks=True)
        rows = self.row_ids()
        cur, prev = r['cur'][rows], r['prev'][rows]
        ids = getattr(self, 'ids', None)
        gone, self._sect_gone = self._sect_gone, []
        out = {}
        for k, name in enumerate(names):
            bit = np.uint64(1) << np.uint64(k)
            c, p = (cur & bit) != 0, (prev & bit) != 0
            arrived, left = rows[c & ~p], rows[p & ~c]
            deleted = [who for who, w in gone if (w >> k) & 1]
            self._sect_gone_total[k] += len(deleted)
            if ids is not None:
                arrived = sorted(ids[i] for i in arrived)
                left = sorted([ids[i] for i in left] + deleted)
            else:
                arrived, left = [int(i) for i in arrived], [int(i) for i in left]
            out[name] = dict(count=int(r['count'][k]), arrived=arrived, left=left, left_deleted=sorted(deleted),
                             arrived_total=int(r['arrived_total'][k]),
                             left_total=int(r['left_total'][k]) + int(self._sect_gone_total[k]), step=r['step'])
            if masks:
                out[name].update(inside=c, inside_before=p)
        return out

    def set_exparea(self, shape_name=None, dt=0.5, every=None, simt=0.0, taxi=True, taxialt=1500 * FT, active=None):
        """The experiment area inside the step (plugins/area.py:107-175; bsa_sim_set_exparea): flight
        statistics per aircraft (2-D / 3-D distance, work) and the exit and taxi deletes.  ``shape_name``: an
        area of ``set_areas`` (``Area.name``), None for no area (everything is outside), False switches the
        stage off.  ``dt``: the plugin's nominal interval, which the accumulators use; the pass runs every
        ``every`` steps counted from the first call, default ``max(dt, simdt) / simdt``, as the step's last
        launch.  ``taxi`` / ``taxialt``: ``Area.swtaxi`` / ``swtaxialt`` (taxi False: an aircraft sinking
        through ``taxialt`` is deleted); ``active``: ``Area.active``, default whether there is an area.
        The first call starts the arrays as ``Area.create`` would for every aircraft at ``simt`` (``inside``
        all False); later calls change the parameters only.  A step with an exit or a taxi delete
        completes, then the batch stops: ``step`` returns early and ``exparea_events()`` lists them
        (``bluesky_amd.exparea.run`` is that loop).  ``work`` needs ``set_forces``: without it, it stays 0.
        One rank only."""
        if shape_name is False:
            self.ctx.sim_set_exparea(False)
            return
        tab = getattr(self, '_area_names', [])
        if shape_name is not None and shape_name not in tab:
            raise ValueError('set_exparea: no area %r (set_areas)' % (shape_name,))
        if every is None:
            every = max(1, int(round(max(dt, self.params.simdt) / self.params.simdt)))
        self.ctx.sim_set_exparea(True, -1 if shape_name is None else tab.index(shape_name), dt, every, simt,
                                 (shape_name is not None) if active is None else active, taxi, taxialt)

    def exparea_events(self):
        """The deletes of the last stop (bsa_sim_exparea_poll): dict of ``delidx`` (exits) and ``delidxalt``
        (taxi deletes), aircraft indices ascending as ``np.where`` gives them, ``step``, and ``records`` -- the
        log columns the device has, per exited aircraft.  Read once; empty without a stop since the last call."""
        return self.ctx.sim_exparea_poll()

    def read_exparea(self):
        """dict of distance2D, distance3D, work, oldalt, create_time, inside by aircraft index (bsa_sim_read_exparea)."""
        return self.ctx.sim_read_exparea()

    def set_trails(self, on=True, active=True, dt=10.0, simt=0.0, lasttim=None, max_segments=1 << 24):
        """Trails.update (traffic/trails.py:71-135) as a stage of every step, after the conditions
        (bsa_sim_set_trails): while ``active`` every aircraft whose last segment is more than ``dt`` old emits
        the segment from its last to its current position, in ascending index order, into buffers on the
        device; ``trails()`` drains them.  ``simt``: the sim time of the next step (the stage's clock then
        accumulates ``simdt`` as the reference's does).  The first call starts ``lastlat`` / ``lastlon`` at
        the current positions and ``lasttim`` at ``lasttim`` (a scalar or one value per aircraft), default
        ``simt - simdt``: the time of the update that preceded a TRAIL ON typed between two steps.  Later
        calls change ``active`` / ``dt`` / ``max_segments`` only; ``active=False`` after True drops the
        undrained segments, as ``setTrails(False)`` does.  A ``step(k)`` that could emit more than
        ``max_segments`` (undrained + n * min(k, k * simdt // dt + 1)) is refused before it runs: drain, or
        step less.  ``on=False`` switches the stage off.  One rank only."""
        if lasttim is None:
            lasttim = simt - self.params.simdt
        self.ctx.sim_set_trails(on, active, dt, simt, lasttim, max_segments)
        self._trails_active = bool(on) and bool(active)

    def trails(self, last=True):
        """The trail part of ScreenIO's ACDATA (screenio.py:217-226) since the last call, which it clears
        (``clearnew``): dict of ``swtrails``, ``traillat0`` / ``traillon0`` / ``traillat1`` / ``traillon1``
        in emission order, with ``last`` ``traillastlat`` / ``traillastlon`` by aircraft index, plus
        ``trailtime`` (the ``t`` of each segment's update) and ``trailidx`` (the aircraft's index when it
        emitted).  Synchronises (bsa_sim_trails_drain)."""
        r = self.ctx.sim_trails_drain(last)
        out = dict(swtrails=getattr(self, '_trails_active', False), traillat0=r['lat0'], traillon0=r['lon0'],
                   traillat1=r['lat1'], traillon1=r['lon1'], trailtime=r['time'], trailidx=r['idx'])
        if last:
            out.update(traillastlat=r['lastlat'], traillastlon=r['lastlon'])
        return out

    def read_trails(self):
        """dict of lastlat, lastlon, lasttim by aircraft index, ``simt`` (the next step's), ``last_t`` (the last
        step's) and ``undrained`` (bsa_sim_read_trails)."""
        return self.ctx.sim_read_trails()

    def set_adsb(self, on=True, noise=False, transerror=(1e-4, 100 * FT), trunctime=0.0, seed=0, draws='shared',
                 simt=0.0, lastupdate=None):
        """ADSB.update (traffic/adsbmodel.py:44-59) as a stage of every step, where Traffic.update runs it: on
        the state the previous step left, before the autopilot (bsa_sim_set_adsb).  An aircraft with
        ``lastupdate + trunctime < simt`` takes the current ``trk tas gs vs`` and ``lat lon alt`` -- with
        ``noise`` plus a normal of ``transerror`` ([deg] for lat / lon, [m] for alt) -- into the picture, and
        its ``lastupdate`` grows by ``trunctime``.  ``simt``: the sim time of the next step (the stage's clock
        then accumulates ``simdt``).  ``draws='shared'`` restates the reference, which draws one normal per
        quantity per call for all updated aircraft; ``'per_aircraft'`` gives each its own.  The draws are
        build-defined (``bluesky_amd.adsb.draws``): a function of ``seed``, the call number (``adsb_call``) and,
        per aircraft, the aircraft's current index, so a run repeats bitwise whatever the batching or the rank
        count.  The first call starts the picture at the current state -- ``vs`` too, where the reference's
        ``create`` leaves 0 -- and ``lastupdate`` at ``lastupdate`` (a scalar or one value per aircraft, default
        0); later calls change the settings only.  ``create`` gives new aircraft ``lastupdate = -trunctime *
        u``, the picture from their state and ``vs = 0``.  ``on=False`` switches the stage off and frees its
        arrays.  The step's own detect still reads the true state.  Sharded: every rank calls it alike."""
        self.ctx.sim_set_adsb(on, noise, transerror, trunctime, seed, draws, simt, lastupdate)

    def read_adsb(self):
        """dict of ``lastupdate lat lon alt trk tas gs vs`` of this rank's rows (by aircraft index; other rows
        0), ``simt`` (the time of the next step's update) and ``call`` (bsa_sim_read_adsb)."""
        return self.ctx.sim_read_adsb()

    def adsb_call(self, set_to=None):
        """The call number of the next noisy update's draws (0 when switched on, + 1 per step while noise is
        on); ``set_to`` continues another sim's stream."""
        return self.ctx.sim_adsb_call(set_to)

    def set_geovectors(self, geovecs, every=1):
        """Geovectoring inside the step (plugins/geovector.py:76-128; bsa_sim_set_geovectors):
        ``geovecs`` is the plugin's list of ``[area, gsmin, gsmax, trkmin, trkmax, vsmin, vsmax]``
        (m/s, deg, m/s; ``bluesky_amd.geovector.geovecs`` is such a list), the areas those of
        ``set_areas``; a geovector on an unknown area is skipped, a limit is on by Python truth.
        Applied as the first stage of a step, every ``every`` steps counted from this call --
        ``every = max(1, round(max(update_interval, simdt) / simdt))``, the first time one interval
        from now.  Needs ``set_areas`` and ``set_fms``; ``set_areas`` forgets the geovectors,
        ``set_fms(None)`` switches them off, as does an empty list.  Sharded: every rank calls it alike."""
        from . import geovector
        rows, _ = geovector.table(geovecs, getattr(self, '_area_names', []))
        self.ctx.sim_set_geovectors(rows, every)

    def geovector_stats(self):
        """dict of ``applies`` (applications since ``set_geovectors``) and ``changed`` (per target
        array, this rank's aircraft changed, summed over the applications)."""
        return self.ctx.sim_geovec_stats()

    def read(self):
        return self.ctx.sim_read()

    def stats(self):
        return self.ctx.sim_stats()

    def aborts(self):
        """Batches that aborted (a buffer overflowed, a kept list went stale) and were re-run from the aborted
        step, since the sim was made (bsa_sim_aborts)."""
        return self.ctx.sim_aborts()

    def asas_stats(self):
        return self.ctx.sim_asas_stats()

    def resopairs(self):
        return self.ctx.sim_resopairs()

    def row_ids(self):
        """Aircraft indices of this rank's rows (ascending)."""
        return self.ctx.sim_row_ids()

    def gather_pairs(self, root=0):
        """C2: the last CD call's pairs of all ranks, on ``root`` (collective)."""
        return self.ctx.gather_pairs(root)

    def acdata_request(self):
        """Enqueue an ACDATA snapshot of this rank's rows behind the queued steps
        (screenio.py:194-239; no host synchronisation)."""
        self.ctx.sim_acdata_request()

    def acdata(self, wait=True):
        """The requested snapshot: dict of per-row arrays (lat lon alt tas cas gs
        trk vs tcpamax inconf asasn asase) plus steps, row_begin/row_end and the
        four pair counts; None while in flight when ``wait`` is False."""
        return self.ctx.sim_acdata_poll(wait)
