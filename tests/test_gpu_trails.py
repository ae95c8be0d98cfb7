"""GPU: trails (traffic/trails.py) -- bsa_trails_update against the reference's golden, and the resident
step's stage: ordered emission over several workgroups and through the home permutation, the flight golden,
one batch against single steps, next to a stop and next to an abort, delete / create, refusals, and the
drop-in attached to a sim."""
import os
import types

import numpy as np
import pytest

from bluesky_amd import _lib, conditional, resident, synth, trails
from tests import trails_np, util
from tests.test_gpu_cond import altitudes, climbers, crossing, movers, traf_of
from tests.test_gpu_multirank import run_ranks
from tests.test_gpu_sim import SCALES
from tests.test_trails_np import CASES, case_of, colours, same

pytestmark = pytest.mark.gpu
KEYS = ('traillat0', 'traillon0', 'traillat1', 'traillon1', 'trailtime', 'trailidx')
SEG = dict(traillat0='lat0', traillon0='lon0', traillat1='lat1', traillon1='lon1', trailtime='time', trailidx='idx')


@pytest.fixture(scope='module')
def upd():
    return dict(np.load(os.path.join(util.GOLDEN, 'trails_update.npz')))


@pytest.fixture(scope='module')
def flight():
    return dict(np.load(os.path.join(util.GOLDEN, 'trails_flight64.npz')))


def stream(parts):
    """Several drains as one stream."""
    return {k: np.concatenate([p[k] for p in parts]) for k in KEYS}


def assert_stream(got, exp):
    """``got`` (ScreenIO's key names) equals the restatement's segments ``exp``, bitwise (a NaN as a NaN)."""
    assert np.array_equal(got['trailidx'], exp['idx'])
    for k in KEYS[:-1]:
        assert same(got[k], exp[SEG[k]]), k


def clock(simdt, nsteps, simt=0.0):
    """The t of every step: simt accumulated in fp64, as the reference's and the stage's clocks do."""
    out = []
    for _ in range(nsteps):
        out.append(simt)
        simt += simdt
    return out


def positions(ctx, init, p, nsteps):
    """lat / lon after 1 .. nsteps steps of the undisturbed sim, one step at a time."""
    sim = resident.ResidentSim(init, p, ctx=ctx)
    out = []
    for _ in range(nsteps):
        assert sim.step(1) == 1
        r = sim.read()
        out.append((r['lat'], r['lon']))
    return out


def expected(pos, ts, st, dt):
    """trails_np over the recorded positions: (segments per step, the arrays at the end)."""
    segs = []
    for (lat, lon), t in zip(pos, ts):
        st, seg = trails_np.update(st, lat, lon, t, dt, True)
        segs.append(seg)
    return segs, st


# ---------------------------------------------------------------- standalone
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
def test_standalone_update_matches_golden(ctx, upd, n):
    """Every recorded case at this n: the segments in order and the three arrays by their bytes, NaNs as NaNs;
    a capacity one below the count is refused with both numbers and leaves the arrays alone."""
    t, dt = float(upd['t']), float(upd['dt'])
    for case in CASES:
        lat, lon, st, active, exp, seg = case_of(upd, n, case)
        got = ctx.trails_update(lat, lon, t=t, dt=dt, active=active, **st)
        for k in trails_np.ARRAYS:
            assert same(got[k], exp[k]), (case, k)
        assert np.array_equal(got['idx'], seg['idx']), case
        for k in trails_np.SEGMENT:
            assert same(got[k], seg[k]), (case, k)
        m = len(seg['idx'])
        if m:
            with pytest.raises(_lib.AccelError, match='%d segments, room for %d' % (m, m - 1)) as e:
                ctx.trails_update(lat, lon, t=t, dt=dt, active=active, cap=m - 1, **st)
            assert e.value.count == m


def test_standalone_empty_launches_nothing(ctx):
    z = np.zeros(0)
    got = ctx.trails_update(z, z, z, z, z, 1.0, 1.0)
    assert len(got['idx']) == 0 and len(got['lasttim']) == 0


# ---------------------------------------------------------------- ordered emission
def test_ordered_emission_over_workgroups_and_the_home_permutation(ctx):
    """n = 4097 (17 workgroups of the pass, 65 waves, 3 scan words past a power of two) in a box whose home
    (spatial) order is not the index order.  Every third aircraft emits in the first pass, all in a later one;
    per emitting step trailidx is strictly ascending, and the whole stream equals tests/trails_np.py run on the
    positions a twin sim read back step by step, with the same clock -- bitwise."""
    n, nsteps, dt = 4097, 8, 0.2
    init = resident.initial_state(synth.box(n, 120.0, seed=5))
    p = resident.params(cd_every=4)
    pos = positions(ctx, init, p, nsteps)
    sim = resident.ResidentSim(init, p, ctx=ctx)
    last = np.where(np.arange(n) % 3 == 0, -1.0, 0.0)
    sim.set_trails(True, True, dt, simt=0.0, lasttim=last)
    assert sim.step(nsteps) == nsteps
    got = sim.trails()
    ts = clock(p.simdt, nsteps)
    segs, st = expected(pos, ts, dict(lastlat=init['lat'], lastlon=init['lon'], lasttim=last), dt)
    counts = [len(s['idx']) for s in segs]
    assert counts[0] == (n + 2) // 3 and n in counts[1:] and sum(counts) == len(got['trailidx'])
    off = np.cumsum([0] + counts)
    for q in range(nsteps):
        part = got['trailidx'][off[q]:off[q + 1]]
        assert (np.diff(part) > 0).all() and (got['trailtime'][off[q]:off[q + 1]] == ts[q]).all()
    assert_stream(got, trails_np.concat(segs))
    r = sim.read_trails()
    for k in trails_np.ARRAYS:
        assert same(r[k], st[k]), k
    assert same(got['traillastlat'], st['lastlat']) and same(got['traillastlon'], st['lastlon'])
    assert got['swtrails'] is True and r['undrained'] == 0 and r['last_t'] == ts[-1]


# ---------------------------------------------------------------- the flight golden
def fly(ctx, g, tr=None, batch=50, snap=None):
    """trails_flight64 through a ResidentSim in batches of at most ``batch`` steps, the commands between them.
    ``tr``: a drop-in to attach (the commands then go through it); ``snap(tag)`` is called before TRAIL OFF
    and at the end.  Returns (the drains, the sim)."""
    init = {k[5:]: np.array(v) for k, v in g.items() if k.startswith('init_')}
    new = {k[4:]: np.array(v) for k, v in g.items() if k.startswith('new_')}
    p = resident.params(simdt=float(g['simdt']), cd_every=1000000, rpz=1.0, hpz=1.0, tla=1.0)   # ASAS inactive, as captured
    sim = resident.ResidentSim({k: init[k] for k in _lib.SIM_STATE_FIELDS}, p, ctx=ctx)
    on, create, delete, off, on2 = [int(x) for x in g['commands']]
    dt, nsteps = float(g['dt']), int(g['nsteps'])
    if tr is not None:
        tr.traf.lat, tr.traf.lon = init['lat'], init['lon']
        tr.create(64)
        tr.attach(sim, simt=0.0)
    else:
        sim.set_trails(True, False, 10.0, simt=0.0)
    step, parts = 0, []
    while step < nsteps:
        if step in (on, on2):
            assert tr.setTrails(True, dt) is True if tr is not None else sim.set_trails(True, True, dt) is None
        if step == off:
            if snap:
                snap('before_off')
            assert tr.setTrails(False) is True if tr is not None else sim.set_trails(True, False, dt) is None
        if step == create:
            sim.create({k: new[k] for k in _lib.SIM_STATE_FIELDS})
            if tr is not None:
                r = sim.read()
                tr.traf.lat, tr.traf.lon = r['lat'], r['lon']
                tr.create(3)
        if step == delete:
            sim.delete(g['deleted'])
            if tr is not None:
                tr.delete(np.array(g['deleted']))
        k = min([batch] + [c - step for c in (on, create, delete, off, on2, nsteps) if c > step])
        assert sim.step(k) == k
        step += k
        if tr is None:
            parts.append(sim.trails())
    if snap:
        snap('final')
    return parts, sim


def test_resident_follows_the_flight_golden(ctx, flight):
    """Exactly: the emitting steps (by their t), the indices per step, trailtime bitwise, the (0, 0) starts of the
    two created aircraft that were not the last of their batch.  Coordinates: the 1e-9 rule of the resident-step
    goldens (the positions come from the device's kinematics)."""
    g = flight
    parts, sim = fly(ctx, g)
    got = stream(parts)
    assert np.array_equal(got['trailidx'], g['ev_idx'])
    assert got['trailtime'].tobytes() == g['ev_time'].tobytes()
    steps = [int(round(t / float(g['simdt']))) + 1 for t in np.unique(got['trailtime'])]
    assert steps == [int(x) for x in g['ev_step']] and np.array_equal(np.unique(got['trailtime']), g['ev_t'])
    zero = np.flatnonzero((g['ev_lat0'] == 0.0) & (g['ev_lon0'] == 0.0))
    assert len(zero) == 2 and (got['traillat0'][zero] == 0.0).all() and (got['traillon0'][zero] == 0.0).all()
    assert list(got['trailidx'][zero]) == [64, 65]
    for k, s in (('traillat0', 'lat'), ('traillat1', 'lat'), ('traillon0', 'lon'), ('traillon1', 'lon')):
        d = np.abs(got[k] - g['ev_' + SEG[k]])
        print(k, 'max abs difference', d.max())
        ok, msg = util.close(got[k], g['ev_' + SEG[k]], SCALES[s])
        assert ok, '%s: %s' % (k, msg)
    r = sim.read_trails()
    assert r['lasttim'].tobytes() == g['final_lasttim'].tobytes() and r['simt'] == float(g['final_simt'])
    for k, s in (('lastlat', 'lat'), ('lastlon', 'lon')):
        ok, msg = util.close(r[k], g['final_' + k], SCALES[s])
        assert ok, '%s: %s' % (k, msg)


@pytest.mark.parametrize('gui', ['qtgl', 'pygame'])
def test_dropin_attached_fills_the_reference_lists(ctx, flight, gui):
    """``collect()`` before TRAIL OFF and at the end: ``new*`` (QtGL) or ``lat0 .. / time / col / fcol`` (pygame)
    as the reference's lists recorded in the flight golden -- time, col and fcol exactly, coordinates by the 1e-9
    rule; TRAIL OFF empties them."""
    g = flight
    tr = trails.Trails(types.SimpleNamespace(lat=None, lon=None, id=[]), gui_type=gui)
    seen = []

    def snap(tag):
        seen.append(tag)
        tr.collect()
        pre = '%s_%s_' % (gui, tag)
        if gui == 'qtgl':
            for k in ('lat0', 'lon0', 'lat1', 'lon1'):
                ok, msg = util.close(np.array(getattr(tr, 'new' + k), dtype=np.float64), g[pre + 'new' + k], SCALES[k[:3]])
                assert ok, (tag, k, msg)
            assert len(tr.lat0) == 0 and len(g[pre + 'newlat0']) > 0
        else:
            for k in ('lat0', 'lon0', 'lat1', 'lon1'):
                ok, msg = util.close(getattr(tr, k), g[pre + k], SCALES[k[:3]])
                assert ok, (tag, k, msg)
            assert same(tr.time, g[pre + 'time']) and same(tr.fcol, g[pre + 'fcol']) and same(colours(tr.col), g[pre + 'col'])
            assert tr.newlat0 == [] and len(tr.time) > 0

    fly(ctx, g, tr=tr, snap=snap)
    assert seen == ['before_off', 'final'] and tr.active


# ---------------------------------------------------------------- batches
def staggered(ctx, n, seed, nsteps, p, dt):
    init = climbers(n, seed, 30.0)
    last = -np.random.default_rng(seed).uniform(0.0, dt, n)
    return init, last, positions(ctx, init, p, nsteps)


def test_one_batch_equals_single_steps(ctx):
    """200 steps as step(200) with one drain and as 200 x step(1) with a drain after every step (CD every 2nd
    step, dt 1 s, lasttim staggered so that some aircraft emit in most steps): the same stream and final arrays,
    and the restatement's on the twin's positions."""
    n, nsteps, dt = 600, 200, 1.0
    p = resident.params(cd_every=2)
    init, last, pos = staggered(ctx, n, 11, nsteps, p, dt)

    def run(chunks, every):
        sim = resident.ResidentSim(init, p, ctx=ctx)
        sim.set_trails(True, True, dt, simt=0.0, lasttim=last)
        parts = []
        for k in chunks:
            assert sim.step(k) == k
            if every:
                parts.append(sim.trails())
        parts.append(sim.trails())
        again = sim.trails()
        assert len(again['trailidx']) == 0 and again['swtrails']          # the drain reset the total
        return stream(parts), sim.read_trails(), sim.read()

    a, ra, sa = run([nsteps], False)
    b, rb, sb = run([1] * nsteps, True)
    for k in KEYS:
        assert same(a[k], b[k]), k
    for k in trails_np.ARRAYS + ('simt', 'last_t'):
        assert same(ra[k], rb[k]), k
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    segs, st = expected(pos, clock(p.simdt, nsteps), dict(lastlat=init['lat'], lastlon=init['lon'], lasttim=last), dt)
    assert_stream(a, trails_np.concat(segs))
    assert sum(1 for s in segs if len(s['idx'])) > 100 and len(a['trailidx']) > 9 * n
    for k in trails_np.ARRAYS:
        assert same(ra[k], st[k]), k


@pytest.mark.parametrize('case', ['stop_in_an_emitting_step', 'abort_then_rerun'])
def test_next_to_a_stop_and_next_to_an_abort(ctx, case):
    """1500 aircraft, CD every step, dt 0.12 s with lasttim -1: all emit in step 1 and then every third step.
    stop_in_an_emitting_step: a condition fires in the second emitting step of a step(12); the drain after the stop
    holds that step's segments once and nothing of the steps behind it; stepping on completes the stream.
    abort_then_rerun: K2 row buckets one pair wide overflow in the first CD step (an emitting one), which is
    re-run.  Both streams equal the restatement's on an undisturbed twin's positions: no segment twice, none
    missing."""
    n, nsteps, dt = 1500, 12, 0.12
    init = climbers(n, 53, 60.0)
    p = resident.params(cd_every=1)
    pos = positions(ctx, init, p, nsteps)
    alts = altitudes(ctx, init, p, nsteps)
    ts = clock(p.simdt, nsteps)
    last = np.full(n, -1.0)
    segs, st = expected(pos, ts, dict(lastlat=init['lat'], lastlon=init['lon'], lasttim=last), dt)
    emitting = [q + 1 for q, s in enumerate(segs) if len(s['idx'])]
    assert emitting[0] == 1 and len(emitting) >= 3 and all(len(segs[q - 1]['idx']) == n for q in emitting)
    c = _lib.Context(0)
    try:
        if case == 'abort_then_rerun':
            c.set_row_bucket(1)
        sim = resident.ResidentSim(init, p, ctx=c)
        sim.set_trails(True, True, dt, simt=0.0, lasttim=last)
        parts = []
        if case == 'stop_in_an_emitting_step':
            at = emitting[1]
            ac = [k for k in movers(alts) if alts[at, k] != alts[at - 1, k]][0]
            cond = conditional.Condition(traf_of(init, n), stack=lambda cmd: None)
            crossing(cond, alts, ac, at, 'C')
            sim.set_conditions(cond)
            assert sim.step(nsteps) == at                     # the batch stopped after the emitting step
            first = sim.trails()
            assert len(first['trailidx']) == n * 2 and (first['trailtime'][n:] == ts[at - 1]).all()
            assert np.array_equal(first['trailidx'][n:], np.arange(n))
            assert len(sim.conditions()[0]) == 1
            parts.append(first)
            assert sim.step(nsteps - at) == nsteps - at
        else:
            assert sim.step(nsteps) == nsteps
        parts.append(sim.trails())
        assert_stream(stream(parts), trails_np.concat(segs))
        r = sim.read_trails()
        for k in trails_np.ARRAYS:
            assert same(r[k], st[k]), k
        assert sim.stats()['steps'] == nsteps and sim.stats()['n_conf'] > 0 and r['simt'] == ts[-1] + p.simdt
    finally:
        c.close()


# ---------------------------------------------------------------- delete / create, off by default
def test_delete_and_create_carry_the_arrays(ctx):
    n, dt = 600, 0.12
    init = climbers(n, 7, 30.0)
    p = resident.params(cd_every=2)
    sim = resident.ResidentSim(init, p, ctx=ctx)
    sim.set_trails(True, True, dt, simt=5.0)
    assert sim.step(4) == 4
    before = sim.read_trails()
    assert before['undrained'] == n and (before['lasttim'] == clock(p.simdt, 3, 5.0)[2]).all()    # 5.1 - 4.95 > 0.12: step 3
    gone = [0, 17, 300, 599]
    sim.delete(gone)
    st = trails_np.delete(before, gone)
    got = sim.read_trails()
    for k in trails_np.ARRAYS:
        assert same(got[k], st[k]), k
    new = {k: v[:3].copy() for k, v in init.items()}
    new['lat'], new['lon'] = np.array([10.0, 11.0, 12.0]), np.array([20.0, 21.0, 22.0])
    sim.create(new)
    r = sim.read()
    st = trails_np.create(st, r['lat'], r['lon'], 3)
    got = sim.read_trails()
    for k in trails_np.ARRAYS:
        assert same(got[k], st[k]), k
    assert list(got['lastlat'][-3:]) == [0.0, 0.0, 12.0] and list(got['lastlon'][-3:]) == [0.0, 0.0, 22.0]
    assert not got['lasttim'][-3:].any()
    first = sim.trails()                                     # the segments of step 3, the indices of their time
    assert len(first['trailidx']) == n and len(sim.trails()['trailidx']) == 0
    t = sim.read_trails()['simt']
    assert sim.step(1) == 1
    r = sim.read()
    st, seg = trails_np.update(st, r['lat'], r['lon'], t, dt, True)
    got = sim.trails()
    assert_stream(got, seg)
    assert list(got['trailidx'][-3:]) == [596, 597, 598] and list(got['traillat0'][-3:]) == [0.0, 0.0, 12.0]
    sim.set_trails(False)
    with pytest.raises(_lib.AccelError, match='off'):
        sim.read_trails()


def test_off_by_default(ctx):
    """Without set_trails: trails() raises, and 20 steps give what a sim that had trails on gives -- the stage
    writes nothing the step reads -- bitwise."""
    init = climbers(600, 7, 30.0)
    p = resident.params(cd_every=2)
    a = resident.ResidentSim(init, p, ctx=ctx)
    with pytest.raises(_lib.AccelError, match='off'):
        a.trails()
    with pytest.raises(_lib.AccelError, match='off'):
        a.read_trails()
    assert a.step(20) == 20
    ra = a.read()
    b = resident.ResidentSim(init, p, ctx=ctx)
    b.set_trails(True, True, 0.2)
    assert b.step(20) == 20 and len(b.trails()['trailidx']) > 0
    rb = b.read()
    c = resident.ResidentSim(init, p, ctx=ctx)               # a new sim on the same context starts with the stage off
    with pytest.raises(_lib.AccelError, match='off'):
        c.trails()
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), k


# ---------------------------------------------------------------- refusals
def test_refusals(ctx):
    n = 600
    init = climbers(n, 7, 30.0)
    p = resident.params()
    sim = resident.ResidentSim(init, p, ctx=ctx)
    for dt in (0.0, -1.0, float('nan')):
        with pytest.raises(_lib.AccelError, match='dt must be > 0'):
            sim.set_trails(True, True, dt)
    with pytest.raises(_lib.AccelError, match='max_segments %d holds less than one pass of %d' % (n - 1, n)):
        sim.set_trails(True, True, 1.0, max_segments=n - 1)
    with pytest.raises(_lib.AccelError, match='off'):
        sim.trails()
    # room for one pass: a batch that may emit more is refused before anything is enqueued
    sim.set_trails(True, True, p.simdt / 2, simt=0.0, max_segments=n)
    assert trails_np.bound(n, 5, p.simdt, p.simdt / 2) == 5 * n
    with pytest.raises(_lib.AccelError, match='drain.*or step less'):
        sim.step(5)
    assert sim.stats()['steps'] == 0 and sim.read_trails()['simt'] == 0.0
    assert sim.step(1) == 1 and sim.read_trails()['undrained'] == n
    with pytest.raises(_lib.AccelError, match='%d undrained' % n):
        sim.step(1)                                          # undrained + one more pass
    assert sim.stats()['steps'] == 1 and len(sim.trails()['trailidx']) == n
    assert sim.step(1) == 1 and sim.stats()['steps'] == 2


def test_refused_on_several_ranks():
    if _lib.load().bsa_device_count() < 2:
        pytest.skip('needs two devices')
    init = climbers(600, 7, 30.0)

    def rank(r, c, group):
        s = resident.ResidentSim(init, resident.params(), ctx=c, rank=r, world=2, group=group)
        with pytest.raises(_lib.AccelError, match='ranks.*not built'):
            s.set_trails()
        return True

    assert run_ranks(2, rank) == [True, True]
