"""GPU: conditional commands (ATALT / ATSPD) -- bsa_cond_update against the reference's
golden, and the resident step's stage with the batch stop it raises: a stopped batch leaves
exactly the state after the step that fired, compared bitwise with twin sims stepped one
step at a time; stops next to aborts; kept detect state after a stop; delete; refusals."""
import os

import numpy as np
import pytest

from bluesky_amd import _lib, conditional, fms, resident, synth
from tests import cond_np, util
from tests.test_gpu_multirank import run_ranks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def upd():
    return dict(np.load(os.path.join(util.GOLDEN, 'cond_update.npz')))


# ---------------------------------------------------------------- standalone
@pytest.mark.parametrize('name', ['n1', 'n63', 'n64', 'n65', 'n257', 'nothing', 'everything'])
def test_standalone_update_matches_golden(ctx, upd, name):
    """The fired list equal and ascending; lastdif bitwise for altitude-type conditions (one
    exact subtraction), within the 1e-9 rule for speed-type ones.  A NaN is compared as a NaN:
    IEEE 754 leaves the sign of a propagated NaN open, and the device's subtraction (an add
    of the negated operand) returns the other one than the host's."""
    g = {k: upd[name + '_' + k] for k in ('idx', 'condtype', 'target', 'lastdif', 'fired', 'newdif')}
    fired, newdif = ctx.cond_update(g['idx'], g['condtype'], g['target'], g['lastdif'], upd['alt'], upd['cas'])
    assert np.array_equal(fired, g['fired']) and np.all(np.diff(fired) > 0)
    alt = g['condtype'] == cond_np.ALT
    num = alt & ~np.isnan(g['newdif'])
    assert newdif[num].tobytes() == g['newdif'][num].tobytes()
    assert np.isnan(newdif[alt & ~num]).all()
    ok, msg = util.close(newdif[~alt], g['newdif'][~alt], 100.0)
    assert ok, msg


def test_standalone_empty_and_refusals(ctx, upd):
    fired, newdif = ctx.cond_update([], [], [], [], upd['alt'], upd['cas'])
    assert len(fired) == 0 and len(newdif) == 0
    with pytest.raises(_lib.AccelError, match='outside'):
        ctx.cond_update([0, 300], [0, 0], [1., 1.], [1., 1.], upd['alt'], upd['cas'])
    with pytest.raises(_lib.AccelError, match='outside'):
        ctx.cond_update([-1], [0], [1.], [1.], upd['alt'], upd['cas'])
    with pytest.raises(_lib.AccelError, match='neither'):
        ctx.cond_update([0], [2], [1.], [1.], upd['alt'], upd['cas'])


# ---------------------------------------------------------------- the flight golden
def test_resident_follows_the_flight_golden(ctx):
    """cond_flight64 (the reference's closed loop with its Condition class and stacked ALT / SPD /
    VS / DEL commands) with conditional.run in batches of 40 and the capture's interpreter
    (cond_np.execute) as ``execute``: every stop at the recorded step with the recorded indices
    and commands -- so every step() count is the recorded one --, the table after every stop
    (idx, type, target exact; lastdif within the 1e-9 rule at the altitude / speed scale), the
    state at every sample within the 1e-9 rule, iactwp / swlnav / swvnav exact."""
    from tests import fms_np
    from tests.fms_cases import FMS_KEYS, compare
    from tests.test_gpu_sim import SCALES
    g = dict(np.load(os.path.join(util.GOLDEN, 'cond_flight64.npz')))
    init = {k[5:]: np.array(v) for k, v in g.items() if k.startswith('init_')}
    n, every = len(init['lat']), int(g['every'])
    p = resident.params(simdt=float(g['simdt']), cd_every=20, rpz=1.0, hpz=1.0, tla=1.0)   # ASAS inactive, as captured
    sim = resident.ResidentSim({k: init[k] for k in _lib.SIM_STATE_FIELDS}, p, ctx=ctx)
    tab = [g['route_rows'], g['rt_off'], g['rt_n']]
    sim.set_fms(*tab, {k: init[k] for k in FMS_KEYS})
    cond = conditional.Condition(traf_of(init, n), stack=lambda cmd: None)
    cond.idx, cond.condtype = np.array(g['cond_idx'], dtype=int), np.array(g['cond_condtype'])
    cond.target, cond.lastdif = np.array(g['cond_target']), np.array(g['cond_lastdif'])
    cond.cmd, cond.ncond = [str(x) for x in g['cond_cmd']], len(g['cond_idx'])
    cond.id = np.array([cond.traf.id[k] for k in cond.idx])
    first = {int(o): q for q, o in enumerate(g['ev_off'][:-1])}      # command number -> the stop it opens
    seen = []

    def execute(cmd):
        if len(seen) in first:                                       # the table as the stop left it
            q = first[len(seen)]
            dev = sim.read_conditions()
            assert np.array_equal(dev['idx'], g['t%02d_idx' % q]) and np.array_equal(dev['condtype'], g['t%02d_condtype' % q])
            assert np.array_equal(dev['target'], g['t%02d_target' % q]), q
            assert np.array_equal(np.asarray(cond.idx), dev['idx']) and np.array_equal(cond.lastdif, dev['lastdif'])
            alt = dev['condtype'] == 0
            for m, scale in ((alt, 1e4), (~alt, 100.0)):
                ok, msg = util.close(dev['lastdif'][m], g['t%02d_lastdif' % q][m], scale)
                assert ok, 'table after stop %d: %s' % (q, msg)
        seen.append(cmd)
        st, tr = sim.read_fms(), sim.read()
        gone = cond_np.execute(st, tr['alt'], cmd)
        if gone is None:
            sim.set_fms(*tab, {k: st[k] for k in FMS_KEYS}, simt=st['simt'], t0=st['t0'])
            sim.update(selalt=st['selalt'])
        else:
            sim.delete([gone])
            tab[:] = cond_np.drop_route(tab[0], tab[1], tab[2], gone)

    events = []
    for q in range(int(g['nsteps']) // every):
        events += conditional.run(sim, every, cond, execute)
        assert sim.stats()['steps'] == (q + 1) * every
        got, tr = sim.read_fms(), sim.read()
        exp = {k: g['s%02d_%s' % (q + 1, k)] for k in fms_np.OUTPUTS + ('lat', 'lon', 'alt', 'tas', 'hdg', 'vs')}
        compare(got, {'out_' + k: exp[k] for k in fms_np.OUTPUTS}, what='sample %d ' % (q + 1))
        for k in ('lat', 'lon', 'alt', 'tas', 'hdg', 'vs'):
            ok, msg = util.close(tr[k], exp[k], SCALES[k])
            assert ok, 'sample %d %s: %s' % (q + 1, k, msg)
    assert [e[0] for e in events] == [int(x) for x in g['ev_step']]
    off = g['ev_off']
    for q, (step, fired, cmds) in enumerate(events):
        assert [int(x) for x in fired] == [int(x) for x in g['ev_idx'][off[q]:off[q + 1]]], q
        assert cmds == [str(x) for x in g['ev_cmd'][off[q]:off[q + 1]]], q
    assert seen == [str(x) for x in g['ev_cmd']] and len(tr['lat']) == n - 1
    assert any(len(e[1]) >= 2 for e in events) and len(events) > 20


# ---------------------------------------------------------------- the resident stage
def climbers(n, seed, spread, nclimb=40):
    """A box whose first ``nclimb`` aircraft climb or descend 600 m from the start (ap_alt /
    selalt off their altitude), so altitude conditions cross at known steps."""
    init = resident.initial_state(synth.box(n, spread, seed=seed))
    d = np.where(np.arange(nclimb) % 2 == 0, 600.0, -600.0)
    for k in ('ap_alt', 'selalt', 'asas_alt'):        # (asas.alt: what the pilot follows while in conflict)
        init[k][:nclimb] += d
    return init


def movers(alts, nclimb=40):
    """The climbers whose altitude changes in every recorded step, ascending."""
    m = np.flatnonzero((np.diff(alts[:, :nclimb], axis=0) != 0).all(axis=0))
    assert len(m) >= 7, len(m)
    return [int(k) for k in m]


def dress(sim, fmsrt=None, gv=None):
    """Guidance and, with ``gv`` = (areas, geovectors, every), geovectoring on ``sim``."""
    if fmsrt is not None:
        sim.set_fms(*fmsrt)
    if gv is not None:
        sim.set_areas(gv[0])
        sim.set_geovectors(gv[1], gv[2])
    return sim


def altitudes(ctx, init, p, nsteps, fmsrt=None, gv=None, tas=None):
    """alt after 0 .. nsteps steps of the undisturbed sim (``tas``: a list that receives tas alike)."""
    sim = dress(resident.ResidentSim(init, p, ctx=ctx), fmsrt, gv)
    r = sim.read()
    out = [r['alt']]
    for k in range(nsteps + 1):
        if tas is not None:
            tas.append(r['tas'])
        if k < nsteps:
            sim.step(1)
            r = sim.read()
            out.append(r['alt'])
    return np.array(out)


def crossing(cond, alts, ac, step, cmd):
    """An altitude condition on ``ac`` that fires at the step after which ``step`` steps have
    run: the target lies between the altitudes before and after that step."""
    assert alts[step, ac] != alts[step - 1, ac]
    cond.traf.alt = alts[0]
    cond.ataltcmd(ac, 0.5 * (alts[step - 1, ac] + alts[step, ac]), cmd)


class Host:
    """The capture-style interpreter: ALT / DEL / CHAIN commands on one sim."""

    def __init__(self, sim, cond, init):
        self.sim, self.cond, self.log = sim, cond, []
        self.selalt, self.ap_alt = init['selalt'].copy(), init['ap_alt'].copy()

    def __call__(self, cmd):
        self.log.append(cmd)
        w = cmd.split()
        if w[0] == 'ALT':
            k = int(w[1])
            self.selalt[k] = self.ap_alt[k] = float(w[2])
            self.sim.update(selalt=self.selalt, ap_alt=self.ap_alt)
        elif w[0] == 'DEL':
            k = int(w[1])
            self.sim.delete([k])
            self.selalt, self.ap_alt = np.delete(self.selalt, k), np.delete(self.ap_alt, k)
        elif w[0] == 'CHAIN' and int(w[1]) > 0:      # a condition that fires at the very next step (lastdif == 0)
            self.cond.addcondition(3, conditional.alttype, 1e5, 1e5, 'CHAIN %d' % (int(w[1]) - 1))


def traf_of(init, n):
    return type('T', (), dict(id=['AC%04d' % k for k in range(n)], alt=init['alt'].copy(), tas=init['tas'].copy(),
                              cas=init['tas'].copy(), ntraf=n))()


def table_of(init, alts, n, chain=0, spd=None):
    """~100 conditions of both types on a box of n: crossings of the first climbers at steps
    2, 2, 7, 30 and 31, a chain, and never-firing ones (their lastdif still moves)."""
    rng = np.random.default_rng(5)
    c = conditional.Condition(traf_of(init, n), stack=lambda cmd: None)
    m = movers(alts)
    last = len(alts) - 1
    alt0 = [float(x) for x in init['alt']]
    crossing(c, alts, m[0], 2, 'ALT %d %r' % (m[0], alt0[m[0]] - 50.0))
    crossing(c, alts, m[1], 2, 'ALT %d %r' % (m[1], alt0[m[1]] + 80.0))
    crossing(c, alts, m[2], 7, 'DEL %d' % m[2])
    crossing(c, alts, m[4], min(30, last - 1), 'ALT %d %r' % (m[4], alt0[m[4]] + 5.0))
    crossing(c, alts, m[5], min(31, last), 'ALT %d %r' % (m[6], alt0[m[6]] + 300.0))
    if chain:
        c.addcondition(3, conditional.alttype, 1e5, 1e5, 'CHAIN %d' % chain)
    if spd is not None:                               # (aircraft, target, CAS at the start): a speed crossing
        c.addcondition(spd[0], conditional.spdtype, spd[1], spd[2], 'SPDX')
    c.traf.alt = alts[0]
    for k in rng.integers(40, n, 90):                 # cruising aircraft: far targets, both types
        if k % 2:
            c.ataltcmd(int(k), float(init['alt'][k] + 5000.0), 'NEVER')
        else:
            c.atspdcmd(int(k), float(init['tas'][k] * 0.3), 'NEVER')
    return c


def run_batches(ctx, init, p, alts, batches, fmsrt=None, chain=0, bucket=None, bucket_after=None, gv=None, spd=None):
    n = len(init['lat'])
    if bucket is not None:
        ctx.set_row_bucket(bucket)
    sim = dress(resident.ResidentSim(init, p, ctx=ctx), fmsrt, gv)
    cond = table_of(init, alts, n, chain, spd)
    host = Host(sim, cond, init)
    events = []
    for q, b in enumerate(batches):
        if bucket_after is not None and q == bucket_after[0]:
            ctx.set_row_bucket(bucket_after[1])
        events += conditional.run(sim, b, cond, host)
    out = dict(read=sim.read(), table=sim.read_conditions(), events=[(s, list(f), c) for s, f, c in events],
               stats=sim.stats(), fms=sim.read_fms() if fmsrt is not None else None, cond=cond,
               gv=sim.geovector_stats() if gv is not None else None)
    return out


def assert_same(a, b):
    for k in a['read']:
        assert np.array_equal(a['read'][k], b['read'][k], equal_nan=True), k
    for k in a['table']:
        assert a['table'][k].tobytes() == b['table'][k].tobytes(), k
    assert a['events'] == b['events'] and a['gv'] == b['gv']
    assert a['stats']['steps'] == b['stats']['steps']
    if a['fms'] is not None:
        for k in a['fms']:
            assert np.array_equal(np.asarray(a['fms'][k]), np.asarray(b['fms'][k]), equal_nan=True), k
    for k in ('idx', 'condtype', 'target', 'lastdif'):
        assert np.array_equal(np.asarray(getattr(a['cond'], k), dtype=np.float64), np.asarray(a['table'][k], dtype=np.float64)), k


def speed_crossing(alts, tas, step, lo=40):
    """(aircraft, target, CAS at the start) of a cruising aircraft whose CAS -- vtas2cas(tas after
    step k, alt before it), traffic.py:434 -- moves one way up to ``step`` and by more than 1e-6
    of itself in that step: the target between the CAS after steps ``step - 1`` and ``step``
    is crossed in step ``step`` and in no earlier one, whatever a device pow's last bit."""
    from oracle.kinematics import vtas2cas
    tas = np.array(tas)
    cas = np.array([vtas2cas(tas[0], alts[0])] + [vtas2cas(tas[k], alts[k - 1]) for k in range(1, step + 1)])
    d = np.diff(cas, axis=0)
    ok = ((d > 0).all(axis=0) | (d < 0).all(axis=0)) & (np.abs(d[-1]) > 1e-6 * cas[-1])
    ok[:lo] = False
    assert ok.any(), 'no aircraft changes its CAS steadily over the first %d steps' % step
    k = int(np.flatnonzero(ok)[0])
    return k, float(0.5 * (cas[step - 1, k] + cas[step, k])), float(cas[0, k])


def test_one_batch_equals_single_steps(ctx):
    """step(45) against 45 x step(1), bitwise: 1500 aircraft, CD and MVP every step, FMS on,
    geovectors on every 3rd step, ~100 conditions, the same interpreter.  From simt 0 the FMS
    ticks in steps 0-20 and 41 and the geovectors apply in the steps after 3, 6, 9 ... completed
    ones, so the stop after step 3 sits on the step before a ticking AND applying step, where
    neither undo set may be put back; two conditions fire in one step; one DEL removes an
    aircraft; a speed condition fires in the step the numpy CAS says."""
    init = climbers(1500, 59, 60.0)
    rt = fms.synthetic_routes(init, seed=59)
    box = [float(init['lat'].min()) - 1., float(init['lon'].min()) - 1., float(init['lat'].max()) + 1.,
           float(init['lon'].max()) + 1.]
    gv = ({'ALL': ('BOX', box, 1e9, -1e9)}, [['ALL', None, float(np.median(init['tas'])), None, None, None, None]], 3)
    p = resident.params(cd_every=1)
    assert fms.tick_schedule(0.0, p.simdt, 45)[0][:21].all()
    tas = []
    alts = altitudes(ctx, init, p, 45, rt, gv, tas)
    spd = speed_crossing(alts, tas, 2)
    a = run_batches(ctx, init, p, alts, [45], rt, chain=3, gv=gv, spd=spd)
    b = run_batches(ctx, init, p, alts, [1] * 45, rt, chain=3, gv=gv, spd=spd)
    assert_same(a, b)
    steps = [s for s, _, _ in a['events']]
    assert len(steps) >= 5 and steps == sorted(steps) and steps[0] == 1
    assert 3 in steps and 3 % gv[2] == 0 and 3 < 20                   # a stop before a ticking and applying step
    assert a['gv']['applies'] == 14 and a['gv']['changed']['selspd'] > 0
    assert any(len(f) >= 2 for _, f, _ in a['events'])
    assert [s for s, _, c in a['events'] if 'SPDX' in c] == [2]        # nothing but the chain ran before step 2
    assert a['stats']['steps'] == 45 and a['stats']['n_conf'] > 0
    assert any(c[0].startswith('DEL') for _, _, c in a['events']) and len(a['read']['lat']) == 1499
    assert a['fms']['ticks'] == 22


def test_stage_follows_the_numpy_restatement(ctx):
    """The stage against tests/cond_np.py, one step at a time with FMS (speeds change) and
    turbulence on: CAS is oracle.kinematics.vtas2cas of the read-back tas and the altitude read
    back BEFORE the step, altitude conditions see the altitude after Woosh, rows are aircraft
    indices whatever the home order.  Fired sets equal (no product within the 1e-9 margin of 0,
    asserted), lastdif bitwise for altitude conditions, within the 1e-9 rule for speed ones."""
    from oracle.kinematics import vtas2cas
    n = 600
    init = climbers(n, 11, 60.0, nclimb=200)
    p = resident.params(cd_every=2)
    sim = dress(resident.ResidentSim(init, p, ctx=ctx), fms.synthetic_routes(init, seed=11))
    sim.set_turbulence(True, (0.5, 0.5, 0.5), seed=3)
    rng = np.random.default_rng(2)
    idx = rng.integers(0, n, 256)
    typ = rng.integers(0, 2, 256)
    cas0 = vtas2cas(init['tas'], init['alt'])
    near = np.where(typ == 0, init['alt'][idx] + rng.uniform(-0.6, 0.6, 256), cas0[idx] + rng.uniform(-0.3, 0.3, 256))
    t = cond_np.table(idx, typ, near, near - np.where(typ == 0, init['alt'][idx], cas0[idx]))
    sim.set_conditions(idx=t['idx'], condtype=t['condtype'], target=t['target'], lastdif=t['lastdif'])
    prev, nfired, kinds = sim.read(), 0, set()
    for step in range(1, 13):
        ran = sim.step(1)
        cur = sim.read()
        assert ran == 1
        cas = vtas2cas(cur['tas'], prev['alt'])
        actual = np.where(t['condtype'] == 0, cur['alt'][t['idx']], cas[t['idx']])
        spd = (t['condtype'] == 1) & (t['lastdif'] != 0)
        assert (cond_np.product_margin(t['target'], t['lastdif'], actual)[spd] > cond_np.MARGIN).all(), step
        fired, newdif = cond_np.update(t['idx'], t['condtype'], t['target'], t['lastdif'], cur['alt'], cas)
        got, at = sim.conditions()
        assert np.array_equal(got, fired) and (at == step or len(fired) == 0), step
        t['lastdif'] = newdif
        nfired += len(fired)
        kinds |= set(int(x) for x in t['condtype'][fired])
        t = cond_np.delcondition(t, fired)
        dev = sim.read_conditions()
        assert np.array_equal(dev['idx'], t['idx']) and np.array_equal(dev['condtype'], t['condtype'])
        alt = t['condtype'] == 0
        assert dev['lastdif'][alt].tobytes() == t['lastdif'][alt].tobytes(), step
        ok, msg = util.close(dev['lastdif'][~alt], t['lastdif'][~alt], 100.0)
        assert ok, 'step %d: %s' % (step, msg)
        prev = cur
    assert nfired > 20 and kinds == {0, 1} and len(t['idx']) > 20


def test_step_returns_the_count_and_poll_is_empty_without_a_stop(ctx):
    init = climbers(600, 7, 30.0)
    p = resident.params(cd_every=2)
    alts = altitudes(ctx, init, p, 8)
    sim = resident.ResidentSim(init, p, ctx=ctx)
    assert sim.step(3) == 3 and sim.ctx.sim_steps_run() == (3, 3)
    sim = resident.ResidentSim(init, p, ctx=ctx)
    c = conditional.Condition(traf_of(init, 600), stack=lambda cmd: None)
    m = movers(alts)
    crossing(c, alts, m[0], 3, 'A')
    crossing(c, alts, m[1], 3, 'B')
    crossing(c, alts, m[6], 5, 'C')
    sim.set_conditions(c)
    assert sim.step(8) == 3 and sim.stats()['steps'] == 3
    assert np.array_equal(sim.read()['alt'], alts[3])
    fired, step = sim.conditions()
    assert list(fired) == [0, 1] and step == 3
    assert list(sim.conditions()[0]) == []
    t = sim.read_conditions()
    assert list(t['idx']) == [m[6]] and t['lastdif'][0] == c.target[2] - alts[3][m[6]]
    assert sim.step(5) == 2 and list(sim.conditions()[0]) == [0]
    assert sim.step(3) == 3 and np.array_equal(sim.read()['alt'], alts[8])
    sim.set_conditions(None)
    assert len(sim.read_conditions()['idx']) == 0


@pytest.mark.parametrize('case', ['abort_then_fire', 'fire_then_overflow', 'same_step'])
def test_stops_and_aborts_together(ctx, case):
    """K2 row buckets one pair wide overflow at the first CD step they meet.  abort_then_fire:
    step 0 aborts and re-runs, conditions fire at steps 2 and 7.  fire_then_overflow: CD every
    4th step from step 1 on, the conditions of step 2 stop the batch before the overflow of
    step 4 -- whose detect, enqueued behind the stop, overflows on the device all the same;
    the overflow is met only when the host resumes.  same_step: a condition with lastdif 0
    fires in the re-run of the aborting step 0, once.  Each against an undisturbed twin
    stepped one step at a time."""
    init = climbers(1500, 53, 60.0)
    p = resident.params(cd_every=4 if case == 'fire_then_overflow' else 1)
    alts = altitudes(ctx, init, p, 12)
    chain = 1 if case == 'same_step' else 0
    twin = run_batches(ctx, init, p, alts, [1] * 12, chain=chain)
    c = _lib.Context(0)
    try:
        if case == 'fire_then_overflow':
            got = run_batches(c, init, p, alts, [1, 11], chain=chain, bucket_after=(1, 1))
        else:
            got = run_batches(c, init, p, alts, [12], chain=chain, bucket=1)
        assert_same(got, twin)
    finally:
        c.close()
    steps = [s for s, _, _ in twin['events']]
    assert steps[:3] == ([1, 2, 7] if case == 'same_step' else [2, 7, 11]) and twin['stats']['n_conf'] > 0


def test_kept_state_after_a_stop(ctx):
    """The detect after a stop gives the same pairs as a fresh sim initialised from the
    read-back state (Change::BatchStopped dropped every list the no-op steps' detects re-armed)."""
    init = climbers(1500, 53, 60.0)
    p = resident.params(cd_every=1)
    alts = altitudes(ctx, init, p, 6)
    sim = resident.ResidentSim(init, p, ctx=ctx)
    c = conditional.Condition(traf_of(init, 1500), stack=lambda cmd: None)
    crossing(c, alts, movers(alts)[0], 4, 'X')
    sim.set_conditions(c)
    assert sim.step(20) == 4 and list(sim.conditions()[0]) == [0]
    st = sim.read()
    sim.step(1)
    s = sim.stats()
    pairs = ctx.fetch_pairs(s['n_conf'], s['n_los'])
    c2 = _lib.Context(0)
    try:
        state = dict(init, **{k: st[k] for k in ('lat', 'lon', 'alt', 'tas', 'hdg', 'vs', 'gs', 'trk', 'gseast', 'gsnorth')})
        fresh = resident.ResidentSim(state, p, ctx=c2)
        fresh.step(1)
        s2 = fresh.stats()
        assert (s2['n_conf'], s2['n_los']) == (s['n_conf'], s['n_los']) and s['n_conf'] > 0
        p2 = c2.fetch_pairs(s2['n_conf'], s2['n_los'])
        for k in ('ci', 'cj', 'li', 'lj'):
            assert np.array_equal(pairs[k], p2[k]), k
    finally:
        c2.close()


def test_delete_applies_delac(ctx):
    init = climbers(600, 7, 30.0)
    p = resident.params(cd_every=2)
    sim = resident.ResidentSim(init, p, ctx=ctx)
    rng = np.random.default_rng(3)
    idx = np.concatenate([[0, 599, 10, 10, 11, 12], rng.integers(0, 600, 60)])
    typ = rng.integers(0, 2, len(idx))
    target = np.where(typ == 0, init['alt'][idx] + 9000.0, 10.0)
    lastdif = np.where(typ == 0, 9000.0, -200.0)
    sim.set_conditions(idx=idx, condtype=typ, target=target, lastdif=lastdif)
    sim.step(2)
    t = sim.read_conditions()
    assert len(t['idx']) == len(idx)
    sim.delete([10, 11, 300])
    exp = cond_np.delac(cond_np.table(t['idx'], t['condtype'], t['target'], t['lastdif']), np.array([10, 11, 300]))
    keep = exp['idx'] < 597
    got = sim.read_conditions()
    for k in ('idx', 'condtype', 'target', 'lastdif'):
        assert np.array_equal(np.asarray(got[k], dtype=np.float64), np.asarray(exp[k][keep], dtype=np.float64)), k
    assert len(got['idx']) < len(idx)
    assert sim.step(2) == 2


def test_delete_keeps_the_attached_condition_in_step(ctx):
    """A multiple delete whose list ends with the last aircraft: the reference's sequential delac
    leaves that aircraft's condition pointing one past the new n.  The device table drops it and
    ``ResidentSim.delete`` drops it from the attached Condition too, so ``conditional.run`` can
    upload the table again."""
    init = climbers(600, 7, 30.0)
    sim = resident.ResidentSim(init, resident.params(cd_every=2), ctx=ctx)
    c = conditional.Condition(traf_of(init, 600), stack=lambda cmd: None)
    for ac in (599, 10, 300, 599, 11):
        c.ataltcmd(ac, float(init['alt'][ac]) + 9000.0, 'X%d' % ac)
    sim.set_conditions(c)
    ref = cond_np.delac(cond_np.table(c.idx, c.condtype, c.target, c.lastdif), np.array([10, 599]))
    assert (ref['idx'] >= 598).sum() == 2                      # the reference keeps both, out of range
    sim.delete([599, 10])
    got = sim.read_conditions()
    assert list(got['idx']) == [299, 10] and list(c.idx) == [299, 10] and c.cmd == ['X300', 'X11']
    sim.set_conditions(c)
    assert sim.step(2) == 2


def test_refusals(ctx):
    init = climbers(600, 7, 30.0)
    sim = resident.ResidentSim(init, resident.params(), ctx=ctx)
    with pytest.raises(_lib.AccelError, match='outside'):
        sim.set_conditions(idx=[600], condtype=[0], target=[1.], lastdif=[1.])
    with pytest.raises(_lib.AccelError, match='neither'):
        sim.set_conditions(idx=[0], condtype=[3], target=[1.], lastdif=[1.])
    assert sim.step(2) == 2

    def rank(r, c, group):
        s = resident.ResidentSim(init, resident.params(), ctx=c, rank=r, world=2, group=group)
        with pytest.raises(_lib.AccelError, match='ranks.*not built'):
            s.set_conditions(idx=[0], condtype=[0], target=[1.], lastdif=[1.])
        return True

    assert run_ranks(2, rank) == [True, True]
