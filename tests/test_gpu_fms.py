"""GPU: Autopilot.update on the device (bsa_fms_update, bluesky_amd.fms.update)
against tests/golden/fms_update2000.npz, one forced FMS tick of the reference's
own Autopilot / ActiveWaypoint / Route objects.  Reals within util.close's 1e-9
rule with the field's largest finite magnitude as scale, NaN positions equal;
flags and iactwp exactly.  Rows within 1e-9 of a threshold (fms_np.near_threshold)
would be skipped, at most 0.1 % of the rows; the golden has none."""
import numpy as np
import pytest

from bluesky_amd import _lib, fms, resident, synth
from tests import fms_np
from tests.test_gpu_multirank import run_ranks
from oracle import step as ostep
from tests import util
from tests.fms_cases import FLIGHT_TRAFFIC, INPUTS, compare, flight_state, load, load_flight
from tests.test_gpu_sim import SCALES, full_state, oracle_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    g, st = load()
    return dict(g=g, st=st, skip=g['near_threshold'].astype(bool))


def prefix(golden, n):
    g = golden['g']
    return g['route_rows'], g['rt_off'][:n], g['rt_n'][:n], {k: v[:n] for k, v in golden['st'].items()}


@pytest.mark.parametrize('n', [2000, 1, 63, 64, 65, 257])
def test_standalone_update_matches_golden(ctx, golden, n):
    rows, off, cnt, st = prefix(golden, n)
    keep = {k: np.array(v) for k, v in st.items()}
    got = fms.update(rows, off, cnt, st, ctx=ctx)
    skip = golden['skip'][:n]
    assert skip.sum() <= 0.001 * n
    compare(got, golden['g'], n=n, skip=skip)
    for k in INPUTS:                                   # the caller's arrays stay as they were
        assert np.array_equal(st[k], keep[k], equal_nan=True), k
    for k in ('selvs', 'apvsdef', 'abco', 'belco'):    # read only
        assert np.array_equal(got[k], st[k]), k
    if n == 2000:
        re_ = golden['g']['reached']
        assert (got['iactwp'][re_] >= st['iactwp'][re_]).all()
        assert np.array_equal(got['iactwp'][~re_], st['iactwp'][~re_])


def test_second_tick_follows_the_helper(ctx, golden):
    """The state after the golden's tick, ticked again: the device against the
    helper on the device's own first result (waypoints just switched to, routes
    just ended)."""
    rows, off, cnt, st = prefix(golden, 2000)
    first = fms.update(rows, off, cnt, st, ctx=ctx)
    st2 = dict(st, **first)
    skip = fms_np.near_threshold(st2, rows, off, cnt)
    assert skip.sum() <= 0.001 * 2000
    exp = fms_np.update(st2, rows, off, cnt)
    got = fms.update(rows, off, cnt, st2, ctx=ctx)
    compare(got, {'out_' + k: exp[k] for k in fms_np.OUTPUTS}, skip=skip)


def test_refusals_launch_nothing(ctx, golden):
    rows, off, cnt, st = prefix(golden, 64)
    with pytest.raises(RuntimeError):                                   # rows past the table
        fms.update(rows[:int(off[63])], off, np.maximum(cnt, 1), st, ctx=ctx)
    with pytest.raises(RuntimeError):
        fms.update(rows, -off - 1, cnt, st, ctx=ctx)                    # a negative offset
    with pytest.raises(RuntimeError):
        fms.update(rows, off, -cnt, dict(st, swlnav=np.zeros(64, bool)), ctx=ctx)
    k = int(np.flatnonzero(cnt > 0)[0])
    bad = np.array(st['iactwp'])
    bad[k] = cnt[k]
    with pytest.raises(RuntimeError):
        fms.update(rows, off, cnt, dict(st, iactwp=bad), ctx=ctx)       # active waypoint past its route
    bad[k] = -1
    with pytest.raises(RuntimeError):
        fms.update(rows, off, cnt, dict(st, iactwp=bad), ctx=ctx)
    with pytest.raises(RuntimeError):                                   # LNAV on an empty route
        fms.update(rows, off, np.zeros(64, np.int32), dict(st, swlnav=np.ones(64, bool)), ctx=ctx)
    with pytest.raises(ValueError):
        fms.update(rows, off, cnt, dict(st, alt=st['alt'][:63]), ctx=ctx)   # a short array
    with pytest.raises(ValueError):
        fms.update(rows, off, cnt[:63], st, ctx=ctx)
    with pytest.raises(ValueError):
        fms.update(rows[:, :7], off, cnt, st, ctx=ctx)                  # not nrows x 8
    # ... and the context still works
    got = fms.update(rows, off, cnt, st, ctx=ctx)
    compare(got, golden['g'], n=64)


def test_empty_call(ctx, golden):
    rows, off, cnt, st = prefix(golden, 0)
    got = fms.update(rows, off, cnt, st, ctx=ctx)
    assert all(len(v) == 0 for v in got.values())


# ---------------------------------------------------------------- the resident step
def fms_traffic(n, seed, spread=60.0):
    init = resident.initial_state(synth.box(n, spread, seed=seed))
    return init, fms.synthetic_routes(init, seed=seed)


def fms_sim(init, rt, p, ctx, simt=0.0, t0=-999., **kw):
    sim = resident.ResidentSim(init, p, ctx=ctx, **kw)
    sim.set_fms(*rt, simt=simt, t0=t0)
    return sim


def read_ax(sim):
    ax = np.zeros(sim.ctx.n)
    sim.ctx.check(sim.ctx.lib.bsa_sim_read_perf(sim.ctx.h, None, _lib.ptr(ax)), 'bsa_sim_read_perf')
    return ax


def same(a, b, what):
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), '%s: %s' % (what, k)


def sim_init(st):
    return {k: np.array(st[k]) for k in _lib.SIM_STATE_FIELDS}


def quiet_params(g):
    """The flight golden has ASAS inactive: a protected zone of 1 m, so no CD call finds a conflict."""
    return resident.params(simdt=float(g['simdt']), cd_every=20, rpz=1.0, hpz=1.0, tla=1.0)


def flight_case():
    g = load_flight()
    st, _, _ = flight_state(g, 0)
    return g, sim_init(st), (g['route_rows'], g['rt_off'], g['rt_n'], {k: st[k] for k in fms_np.REALS + fms_np.FLAGS + ('iactwp',)})


@pytest.mark.parametrize('case', ['flight64', 'box1500', 'dense'])
def test_resident_step_follows_the_helper(ctx, case):
    """45 steps from simt 0, re-anchored every step: exp = fms_np.update(prev), then
    oracle/step.py's composed step on the targets it wrote; the device's traffic
    and read_fms() against both (steps 0-20 and 41 tick, the rest evaluate
    ap.tas only), and the tick count.  flight64: the flight golden's initial
    state; box1500: a synth.box with generated routes, CD every 8th step;
    dense: CD and MVP every step in a box with conflicts, so asas.active
    aircraft and guidance coexist (300 aircraft: the oracle's detect is N^2)."""
    if case == 'flight64':
        _, init, rt = flight_case()
    else:
        init, rt = fms_traffic(300 if case == 'dense' else 1500, 17, spread=10.0 if case == 'dense' else 60.0)
    rows, off, cnt, st = rt
    n = len(init['lat'])
    p = resident.params(cd_every=1 if case == 'dense' else 8)
    op = oracle_params(p)
    sim = fms_sim(init, rt, p, ctx)
    sched, _, _ = fms.tick_schedule(0.0, p.simdt, 45)
    assert sched[:21].all() and sched[41] and sched.sum() == 22
    prev = dict(init, **st)
    prev.update(asas_trk=init['trk'].copy(), asas_tas=init['tas'].copy(), asas_vs=np.zeros(n),
                active=np.zeros(n, bool), ax=np.zeros(n))
    switched = np.zeros(n, bool)
    for k in range(45):
        skip = fms_np.near_threshold(prev, rows, off, cnt, tick=bool(sched[k]))
        assert skip.sum() <= 0.001 * n
        exp = fms_np.update(prev, rows, off, cnt, tick=bool(sched[k]))
        ost = ostep.sim_step({q: exp[q] for q in exp if q not in fms_np.REALS + fms_np.FLAGS + ('iactwp',)}, op,
                             do_cd=(k % p.cd_every == 0))
        sim.step(1)
        got, tr = sim.read_fms(), sim.read()
        compare(got, {'out_' + q: exp[q] for q in fms_np.OUTPUTS}, skip=skip, what='step %d ' % k)
        for q, scale in SCALES.items():
            ok, msg = util.close(tr[q][~skip], ost[q][~skip], scale)
            assert ok, 'step %d traffic %s: %s' % (k, q, msg)
        assert np.array_equal(tr['active'], ost['active']), 'step %d active' % k
        assert got['ticks'] == sched[:k + 1].sum()
        switched |= got['iactwp'] != prev['iactwp']
        prev = full_state(dict(init, **got), tr)
        prev['ax'] = read_ax(sim)
    assert switched.sum() > (3 if case == 'flight64' else 20)
    if case == 'dense':
        assert sim.stats()['n_conf'] > 0 and tr['active'].any()
    assert not np.array_equal(tr['hdg'], init['hdg'])


def test_flight_follows_the_reference(ctx):
    """The 2400 steps of the flight golden in batches of 40: iactwp, swlnav and
    swvnav equal every sample exactly, so every waypoint switch lands in its
    recorded 40-step window, and the tick count is the reference's."""
    g, init, rt = flight_case()
    sim = fms_sim(init, rt, quiet_params(g), ctx)
    every = int(g['every'])
    windows = np.zeros((60, 64), int)
    np.add.at(windows, (g['sw_step'] // every, g['sw_ac']), 1)
    prev = g['s_iactwp'][0]
    for s in range(1, 61):
        sim.step(every)
        got = sim.read_fms()
        for k in ('iactwp', 'swlnav', 'swvnav'):
            assert np.array_equal(got[k], g['s_' + k][s]), 'sample %d %s' % (s, k)
        assert np.array_equal(got['iactwp'] - prev, windows[s - 1]), 'switches of window %d' % (s - 1)
        prev = got['iactwp']
    assert got['ticks'] == int(g['nticks']) and got['simt'] == g['s_simt'][60] and got['t0'] == g['s_t0'][60]


def test_flight_forty_steps_from_three_samples(ctx):
    """Re-initialised from the first sample, a middle one and one just before a
    recorded switch, 40 steps: reals against the next sample.  The same 40-step
    drift of fms_np + oracle/step.py against the golden, measured on the CPU
    with the capture's numpy, is 0 (bitwise: tools/make_golden.py asserts it
    after every step, tests/test_fms_cpu.py at every sample), so ten times it is
    0 and the bound is util.close's 1e-9 rule.  A re-initialised sim starts with
    traf.ax = 0 as Traffic.create does; ax is read only by a tick and rewritten
    by every step, so samples whose first step does not tick are taken (the
    first sample's ax is 0 in the reference too)."""
    g = load_flight()
    every = int(g['every'])
    sw_windows = set((g['sw_step'] // every).tolist())

    def no_tick(s):
        return not fms_np.ticks(float(g['s_simt'][s]), float(g['s_t0'][s]))
    middle = next(s for s in range(30, 60) if no_tick(s))
    before_switch = next(s for s in range(5, 60) if s != middle and s in sw_windows and no_tick(s))
    for s in (0, middle, before_switch):
        st, simt, t0 = flight_state(g, s)
        rt = (g['route_rows'], g['rt_off'], g['rt_n'], {k: st[k] for k in fms_np.REALS + fms_np.FLAGS + ('iactwp',)})
        sim = fms_sim(sim_init(st), rt, quiet_params(g), ctx, simt=simt, t0=t0)
        sim.step(every)
        got, tr = sim.read_fms(), sim.read()
        compare(got, {'out_' + k: g['s_' + k][s + 1] for k in fms_np.OUTPUTS}, what='from sample %d ' % s)
        for k in FLIGHT_TRAFFIC[:-1]:
            ok, msg = util.close(tr[k], g['s_' + k][s + 1], SCALES[k])
            assert ok, 'from sample %d %s: %s' % (s, k, msg)
        ok, msg = util.close(read_ax(sim), g['s_ax'][s + 1], 1.0)
        assert ok, 'from sample %d ax: %s' % (s, msg)


@pytest.mark.parametrize('simt0,tick', [(0.0, True), (0.9, False)])
def test_abort_in_mid_batch_is_exact(ctx, simt0, tick):
    """A candidate list far too small, CD every 4th step: the batch of steps 1-30
    completes steps 1-3, aborts at step 4 and re-runs from there.  The clock is
    replayed over the three completed steps; from simt 0 step 4 ticks (undo set
    restored), from simt 0.9 steps 1-2 tick and the aborted step 4 does not, so
    the undo set holds step 2's values and must be left alone."""
    init, rt = fms_traffic(1500, 71)
    p = resident.params(cd_every=4)
    sched = fms.tick_schedule(simt0, p.simdt, 5)[0]
    assert sched[4] == tick and sched[1] and sched[2]
    ref = fms_sim(init, rt, p, ctx, simt0)
    ref.step(1)
    ref.step(30)
    exp, exp_st, exp_stats = ref.read_fms(), ref.read(), ref.stats()
    c = _lib.Context(0)
    try:
        sim = fms_sim(init, rt, p, c, simt0)
        c.set_candidate_capacity(16)
        sim.step(1)
        c.set_candidate_capacity(16)
        sim.step(30)
        same(sim.read_fms(), exp, 'after the re-run')
        same(sim.read(), exp_st, 'after the re-run')
        assert sim.stats()['cd_calls'] == exp_stats['cd_calls'] == 8 and exp_stats['n_conf'] > 0
    finally:
        c.close()
    assert (exp['iactwp'] > 0).any()


@pytest.mark.parametrize('simt,t0,tick', [(0.0, -999., True), (5.0, 4.5, False)])
def test_abort_and_rerun_is_exact(ctx, simt, t0, tick):
    """K2 row buckets one pair wide overflow at the first dense row: step 0 aborts
    and re-runs.  On a tick step the undo set puts the FMS state back first; on
    a non-tick step nothing was changed.  Traffic and read_fms() equal the
    undisturbed run bitwise."""
    init, rt = fms_traffic(1500, 53)
    p = resident.params(cd_every=1)
    assert fms.tick_schedule(simt, p.simdt, 1, t0)[0][0] == tick
    ref = fms_sim(init, rt, p, ctx, simt, t0)
    ref.step(6)
    exp, exp_st = ref.read_fms(), ref.read()
    c = _lib.Context(0)
    try:
        c.set_row_bucket(1)
        sim = fms_sim(init, rt, p, c, simt, t0)
        sim.step(6)
        same(sim.read_fms(), exp, 'after the re-run')
        same(sim.read(), exp_st, 'after the re-run')
        assert sim.stats()['n_conf'] == ref.stats()['n_conf'] > 0
    finally:
        c.close()
    assert (exp['iactwp'] > 0).any() == tick


def test_one_batch_equals_single_steps(ctx):
    init, rt = fms_traffic(1500, 59)
    p = resident.params(cd_every=4)
    a = fms_sim(init, rt, p, ctx)
    a.step(45)
    ea, ta = a.read_fms(), a.read()
    b = fms_sim(init, rt, p, ctx)
    for _ in range(45):
        b.step(1)
    same(b.read_fms(), ea, '45 x step(1)')
    same(b.read(), ta, '45 x step(1)')
    assert ea['ticks'] == 22 and (ea['iactwp'] > 0).any()


def test_two_ranks_equal_one(ctx):
    init, rt = fms_traffic(1500, 61)
    p = resident.params(cd_every=1)
    ref = fms_sim(init, rt, p, ctx)
    ref.step(25)
    exp = ref.read_fms()

    def rank(r, c, g):
        sim = fms_sim(init, rt, p, c, rank=r, world=2, group=g)
        sim.step(10)
        sim.step(15)
        with pytest.raises(RuntimeError):
            sim.delete([1])                       # refused on several ranks with guidance on
        return sim.read_fms(), sim.row_ids()

    res = run_ranks(2, rank)
    ids = np.concatenate([i for _, i in res])
    assert np.array_equal(np.sort(ids), np.arange(1500))
    for k in fms_np.OUTPUTS:
        full = np.zeros(1500, dtype=np.asarray(exp[k]).dtype)
        for got, i in res:
            full[i] = got[k][i]
        assert np.array_equal(full, exp[k], equal_nan=True), k
    assert all(got['ticks'] == exp['ticks'] for got, _ in res)


def test_delete_carries_the_routes_along(ctx):
    """Five of 300 aircraft deleted mid-route on one rank.  With resolution off no
    aircraft's flight depends on another's, so the survivors must continue
    bitwise as in a twin sim that keeps all 300."""
    init, rt = fms_traffic(300, 89, spread=30.0)
    p = resident.params(reso=False)
    c2 = _lib.Context(0)                       # (one resident sim per context)
    try:
        _delete_and_continue(init, rt, p, ctx, c2)
    finally:
        c2.close()


def _delete_and_continue(init, rt, p, ctx, c2):
    sim, twin = fms_sim(init, rt, p, ctx), fms_sim(init, rt, p, c2)
    sim.step(10)
    twin.step(10)
    gone = [3, 7, 100, 101, 299]
    before = sim.read_fms()
    sim.delete(gone)
    after = sim.read_fms()
    for k in fms_np.OUTPUTS:
        assert np.array_equal(after[k], np.delete(before[k], gone), equal_nan=True), k
    sim.step(35)
    twin.step(35)
    got, exp, tg, te = sim.read_fms(), twin.read_fms(), sim.read(), twin.read()
    assert len(got['iactwp']) == 295 and got['ticks'] == exp['ticks'] == 22
    for k in fms_np.OUTPUTS:
        assert np.array_equal(got[k], np.delete(exp[k], gone), equal_nan=True), k
    for k in ('lat', 'lon', 'alt', 'tas', 'hdg'):
        assert np.array_equal(tg[k], np.delete(te[k], gone)), k
    assert (got['iactwp'] > np.delete(before['iactwp'], gone)).any()      # waypoints passed after the delete
    with pytest.raises(RuntimeError):
        sim.create({k: v[:2] for k, v in init.items()})
    sim.set_fms(None)
    twin.set_fms(None)


def test_feature_off_is_untouched(ctx):
    init, rt = fms_traffic(1500, 67)
    p = resident.params(cd_every=2)
    a = resident.ResidentSim(init, p, ctx=ctx)
    with pytest.raises(RuntimeError):
        a.read_fms()
    a.step(8)
    ea = a.read()
    b = fms_sim(init, rt, p, ctx)
    b.set_fms(None)                                # switched off again: steps as if never on
    with pytest.raises(RuntimeError):
        b.read_fms()
    b.step(8)
    same(b.read(), ea, 'feature off')
