"""GPU: waypoint recovery after ResumeNav on the device -- the standalone call
(bsa_fms_recover, bluesky_amd.fms.recover) against tests/golden/fms_recover2000.npz,
Route.findact + Route.direct of the reference's own Route / Autopilot objects
applied count times per aircraft, and the resident step's launch
(bsa_sim_set_recovery) against tests/recover_np.py composed with oracle/asas.py
and oracle/step.py and against tests/golden/fms_recover_flight.npz, the
reference's closed loop with ASAS.  Reals within util.close's 1e-9 rule with the field's
largest finite magnitude as scale, NaN positions equal; flags and iactwp
exactly.  The golden holds no comparison within 1e-9 relative of equality."""
import numpy as np
import pytest

from bluesky_amd import fms
from tests import fms_np, recover_np
from tests.recover_cases import INPUTS, compare, load

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    g, st = load()
    return dict(g=g, st=st, exp={k: g['out_' + k] for k in recover_np.OUTPUTS})


def prefix(golden, n):
    g = golden['g']
    return g['route_rows'], g['rt_off'][:n], g['rt_n'][:n], {k: v[:n] for k, v in golden['st'].items()}, g['count'][:n]


@pytest.mark.parametrize('n', [2000, 1, 63, 64, 65, 257])
def test_standalone_recover_matches_golden(ctx, golden, n):
    rows, off, cnt, st, count = prefix(golden, n)
    keep = {k: np.array(v) for k, v in st.items()}
    got = fms.recover(rows, off, cnt, st, count, ctx=ctx)
    compare(got, golden['exp'], n=n)
    for k in INPUTS:                                   # the caller's arrays stay as they were
        assert np.array_equal(st[k], keep[k], equal_nan=True), k
    for k in recover_np.UNTOUCHED:                     # read only, or not part of a recovery at all
        if k in got:
            assert np.array_equal(got[k], st[k], equal_nan=True), k
    assert (got['iactwp'] >= st['iactwp']).all()       # findact never walks back


def test_zero_counts_leave_everything_bitwise(ctx, golden):
    rows, off, cnt, st, count = prefix(golden, 2000)
    got = fms.recover(rows, off, cnt, st, np.zeros_like(count), ctx=ctx)
    for k in got:
        assert np.array_equal(got[k], st[k], equal_nan=True), k


def test_standalone_refusals_launch_nothing(ctx, golden):
    rows, off, cnt, st, count = prefix(golden, 64)
    with pytest.raises(RuntimeError):                                   # rows past the table
        fms.recover(rows[:int(off[63])], off, np.maximum(cnt, 1), st, count, ctx=ctx)
    k = int(np.flatnonzero(cnt > 0)[0])
    bad = np.array(st['iactwp'])
    bad[k] = cnt[k]
    with pytest.raises(RuntimeError):                                   # active waypoint past its route
        fms.recover(rows, off, cnt, dict(st, iactwp=bad), count, ctx=ctx)
    with pytest.raises(RuntimeError):
        fms.recover(rows, off, cnt, st, -count - 1, ctx=ctx)            # a negative count
    with pytest.raises(ValueError):
        fms.recover(rows, off, cnt, st, count[:63], ctx=ctx)            # a short array
    got = fms.recover(rows, off, cnt, st, count, ctx=ctx)               # ... and the context still works
    compare(got, golden['exp'], n=64)


# ---------------------------------------------------------------- the resident step
# 300 aircraft in a 10 NM box with generated routes, a 1 NM protected zone, 1 s
# steps and a CD call every step: from step 1 on ResumeNav drops 10 - 30
# resopairs per call (some ownships two at once), steps 0, 1, 3, 5 .. tick and
# 2, 4 .. do not.  The expected values are tests/recover_cases.recover_step, the
# composition asserted bitwise against the reference's closed loop with ASAS
# when tests/golden/fms_recover_flight.npz was captured (its tests: further down).
from bluesky_amd import _lib, resident                                         # noqa: E402
from oracle import asas as oasas                                               # noqa: E402
from tests import util                                                         # noqa: E402
from tests.fms_cases import compare as compare_fms                             # noqa: E402
from tests.recover_cases import recover_step                                   # noqa: E402
from tests.test_gpu_fms import fms_sim, fms_traffic, read_ax, same             # noqa: E402
from tests.test_gpu_multirank import run_ranks                                 # noqa: E402
from tests.test_gpu_sim import SCALES, full_state, oracle_params               # noqa: E402

N = 300


def dense():
    init, rt = fms_traffic(N, 17, spread=10.0)
    return init, rt, resident.params(simdt=1.0, rpz=1852.0, cd_every=1, resume_nav=True)


def recover_sim(init, rt, p, ctx, on=True, **kw):
    sim = fms_sim(init, rt, p, ctx, **kw)
    if on:
        sim.set_recovery()
    return sim


def start_state(init, st):
    n = len(init['lat'])
    prev = dict(init, **st)
    prev.update(asas_trk=init['trk'].copy(), asas_tas=init['tas'].copy(), asas_vs=np.zeros(n),
                active=np.zeros(n, bool), ax=np.zeros(n))
    return prev


def test_resident_step_follows_the_helper(ctx):
    """24 steps, re-anchored every step on the device's own state: exp =
    recover_step(prev) -- fms_np.update, oracle detect + MVP + ResumeNav,
    recover_np.recover once per dropped pair, pilot and kinematics.  Drop counts,
    active, flags and iactwp exactly, reals under the 1e-9 rule; ap_alt as read
    back is the post-recovery value where ComputeVNAV dialled a new altitude in."""
    init, rt, p = dense()
    rows, off, cnt, st = rt
    op = oracle_params(p)
    sim = recover_sim(init, rt, p, ctx)
    sched, _, _ = fms.tick_schedule(0.0, p.simdt, 24)
    bk = oasas.Bookkeeping(N)
    prev = start_state(init, st)
    recovered = np.zeros(N, bool)
    twice = moved = lnav_on = dialled = 0
    for k in range(24):
        skip = fms_np.near_threshold(prev, rows, off, cnt, tick=bool(sched[k]))
        exp, count = recover_step(prev, rows, off, cnt, op, bk, bool(sched[k]), True)
        ticked = fms_np.update(prev, rows, off, cnt, tick=bool(sched[k]))
        with np.errstate(all='ignore'):
            skip |= recover_np.near_threshold(dict(prev, **{q: ticked[q] for q in fms_np.OUTPUTS}), rows, off, cnt, count)
        assert skip.sum() <= 0.001 * N
        sim.step(1)
        got, tr = sim.read_fms(), sim.read()
        assert np.array_equal(sim.read_dropcount(), count), 'step %d drop counts' % k
        assert np.array_equal(sim.ctx.sim_read_asas()['dropped'], count > 0), 'step %d dropped flags' % k
        compare_fms(got, {'out_' + q: exp[q] for q in fms_np.OUTPUTS}, what='step %d ' % k)
        for q, scale in SCALES.items():
            ok, msg = util.close(tr[q], exp[q], scale)
            assert ok, 'step %d traffic %s: %s' % (k, q, msg)
        assert np.array_equal(tr['active'], exp['active']), 'step %d active' % k
        r = count > 0
        recovered |= r
        twice += int((count >= 2).sum())
        moved += int((exp['iactwp'][r] != prev['iactwp'][r]).sum())
        lnav_on += int((exp['swlnav'][r] & ~ticked['swlnav'][r]).sum())
        new_alt = r & (exp['ap_alt'] != ticked['ap_alt'])
        dialled += int(new_alt.sum())
        assert np.array_equal(got['ap_alt'][new_alt], exp['ap_alt'][new_alt])      # (assigned, not computed: exact)
        prev = full_state(dict(init, **got), tr)
        prev['ax'] = read_ax(sim)
    assert recovered.sum() >= 8 and twice > 0 and moved > 0 and lnav_on > 0 and dialled > 0


def run(sim, batches):
    for b in batches:
        sim.step(b)
    return sim.read_fms(), sim.read(), sim.read_dropcount()


def test_one_batch_equals_single_steps(ctx):
    init, rt, p = dense()
    ea, ta, ca = run(recover_sim(init, rt, p, ctx), [45])
    eb, tb, cb = run(recover_sim(init, rt, p, ctx), [1] * 45)
    same(eb, ea, '45 x step(1)')
    same(tb, ta, '45 x step(1)')
    assert np.array_equal(ca, cb) and ca.any()
    ec, tc, _ = run(recover_sim(init, rt, p, ctx), [40, 5])
    same(ec, ea, 'batches of 40')
    same(tc, ta, 'batches of 40')


def test_switch_off_is_the_step_as_it_was(ctx):
    """set_recovery never called: bitwise the run in which it was switched on and
    off again before the first step, the same drop counts as with recovery on
    at the first CD call that drops a pair -- and from there another flight: the
    recovered aircraft got new waypoints and LNAV, the others did not."""
    init, rt, p = dense()
    never = recover_sim(init, rt, p, ctx, on=False)
    e0, t0, c0 = run(never, [2])
    e0b, t0b, _ = run(never, [28])
    onoff = recover_sim(init, rt, p, ctx)
    onoff.set_recovery(False)
    e1, t1, c1 = run(onoff, [2])
    same(e1, e0, 'switched off again')
    same(t1, t0, 'switched off again')
    on = recover_sim(init, rt, p, ctx)
    e2, t2, c2 = run(on, [2])
    assert np.array_equal(c0, c2) and c0.any()
    r = c0 > 0
    for k in fms_np.OUTPUTS:                            # the aircraft that lost no pair: untouched by the switch
        assert np.array_equal(e0[k][~r], e2[k][~r], equal_nan=True), k
    assert not np.array_equal(e0['actwp_turndist'][r], e2['actwp_turndist'][r])
    assert e2['swlnav'][r].all()
    e2b, t2b, _ = run(on, [28])
    assert not np.array_equal(e0b['iactwp'], e2b['iactwp']) or not np.array_equal(e0b['swlnav'], e2b['swlnav'])
    assert not np.array_equal(t0b['lat'], t2b['lat'])


@pytest.mark.parametrize('k0,tick', [(3, True), (4, False)])
def test_abort_and_rerun_is_exact(ctx, k0, tick):
    """K2 row buckets one pair wide from step k0 on: that CD step -- one in which
    ResumeNav drops pairs and recovery runs -- aborts and re-runs, once on a
    ticking step and once on one that does not tick.  The aborted attempt never
    reached its recovery launch, so FMS state, traffic and drop counts equal the
    undisturbed run bitwise."""
    init, rt, p = dense()
    assert fms.tick_schedule(0.0, p.simdt, k0 + 1)[0][k0] == tick
    ref = recover_sim(init, rt, p, ctx)
    ref.step(k0)
    ref.step(1)
    at_k0 = ref.read_dropcount()
    assert at_k0.any()
    ref.step(5)
    exp, exp_st, exp_c = ref.read_fms(), ref.read(), ref.read_dropcount()
    c = _lib.Context(0)
    try:
        sim = recover_sim(init, rt, p, c)
        sim.step(k0)
        c.set_row_bucket(1)
        sim.step(6)
        same(sim.read_fms(), exp, 'after the re-run')
        same(sim.read(), exp_st, 'after the re-run')
        assert np.array_equal(sim.read_dropcount(), exp_c)
        assert sim.stats()['n_conf'] == ref.stats()['n_conf'] > 0
    finally:
        c.close()


def test_deleted_intruder_starts_recovery(ctx):
    """The intruder of a live resopair is deleted: at the next CD call ResumeNav
    drops the pair (idx2 < 0) and its ownship recovers, like any other."""
    init, rt, p = dense()
    rows, off, cnt, st = rt
    sim = recover_sim(init, rt, p, ctx)
    sim.step(4)
    i1, i2 = sim.resopairs()
    own, gone = int(i1[0]), int(i2[0])
    sim.delete([gone])
    own -= 1 if gone < own else 0
    keep = np.arange(N) != gone
    i1, i2 = sim.resopairs()
    assert (i2[i1 == own] == -1).sum() == 1
    got0, tr0 = sim.read_fms(), sim.read()
    prev = full_state({k: v[keep] for k, v in init.items()}, tr0)
    prev.update({k: got0[k] for k in fms_np.REALS + fms_np.FLAGS + fms_np.TARGETS + ('iactwp',)})
    prev['ax'] = read_ax(sim)
    roff = np.concatenate([[0], np.cumsum(cnt[keep])[:-1]]).astype(np.int32)
    rrows = np.concatenate([rows[off[k]:off[k] + cnt[k]] for k in np.flatnonzero(keep)])
    bk = oasas.Bookkeeping(N - 1)
    bk.resopairs = set(zip(i1.tolist(), i2.tolist()))
    bk.active = tr0['active'].copy()
    tick = fms_np.ticks(got0['simt'], got0['t0'])
    exp, count = recover_step(prev, rrows, roff, cnt[keep], oracle_params(p), bk, tick, True)
    assert count[own] >= 1
    sim.step(1)
    got, tr = sim.read_fms(), sim.read()
    assert np.array_equal(sim.read_dropcount(), count)
    compare_fms(got, {'out_' + q: exp[q] for q in fms_np.OUTPUTS}, what='after the delete ')
    for q, scale in SCALES.items():
        ok, msg = util.close(tr[q], exp[q], scale)
        assert ok, 'after the delete %s: %s' % (q, msg)
    assert np.array_equal(tr['active'], exp['active'])       # (off only if the ownship keeps no other pair)
    assert got['swlnav'][own]


def test_two_ranks_equal_one(ctx):
    init, rt, p = dense()
    exp, exp_t, exp_c = run(recover_sim(init, rt, p, ctx), [30])

    def rank(r, c, g):
        sim = recover_sim(init, rt, p, c, rank=r, world=2, group=g)
        sim.step(10)
        sim.step(20)
        return sim.read_fms(), sim.read_dropcount(), sim.row_ids(), sim.read()

    res = run_ranks(2, rank)
    ids = np.concatenate([i for _, _, i, _ in res])
    assert np.array_equal(np.sort(ids), np.arange(N))
    for k in fms_np.OUTPUTS:
        full = np.zeros(N, dtype=np.asarray(exp[k]).dtype)
        for got, _, i, _ in res:
            full[i] = got[k][i]
        assert np.array_equal(full, exp[k], equal_nan=True), k
    full = np.zeros(N, np.int32)
    for _, c, i, _ in res:
        full[i] = c[i]
    assert np.array_equal(full, exp_c) and exp_c.any()
    for _, _, _, tr in res:                              # (read gathers every rank's rows)
        same(tr, exp_t, 'two ranks')


def test_refusals(ctx):
    init, rt, p = dense()
    sim = resident.ResidentSim(init, p, ctx=ctx)
    with pytest.raises(RuntimeError, match='FMS'):
        sim.set_recovery()                                # no guidance, no recovery
    sim.set_fms(*rt)
    sim.set_recovery()
    sim.set_fms(None)                                     # ... and off with it
    with pytest.raises(RuntimeError, match='FMS'):
        sim.set_recovery()
    sim.set_recovery(False)                               # switching off is always allowed
    e1 = run_plain(sim)
    e0 = run_plain(resident.ResidentSim(init, p, ctx=ctx))         # (one resident sim per context: after the other)
    same(e1, e0, 'recovery off with the guidance')


def run_plain(sim):
    sim.step(3)
    return sim.read()


def test_inert_without_resume_nav(ctx):
    init, rt, _ = dense()
    p = resident.params(simdt=1.0, rpz=1852.0, cd_every=1)
    a, ta, _ = run(fms_sim(init, rt, p, ctx), [6])
    b, tb, cb = run(recover_sim(init, rt, p, ctx), [6])
    same(b, a, 'resume_nav off')
    same(tb, ta, 'resume_nav off')
    assert not cb.any()


# ---------------------------------------------------------------- the reference's closed loop with ASAS
from tests.recover_cases import flight_params, flight_run, load_flight          # noqa: E402


def flight_sim(g, ctx, on=True, **kw):
    st = {k[5:]: np.array(v) for k, v in g.items() if k.startswith('init_')}
    init = {k: st[k] for k in _lib.SIM_STATE_FIELDS}
    rt = (g['route_rows'], g['rt_off'], g['rt_n'], {k: st[k] for k in fms_np.REALS + fms_np.FLAGS + ('iactwp',)})
    p = resident.params(simdt=float(g['simdt']), rpz=float(g['rpz']), hpz=float(g['hpz']), tla=float(g['tla']),
                        mar=float(g['mar']), cd_every=int(g['cd_every']), resume_nav=True)
    return recover_sim(init, rt, p, ctx, on=on, **kw)


def test_flight_follows_the_reference(ctx):
    """The 1920 steps of the flight golden in batches of 40: the recovery events
    (CD call, aircraft, count, iactwp read right after the CD step) equal the
    reference's; iactwp, swlnav and swvnav equal every sample exactly, so every
    waypoint switch falls in its recorded 40-step window.  (A batch that holds
    a CD step is split after that step.)"""
    g = load_flight()
    sim = flight_sim(g, ctx)
    every, cd_every, nb = int(g['every']), int(g['cd_every']), int(g['nsteps']) // int(g['every'])
    n = len(g['rt_n'])
    windows = np.zeros((nb, n), int)
    np.add.at(windows, (g['sw_step'] // every, g['sw_ac']), 1)
    want = list(zip(g['ev_cd'].tolist(), g['ev_ac'].tolist(), g['ev_count'].tolist()))
    want = [w + (int(i),) for w, i in zip(want, g['ev_iactwp'])]
    events, sw = [], np.zeros((nb, n), int)
    prev = g['s_iactwp'][0]
    for s in range(1, nb + 1):
        first = (s - 1) * every
        cds = [c for c in range(first, s * every) if c % cd_every == 0]
        assert len(cds) <= 1
        if cds:                              # up to and with the CD step, so that iactwp is read right after it
            sim.step(cds[0] - first + 1)
            count, now = sim.read_dropcount(), sim.read_fms()['iactwp']
            events += [(cds[0] // cd_every, int(k), int(count[k]), int(now[k])) for k in np.flatnonzero(count)]
            if s * every - cds[0] - 1:
                sim.step(s * every - cds[0] - 1)
        else:
            sim.step(every)
        got = sim.read_fms()
        for k in ('iactwp', 'swlnav', 'swvnav'):
            assert np.array_equal(got[k], g['s_' + k][s]), 'sample %d %s' % (s, k)
        sw[s - 1] = got['iactwp'] != prev
        assert (sw[s - 1] <= (windows[s - 1] > 0)).all(), 'a switch outside its window %d' % (s - 1)
        prev = got['iactwp']
    assert events == want
    tr = sim.read()
    assert np.array_equal(tr['active'], g['s_active'][nb])


def test_flight_switch_off_is_the_parent(ctx):
    """set_recovery never called, on the reference's scenario: the step as it was
    -- the helper composition with recovery emulated as "never" -- for 800 steps
    (13 CD calls, the first drops among them), and its waypoints are not the
    golden's.  A free run of the device against numpy, not re-anchored: flags,
    iactwp and active exactly, reals within 1e-6 of the scale (800 steps under
    the per-step 1e-9 rule), not bitwise.  That the event and switch lists of a
    run without recovery differ from the golden's is asserted on the CPU
    (tests/test_recover_np.py); here the state at sample 20 differs."""
    g = load_flight()
    sim = flight_sim(g, ctx, on=False)
    sim.step(800)
    got, tr = sim.read_fms(), sim.read()
    samples, ev_never, _ = flight_run(g, 800, recovery=False)
    exp = samples[-1]
    assert any(c < 13 for c, _, _, _ in ev_never)
    for q in ('iactwp', 'swlnav', 'swvnav'):
        assert np.array_equal(got[q], exp[q]), 'never ' + q
    for q, scale in SCALES.items():      # 800 free steps under the per-step 1e-9 rule: 800 x 1e-9 < 1e-6 of the scale
        ok, msg = util.close(tr[q], exp[q], scale * 1e3)
        assert ok, 'never %s: %s' % (q, msg)
    assert np.array_equal(tr['active'], exp['active'])
    with_rec = g['s_iactwp'][20], g['s_swlnav'][20], g['s_actwp_turndist'][20]
    assert not (np.array_equal(got['iactwp'], with_rec[0]) and np.array_equal(got['swlnav'], with_rec[1])
                and np.array_equal(got['actwp_turndist'], with_rec[2]))


def test_flight_two_ranks_equal_one(ctx):
    g = load_flight()
    one = flight_sim(g, ctx)
    one.step(200)
    exp, exp_t = one.read_fms(), one.read()

    def rank(r, c, grp):
        sim = flight_sim(g, c, rank=r, world=2, group=grp)
        sim.step(200)
        return sim.read_fms(), sim.row_ids(), sim.read()

    res = run_ranks(2, rank)
    for k in fms_np.OUTPUTS:
        full = np.zeros(len(g['rt_n']), dtype=np.asarray(exp[k]).dtype)
        for got, i, _ in res:
            full[i] = got[k][i]
        assert np.array_equal(full, exp[k], equal_nan=True), k
    for _, _, tr in res:
        same(tr, exp_t, 'two ranks')


def test_flight_reanchored_at_every_recovery(ctx):
    """Every step of the flight golden in which a recovery occurs, and 2 steps
    either side: one sim runs from step 0 (so it holds the run's resopairs);
    before each of these steps its traffic is overwritten with bsa_sim_update and
    its FMS state and clock with set_fms from the helper composition's state at
    step k -- bitwise the reference's (tests/test_recover_np.py) -- then one step,
    compared with the composition's step k + 1 under the 1e-9 rule; drop counts,
    active, flags and iactwp exactly.  On the recoveries whose ComputeVNAV took
    the urgent descent (legdist < dist2vs) ap_alt as read back is the dialled-in
    nextaltco, exactly."""
    g = load_flight()
    rows, off, cnt = g['route_rows'], g['rt_off'], g['rt_n']
    nsteps, cd_every = int(g['nsteps']), int(g['cd_every'])
    window = sorted({int(s) + d for s in g['ev_step'] for d in range(-2, 3) if 0 <= int(s) + d < nsteps})
    _, _, _, kept = flight_run(g, max(window) + 1, keep=set(window))
    sim = flight_sim(g, ctx)
    at = urgent_seen = 0
    for k in window:
        if k > at:
            sim.step(k - at)
        before, simt, t0, exp, count = kept[k]
        sim.update(**{f: before[f] for f in _lib.SIM_STATE_FIELDS})
        sim.set_fms(rows, off, cnt, {f: before[f] for f in fms_np.REALS + fms_np.FLAGS + ('iactwp',)}, simt=simt, t0=t0)
        sim.step(1)
        at = k + 1
        got, tr = sim.read_fms(), sim.read()
        what = 'step %d ' % k
        compare_fms(got, {'out_' + q: exp[q] for q in fms_np.OUTPUTS}, what=what)
        for q, scale in SCALES.items():
            ok, msg = util.close(tr[q], exp[q], scale)
            assert ok, '%straffic %s: %s' % (what, q, msg)
        assert np.array_equal(tr['active'], exp['active']), what + 'active'
        if k % cd_every == 0:
            assert np.array_equal(sim.read_dropcount(), count), what + 'drop counts'
            assert count.any() == (k in g['ev_step'])
            for ac in g['ev_ac'][(g['ev_step'] == k) & (g['ev_urgent'] > 0)]:
                assert got['ap_alt'][ac] == exp['ap_alt'][ac] == exp['actwp_nextaltco'][ac], what + 'urgent descent'
                assert exp['ap_alt'][ac] != before['ap_alt'][ac] or exp['ap_alt'][ac] != before['alt'][ac]
                urgent_seen += 1
    assert urgent_seen > 0 and len(window) >= 5 * len(np.unique(g['ev_step'])) - 4
