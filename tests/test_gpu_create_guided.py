"""GPU: aircraft created while OpenAP, its limits, the forces, the autopilot guidance and waypoint
recovery run (bsa_sim_create_with, ResidentSim.create(..., perf=, mass=, fms=)).
Everything is compared bitwise: against sims that never saw a create (separated groups), and against
the sequence the refusal of plain create prescribes -- read back, stages off, create, stages on again.
Shapes around the 512-row tile edge of the home order: 500 + 40 crosses it, 700 + 1, 700 + 37 + 37."""
import numpy as np
import pytest

from bluesky_amd import _lib, fms, resident
from tests.test_gpu_perf_forces import traffic

pytestmark = pytest.mark.gpu

K = 25            # steps before and after the create: steps 0-20 and 41 tick the FMS, so the create falls
SHAPES = [(500, (40,)), (700, (1,)), (700, (37, 37))]      # between two ticks and one follows it
FMS_FIELDS = _lib.FMS_REALS + _lib.FMS_FLAGS + _lib.FMS_TARGETS + ('iactwp',)
FMS_STATE = _lib.FMS_REALS + _lib.FMS_FLAGS + ('iactwp',)


def scene(n, m, seed, far):
    """n old and m new aircraft with OpenAP types of one table, masses and routes of their own.  far: the
    new ones 30 deg of longitude away, where no pair of old and new comes within the look-ahead."""
    tr = traffic(n + m, seed, spread=30.0)
    init = tr['init']
    if far:
        init['lon'][n:] += 30.0
    cut = lambda a, b: {k: v[a:b].copy() for k, v in init.items()}
    old, new = cut(0, n), cut(n, n + m)
    return dict(n=n, m=m, old=old, new=new, table=tr['table'], ftable=tr['ftable'], tidx=tr['tidx'], mass=tr['mass'],
                rt_old=fms.synthetic_routes(old, seed=seed), rt_new=fms.synthetic_routes(new, seed=seed + 1))


def params():
    return resident.params(cd_every=1, resume_nav=True)


def guided(init, tidx, mass, rt, sc, ctx, simt=0.0, t0=-999.):
    sim = resident.ResidentSim(init, params(), ctx=ctx)
    sim.set_perf(sc['table'], tidx)
    sim.set_forces(sc['ftable'], mass)
    sim.set_fms(*rt, simt=simt, t0=t0)
    sim.set_recovery(True)
    return sim


def part(sc, a, b):
    """The new aircraft [a, b) of the scene as create takes them: state, perf, mass, fms."""
    n = sc['n']
    rows, off, cnt, st = sc['rt_new']
    lo, hi = (int(off[a]), int(off[b - 1] + cnt[b - 1])) if b > a else (0, 0)
    rt = (rows[lo:hi], off[a:b] - lo, cnt[a:b], {k: np.asarray(v)[a:b] for k, v in st.items()})
    return ({k: v[a:b] for k, v in sc['new'].items()},
            dict(perf=sc['tidx'][n + a:n + b], mass=sc['mass'][n + a:n + b], fms=rt))


def parts(sc, groups):
    out, a = [], 0
    for g in groups:
        out.append(part(sc, a, a + g))
        a += g
    return out


def snapshot(sim):
    ph, ax = sim.read_perf()
    return dict(read=sim.read(), fms=sim.read_fms(), forces=sim.read_forces(), phase=ph, ax=ax)


def rows_equal(got, exp, sel, what, fuel=True):
    """got's rows sel equal exp, bitwise, in read(), read_fms(), read_perf() and read_forces()."""
    for k, v in exp['read'].items():
        assert np.array_equal(got['read'][k][sel], v, equal_nan=True), '%s read %s' % (what, k)
    for k in FMS_FIELDS:
        assert np.array_equal(got['fms'][k][sel], exp['fms'][k], equal_nan=True), '%s read_fms %s' % (what, k)
    for k in ('phase', 'ax'):
        assert np.array_equal(got[k][sel], exp[k], equal_nan=True), '%s read_perf %s' % (what, k)
    for k, v in exp['forces'].items():
        if fuel or k != 'fuel_used':
            assert np.array_equal(got['forces'][k][sel], v, equal_nan=True), '%s read_forces %s' % (what, k)


def take(snap, sel):
    return {k: ({q: (w[sel] if isinstance(w, np.ndarray) else w) for q, w in v.items()} if isinstance(v, dict) else v[sel])
            for k, v in snap.items()}


def with_decoys(sc):
    """The new aircraft followed by 60 of the old ones, another 60 deg away, as one sim's arrays.  ASAS.update
    calls resolve only while the sim holds a conflict somewhere, and resolve then writes asas.trk / tas / vs of
    EVERY aircraft (asas.py:486-487): in A the old group's conflicts refresh the new aircraft's asas.* each CD
    call, so a D without any conflict -- a lone aircraft -- would keep its initial ones.  The decoys give D
    conflicts of its own, out of the new aircraft's reach."""
    n, q = sc['n'], 60
    dec = {k: v[:q].copy() for k, v in sc['old'].items()}
    dec['lon'] += 60.0
    rt = fms.synthetic_routes(dec, seed=5)
    init = {k: np.concatenate([sc['new'][k], dec[k]]) for k in dec}
    rows, off, cnt = fms.append_routes(*sc['rt_new'][:3], *rt[:3])
    st = {k: np.concatenate([np.asarray(sc['rt_new'][3][k]), np.asarray(rt[3][k])]) for k in FMS_STATE}
    return (init, np.concatenate([sc['tidx'][n:], sc['tidx'][:q]]), np.concatenate([sc['mass'][n:], sc['mass'][:q]]),
            (rows, off, cnt, st))


@pytest.fixture
def second():
    c = _lib.Context(0)                     # (one resident sim per context)
    yield c
    c.close()


@pytest.mark.parametrize('n,groups', SHAPES)
def test_separated_groups_fly_as_if_alone(ctx, n, groups):
    """The pin.  A: K steps, create, K more.  C: the old aircraft alone, 2K steps.  D: the new ones alone,
    fresh at A's simt / t0 of the create, K steps.  A's old rows equal C and its new rows D in every array
    the sim hands back -- fuel burnt too: the old keep their sum, the new count from the create."""
    m = sum(groups)
    sc = scene(n, m, 101 + n + m, far=True)
    a = guided(sc['old'], sc['tidx'][:n], sc['mass'][:n], sc['rt_old'], sc, ctx)
    a.step(K)
    at = a.read_fms()
    fuel_k = a.read_forces()['fuel_used']
    for state, kw in parts(sc, groups):
        a.create(state, **kw)
    assert a.ctx.n == n + m
    mid = snapshot(a)
    assert mid['fms']['ticks'] == at['ticks'] and mid['fms']['simt'] == at['simt'] and mid['fms']['t0'] == at['t0']
    assert np.array_equal(mid['forces']['fuel_used'][:n], fuel_k) and fuel_k.max() > 0      # not reset
    assert not mid['forces']['fuel_used'][n:].any() and not mid['phase'][n:].any()
    for k in ('cd0', 'drag', 'thrustratio', 'thrust', 'fuelflow', 'bank'):
        assert not mid['forces'][k][n:].any(), k
    for k in FMS_STATE:                                                                      # as handed in
        assert np.array_equal(mid['fms'][k][n:], np.asarray(sc['rt_new'][3][k]), equal_nan=True), k
    a.step(K)
    got = snapshot(a)
    assert got['fms']['ticks'] == 22 and len(got['read']['lat']) == n + m
    c = guided(sc['old'], sc['tidx'][:n], sc['mass'][:n], sc['rt_old'], sc, ctx)
    c.step(2 * K)
    exp_old = snapshot(c)
    alone = (sc['new'], sc['tidx'][n:], sc['mass'][n:], sc['rt_new'])
    d = guided(*(alone if m > 1 else with_decoys(sc)), sc, ctx, simt=at['simt'], t0=at['t0'])
    d.step(K)
    assert d.stats()['n_conf'] > 0
    exp_new = take(snapshot(d), slice(0, m))
    rows_equal(got, exp_old, slice(0, n), 'old rows')
    rows_equal(got, exp_new, slice(n, n + m), 'new rows')
    assert exp_old['fms']['ticks'] == 22 and got['fms']['simt'] == exp_old['fms']['simt'] == exp_new['fms']['simt']
    assert got['fms']['t0'] == exp_old['fms']['t0'] == exp_new['fms']['t0']
    assert (got['fms']['iactwp'][:n] > 0).any()
    assert m == 1 or got['forces']['fuel_used'][n:].max() > 0       # (a lone aircraft may be a rotor: no fuel flow)
    assert c.stats()['n_conf'] > 0                     # resolution and recovery had work to do


def workaround(b, sc, state, tidx, mass, rt, gone=()):
    """What the refusal of plain create tells the caller to do, on sim b: read back, switch the stages off,
    (delete ``gone``,) create, set the stages again with the concatenated arrays and the read-back clock.
    ``tidx / mass / rt``: the arrays of the aircraft in the sim now; returns them for the sim after it."""
    f = b.read_fms()
    b.set_fms(None)
    b.set_forces(None)
    b.set_perf(None)
    keep = np.ones(b.ctx.n, bool)
    keep[list(gone)] = False
    if len(gone):
        b.delete(list(gone))
    b.create(state[0])
    rows, off, cnt = fms.append_routes(rt[0], rt[1][keep], rt[2][keep], *state[1]['fms'][:3])
    st = {k: np.concatenate([np.asarray(f[k])[keep], np.asarray(state[1]['fms'][3][k])]) for k in FMS_STATE}
    tidx = np.concatenate([tidx[keep], state[1]['perf']])
    mass = np.concatenate([mass[keep], state[1]['mass']])
    b.set_perf(sc['table'], tidx)
    b.set_forces(sc['ftable'], mass)
    b.set_fms(rows, off, cnt, st, simt=f['simt'], t0=f['t0'])
    b.set_recovery(True)
    return tidx, mass, (rows, off, cnt)


def same_flight(a, b, new, ticks_a0, what, stepped=True):
    """A and B agree bitwise in read(), the read_fms() fields and the phase; in the fuel burnt and the tick
    count for what happened since the create (B's set_forces / set_fms zero the rest by design).  The phase
    is the last step's output, which B's set_perf zeroes too: compared once a step has written it."""
    ga, gb = snapshot(a), snapshot(b)
    for k, v in gb['read'].items():
        assert np.array_equal(ga['read'][k], v, equal_nan=True), '%s read %s' % (what, k)
    for k in FMS_FIELDS:
        assert np.array_equal(ga['fms'][k], gb['fms'][k], equal_nan=True), '%s read_fms %s' % (what, k)
    assert (not stepped or np.array_equal(ga['phase'], gb['phase'])) and np.array_equal(ga['ax'], gb['ax']), what
    assert np.array_equal(ga['forces']['fuel_used'][new], gb['forces']['fuel_used'][new]), what
    assert ga['fms']['ticks'] - ticks_a0 == gb['fms']['ticks'], what
    assert ga['fms']['simt'] == gb['fms']['simt'] and ga['fms']['t0'] == gb['fms']['t0'], what
    return ga


@pytest.mark.parametrize('n,groups', SHAPES)
def test_interacting_traffic_equals_the_workaround(ctx, second, n, groups):
    """New aircraft among the old ones, resolution on.  A creates in place; B does at the same step what the
    refusal message prescribes.  Step by step for K more steps the two agree."""
    m = sum(groups)
    sc = scene(n, m, 211 + n + m, far=False)
    a = guided(sc['old'], sc['tidx'][:n], sc['mass'][:n], sc['rt_old'], sc, ctx)
    b = guided(sc['old'], sc['tidx'][:n], sc['mass'][:n], sc['rt_old'], sc, second)
    a.step(K)
    b.step(K)
    ticks0 = a.read_fms()['ticks']
    tidx, mass, rt = sc['tidx'][:n], sc['mass'][:n], sc['rt_old'][:3]
    for state in parts(sc, groups):
        a.create(state[0], **state[1])
        tidx, mass, rt = workaround(b, sc, state, tidx, mass, rt)
    new = slice(n, n + m)
    same_flight(a, b, new, ticks0, 'after the create', stepped=False)
    active = False
    for s in range(K):
        a.step(1)
        b.step(1)
        ga = same_flight(a, b, new, ticks0, 'step %d' % s)
        active = active or bool(ga['read']['active'][new].any())
    assert active and a.stats()['n_conf'] > 0 and ga['fms']['ticks'] == 22
    assert ga['forces']['fuel_used'][new].max() > 0 and len(ga['read']['lat']) == n + m


def test_create_then_delete_across_old_and_new(ctx, second):
    """700 + 37 + 37, then aircraft of the old set, of the first and of the second created group leave
    (the first and the last index among them), then K steps: as a sim that was given the surviving set by
    the workaround."""
    n, groups = 700, (37, 37)
    sc = scene(n, 74, 307, far=False)
    a = guided(sc['old'], sc['tidx'][:n], sc['mass'][:n], sc['rt_old'], sc, ctx)
    b = guided(sc['old'], sc['tidx'][:n], sc['mass'][:n], sc['rt_old'], sc, second)
    a.step(K)
    b.step(K)
    ticks0 = a.read_fms()['ticks']
    for state, kw in parts(sc, groups):
        a.create(state, **kw)
    gone = np.array([0, 5, 511, 512, 699, 700, 701, 736, 737, 750, 773])
    before = snapshot(a)
    a.delete(gone)
    after = snapshot(a)
    for k in FMS_FIELDS:                                    # the survivors keep everything, in order
        assert np.array_equal(after['fms'][k], np.delete(before['fms'][k], gone), equal_nan=True), k
    assert np.array_equal(after['forces']['fuel_used'], np.delete(before['forces']['fuel_used'], gone))
    # B: the old ones that leave are deleted inside the workaround, the new ones that leave never arrive
    stay = np.setdiff1d(np.arange(74), gone[gone >= n] - n)
    state, kw = part(sc, 0, 74)
    rows, off, cnt, st = kw['fms']
    kw = dict(perf=kw['perf'][stay], mass=kw['mass'][stay],
              fms=(rows, off[stay], cnt[stay], {k: np.asarray(v)[stay] for k, v in st.items()}))
    workaround(b, sc, ({k: v[stay] for k, v in state.items()}, kw), sc['tidx'][:n], sc['mass'][:n], sc['rt_old'][:3],
               gone=gone[gone < n])
    nold = n - int((gone < n).sum())
    new = slice(nold, nold + len(stay))
    assert a.ctx.n == b.ctx.n == nold + len(stay) == 763
    same_flight(a, b, new, ticks0, 'after the delete', stepped=False)
    a.step(K)
    b.step(K)
    ga = same_flight(a, b, new, ticks0, 'after %d steps' % K)
    assert (ga['fms']['iactwp'] > after['fms']['iactwp']).any() and ga['forces']['fuel_used'][new].max() > 0


def test_refusals_change_nothing(ctx):
    """Every refusal comes from the host's validation, in front of the first launch or copy: read(),
    read_fms() and read_forces() are bitwise what they were."""
    n, m = 500, 40
    sc = scene(n, m, 401, far=False)
    sim = guided(sc['old'], sc['tidx'][:n], sc['mass'][:n], sc['rt_old'], sc, ctx)
    sim.step(3)
    before = snapshot(sim)
    state, kw = part(sc, 0, m)
    rows, off, cnt, st = kw['fms']
    env = {k: np.full(m, v) for k, v in dict(hmax=2e4, vmin=50., vmax=300., vsmin=-20., vsmax=20., axmax=1.).items()}
    late = int(np.argmax(off))                              # the aircraft whose route ends the table
    past = dict(st, iactwp=np.where(np.arange(m) == 7, cnt, st['iactwp']))
    flag = dict(st, swvnav=np.where(np.arange(m) == 3, 2, np.asarray(st['swvnav']).astype(np.uint8)))
    cases = [
        (RuntimeError, dict(perf=kw['perf'], mass=kw['mass'])),                          # no part for the guidance
        (RuntimeError, dict(perf=kw['perf'], fms=kw['fms'])),                            # ... the forces
        (RuntimeError, dict(mass=kw['mass'], fms=kw['fms'])),                            # ... OpenAP
        (RuntimeError, dict(kw, limits=env)),                                            # a part for a stage that is off
        (RuntimeError, dict(kw, perf=np.where(np.arange(m) == m - 1, len(sc['table']), kw['perf']))),
        (RuntimeError, dict(kw, perf=np.where(np.arange(m) == 0, -1, kw['perf']))),
        (RuntimeError, dict(kw, fms=(rows[:-1], off, cnt, st))),                         # rt_off + rt_n > nrows
        (RuntimeError, dict(kw, fms=(rows, np.where(np.arange(m) == late, off + 1, off), cnt, st))),
        (RuntimeError, dict(kw, fms=(rows, off, cnt, past))),                            # iactwp == rt_n
        (RuntimeError, dict(kw, fms=(rows, off, cnt, dict(st, iactwp=np.full(m, -1))))),
        (RuntimeError, dict(kw, fms=(rows, off, np.zeros(m, np.int32), st))),            # LNAV on without a route
        (RuntimeError, dict(kw, fms=(rows, off, cnt, flag))),                            # a flag that is neither 0 nor 1
        (ValueError, dict(kw, mass=kw['mass'][:-1])),                                    # lengths
        (ValueError, dict(kw, perf=kw['perf'][:-1])),
        (ValueError, dict(kw, fms=(rows, off[:-1], cnt, st))),
        (ValueError, dict(kw, fms=(rows, off, cnt, dict(st, selspd=st['selspd'][:-1])))),
        (ValueError, dict(kw, fms=(rows[:, :7], off, cnt, st))),
        (ValueError, dict(kw, perf=kw['perf'].astype(np.float64))),                      # dtypes that would be truncated
        (ValueError, dict(kw, fms=(rows, off.astype(np.float64), cnt, st))),
    ]
    for k, (err, bad) in enumerate(cases):
        with pytest.raises(err):
            sim.create(state, **bad)
        assert sim.ctx.n == n, k
        now = snapshot(sim)
        rows_equal(now, before, slice(0, n), 'refusal %d' % k)
        assert now['fms']['ticks'] == before['fms']['ticks'] and now['fms']['simt'] == before['fms']['simt'], k
    with pytest.raises(ValueError):
        sim.create({k: (v[:-1] if k == 'alt' else v) for k, v in state.items()}, **kw)
    sim.create(state, **kw)                                 # ... and the sim still takes a good one
    sim.step(2)
    assert sim.ctx.n == n + m and len(sim.read()['lat']) == n + m


def test_plain_create_still_refused(ctx):
    """bsa_sim_create keeps its refusals: the two entries are not one."""
    n, m = 500, 40
    sc = scene(n, m, 503, far=False)
    sim = resident.ResidentSim(sc['old'], params(), ctx=ctx)
    sim.set_perf(sc['table'], sc['tidx'][:n])
    with pytest.raises(RuntimeError, match='OpenAP limits on'):
        sim.create(sc['new'])
    with pytest.raises(RuntimeError, match='OpenAP limits on'):
        sim.ctx.sim_create(sc['new'])
    sim.set_perf(None)
    sim.set_fms(*sc['rt_old'])
    with pytest.raises(RuntimeError, match='autopilot guidance on'):
        sim.create(sc['new'])
    state, kw = part(sc, 0, m)
    with pytest.raises(RuntimeError):
        sim.create(state, **kw)                             # perf and forces are off now: their parts are refused
    sim.create(state, fms=kw['fms'])
    sim.set_fms(None)
    sim.create(sc['new'])                                   # every stage off: plain create, as ever
    with pytest.raises(RuntimeError):
        sim.create(state, fms=kw['fms'])
    assert sim.ctx.n == n + 2 * m
    sim.step(1)


def test_envelope_rows_follow_the_create(ctx, second):
    """bsa_sim_set_limits on (no OpenAP): the six envelope arrays of the new aircraft, against switching the
    limits off, creating and setting the concatenated envelope -- 500 + 40, narrow limits that bind."""
    n, m = 500, 40
    sc = scene(n, m, 601, far=False)
    rng = np.random.default_rng(601)
    env = dict(hmax=rng.uniform(3000., 12000., n + m), vmin=rng.uniform(60., 120., n + m), vmax=rng.uniform(150., 260., n + m),
               vsmin=rng.uniform(-15., -2., n + m), vsmax=rng.uniform(2., 15., n + m), axmax=rng.uniform(0.3, 2.0, n + m))
    cut = lambda a, b: {k: v[a:b] for k, v in env.items()}
    a = resident.ResidentSim(sc['old'], params(), ctx=ctx, limits=cut(0, n))
    b = resident.ResidentSim(sc['old'], params(), ctx=second, limits=cut(0, n))
    a.step(5)
    b.step(5)
    with pytest.raises(RuntimeError):
        a.create(sc['new'])
    with pytest.raises(RuntimeError):
        a.create(sc['new'], limits=cut(n, n + m), perf=sc['tidx'][n:])      # OpenAP is off
    with pytest.raises(ValueError):
        a.create(sc['new'], limits=cut(n, n + m - 1))
    a.create(sc['new'], limits=cut(n, n + m))
    b.ctx.sim_set_limits(None)
    b.create(sc['new'])
    b.ctx.sim_set_limits(env)
    for s in range(5):
        a.step(1)
        b.step(1)
        ga, gb = a.read(), b.read()
        for k in gb:
            assert np.array_equal(ga[k], gb[k], equal_nan=True), 'step %d %s' % (s, k)
    assert not np.array_equal(ga['tas'][n:], sc['new']['tas'])
