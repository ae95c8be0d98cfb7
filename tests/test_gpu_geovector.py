"""GPU: geovectoring on the device (bsa_geovec_apply, bluesky_amd.geovector, and the resident
step's stage bsa_sim_set_geovectors) against tests/golden/geovec_apply.npz, the reference plugin's
own results, and against tests/geovec_np.py composed with fms_np and oracle/step.py.

ap_trk, selvs and selalt are copies of bounds or one fp64 addition: exact.  selspd is vtas2cas (two
pow calls): WHICH aircraft changed is exact -- the golden keeps every random selspd 1e-6 relative
away from a clamp value and holds the exactly-equal rows -- the values within util.close's 1e-9
rule.  Untouched aircraft keep their bits in all four arrays."""
import os
import types

import numpy as np
import pytest

from bluesky_amd import _lib, areafilter, fms, geovector, resident, synth
from oracle import statebased as ocd
from oracle import step as ostep
from tests import fms_np, geovec_np, util
from tests.fms_cases import compare
from tests.test_gpu_multirank import run_ranks
from tests.test_gpu_sim import SCALES, full_state, oracle_params

pytestmark = pytest.mark.gpu

T = geovec_np.TARGETS


@pytest.fixture(scope='module')
def golden():
    g = dict(np.load(os.path.join(util.GOLDEN, 'geovec_apply.npz')))
    return dict(g=g, lists=geovec_np.load_lists(g), areas=geovec_np.load_areas(g), names=[str(x) for x in g['list_names']])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_against(got, changed, st, exp, what):
    """got / exp: dicts of the four arrays; st: the input"""
    for k in ('ap_trk', 'selvs', 'selalt'):
        assert np.array_equal(bits(got[k]), bits(exp[k])), '%s %s' % (what, k)
    cnt_e, me = geovec_np.changed(st, exp)
    cnt_g, mg = geovec_np.changed(st, got)
    assert np.array_equal(mg['selspd'], me['selspd']), '%s: which selspd changed' % what
    ok, msg = util.close(got['selspd'], exp['selspd'], 100.0)
    assert ok, '%s selspd: %s' % (what, msg)
    assert np.array_equal(bits(got['selspd'])[~me['selspd']], bits(st['selspd'])[~me['selspd']]), '%s: untouched selspd' % what
    assert np.array_equal(changed, cnt_e) and np.array_equal(cnt_g, cnt_e), '%s: changed %s, expected %s' % (what, changed, cnt_e)


@pytest.mark.parametrize('n', [1000, 1, 63, 64, 65, 257])
def test_standalone_apply_matches_golden(ctx, golden, n):
    """Every golden list on a prefix of the golden (a prefix's golden is the golden's prefix: one lane
    per aircraft), cull on and off."""
    g = golden['g']
    st = geovec_np.load_state(g, n)
    keep = {k: v.copy() for k, v in st.items()}
    args = [st[k] for k in ('lat', 'lon', 'alt', 'trk', 'vs') + T]
    for q, name in enumerate(golden['names']):
        exp = {k: g['out_' + k][q][:n] for k in T}
        got, changed = geovector.apply_arrays(golden['lists'][name], golden['areas'], *args, ctx=ctx)
        check_against(got, changed, st, exp, '%s n=%d' % (name, n))
        if n == 1000:
            assert np.array_equal(changed, g['changed'][q]), name
        raw, changed_raw = geovector.apply_arrays(golden['lists'][name], golden['areas'], *args, ctx=ctx, nocull=True)
        for k in T:
            assert np.array_equal(bits(raw[k]), bits(got[k])), '%s n=%d %s: cull on / off' % (name, n, k)
        assert np.array_equal(changed_raw, changed)
    for k in st:                                     # the caller's arrays stay as they were
        assert np.array_equal(bits(st[k]), bits(keep[k])), k


def test_dropin_writes_the_traffic_object_in_place(ctx, golden):
    g = golden['g']
    st = geovec_np.load_state(g)
    q = golden['names'].index('three_areas')
    traf = types.SimpleNamespace(ntraf=len(st['lat']), ap=types.SimpleNamespace(trk=st['ap_trk'].copy()),
                                 **{k: st[k].copy() for k in ('lat', 'lon', 'alt', 'trk', 'vs', 'selspd', 'selvs', 'selalt')})
    holders = dict(selspd=traf.selspd, ap_trk=traf.ap.trk, selvs=traf.selvs, selalt=traf.selalt)
    areafilter.reset()
    geovector.reset()
    try:
        for name, (typ, co, top, bottom) in golden['areas'].items():
            areafilter.defineArea(name, typ, co, top, bottom)
        for vec in golden['lists']['three_areas']:
            assert geovector.defgeovec(*vec) is True
        assert geovector.defgeovec('NOSUCH', 100., 120.) is True      # skipped at apply time
        geovector.applygeovec(traf, ctx=ctx)
    finally:
        areafilter.reset()
        geovector.reset()
    got = dict(selspd=traf.selspd, ap_trk=traf.ap.trk, selvs=traf.selvs, selalt=traf.selalt)
    assert all(got[k] is holders[k] for k in T)                        # written in place
    cnt, _ = geovec_np.changed(st, got)
    check_against(got, cnt, st, {k: g['out_' + k][q] for k in T}, 'drop-in')
    for k in ('lat', 'lon', 'alt', 'trk', 'vs'):
        assert np.array_equal(bits(getattr(traf, k)), bits(st[k])), k


def test_standalone_refusals_launch_nothing(ctx, golden):
    g = golden['g']
    st = geovec_np.load_state(g, 64)
    areas = list(golden['areas'].values())
    args = [st[k] for k in ('lat', 'lon', 'alt', 'trk', 'vs') + T]
    ok = (0, _lib.GEOVEC_GSMAX, 0., 150., 0., 0., 0., 0.)
    for bad, match in [((len(areas), _lib.GEOVEC_GSMAX, 0., 150., 0., 0., 0., 0.), 'names shape'),
                       ((-1, _lib.GEOVEC_GSMAX, 0., 150., 0., 0., 0., 0.), 'names shape'),
                       ((0, 32, 0., 150., 0., 0., 0., 0.), 'unknown given'),
                       ((0, _lib.GEOVEC_GSMIN, 0., 150., 0., 0., 0., 0.), 'gsmin is given and exactly 0'),
                       ((0, _lib.GEOVEC_TRK, 0., 0., 0., 90., 0., 0.), 'trkmin is given and exactly 0'),
                       ((0, _lib.GEOVEC_TRK, 0., 0., 350., -0., 0., 0.), 'trkmax is given and exactly 0'),
                       ((0, _lib.GEOVEC_VSMAX, 0., 0., 0., 0., 0., 0.), 'vsmax is given and exactly 0')]:
        with pytest.raises(_lib.AccelError, match=match):
            ctx.geovec_apply(areas, [ok, bad], *args)
    with pytest.raises(_lib.AccelError, match='at most'):
        ctx.geovec_apply(areas, [ok] * (_lib.GEOVEC_MAX + 1), *args)
    with pytest.raises(_lib.AccelError, match='unknown type'):
        _bad_table(ctx, args)
    with pytest.raises(ValueError):
        ctx.geovec_apply(areas, [ok], *(args[:8] + [st['selalt'][:63]]))
    # an off bound may hold anything, 0 included; and the context still works
    got, changed = ctx.geovec_apply(areas, [(0, _lib.GEOVEC_GSMAX, 0., 120., 0., 0., 0., 0.)], *args)
    q = golden['names'].index('gsmax_only')
    assert list(golden['areas'])[0] == 'BOXSWAP'
    check_against(got, changed, st, {k: g['out_' + k][q][:64] for k in T}, 'after the refusals')
    empty, changed = ctx.geovec_apply(areas, [], *args)
    assert changed.sum() == 0 and all(np.array_equal(bits(empty[k]), bits(st[k])) for k in T)


def _bad_table(ctx, args):
    """a shape of an unknown type: the area table's own check, before any launch"""
    tab, verts = _lib.area_table([('BOX', (51., 3., 53., 5.), 1e9, -1e9)])
    tab[0].type = 9
    gv, m = _lib.geovec_rows([(0, _lib.GEOVEC_GSMAX, 0., 150., 0., 0., 0., 0.)])
    io = [np.array(a) for a in args[5:]]
    ctx.check(ctx.lib.bsa_geovec_apply(ctx.h, 64, *[_lib.ptr(a) for a in args[:5]], 1, tab, 0, None, m, gv, 0,
                                       *[_lib.ptr(a) for a in io], None), 'bsa_geovec_apply')


# ---------------------------------------------------------------- the resident step
SIMDT, EVERY, STEPS = 0.05, 4, 45
GEOVECS = [['BOXSWAP', 150., 210., 100., 200., -5., 5.], ['CIRC', None, 140., 350., 30., None, 3.],
           ['SEAM', 120., None, None, None, -2., None]]
SIM_AREAS = ('BOXSWAP', 'CIRC', 'SEAM')


def traffic(n, seed, spread):
    init = resident.initial_state(synth.box(n, spread, seed=seed))
    return init, fms.synthetic_routes(init, seed=seed)


def gv_sim(init, rt, p, ctx, areas, geovecs=GEOVECS, every=EVERY, simt=0.0, t0=-999., **kw):
    sim = resident.ResidentSim(init, p, ctx=ctx, **kw)
    sim.set_fms(*rt, simt=simt, t0=t0)
    sim.set_areas({k: areas[k] for k in SIM_AREAS})
    sim.set_geovectors(geovecs, every)
    return sim


def same(a, b, what):
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), '%s: %s' % (what, k)


def read_all(sim):
    return sim.read_fms(), sim.read(), sim.geovector_stats()


def test_resident_step_follows_the_composed_oracle(ctx, golden):
    """45 steps, re-anchored every step: geovec_np.apply on the applying steps (4, 8, ... 44: the first
    one interval after set_geovectors), then fms_np.update, then oracle/step.py.  The ap_tas of an
    applying step already comes from the clamped selspd."""
    n = 300
    areas = golden['areas']
    init, rt = traffic(n, 31, 150.0)
    rows, off, cnt, st = rt
    p = resident.params(simdt=SIMDT, cd_every=8)
    op = oracle_params(p)
    sim = gv_sim(init, rt, p, ctx, areas)
    sched, _, _ = fms.tick_schedule(0.0, p.simdt, STEPS)
    prev = dict(init, **st)
    prev.update(asas_trk=init['trk'].copy(), asas_tas=init['tas'].copy(), asas_vs=np.zeros(n), active=np.zeros(n, bool),
                ax=np.zeros(n))
    applied, clamped_tas, real_spd, touched = 0, 0, 0, np.zeros(4, dtype=np.int64)
    for k in range(STEPS):
        pre = dict(prev)
        if k > 0 and k % EVERY == 0:
            out = geovec_np.apply(GEOVECS, areas, prev)
            touched += geovec_np.changed(prev, out)[0].astype(np.int64)
            # a level aircraft clamped before sits exactly on the device's clamp value, where this numpy's pow may
            # say one ulp more: not a change on the device
            real_spd += int((np.abs(out['selspd'] - prev['selspd']) > 1e-7).sum())
            pre.update(out)
            applied += 1
        skip = fms_np.near_threshold(pre, rows, off, cnt, tick=bool(sched[k]))
        assert skip.sum() <= 0.001 * n
        exp = fms_np.update(pre, rows, off, cnt, tick=bool(sched[k]))
        if pre is not prev and k % EVERY == 0 and k > 0:
            plain = fms_np.update(prev, rows, off, cnt, tick=bool(sched[k]))
            clamped_tas += int((plain['ap_tas'] != exp['ap_tas']).sum())
        ost = ostep.sim_step({q: exp[q] for q in exp if q not in fms_np.REALS + fms_np.FLAGS + ('iactwp',)}, op,
                             do_cd=(k % p.cd_every == 0))
        sim.step(1)
        got, tr = sim.read_fms(), sim.read()
        compare(got, {'out_' + q: exp[q] for q in fms_np.OUTPUTS}, skip=skip, what='step %d ' % k)
        assert np.array_equal(bits(got['selvs']), bits(pre['selvs'])), 'step %d selvs' % k
        for q, scale in SCALES.items():
            ok, msg = util.close(tr[q][~skip], ost[q][~skip], scale)
            assert ok, 'step %d traffic %s: %s' % (k, q, msg)
        prev = full_state(dict(init, **got), tr)
        ax = np.zeros(n)
        sim.ctx.check(sim.ctx.lib.bsa_sim_read_perf(sim.ctx.h, None, _lib.ptr(ax)), 'bsa_sim_read_perf')
        prev['ax'] = ax
    stats = sim.geovector_stats()
    assert applied == 11 and stats['applies'] == 11
    assert clamped_tas > 20 and (touched > 20).all()
    assert stats['changed'] == dict(selspd=real_spd, ap_trk=touched[1], selvs=touched[2], selalt=touched[3])
    assert real_spd > 20


def test_one_batch_equals_single_steps(ctx, golden):
    init, rt = traffic(300, 37, 150.0)
    p = resident.params(simdt=SIMDT, cd_every=4)
    a = gv_sim(init, rt, p, ctx, golden['areas'])
    a.step(STEPS)
    ea = read_all(a)
    b = gv_sim(init, rt, p, ctx, golden['areas'])
    for _ in range(STEPS):
        b.step(1)
    eb = read_all(b)
    same(eb[0], ea[0], '45 x step(1)')
    same(eb[1], ea[1], '45 x step(1)')
    assert eb[2] == ea[2] and ea[2]['applies'] == 11 and min(ea[2]['changed'].values()) > 0
    # ... and differs from a run without geovectors
    off = gv_sim(init, rt, p, ctx, golden['areas'], geovecs=[])
    off.step(STEPS)
    assert not np.array_equal(off.read()['hdg'], ea[1]['hdg'])


@pytest.mark.parametrize('case', ['applying_tick', 'applying_no_tick', 'after_applied'])
def test_forced_abort_is_exact(ctx, golden, case):
    """K2 row buckets one pair wide from a given step on: the next CD step with a two-pair row aborts and
    re-runs.  applying_tick: step 4 applies and is an FMS tick (FMS undo set, then the geovector one);
    applying_no_tick: from simt 5 step 4 applies and does not tick; after_applied: CD every 5th step, step 5
    aborts right after step 4 applied -- the undo set holds step 4's start and must be left alone."""
    simt, t0 = (5.0, 4.5) if case == 'applying_no_tick' else (0.0, -999.)
    cd_every = 5 if case == 'after_applied' else 4
    first, rest = cd_every, 8
    init, rt = traffic(600, 43, 40.0)
    p = resident.params(simdt=SIMDT, cd_every=cd_every)
    sched = fms.tick_schedule(simt, SIMDT, first + 1, t0)[0]
    assert bool(sched[first]) == (case != 'applying_no_tick')
    ref = gv_sim(init, rt, p, ctx, golden['areas'], simt=simt, t0=t0)
    ref.step(first)
    s = ref.read()
    pairs = ocd.detect_arrays(*[synth.Traffic(s['lat'], s['lon'], s['alt'], s['trk'], s['gs'], s['vs'])] * 2, p.rpz, p.hpz, p.tla)
    assert np.bincount(pairs['ci']).max() >= 2         # a row of two pairs: the aborting CD step has one
    ref.step(rest)
    exp = read_all(ref)
    c = _lib.Context(0)
    try:
        sim = gv_sim(init, rt, p, c, golden['areas'], simt=simt, t0=t0)
        sim.step(first)
        c.set_row_bucket(1)
        sim.step(rest)
        got = read_all(sim)
        same(got[0], exp[0], 'after the re-run')
        same(got[1], exp[1], 'after the re-run')
        assert got[2] == exp[2] and exp[2]['applies'] == (first + rest - 1) // EVERY
        assert sim.stats() == ref.stats()
    finally:
        c.close()
    assert min(exp[2]['changed'].values()) > 0


def test_two_ranks_equal_one(ctx, golden):
    n = 600
    init, rt = traffic(n, 47, 60.0)
    p = resident.params(simdt=SIMDT, cd_every=4)
    one = gv_sim(init, rt, p, ctx, golden['areas'])
    one.step(10)
    one.step(15)
    exp, exp_tr, exp_st = read_all(one)

    def rank(r, c, g):
        sim = gv_sim(init, rt, p, c, golden['areas'], rank=r, world=2, group=g)
        sim.step(10)
        sim.step(15)
        return sim.read_fms(), sim.read(), sim.geovector_stats(), sim.row_ids()

    res = run_ranks(2, rank)
    assert np.array_equal(np.sort(np.concatenate([r[3] for r in res])), np.arange(n))
    for k in fms_np.OUTPUTS + ('selvs',):
        full = np.zeros(n, dtype=np.asarray(exp[k]).dtype)
        for got, _, _, ids in res:
            full[ids] = got[k][ids]
        assert np.array_equal(full, exp[k], equal_nan=True), k
    for k in ('lat', 'lon', 'alt', 'hdg', 'tas', 'vs'):
        assert np.array_equal(res[0][1][k], exp_tr[k]), k
    assert all(r[2]['applies'] == exp_st['applies'] == 6 for r in res)
    for k in T:
        assert sum(r[2]['changed'][k] for r in res) == exp_st['changed'][k] > 0, k


def test_refusals_and_switches(ctx, golden):
    areas = golden['areas']
    init, rt = traffic(300, 53, 150.0)
    p = resident.params(simdt=SIMDT, cd_every=4)
    plain = resident.ResidentSim(init, p, ctx=ctx)
    plain.set_fms(*rt)
    plain.step(12)
    exp_fms, exp_tr = plain.read_fms(), plain.read()

    sim = resident.ResidentSim(init, p, ctx=ctx)
    with pytest.raises(_lib.AccelError, match='no geovectors'):
        sim.geovector_stats()
    sim.set_fms(*rt)
    with pytest.raises(_lib.AccelError, match='no areas'):           # guidance, no areas
        sim.ctx.sim_set_geovectors([(0, _lib.GEOVEC_GSMAX, 0., 150., 0., 0., 0., 0.)], 1)
    sim.set_fms(None)
    sim.set_areas({k: areas[k] for k in SIM_AREAS})
    with pytest.raises(_lib.AccelError, match='FMS guidance'):       # areas, no guidance
        sim.set_geovectors(GEOVECS, EVERY)
    sim.set_fms(*rt)
    with pytest.raises(_lib.AccelError, match='every'):
        sim.set_geovectors(GEOVECS, 0)
    with pytest.raises(_lib.AccelError, match='names shape'):        # a shape index out of range
        sim.ctx.sim_set_geovectors([(len(SIM_AREAS), _lib.GEOVEC_GSMAX, 0., 150., 0., 0., 0., 0.)], 1)
    with pytest.raises(_lib.AccelError, match='exactly 0'):          # a given bound equal to 0
        sim.ctx.sim_set_geovectors([(0, _lib.GEOVEC_VSMIN, 0., 0., 0., 0., 0., 0.)], 1)
    with pytest.raises(_lib.AccelError, match='no geovectors'):      # nothing of the refused calls stuck
        sim.geovector_stats()
    # set_areas forgets the geovectors
    sim.set_geovectors(GEOVECS, EVERY)
    assert sim.geovector_stats() == dict(applies=0, changed=dict.fromkeys(T, 0))
    sim.set_areas({k: areas[k] for k in SIM_AREAS})
    with pytest.raises(_lib.AccelError, match='no geovectors'):
        sim.geovector_stats()
    # set_fms(None) switches the stage off; switching the guidance on again does not bring it back
    sim.set_geovectors(GEOVECS, EVERY)
    sim.set_fms(None)
    with pytest.raises(_lib.AccelError, match='no geovectors'):
        sim.geovector_stats()
    sim.set_fms(*rt)
    with pytest.raises(_lib.AccelError, match='no geovectors'):
        sim.geovector_stats()
    # an empty list, and one whose areas are all unknown, is off: the steps are those of a sim that never had any
    sim.set_geovectors(GEOVECS, EVERY)
    sim.set_geovectors([['NOSUCH', 100., 120., None, None, None, None]], EVERY)
    with pytest.raises(_lib.AccelError, match='no geovectors'):
        sim.geovector_stats()
    sim.step(12)
    same(sim.read_fms(), exp_fms, 'geovectors off')
    same(sim.read(), exp_tr, 'geovectors off')
    # the cadence counts from set_geovectors, not from the sim's start
    sim.set_geovectors(GEOVECS, 3)
    sim.step(3)
    assert sim.geovector_stats()['applies'] == 0
    sim.step(1)
    assert sim.geovector_stats()['applies'] == 1
    sim.step(6)
    assert sim.geovector_stats()['applies'] == 3
