"""GPU: route edits on the device (bsa_route_edit, bsa_sim_route_edit; DESIGN.md
3.33) against tests/route_np.py.  Table: lat, lon, alt, spd, flyby, the waypoint
types, offsets and counts exactly; xtoalt, toalt, nextqdr and the FMS reals
within util.close's 1e-9 rule (the device's qdrdist is not numpy's bit for bit,
DESIGN.md 3.21); flags and iactwp exactly.  Aircraft whose ``direct`` holds a
comparison within 1e-9 relative of equality (route_np.near_threshold) are left
out: at most 1 % of a case's edited aircraft, asserted per case.  Counted on the
CPU with route_np alone for the seeds below: 0 excluded in every case.
"""
import numpy as np
import pytest

from bluesky_amd import fms, resident, synth
from tests import recover_np, route_np, util
from tests.recover_cases import compare

pytestmark = pytest.mark.gpu

I, O, D, X = fms.INSERT, fms.OVERWRITE, fms.DELETE, fms.DIRECT


def traffic(n, seed, nwp=4):
    """(init, (rows, off, n, fms state), standalone state) of n aircraft with nwp-waypoint routes."""
    init = resident.initial_state(synth.box(n, 60.0, seed=seed))
    rt = fms.synthetic_routes(init, seed=seed, nwp=nwp)
    st = dict(rt[3])
    st.update({k: np.array(init[k], dtype=np.float64) for k in recover_np.TRAFFIC})
    st['ap_alt'] = np.array(init['alt'], dtype=np.float64)
    return init, rt, st


def new_wp(rng, rt, k, **kw):
    """A record's waypoint near aircraft k's first waypoint, with mixed constraints."""
    rows, off = rt[0], rt[1]
    la, lo = (rows[off[k], 0], rows[off[k], 1]) if rt[2][k] else (52.0, 4.0)
    return dict(lat=la + rng.uniform(-0.2, 0.2), lon=lo + rng.uniform(-0.2, 0.2),
                alt=float(rng.choice([-999., 3000., 9000.])), spd=float(rng.choice([-999., 130., 0.7])),
                flyby=bool(rng.random() < 0.8), **kw)


def check(ctx, rt, st, recs, wptype=None, ops=None):
    rows, off, cnt = rt[0], rt[1], rt[2]
    exp = route_np.edit(st, rows, off, cnt, recs, wptype)
    with np.errstate(all='ignore'):
        skip = route_np.near_threshold(st, rows, off, cnt, recs, wptype)
    edited = np.unique([r['aircraft'] for r in recs])
    assert skip[edited].sum() <= 0.01 * len(edited), 'excluded %d of %d' % (skip[edited].sum(), len(edited))
    for op in set(r['op'] for r in recs):                       # never all aircraft of one op kind
        of = np.unique([r['aircraft'] for r in recs if r['op'] == op])
        assert not skip[of].all()
    got = fms.edit(rows, off, cnt, st, recs, wptype, ctx=ctx)
    table_equal(got[:4], exp[:4], skip)
    compare(dict(got[4]), exp[4], skip=skip)
    ok, msg = util.close(got[4]['actwp_next_qdr'][~skip], exp[4]['actwp_next_qdr'][~skip], 360.)
    assert ok, msg
    for k in route_np.UNTOUCHED:
        if k in got[4]:
            assert np.array_equal(got[4][k], st[k], equal_nan=True), k
    return got, exp


def table_equal(got, exp, skip=None, exact=False):
    grows, goff, gcnt, gtype = got
    erows, eoff, ecnt, etype = exp
    assert np.array_equal(goff, eoff) and np.array_equal(gcnt, ecnt) and np.array_equal(gtype, etype)
    keep = np.ones(len(erows), bool)
    for k in np.flatnonzero(skip) if skip is not None else []:
        keep[eoff[k]:eoff[k] + ecnt[k]] = False
    for col in (0, 1, 2, 3, 6):
        assert np.array_equal(grows[keep, col], erows[keep, col]), col
    for col, scale in ((4, None), (5, None), (7, 360.)):
        a, e = grows[keep, col], erows[keep, col]
        if exact:
            assert np.array_equal(a, e), col
            continue
        fin = np.abs(e[np.isfinite(e)])
        ok, msg = util.close(a, e, scale or (fin.max() if len(fin) and fin.max() > 0 else 1.0))
        assert ok, 'column %d: %s' % (col, msg)


def test_one_aircraft_one_waypoint_insert_at_0(ctx):
    _, rt, st = traffic(1, 3, nwp=1)
    rng = np.random.default_rng(1)
    got, _ = check(ctx, rt, st, [fms.record(0, I, 0, **new_wp(rng, rt, 0))])
    assert got[2][0] == 2


def test_empty_route_gets_its_first_waypoint_and_loses_its_only_one(ctx):
    _, rt, st = traffic(3, 4, nwp=1)
    rng = np.random.default_rng(2)
    # aircraft 1 starts without a route: LNAV off, iactwp -1 (Route.__init__)
    cnt = rt[2].copy()
    cnt[1] = 0
    st = dict(st, iactwp=np.array([0, -1, 0], np.int32), swlnav=np.array([True, False, True]))
    rt = (rt[0], rt[1], cnt, rt[3])
    got, _ = check(ctx, rt, st, [fms.record(1, I, 0, **new_wp(rng, rt, 1)), fms.record(2, D, 0)])
    assert list(got[2]) == [1, 1, 0] and got[4]['iactwp'][2] == -1 and not got[4]['swlnav'][2]
    assert got[4]['iactwp'][1] == -1                      # the reference leaves a first waypoint inactive


@pytest.mark.parametrize('nwp, ops', [(64, [I]), (65, [I, D, D]), (63, [I, I]), (130, [D, I, I])])
def test_chunk_edges(ctx, nwp, ops):
    """64 -> 65, 65 -> 66 -> 64, 63 -> 65 and a three-chunk route, edited at the front
    (every row moves), in the middle and at the end."""
    _, rt, st = traffic(3, 5, nwp=nwp)
    rng = np.random.default_rng(nwp)
    recs = []
    for k, where in enumerate(('front', 'mid', 'end')):
        n = nwp
        for op in ops:
            pos = {'front': 0, 'mid': n // 2, 'end': n if op == I else n - 1}[where]
            recs.append(fms.record(k, op, pos, **(new_wp(rng, rt, k) if op == I else {})))
            n += 1 if op == I else -1
    got, _ = check(ctx, rt, st, recs)
    assert got[2][0] == nwp + sum(1 if op == I else -1 for op in ops)


def mixed_batch(rt, st, rng, aircraft, per=(1, 2, 3)):
    """Inserts before / at / after the active waypoint with and without AFTER, overwrites,
    deletes and directs, up to three per aircraft, interleaved across the batch."""
    seqs = []
    for k in aircraft:
        n, out = int(rt[2][k]), []
        for _ in range(int(rng.choice(per))):
            op = int(rng.choice([I, I, O, D, X])) if n > 1 else I
            if op == I:
                pos = int(rng.integers(0, n + 1))
                out.append(fms.record(k, I, pos, bump_active=bool(rng.random() < 0.5), **new_wp(rng, rt, k)))
                n += 1
            elif op == O:
                out.append(fms.record(k, O, int(rng.integers(0, n)), **new_wp(rng, rt, k)))
            else:
                out.append(fms.record(k, op, int(rng.integers(0, n))))
                n -= op == D
        seqs.append(out)
    recs = []
    while any(seqs):                                     # round-robin: one aircraft's records are not adjacent
        for s in seqs:
            if s:
                recs.append(s.pop(0))
    return recs


def test_130_aircraft_3_edited_not_adjacent_in_the_batch(ctx):
    _, rt, st = traffic(130, 6)
    recs = mixed_batch(rt, st, np.random.default_rng(6), [5, 64, 129], per=(3,))
    assert recs[0]['aircraft'] != recs[1]['aircraft']
    got, exp = check(ctx, rt, st, recs)
    for k in set(range(130)) - {5, 64, 129}:             # untouched routes bitwise
        assert np.array_equal(got[0][got[1][k]:got[1][k] + got[2][k]], rt[0][rt[1][k]:rt[1][k] + rt[2][k]])


@pytest.mark.parametrize('seed', [11, 12])
def test_random_batches_every_op(ctx, seed):
    _, rt, st = traffic(300, seed)
    rng = np.random.default_rng(seed)
    st['iactwp'] = rng.integers(0, 4, 300).astype(np.int32)
    wptype = np.zeros(len(rt[0]), np.uint8)
    wptype[rt[1][::3] + 3] = fms.WP_DEST                  # every third route ends at a destination
    recs = mixed_batch(rt, st, rng, rng.choice(300, 200, replace=False))
    assert {r['op'] for r in recs} == {I, O, D, X}
    check(ctx, rt, st, recs, wptype)


def test_refusals_change_nothing(ctx):
    init, rt, st = traffic(20, 7)
    p = resident.params(simdt=1.0)
    sim = resident.ResidentSim(init, p, ctx=ctx)
    sim.set_fms(*rt)
    sim.step(3)
    wp = dict(lat=52., lon=4.)
    ok = fms.record(2, I, 1, **wp)
    bad = [(fms.record(3, I, 1, wptype=5, **wp), 4), (fms.record(3, O, 1, wptype=4, **wp), 4),
           (fms.record(3, I, 1, lat=np.nan, lon=4.), 5), (fms.record(3, I, 1, lat=52., lon=np.inf), 5),
           (fms.record(3, I, 6, **wp), 3), (fms.record(3, D, 4), 3), (fms.record(3, X, -1), 3),
           (fms.record(20, D, 0), 1), (fms.record(-1, D, 0), 1), (fms.record(3, 9, 0), 2)]
    for rec, code in bad:
        for batch in ([rec], [ok, rec]):                  # alone, and behind a record that is fine
            with pytest.raises(fms.RouteEditRefused) as e:
                sim.edit_routes(batch)
            assert e.value.code == code
            with pytest.raises(fms.RouteEditRefused) as e:
                fms.edit(rt[0], rt[1], rt[2], st, batch, ctx=ctx)
            assert e.value.code == code
    # pos is judged against the route the earlier records left: 4 waypoints, a delete, then pos 4 is past it
    with pytest.raises(fms.RouteEditRefused):
        sim.edit_routes([fms.record(3, D, 0), fms.record(3, I, 4, **wp)])
    sim.edit_routes([fms.record(3, I, 4, **wp), fms.record(3, D, 4)])   # ... and the other way round is fine
    after = (sim.read_routes(), sim.read_fms(), sim.route_stats())
    sim2 = resident.ResidentSim(init, p, ctx=ctx)
    sim2.set_fms(*rt)
    sim2.step(3)
    sim2.edit_routes([fms.record(3, I, 4, **wp), fms.record(3, D, 4)])
    ref = (sim2.read_routes(), sim2.read_fms(), sim2.route_stats())
    for a, b in zip(after[0], ref[0]):
        assert np.array_equal(a, b, equal_nan=True)
    for k in after[1]:
        assert np.array_equal(after[1][k], ref[1][k], equal_nan=True), k
    assert after[2] == ref[2]


def test_refused_batch_leaves_reads_bitwise(ctx):
    init, rt, st = traffic(20, 8)
    sim = resident.ResidentSim(init, resident.params(simdt=1.0), ctx=ctx)
    sim.set_fms(*rt)
    sim.edit_routes([fms.record(1, I, 0, lat=52., lon=4.)])
    before = (sim.read_routes(), sim.read_fms(), sim.route_stats())
    with pytest.raises(fms.RouteEditRefused):
        sim.edit_routes([fms.record(2, I, 0, lat=52., lon=4.), fms.record(1, D, 9)])
    after = (sim.read_routes(), sim.read_fms(), sim.route_stats())
    for a, b in zip(before[0], after[0]):
        assert np.array_equal(a, b, equal_nan=True)
    for k in before[1]:
        assert np.array_equal(before[1][k], after[1][k], equal_nan=True), k
    assert before[2] == after[2]


def test_resident_edit_equals_set_fms_with_its_own_table_bitwise(ctx):
    """A: set_fms, step, edit, step.  B: the same up to the edit, then set_fms with A's
    own read_routes / read_fms (clock carried), step.  Bitwise: nothing stale is left."""
    init, rt, st = traffic(200, 9)
    p = resident.params(simdt=1.0, rpz=1852.0, cd_every=1, resume_nav=True)
    rng = np.random.default_rng(9)

    def start():
        sim = resident.ResidentSim(init, p, ctx=ctx)
        sim.set_fms(*rt)
        sim.set_recovery()
        sim.step(7)
        return sim
    a = start()
    n_now = a.read_routes()[2]
    recs = mixed_batch((rt[0], rt[1], n_now, None), st, rng, rng.choice(200, 40, replace=False))
    a.edit_routes(recs)
    rows, off, cnt, _ = a.read_routes()
    f = a.read_fms()
    b = start()
    b.set_fms(rows, off, cnt, f, simt=f['simt'], t0=f['t0'])
    b.set_recovery()
    a.step(9), b.step(9)
    ra, rb = a.read(), b.read()
    for k in ra:
        assert np.array_equal(np.asarray(ra[k]), np.asarray(rb[k]), equal_nan=True), k
    fa, fb = a.read_fms(), b.read_fms()
    for k in fa:
        if k != 'ticks':                                   # (B's count restarts at its set_fms)
            assert np.array_equal(np.asarray(fa[k]), np.asarray(fb[k]), equal_nan=True), k
    for x, y in zip(a.read_routes(), b.read_routes()):
        assert np.array_equal(x, y, equal_nan=True)
    pa, pb = a.resopairs(), b.resopairs()
    assert len(pa) and np.array_equal(np.asarray(pa), np.asarray(pb))
    assert a.asas_stats() == b.asas_stats()


def test_work_count_regrow_and_one_compaction(ctx):
    """2 000 aircraft: ten single inserts write the ten new routes' rows, not the table;
    the table regrows behind its tail; batches of deletes cross dead > live exactly once."""
    init, rt, st = traffic(2000, 10)
    sim = resident.ResidentSim(init, resident.params(simdt=1.0), ctx=ctx)
    sim.set_fms(*rt)
    assert sim.route_stats() == dict(live=8000, dead=0, written=0, compactions=0)
    rng = np.random.default_rng(10)
    ten = rng.choice(2000, 10, replace=False)
    sim.edit_routes([fms.record(k, I, 2, **new_wp(rng, rt, k)) for k in ten])
    assert sim.route_stats() == dict(live=8010, dead=40, written=50, compactions=0)
    # every aircraft loses a waypoint per batch: live 8010 -> 6010 -> 4010, dead 40 -> 8040 > 6010: compacted
    dele = [fms.record(k, D, 0) for k in range(2000)]
    before = sim.read_routes()
    sim.edit_routes(dele)
    s = sim.route_stats()
    assert s['compactions'] == 1 and s['dead'] == 0 and s['live'] == 6010 and s['written'] == 6010
    after = sim.read_routes()
    assert np.array_equal(after[2], before[2] - 1)
    for k in (0, 1, 999, 1999, int(ten[0])):
        o0, o1, n1 = before[1][k], after[1][k], after[2][k]
        assert np.array_equal(after[0][o1:o1 + n1, :4], before[0][o0 + 1:o0 + 1 + n1, :4])
    sim.edit_routes(dele[:100])                            # the next batch does not compact again
    assert sim.route_stats()['compactions'] == 1
    sim.step(3)                                            # ... and the sim flies on the compacted table


def test_edit_then_delete_then_create_then_step(ctx):
    """edit -> delete(idx) -> create(fms=...) -> step equals a fresh sim built from the
    host's own table (RouteNames + append_routes)."""
    init, rt, st = traffic(60, 13)
    new_init, new_rt, _ = traffic(5, 14)
    p = resident.params(simdt=1.0)
    rng = np.random.default_rng(13)
    names = fms.RouteNames([['W%d' % i for i in range(4)] for _ in range(60)])
    recs = []
    for k in (3, 17, 59):
        recs += names.addwpt(k, 'NEW', 1, afterwp='W1', **{q: v for q, v in new_wp(rng, rt, k).items()})
    recs += names.delwpt(20, 'W3') + names.direct(41, 'W2') + names.addwpt(17, 'NEW', 1, lat=52.3, lon=4.1)
    assert names.names[17] == ['W0', 'W1', 'NEW', 'W2', 'W3', 'NEW01']
    sim = resident.ResidentSim(init, p, ctx=ctx)
    sim.set_fms(*rt)
    sim.edit_routes(recs)
    f0 = sim.read_fms()
    gone = [5, 17]
    sim.delete(gone)
    names.delete(gone)
    sim.create(new_init, fms=new_rt)
    names.create([['W%d' % i for i in range(4)] for _ in range(5)])
    assert len(names.names) == 63
    # the host's own table: the standalone edit, the deleted aircraft dropped, the new ones appended
    hrows, hoff, hcnt, _, hst = route_np.edit(st, rt[0], rt[1], rt[2], recs)
    keep = np.setdiff1d(np.arange(60), gone)
    rows, off, cnt = fms.append_routes(hrows, hoff[keep], hcnt[keep], new_rt[0], new_rt[1], new_rt[2])
    got = sim.read_routes()
    assert np.array_equal(got[2], cnt) and [len(r) for r in names.names] == list(cnt)
    for k in range(63):
        a, e = got[0][got[1][k]:got[1][k] + got[2][k]], rows[off[k]:off[k] + cnt[k]]
        assert np.array_equal(a[:, :4], e[:, :4]) and np.allclose(a, e, rtol=1e-9, atol=1e-6)
    fresh_init = {k: np.concatenate([np.asarray(init[k])[keep], np.asarray(new_init[k])]) for k in init}
    fst = {k: np.concatenate([np.asarray(f0[k])[keep], np.asarray(new_rt[3][k])]) for k in new_rt[3]}
    fresh = resident.ResidentSim(fresh_init, p, ctx=ctx)
    fresh.set_fms(got[0], got[1], got[2], fst)
    sim.step(5), fresh.step(5)
    ra, rb = sim.read(), fresh.read()
    for k in ('lat', 'lon', 'alt', 'tas', 'trk', 'vs'):
        ok, msg = util.close(np.asarray(ra[k]), np.asarray(rb[k]), max(1.0, np.abs(np.asarray(rb[k])).max()))
        assert ok, '%s: %s' % (k, msg)


# ---------------------------------------------------------------- the captured fixtures
from bluesky_amd import _lib                                                   # noqa: E402
from tests import route_cases                                                  # noqa: E402
from tests.test_gpu_multirank import run_ranks                                 # noqa: E402


@pytest.mark.parametrize('path', route_cases.FIXTURES, ids=lambda p: p.split('/')[-1])
def test_device_reproduces_the_reference_fixture(ctx, path):
    """bsa_route_edit on the commands the reference's own Route objects executed
    (tools/make_golden.py --route-edit), resolved by fms.RouteNames.  The fixture holds no
    comparison within 1e-9 relative of equality: no aircraft is excluded."""
    g, st, recs, table, exp = route_cases.load(path)
    resolved, _ = route_cases.resolve(g)
    assert np.array_equal(resolved, recs)
    got = fms.edit(g['route_rows'], g['rt_off'], g['rt_n'], st, resolved, g['wptype'], ctx=ctx)
    table_equal(got[:4], table)
    route_cases.compare_state(dict(got[4]), st, exp)


def test_refused_on_several_ranks_and_nothing_changes():
    init, rt, st = traffic(64, 15)
    p = resident.params(simdt=1.0)

    def rank(r, c, g):
        sim = resident.ResidentSim(init, p, ctx=c, rank=r, world=2, group=g)
        sim.set_fms(*rt)
        sim.step(2)
        before = sim.read_fms()
        codes = []
        for call in (lambda: sim.edit_routes([fms.record(3, D, 0)]), sim.read_routes, sim.route_stats):
            with pytest.raises(fms.RouteEditRefused) as e:
                call()
            codes.append(e.value.code)
        after = sim.read_fms()
        sim.step(2)
        return codes, before, after

    for codes, before, after in run_ranks(2, rank):
        assert codes == [6, 6, 6]
        for k in before:
            assert np.array_equal(before[k], after[k], equal_nan=True), k


def test_small_batch_tips_the_compaction_and_nothing_else_changes(ctx):
    """Batches of single inserts until dead rows are one short of the live ones, then one
    more record: that batch compacts (compactions 0 -> 1).  A twin with the same history
    whose table was uploaded again just before (no dead rows) applies the same last batch
    without compacting; read_routes, read_fms and the steps after are bitwise equal."""
    init, rt, st = traffic(50, 16)                         # 200 live rows
    p = resident.params(simdt=1.0, rpz=1852.0, cd_every=1, resume_nav=True)
    rng = np.random.default_rng(16)
    a = resident.ResidentSim(init, p, ctx=ctx)
    a.set_fms(*rt)
    a.step(3)
    # an insert into an n-waypoint route kills n rows and adds n + 1 live ones
    done = []
    while True:
        s = a.route_stats()
        k = int(rng.integers(0, 50))
        n = int(a.read_routes()[2][k])
        last = [fms.record(k, I, int(rng.integers(0, n + 1)), **new_wp(rng, rt, k))]
        if s['dead'] + n > s['live'] + 1:
            break
        a.edit_routes(last)
        done.append(last)
        assert a.route_stats()['compactions'] == 0
    assert len(done) > 20
    # the twin: the same history, then its own table uploaded again -- compact, no dead rows
    cb = _lib.Context(0)
    b = resident.ResidentSim(init, p, ctx=cb)
    b.set_fms(*rt)
    b.step(3)
    for batch in done:
        b.edit_routes(batch)
    rows, off, cnt, wt = b.read_routes()
    f = b.read_fms()
    b.set_fms(rows, off, cnt, f, simt=f['simt'], t0=f['t0'])
    a.edit_routes(last), b.edit_routes(last)
    assert a.route_stats()['compactions'] == 1 and a.route_stats()['dead'] == 0
    assert b.route_stats()['compactions'] == 0 and b.route_stats()['dead'] == n
    for x, y in zip(a.read_routes(), b.read_routes()):
        assert np.array_equal(x, y, equal_nan=True)
    for q in range(2):
        fa, fb = a.read_fms(), b.read_fms()
        for k in fa:
            if k != 'ticks':
                assert np.array_equal(np.asarray(fa[k]), np.asarray(fb[k]), equal_nan=True), k
        a.step(4), b.step(4)
        ra, rb = a.read(), b.read()
        for k in ra:
            assert np.array_equal(np.asarray(ra[k]), np.asarray(rb[k]), equal_nan=True), k
        assert np.array_equal(np.asarray(a.resopairs()), np.asarray(b.resopairs()))
    cb.close()


def test_edit_drops_no_kept_detect_state(ctx):
    """Tile reuse on, 1 500 aircraft flying routes at simdt 0.05: an edit of 60 routes
    between two batches.  The counters of tests/test_gpu_kept_state.py: the detects after the
    edit keep the tile-pair list and the HK history exactly as those of a twin without the edit
    (no build is the edit's doing), at least one of them is a list detect that did not build,
    and state and pairs of every batch equal a sim with reuse off that takes the same edit."""
    from tests.test_gpu_kept_state import TILE, delta, snap
    from tests.util import same as same_all
    n, K, M = 1500, 24, 8
    init = resident.initial_state(synth.box(n, 80.0, seed=21))
    rt = fms.synthetic_routes(init, seed=21)
    p = resident.params(simdt=0.05)
    recs = mixed_batch(rt, None, np.random.default_rng(21), np.random.default_rng(22).choice(n, 60, replace=False))

    def run(reuse, edit):
        c = _lib.Context(0)
        try:
            c.set_tile_reuse(reuse, *TILE)
            sim = resident.ResidentSim(init, p, ctx=c)
            sim.set_fms(*rt)
            sim.step(K)
            t0, h0 = c.tile_reuse_stats(), c.hk_stats()
            if edit:
                sim.edit_routes(recs)
            out, per = [], []
            for _ in range(M):
                sim.step(1)
                out.append(snap(c, sim))
                per.append((delta(c.tile_reuse_stats(), t0), delta(c.hk_stats(), h0)))
            return out, per, sim.read_fms()
        finally:
            c.close()
    edited, per_e, fe = run(True, True)
    control, per_c, fc = run(True, False)
    plain, _, fp = run(False, True)
    print('edited', per_e[-1], 'control', per_c[-1])
    assert not np.array_equal(fe['actwp_lat'], fc['actwp_lat'])          # the edit did change the guidance
    assert per_e == per_c                                              # ... and no counter of the kept state
    assert per_e[-1][0]['detects'] - per_e[-1][0]['builds'] >= 1
    same_all(edited, plain)
    for k in fe:
        assert np.array_equal(np.asarray(fe[k]), np.asarray(fp[k]), equal_nan=True), k
