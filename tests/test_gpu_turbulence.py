"""GPU: Turbulence.Woosh on the device (bsa_turb_draws / bsa_turb_apply /
bsa_sim_set_turbulence) against tests/turb_np.py, the reference's golden and
oracle/step.py, and bitwise against itself across batching, reuse settings,
rank counts, an aborted batch and a delete."""
import os

import numpy as np
import pytest

from bluesky_amd import _lib, resident, synth, turbulence
from oracle import statebased as ocd
from oracle import step as ostep
from tests import turb_np, util
from tests.test_gpu_multirank import run_ranks
from tests.test_gpu_sim import SCALES, compare, full_state, oracle_params
from tests.test_turb_np import STAT_CALL, STAT_DT, STAT_N, STAT_SD, STAT_SEED, stat_check

pytestmark = pytest.mark.gpu

SD = (1.0, 2.0, 0.5)
SEED = 20261020


@pytest.fixture(scope='module')
def woosh():
    return dict(np.load(os.path.join(util.GOLDEN, 'turb_woosh300.npz')))


def close_normals(got, exp):
    ok, msg = util.close(got.ravel(), exp.ravel(), 1.0)   # unit normals: scale 1, the floor covers sin near 0
    assert ok, msg


# ---------------------------------------------------------------- 1. the draws
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
def test_draws_match_helper(ctx, n):
    for seed, call, first in [(0, 0, 0), (SEED, 0, 0), (SEED, 7, 0), (SEED, 7, 1000), (2 ** 64 - 1, 2 ** 40, 2 ** 33)]:
        raw, z = turbulence.draws(n, seed, call, first, ctx=ctx, raw=True)
        exp = turb_np.raw_words(n, seed, call, first)
        assert np.array_equal(raw, exp), (seed, call, first)
        close_normals(z, turb_np.normals(exp))
        assert np.array_equal(turbulence.draws(n, seed, call, first, ctx=ctx), z)   # without the words


def test_draw_slices_are_position_independent(ctx):
    raw, z = turbulence.draws(257, SEED, 3, ctx=ctx, raw=True)
    raw2, z2 = turbulence.draws(65, SEED, 3, first_index=100, ctx=ctx, raw=True)
    assert np.array_equal(raw[100:165], raw2) and np.array_equal(z[100:165], z2)
    assert not np.array_equal(raw, turbulence.draws(257, SEED + 1, 3, ctx=ctx, raw=True)[0])
    assert not np.array_equal(raw, turbulence.draws(257, SEED, 4, ctx=ctx, raw=True)[0])


# ---------------------------------------------------------------- 2. apply
@pytest.mark.parametrize('q', [0, 1])
@pytest.mark.parametrize('n', [300, 1, 64, 65])
def test_apply_matches_reference(ctx, woosh, q, n):
    g = woosh
    z = g['z%d' % q][:n]
    lat, lon, alt = ctx.turb_apply(float(g['dt']), g['sd%d' % q], g['trk'][:n], g['coslat'][:n], g['lat'][:n],
                                   g['lon'][:n], g['alt'][:n], draws=(z[:, 0], z[:, 1], z[:, 2]))
    for k, got in (('lat', lat), ('lon', lon), ('alt', alt)):
        ok, msg = util.close(got, g['out_%s%d' % (k, q)][:n], SCALES[k])
        assert ok, '%s: %s' % (k, msg)
    assert not np.array_equal(lat, g['lat'][:n])


def test_apply_generates_its_draws(ctx, woosh):
    g = woosh
    args = (float(g['dt']), SD, g['trk'], g['coslat'], g['lat'], g['lon'], g['alt'])
    got = ctx.turb_apply(*args, seed=SEED, call=5)
    exp = turb_np.woosh_apply(turb_np.draws(300, SEED, 5), *args)
    for k, a, b in zip(('lat', 'lon', 'alt'), got, exp):
        ok, msg = util.close(a, b, SCALES[k])
        assert ok, '%s: %s' % (k, msg)
    z = turbulence.draws(300, SEED, 5, ctx=ctx)
    same = ctx.turb_apply(*args, draws=(z[:, 0], z[:, 1], z[:, 2]))
    assert all(np.array_equal(a, b) for a, b in zip(got, same))


def test_dropin_woosh(ctx, woosh):
    g = woosh

    class Traf:
        pass
    traf = Traf()
    traf.ntraf = 300
    for k in ('lat', 'lon', 'alt', 'trk', 'coslat'):
        setattr(traf, k, g[k].copy())
    tb = turbulence.install(traf, seed=SEED, ctx=ctx)
    tb.Woosh(0.05)
    assert np.array_equal(traf.lat, g['lat']) and tb.call == 0           # inactive: nothing, no draw spent
    tb.SetNoise(True)
    tb.SetStandards([0, 0.1, 0.1])
    assert tb.sd[0] == 1e-6
    tb.Woosh(0.05)
    tb.Woosh(0.05)
    assert tb.call == 2
    exp = (g['lat'], g['lon'], g['alt'])
    for c in range(2):
        exp = turb_np.woosh_apply(turb_np.draws(300, SEED, c), 0.05, [0, 0.1, 0.1], g['trk'], g['coslat'], *exp)
    for k, b in zip(('lat', 'lon', 'alt'), exp):
        ok, msg = util.close(getattr(traf, k), b, SCALES[k])
        assert ok, '%s: %s' % (k, msg)
    with pytest.raises(ValueError):
        tb.SetStandards([1, -1, 0])


def test_refusals(ctx):
    init = resident.initial_state(synth.box(200, 20.0, seed=5))
    sim = resident.ResidentSim(init, resident.params(), ctx=ctx)
    for sd in ([1, np.nan, 1], [1, -0.5, 1], [np.inf, 0, 0]):
        with pytest.raises(_lib.AccelError):
            sim.set_turbulence(True, sd)
    with pytest.raises(ValueError):
        sim.set_turbulence(True, [1, 2])
    with pytest.raises(_lib.AccelError):
        sim.turb_call(-1)
    z = np.zeros(4)
    with pytest.raises(_lib.AccelError):
        ctx.turb_apply(-1.0, SD, z, z + 1, z, z, z)
    sim.step(2)
    assert sim.turb_call() == 0      # never switched on: no call spent


# ---------------------------------------------------------------- 3. the resident step against the oracle
def test_resident_step_matches_oracle(ctx):
    n = 1500
    t = synth.box(n, 60.0, seed=23)
    init = resident.initial_state(t)
    p = resident.params(cd_every=1, turbulence=dict(sd=SD, seed=SEED))
    sim = resident.ResidentSim(init, p, ctx=ctx)
    op = oracle_params(p)
    prev = dict(init)
    prev.update(asas_trk=init['trk'].copy(), asas_tas=init['tas'].copy(), asas_vs=np.zeros(n),
                active=np.zeros(n, bool))
    nconf = 0
    for k in range(20):
        traf = {f: prev[f] for f in ('lat', 'lon', 'trk', 'gs', 'alt', 'vs')}
        cd = ocd.detect_arrays(traf, traf, p.rpz, p.hpz, p.tla)
        exp = ostep.sim_step(prev, op, do_cd=True, cd=cd)
        coslat = np.cos(np.deg2rad(exp['lat']))       # traffic.py:482
        exp['lat'], exp['lon'], exp['alt'] = turb_np.woosh_apply(
            turb_np.draws(n, SEED, k), p.simdt, SD, exp['trk'], coslat, exp['lat'], exp['lon'], exp['alt'])
        sim.step(1)
        got = full_state(init, sim.read())
        compare(got, exp, k)
        st = sim.stats()
        assert st['n_conf'] == len(cd['ci']) and st['n_los'] == len(cd['li'])
        pairs = ctx.fetch_pairs(st['n_conf'], st['n_los'])
        for f in ('ci', 'cj', 'li', 'lj'):
            assert np.array_equal(pairs[f], cd[f]), 'step %d %s' % (k, f)
        nconf += st['n_conf']
        prev = got
    assert nconf > 0 and sim.turb_call() == 20


# ---------------------------------------------------------------- 4. bitwise against itself
BOX = dict(n=20000, side=300.0, seed=131)


def turb_sim(init, c, p=None, **kw):
    sim = resident.ResidentSim(init, p or resident.params(cd_every=1), ctx=c, **kw)
    sim.set_turbulence(True, SD, SEED)
    return sim


def same(a, b, what):
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), '%s: %s' % (what, k)


@pytest.fixture(scope='module')
def box20(ctx):
    """The 20k box and its 20 steps in one batch (the expectation of the tests below; not modified)."""
    init = resident.initial_state(synth.box(BOX['n'], BOX['side'], seed=BOX['seed']))
    sim = turb_sim(init, ctx)
    sim.step(20)
    exp, st = sim.read(), sim.stats()
    assert st['n_conf'] > 0 and sim.turb_call() == 20
    return init, exp, st


def test_turbulence_moves_the_traffic(ctx, box20):
    init, exp, _ = box20
    calm = resident.ResidentSim(init, resident.params(cd_every=1), ctx=ctx)
    calm.step(20)
    got = calm.read()
    for k in ('lat', 'lon', 'alt'):
        assert not np.array_equal(got[k], exp[k]), k


def test_batch_equals_single_steps(ctx, box20):
    init, exp, st = box20
    sim = turb_sim(init, ctx)
    for _ in range(20):
        sim.step(1)
    same(sim.read(), exp, '20 x step(1)')
    assert sim.stats() == st


@pytest.mark.parametrize('what', ['tile_reuse_off', 'hk_off'])
def test_reuse_settings_do_not_matter(ctx, box20, what):
    """(The tile-reuse switch is bsa_set_tile_reuse: the environment's is read once per process.)"""
    init, exp, st = box20
    try:
        if what == 'tile_reuse_off':
            ctx.set_tile_reuse(False)
        else:
            ctx.set_hk(False)
        sim = turb_sim(init, ctx)
        sim.step(7)
        sim.step(13)
        same(sim.read(), exp, what)
        assert sim.stats() == st
    finally:
        ctx.set_tile_reuse(True)
        ctx.set_hk(True, 0.75)


def test_two_ranks_equal_one(ctx, box20):
    init, exp, st = box20
    n = BOX['n']

    def rank(r, c, g):
        sim = turb_sim(init, c, rank=r, world=2, group=g)
        sim.step(8)
        sim.step(12)
        return sim.read(), sim.row_ids(), sim.turb_call()

    res = run_ranks(2, rank)
    assert np.array_equal(np.sort(np.concatenate([i for _, i, _ in res])), np.arange(n))
    for k in ('lat', 'lon', 'alt', 'trk', 'gs', 'vs', 'tas', 'hdg'):
        full = np.zeros(n)
        for got, ids, _ in res:
            full[ids] = got[k][ids]
        assert np.array_equal(full, exp[k]), k
    assert all(call == 20 for _, _, call in res)


def test_abort_in_mid_batch_is_exact(ctx):
    """A candidate list far too small, CD every 4th step (as tests/test_gpu_fms.py forces it): the
    batch of steps 1-12 completes steps 1-3 with their draws, aborts at step 4 and re-runs from
    there; the host replays the call number over the three completed steps."""
    init = resident.initial_state(synth.box(5000, 120.0, seed=149))
    p = resident.params(cd_every=4)
    ref = turb_sim(init, ctx, p)
    ref.step(1)
    ref.step(12)
    exp, st = ref.read(), ref.stats()
    assert st['n_conf'] > 0
    c = _lib.Context(0)
    try:
        sim = turb_sim(init, c, p)
        c.set_candidate_capacity(16)
        sim.step(1)
        c.set_candidate_capacity(16)
        sim.step(12)
        same(sim.read(), exp, 'after the re-run')
        assert sim.stats() == st and sim.turb_call() == 13
    finally:
        c.close()


def test_abort_and_rerun_is_exact(ctx, box20):
    """K2 row buckets one pair wide overflow at the first row with two pairs: the batch
    aborts there, the host replays the call number over the completed steps and re-runs."""
    init, exp, st = box20
    c = _lib.Context(0)
    try:
        c.set_row_bucket(1)
        sim = turb_sim(init, c)
        sim.step(20)
        same(sim.read(), exp, 'after the re-run')
        assert sim.stats() == st and sim.turb_call() == 20
    finally:
        c.close()


def test_delete_follows_the_compacted_index(ctx):
    """5 of 3000 aircraft deleted after step 5: the survivors continue as in a twin sim built
    from them, with the same seed and call number -- the draws follow the new indices."""
    n = 3000
    init = resident.initial_state(synth.box(n, 100.0, seed=137))
    p = resident.params(cd_every=1, reso=False)
    gone = np.array([0, 17, 1499, 2000, 2999])
    keep = np.setdiff1d(np.arange(n), gone)
    sim = turb_sim(init, ctx, p)
    sim.step(5)
    mid = full_state(init, sim.read())
    sim.delete(gone)
    sim.step(5)
    got = sim.read()
    c2 = _lib.Context(0)
    try:
        state = {k: np.ascontiguousarray(mid[k][keep]) for k in _lib.SIM_STATE_FIELDS}
        twin = turb_sim(state, c2, p)
        assert twin.turb_call(5) == 5
        twin.step(5)
        exp = twin.read()
        for k in ('lat', 'lon', 'alt', 'trk', 'gs', 'vs', 'tas', 'hdg'):
            assert np.array_equal(got[k], exp[k]), k
        assert sim.turb_call() == twin.turb_call() == 10
    finally:
        c2.close()


# ---------------------------------------------------------------- 5. off is off
@pytest.mark.parametrize('how', ['on_false', 'sd_only'])
def test_switched_off_is_untouched(ctx, how):
    init = resident.initial_state(synth.box(5000, 120.0, seed=139))
    p = resident.params(cd_every=1)
    ref = resident.ResidentSim(init, p, ctx=ctx)
    ref.step(10)
    exp, st = ref.read(), ref.stats()
    sim = resident.ResidentSim(init, p, ctx=ctx)
    if how == 'on_false':
        sim.set_turbulence(True, SD, SEED)
        sim.set_turbulence(False, SD, SEED)
    else:
        sim.set_turbulence(on=False, sd=(5, 5, 5), seed=1)
    sim.step(10)
    same(sim.read(), exp, how)
    assert sim.stats() == st and sim.turb_call() == 0


# ---------------------------------------------------------------- 6. statistics
def test_statistics(ctx):
    """The issue's bounds on one call of 4096 draws; the helper's stream passes them on the CPU
    (tests/test_turb_np.py), and the device's normals are the helper's within 1e-9."""
    z = turbulence.draws(STAT_N, STAT_SEED, STAT_CALL, ctx=ctx)
    print('mean, variance ratio per component:', stat_check(z, STAT_SD, STAT_DT))
