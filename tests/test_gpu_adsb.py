"""GPU: the ADS-B model on the device (bsa_adsb_draws / bsa_adsb_update / bsa_sim_set_adsb) against the reference's
goldens and tests/adsb_np.py, and bitwise against itself across batching, an aborted batch, delete / create and the
rank count."""
import os
import types

import numpy as np
import pytest

from bluesky_amd import _lib, adsb, resident, statebased, synth
from oracle import statebased as ocd
from tests import adsb_np, turb_np, util
from tests.test_gpu_multirank import run_ranks
from tests.test_gpu_sim import SCALES, full_state

pytestmark = pytest.mark.gpu

SEED = 20261022
TE = adsb_np.TRANSERROR
NS = (1, 63, 64, 65, 257)
COPIED = ('lastupdate', 'trk', 'tas', 'gs', 'vs')
NOISY = ('lat', 'lon', 'alt')


@pytest.fixture(scope='module')
def upd():
    return dict(np.load(os.path.join(util.GOLDEN, 'adsb_update.npz')))


@pytest.fixture(scope='module')
def flight():
    return dict(np.load(os.path.join(util.GOLDEN, 'adsb_flight64.npz')))


def case_of(g, name):
    return ({k: g['%s_traf_%s' % (name, k)] for k in adsb_np.FIELDS}, {k: g['%s_in_%s' % (name, k)] for k in adsb_np.ARRAYS},
            {k: g['%s_out_%s' % (name, k)] for k in adsb_np.ARRAYS}, g[name + '_z'], float(g[name + '_trunctime']),
            '_noise1_' in name)


def bitwise(got, exp, what, keys=adsb_np.ARRAYS):
    for k in keys:
        assert np.array_equal(np.asarray(got[k]), np.asarray(exp[k]), equal_nan=True), '%s: %s' % (what, k)


def close(got, exp, what, keys=NOISY):
    for k in keys:
        ok, msg = util.close(got[k], exp[k], SCALES[k])
        assert ok, '%s %s: %s' % (what, k, msg)


def np_normals(mode, n, call, first=0):
    """adsb_np's unit normals as ``adsb_np.update`` takes them: (3,) shared, (3, n) per aircraft."""
    return adsb_np.draws(1, SEED, call)[0] if mode == 'shared' else adsb_np.draws(n, SEED, call, first).T


# ---------------------------------------------------------------- 1. standalone against the golden
@pytest.mark.parametrize('n', NS)
def test_update_equals_the_reference(ctx, upd, n):
    names = [str(x) for x in upd['names'] if str(x).startswith('n%d_' % n)]
    assert len(names) == 4
    for name in names:
        traf, st, exp, z, trunctime, noise = case_of(upd, name)
        got = ctx.adsb_update(float(upd['time']), traf, st, trunctime=trunctime, noise=noise, transerror=TE, given=z)
        bitwise(got, exp, name)      # the noisy ones too: one multiply and one add, no contraction
        assert not np.array_equal(got['trk'], st['trk'])


def test_update_at_time_zero_updates_nobody(ctx, upd):
    traf = {k: upd['zero_traf_' + k] for k in adsb_np.FIELDS}
    st = {k: upd['zero_in_' + k] for k in adsb_np.ARRAYS}
    bitwise(ctx.adsb_update(0.0, traf, st, noise=True, given=upd['zero_z']), st, 'time 0')


# ---------------------------------------------------------------- 2. device-generated draws
@pytest.mark.parametrize('n', NS)
def test_draw_words_match_helper(ctx, n):
    for seed, call, first in [(0, 0, 0), (SEED, 7, 1000), (2 ** 64 - 1, 2 ** 40, 2 ** 33)]:
        raw, z = adsb.draws(n, seed, call, first, ctx=ctx, raw=True)
        exp = adsb_np.raw_words(n, seed, call, first)
        assert np.array_equal(raw, exp), (seed, call, first)
        ok, msg = util.close(z.ravel(), turb_np.normals(exp).ravel(), 1.0)
        assert ok, msg
        u = adsb.create_uniforms(n, seed, call, first, ctx=ctx)
        assert np.array_equal(u, adsb_np.create_uniforms(n, seed, call, first))      # (exact: integer to fp64, one scale)
        assert not np.array_equal(raw, turb_np.raw_words(n, seed, call, first))   # not turbulence's block


@pytest.mark.parametrize('mode', ['shared', 'per_aircraft'])
def test_update_generates_its_draws(ctx, upd, mode):
    for name in ('n257_noise1_trunc5', 'n65_noise1_trunc0', 'n1_noise1_trunc5'):
        traf, st, _, _, trunctime, _ = case_of(upd, name)
        n, t, call = len(st['lat']), float(upd['time']), 5
        got = ctx.adsb_update(t, traf, st, trunctime=trunctime, noise=True, transerror=TE, draws=mode, seed=SEED, call=call)
        exp = adsb_np.update(st, traf, t, trunctime, True, TE, np_normals(mode, n, call))
        bitwise(got, exp, name, COPIED)
        close(got, exp, name)
        up = adsb_np.due(st['lastupdate'], trunctime, t)
        assert len(up)
        # the device's own normals, injected, give the same bits
        z = adsb.draws(1, SEED, call, ctx=ctx)[0] if mode == 'shared' else adsb.draws(n, SEED, call, ctx=ctx).T
        bitwise(ctx.adsb_update(t, traf, st, trunctime=trunctime, noise=True, transerror=TE, draws=mode, given=z), got, name)
        if mode == 'shared':           # every updated aircraft carries the same three offsets
            for q, k in enumerate(NOISY):
                e = 0.0 + TE[0 if q < 2 else 1] * z[q]
                assert np.array_equal(got[k][up], traf[k][up] + e, equal_nan=True), k
        else:                          # rows 100.. alone, told their index, equal rows 100.. of the full call
            if n > 100:
                part = ctx.adsb_update(t, {k: v[100:] for k, v in traf.items()}, {k: v[100:] for k, v in st.items()},
                                       trunctime=trunctime, noise=True, transerror=TE, draws=mode, seed=SEED, call=call,
                                       first_index=100)
                bitwise(part, {k: v[100:] for k, v in got.items()}, name + ' slice')
                assert len(np.unique(got['lat'][up] - traf['lat'][up])) > len(up) // 2


# ---------------------------------------------------------------- 3. the drop-in on the flight golden
def flight_dropin(ctx, g, noise, **kw):
    traf = types.SimpleNamespace(**{k: g['traf_' + k][0] for k in adsb_np.FIELDS})
    ad = adsb.ADSB(traf, ctx=ctx, **kw)
    ad.SetNoise(noise)
    ad.trunctime = float(g['trunctime'])
    for k in adsb_np.ARRAYS:
        setattr(ad, k, g['init_' + k].copy())
    return traf, ad


@pytest.mark.parametrize('how', ['off', 'given', 'own'])
def test_dropin_flies_the_reference_flight(ctx, flight, how):
    g = flight
    traf, ad = flight_dropin(ctx, g, how != 'off', seed=SEED)
    hist = 'off_hist_' if how == 'off' else 'on_hist_'
    for c in range(int(g['ncalls'])):
        for k in adsb_np.FIELDS:
            setattr(traf, k, g['traf_' + k][c])
        ad.update(float(g['t'][c]), given=g['on_z'][c] if how == 'given' else None)
        got = {k: getattr(ad, k) for k in adsb_np.ARRAYS}
        bitwise(got, {k: g[hist + k][c] for k in adsb_np.ARRAYS}, 'call %d' % c, COPIED if how == 'own' else adsb_np.ARRAYS)
    assert ad.call == (0 if how == 'off' else 40)


def test_dropin_surface(ctx, upd):
    g = upd
    n = 65
    traf = types.SimpleNamespace(**{k: g['create_traf_' + k][:n].copy() for k in adsb_np.FIELDS})
    old = types.SimpleNamespace(transnoise=True, truncated=True, transerror=[2e-4, 50.0], trunctime=5,
                                **{k: g['create_in_' + k].copy() for k in adsb_np.ARRAYS})
    traf.adsb = old
    ad = adsb.install(traf, seed=SEED, ctx=ctx)
    assert traf.adsb is ad and ad.transerror == [2e-4, 50.0] and ad.trunctime == 5 and ad.transnoise is True
    for k in adsb_np.FIELDS:
        setattr(traf, k, g['create_traf_' + k].copy())               # Traffic.create appended three
    ad.create(3)
    exp = adsb_np.create({k: getattr(old, k) for k in adsb_np.ARRAYS}, {k: getattr(traf, k) for k in adsb_np.FIELDS}, 3, 5,
                         adsb_np.create_uniforms(3, SEED, 0, n))
    bitwise({k: getattr(ad, k) for k in adsb_np.ARRAYS}, exp, 'create')
    ad.delete(np.array([1, 66]))
    bitwise({k: getattr(ad, k) for k in adsb_np.ARRAYS}, adsb_np.delete(exp, [1, 66]), 'delete')
    ad.SetNoise(False)
    assert (ad.transnoise, ad.truncated, ad.transerror, ad.trunctime) == adsb_np.set_noise(False)
    with pytest.raises(ValueError):
        adsb.ADSB(traf, draws='each')


def test_dropin_in_a_traffic_tree(ctx):
    """``install`` puts the object among the parent's children: the parent's create / delete reach it, and the
    update that follows finds arrays of the traffic's length (trunctime 5: create's uniforms are the device's)."""
    traf = adsb_np.ArrayTree()
    old = adsb_np.ArrayTree(adsb_np.ARRAYS)
    old.transnoise, old.truncated, old.transerror, old.trunctime = False, False, list(TE), 5
    old.parent, traf.adsb = traf, old
    traf.children.append(old)
    ad = adsb.install(traf, seed=SEED, ctx=ctx)
    assert traf.children == [ad]
    first = {k: np.arange(4) + 10.0 * q + 1.0 for q, k in enumerate(adsb_np.FIELDS)}
    traf.create(4, **first)
    more = {k: np.arange(3) + 10.0 * q + 5.5 for q, k in enumerate(adsb_np.FIELDS)}
    traf.create(3, **more)
    exp = adsb_np.create({k: np.zeros(0) for k in adsb_np.ARRAYS}, first, 4, 5, adsb_np.create_uniforms(4, SEED, 0, 0))
    exp = adsb_np.create(exp, {k: getattr(traf, k) for k in adsb_np.FIELDS}, 3, 5, adsb_np.create_uniforms(3, SEED, 0, 4))
    bitwise({k: getattr(ad, k) for k in adsb_np.ARRAYS}, exp, 'two creates')
    assert np.all(ad.lastupdate < 0) and len(np.unique(ad.lastupdate)) == 7
    traf.delete(np.array([1, 5]))
    exp = adsb_np.delete(exp, [1, 5])
    traf.vs = traf.vs + 1.0
    traf.adsb.update(0.0)                                         # lastupdate + 5 = 5 (1 - u) >= 0: nobody is due
    bitwise({k: getattr(ad, k) for k in adsb_np.ARRAYS}, exp, 'not yet due')
    traf.adsb.update(6.0)
    exp = adsb_np.update(exp, {k: getattr(traf, k) for k in adsb_np.FIELDS}, 6.0, 5)
    bitwise({k: getattr(ad, k) for k in adsb_np.ARRAYS}, exp, 'after the update')
    assert len(ad.vs) == traf.ntraf == 5 and np.array_equal(ad.vs, traf.vs)
    traf.reset()
    assert len(ad.lastupdate) == 0


def test_refusals(ctx):
    init = resident.initial_state(synth.box(200, 20.0, seed=5))
    sim = resident.ResidentSim(init, resident.params(), ctx=ctx)
    for kw in (dict(transerror=(np.nan, 1.0)), dict(transerror=(1.0, -1.0)), dict(trunctime=-1.0), dict(trunctime=np.inf)):
        with pytest.raises(_lib.AccelError):
            sim.set_adsb(True, **kw)
    with pytest.raises(ValueError):
        sim.set_adsb(True, draws='each')
    with pytest.raises(ValueError):
        sim.set_adsb(True, transerror=(1.0,))
    with pytest.raises(_lib.AccelError):
        sim.read_adsb()                      # off: nothing to read
    with pytest.raises(_lib.AccelError):
        sim.adsb_call(-1)
    sim.step(2)
    assert sim.adsb_call() == 0


# ---------------------------------------------------------------- 4. the resident stage
N, SIMT0 = 257, 40.0


@pytest.fixture(scope='module')
def box257():
    """The 257-aircraft box and a staggered lastupdate (not modified)."""
    init = resident.initial_state(synth.box(N, 20.0, seed=157))
    init['vs'] = np.linspace(-5.0, 5.0, N)
    p = resident.params(cd_every=1)
    trunc = 3 * p.simdt
    last = SIMT0 - trunc * np.random.default_rng(7).random(N)
    return init, p, trunc, last


def adsb_sim(box, c, noise=True, mode='per_aircraft', **kw):
    init, p, trunc, last = box
    sim = resident.ResidentSim(init, p, ctx=c, **kw)
    sim.set_adsb(True, noise=noise, transerror=TE, trunctime=trunc, seed=SEED, draws=mode, simt=SIMT0, lastupdate=last)
    return sim


def picture_of(state, last):
    exp = {k: np.array(state[k]) for k in adsb_np.FIELDS}
    exp['lastupdate'] = np.array(last)
    return exp


def follow(sim, init, exp, simt, call, steps, trunc, noise, mode):
    """``steps`` x step(1), the restatement driven by the state read before each step; returns (exp, simt, call)."""
    for _ in range(steps):
        state = full_state(init, sim.read())
        n = len(state['lat'])
        exp = adsb_np.update(exp, state, simt, trunc, noise, TE, np_normals(mode, n, call) if noise else None)
        sim.step(1)
        simt += sim.params.simdt
        call += int(noise)
    return exp, simt, call


def check(sim, exp, simt, call, noise, what):
    got = sim.read_adsb()
    assert got['simt'] == simt and got['call'] == call == sim.adsb_call(), what
    bitwise(got, exp, what, COPIED if noise else adsb_np.ARRAYS)
    if noise:
        close(got, exp, what)
    return got


@pytest.mark.parametrize('noise,mode', [(False, 'shared'), (True, 'shared'), (True, 'per_aircraft')])
def test_stage_follows_the_restatement(ctx, box257, noise, mode):
    init, p, trunc, last = box257
    sim = adsb_sim(box257, ctx, noise, mode)
    exp = picture_of(init, last)
    check(sim, exp, SIMT0, 0, noise, 'enabled')                        # the picture is the state, vs too
    exp, simt, call = follow(sim, init, exp, SIMT0, 0, 12, trunc, noise, mode)
    got = check(sim, exp, simt, call, noise, '12 steps')
    moved = got['lastupdate'] != last
    assert moved.all() and len(np.unique(np.round((got['lastupdate'] - last) / trunc))) > 1
    assert not np.array_equal(got['lat'], sim.read()['lat'])          # truncated: the picture lags the state


@pytest.mark.parametrize('mode', ['shared', 'per_aircraft'])
def test_batch_equals_single_steps(ctx, box257, mode):
    one = adsb_sim(box257, ctx, True, mode)
    for _ in range(12):
        one.step(1)
    sim = adsb_sim(box257, ctx, True, mode)
    sim.step(12)
    a, b = sim.read_adsb(), one.read_adsb()
    bitwise(a, b, 'step(12)')
    assert a['simt'] == b['simt'] and a['call'] == b['call'] == 12
    bitwise(sim.read(), one.read(), 'state', sim.read().keys())


# ---------------------------------------------------------------- 5. an aborted batch
def test_abort_in_mid_batch_is_exact(ctx):
    """test_gpu_turbulence's set-up: a candidate list far too small, CD every 4th step.  The batch of steps 1-12
    completes steps 1-3, aborts at step 4 -- whose ADS-B launch had already run -- and re-runs from there."""
    init = resident.initial_state(synth.box(5000, 120.0, seed=149))
    p = resident.params(cd_every=4)
    trunc = 3 * p.simdt
    last = -trunc * np.random.default_rng(8).random(5000)
    box = (init, p, trunc, last)

    def run(c, small):
        sim = adsb_sim(box, c)
        if small:
            c.set_candidate_capacity(16)
        sim.step(1)
        if small:
            c.set_candidate_capacity(16)
        sim.step(12)
        return sim.read_adsb(), sim.adsb_call(), sim.read(), sim.stats(), sim.aborts()

    exp = run(ctx, False)
    assert exp[3]['n_conf'] > 0 and exp[1] == 13
    c = _lib.Context(0)
    try:
        got = run(c, True)
    finally:
        c.close()
    assert got[4] >= 2                               # the small list did abort both batches, which were re-run
    bitwise(got[0], exp[0], 'after the re-run')      # a doubled lastupdate += trunctime would show here
    assert got[0]['simt'] == exp[0]['simt'] and got[0]['call'] == exp[0]['call'] and got[1] == exp[1]
    bitwise(got[2], exp[2], 'state', exp[2].keys())
    assert got[3] == exp[3]


# ---------------------------------------------------------------- 6. delete and create between batches
def test_delete_and_create_between_batches(ctx, box257):
    init, p, trunc, last = box257
    noise, mode = True, 'per_aircraft'
    sim = adsb_sim(box257, ctx, noise, mode)
    exp, simt, call = follow(sim, init, picture_of(init, last), SIMT0, 0, 4, trunc, noise, mode)
    before = check(sim, exp, simt, call, noise, 'before the delete')
    gone = np.array([0, 100, 256])
    sim.delete(gone)
    after = sim.read_adsb()
    bitwise(after, {k: np.delete(before[k], gone) for k in adsb_np.ARRAYS}, 'survivors')     # unchanged, in index order
    exp = adsb_np.delete(exp, gone)
    state = {k: np.delete(v, gone) for k, v in full_state(init, {}).items()}
    exp, simt, call = follow(sim, state, exp, simt, call, 3, trunc, noise, mode)            # draws by the new indices
    before = check(sim, exp, simt, call, noise, 'after the delete')
    new = resident.initial_state(synth.box(2, 5.0, seed=158))
    new['vs'] = np.array([3.0, -2.0])
    sim.create(new)
    n = N - 3
    after = sim.read_adsb()
    bitwise({k: after[k][:n] for k in adsb_np.ARRAYS}, before, 'the others')
    assert np.array_equal(after['lastupdate'][n:], -trunc * adsb_np.create_uniforms(2, SEED, call, n))   # rule 7
    assert np.all(after['lastupdate'][n:] < 0) and not after['vs'][n:].any()
    bitwise({k: after[k][n:] for k in adsb_np.FIELDS[:-1]}, new, 'created', adsb_np.FIELDS[:-1])
    state = {k: np.append(state[k], new[k]) for k in state}
    exp = {k: after[k] for k in adsb_np.ARRAYS}
    exp, simt, call = follow(sim, state, exp, simt, call, 3, trunc, noise, mode)
    check(sim, exp, simt, call, noise, 'after the create')


# ---------------------------------------------------------------- 7. two in-process ranks
def test_two_ranks_equal_one(ctx):
    n = 1300                                      # both ranks own rows (1024 + 276)
    init = resident.initial_state(synth.box(n, 40.0, seed=159))
    p = resident.params(cd_every=2)
    trunc = 3 * p.simdt
    box = (init, p, trunc, SIMT0 - trunc * np.random.default_rng(9).random(n))
    one = adsb_sim(box, ctx)
    one.step(4)
    one.step(6)
    exp = one.read_adsb()

    def rank(r, c, g):
        sim = adsb_sim(box, c, rank=r, world=2, group=g)
        sim.step(4)
        sim.step(6)
        return sim.read_adsb(), sim.row_ids()

    res = run_ranks(2, rank)
    assert np.array_equal(np.sort(np.concatenate([i for _, i in res])), np.arange(n)) and all(len(i) for _, i in res)
    for k in adsb_np.ARRAYS:
        full = np.zeros(n)
        for got, ids in res:
            full[ids] = got[k][ids]
        assert np.array_equal(full, exp[k]), k
    assert all(got['call'] == exp['call'] == 10 and got['simt'] == exp['simt'] for got, _ in res)


# ---------------------------------------------------------------- 8. off is off
def test_off_is_off(ctx, box257):
    init, p, trunc, last = box257
    ref = resident.ResidentSim(init, p, ctx=ctx)
    ref.step(20)
    exp, st = ref.read(), ref.stats()
    sim = adsb_sim(box257, ctx)
    sim.set_adsb(on=False)
    sim.step(20)
    bitwise(sim.read(), exp, 'on, then off', exp.keys())
    assert sim.stats() == st and sim.adsb_call() == 0
    with pytest.raises(_lib.AccelError):
        sim.read_adsb()
    on = adsb_sim(box257, ctx)
    on.step(20)
    bitwise(on.read(), exp, 'on', exp.keys())       # the stage writes only its own arrays
    assert on.stats() == st and on.adsb_call() == 20


# ---------------------------------------------------------------- 9. detect against the picture
def test_detect_against_the_picture(ctx):
    n = 300
    t = synth.box(n, 30.0, seed=160)
    traf = types.SimpleNamespace(lat=t.lat, lon=t.lon, alt=t.alt, trk=t.trk, gs=t.gs, vs=t.vs, tas=np.array(t.gs), id=t.id,
                                 ntraf=n)
    ad = adsb.install(traf, seed=SEED, draws='per_aircraft', ctx=ctx)
    ad.create(n)
    ad.SetNoise(True)
    ad.update(1.0)
    assert ad.call == 1 and not np.array_equal(ad.lat, traf.lat) and np.array_equal(ad.gs, traf.gs)
    got = statebased.detect_indices(traf, ad, synth.RPZ, synth.HPZ, synth.TLOOKAHEAD, ctx=ctx)
    exp = ocd.detect_arrays(traf, ad, synth.RPZ, synth.HPZ, synth.TLOOKAHEAD)
    assert len(exp['ci']) > 0
    util.assert_detect_equal(got, exp, synth.RPZ, synth.TLOOKAHEAD)
    res = statebased.detect(traf, traf.adsb, synth.RPZ, synth.HPZ, synth.TLOOKAHEAD, ctx=ctx)
    assert res[0] == [(t.id[i], t.id[j]) for i, j in zip(exp['ci'], exp['cj'])]
