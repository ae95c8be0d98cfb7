"""What a detect keeps from earlier calls, and the events that drop it
(DESIGN.md 3.24): the spatial order, the candidate list, the tile-pair list
with its halo plan, the column records K4' prepared, the counters the last K2
zeroed and the host-known (HK) build history.  None of them may change a
result, so after every event E -- edited arrays, new parameters, created and
deleted traffic, the probe's other rows, the configuration setters called
again, an aborted batch, a standalone detect -- the running sim continues
BITWISE as a sim built afresh from the state read right after E: state arrays
and pair lists after every batch.

5 000 aircraft in a 150 NM box: 10 column tiles of 512, the last one partial,
several row tiles, near and far tile pairs, ~3e4 conflict pairs.  Every case
runs at simdt 0.05 s (lists are kept, HK keeps) and at 1.0 s (250 m per step:
frequent rebuilds).  The event comes after 24 steps: the first steps of a sim are
its vertical transient (aircraft levelling off), which rebuilds every list.

One-rank list detects: an event that drops K4''s prepared records makes the
next detect a plain one (no list); the first LIST detect after E is the one
after it, and must be a build."""
import numpy as np
import pytest

from bluesky_amd import _lib, resident, synth
from tests.util import same

pytestmark = pytest.mark.gpu

N, SIDE, SEED = 5000, 150.0, 131
K, M = 24, 8                     # steps before the event, steps after it
TILE = (2016.0, 300.0)           # the default tile-pair list budgets
CD = (synth.RPZ, synth.HPZ, synth.TLOOKAHEAD)


def sim_params(simdt, **kw):
    return resident.params(simdt=simdt, **kw)


def snap(c, sim):
    st = sim.stats()
    return sim.read(), c.fetch_pairs(st['n_conf'], st['n_los'])


def carried(host, read):
    """bsa_sim_init's arrays for a sim continuing from ``read``: the state and
    asas.alt as read, the arrays no read returns from the host's copy."""
    st = dict(host)
    st.update({k: v for k, v in read.items() if k in _lib.SIM_STATE_FIELDS})
    return st


# ---------------------------------------------------------------- the events: E(sim, host, p) -> (host, p)
def ev_none(sim, host, p):
    return host, p


def ev_selalt(sim, host, p):
    host = dict(host, selalt=host['selalt'] + 300.0)
    sim.update(selalt=host['selalt'])
    return host, p


def ev_selalt_same(sim, host, p):
    sim.update(selalt=host['selalt'])
    return host, p


def ev_jump(sim, host, p):
    """one aircraft moves 40 km north and 30 km east"""
    st = sim.read()
    lat, lon = st['lat'].copy(), st['lon'].copy()
    lat[7] += 40.0 / 111.19
    lon[7] += 30.0 / (111.19 * np.cos(np.radians(lat[7])))
    sim.update(lat=lat, lon=lon)
    return host, p


def ev_rpz(sim, host, p):
    p = sim_params(p.simdt, rpz=6.0 * resident.NM, reso=bool(p.reso))
    sim.set_params(p)
    return host, p


def ev_same_params(sim, host, p):
    sim.set_params(sim_params(p.simdt, reso=bool(p.reso)))
    return host, p


def ev_traffic(sim, host, p):
    """3 aircraft created in the middle of the box, 2 deleted"""
    new = resident.initial_state(synth.box(3, 20.0, seed=SEED + 1))
    gone = [10, 4000]
    sim.create(new)
    sim.delete(gone)
    return {k: np.delete(np.concatenate([host[k], new[k]]), gone) for k in host}, p


def ev_probe(sim, host, p):
    sim.ctx.sim_probe_rank(1, 2)
    sim.ctx.sim_probe_rank(0, 1)
    return host, p


def ev_tile_reuse(sim, host, p):
    sim.ctx.set_tile_reuse(True, *TILE)
    return host, p


def ev_hk(sim, host, p):
    sim.ctx.set_hk(True, 0.75)
    return host, p


def ev_overflow(sim, host, p):
    """a candidate list far too small: the next batch aborts, grows it and re-runs"""
    sim.ctx.set_candidate_capacity(16)
    sim.step(1)
    return host, p


def ev_detect(sim, host, p):
    """a standalone detect of the same traffic on the sim's context (bsa_set_state
    replaces a resident sim: the sim goes on from the state read before it)"""
    st = carried(host, sim.read())
    sim.ctx.set_state(*[st[k] for k in ('lat', 'lon', 'trk', 'gs', 'alt', 'vs')])
    nc, _ = sim.ctx.detect(*CD)
    assert nc > 0
    sim.ctx.sim_init(st, p)
    return host, p


EVENTS = dict(selalt=ev_selalt, selalt_same=ev_selalt_same, jump=ev_jump, rpz=ev_rpz, same_params=ev_same_params, traffic=ev_traffic,
              probe=ev_probe, tile_reuse=ev_tile_reuse, hk=ev_hk, overflow=ev_overflow, detect=ev_detect)
# the rows of the table that drop the tile-pair list (set_hk's keeps it: only the HK history goes)
LIST_REBUILT = tuple(k for k in EVENTS if k != 'hk')
BITWISE = tuple(k for k in EVENTS if k != 'selalt_same')


def delta(a, b):
    return {k: a[k] - b[k] for k in a if isinstance(a[k], int) and not isinstance(a[k], bool)}


def run_event(ctx, simdt, event, reuse=None, k=K):
    """Sim A: k steps, the event, M more steps -- single steps up to the first
    list detect, the rest as one batch.  Sim B, afresh from A's state as read
    right after the event, runs the same batches on ``ctx``.  Returns A's and
    B's [(state, pairs)] per batch and A's statistics deltas."""
    t = synth.box(N, SIDE, seed=SEED)
    host = resident.initial_state(t)
    p = sim_params(simdt, reso=reuse is None)
    a = _lib.Context(0)
    try:
        a.set_tile_reuse(True, *TILE)
        if reuse:
            a.set_candidate_reuse(True, *reuse)
        sim = resident.ResidentSim(host, p, ctx=a)
        sim.step(k)
        r0 = a.reuse_stats()
        host, p = event(sim, host, p)
        start = carried(host, sim.read())
        t0, h0 = a.tile_reuse_stats(), a.hk_stats()
        got, batches, first = [], [], None
        while sum(batches) < 3:   # one-rank sims: the second detect after E at the latest
            sim.step(1)
            batches.append(1)
            got.append(snap(a, sim))
            if first is None:
                first = dict(reuse=delta(a.reuse_stats(), r0))
            if a.tile_reuse_stats()['detects'] > t0['detects']:
                break
        first.update(tile=delta(a.tile_reuse_stats(), t0), hk=delta(a.hk_stats(), h0), steps=sum(batches))
        batches.append(M - sum(batches))
        sim.step(batches[-1])
        got.append(snap(a, sim))
        span = dict(tile=delta(a.tile_reuse_stats(), t0), hk=delta(a.hk_stats(), h0))
    finally:
        a.close()
    b = resident.ResidentSim(start, p, ctx=ctx)
    exp = []
    for k in batches:
        b.step(k)
        exp.append(snap(ctx, b))
    print('%s simdt %g reuse %s: first %s span %s' % (event.__name__, simdt, reuse, first, span))
    assert sum(len(x[1]['ci']) for x in exp) > 0
    return got, exp, first, span


@pytest.mark.parametrize('simdt', [0.05, 1.0])
@pytest.mark.parametrize('name', BITWISE)
def test_sim_continues_bitwise_after_event(ctx, name, simdt):
    got, exp, first, _ = run_event(ctx, simdt, EVENTS[name])
    same(got, exp)
    if name in LIST_REBUILT:   # the first list detect after E was a build
        assert first['tile']['detects'] == 1 and first['tile']['builds'] == 1 and first['hk']['keeps'] == 0, first


def test_control_keeps_its_list(ctx):
    """No event, simdt 0.05: a detect of the same span keeps its list (decided by
    the host or on the device: a list detect that did not build), so a build
    right after an event is the event's doing."""
    got, exp, first, span = run_event(ctx, 0.05, ev_none)
    same(got, exp)
    assert span['tile']['detects'] - span['tile']['builds'] >= 1, span


@pytest.mark.parametrize('simdt', [0.05, 1.0])
@pytest.mark.parametrize('name, builds', [('selalt_same', 0), ('jump', 1), ('traffic', 1), ('overflow', 1)])
def test_candidate_list_rebuilt_once(ctx, name, builds, simdt):
    """Candidate-list reuse on a one-rank sim: from before the event to the end of
    the first step after it the list is rebuilt exactly once after a position
    jump, created / deleted traffic and an overflow, and not after an edited
    selalt, which is also the control: no drift rebuild falls on that step.

    K0b rebuilds the list by itself once an aircraft's position change plus 300 s
    of its velocity change leaves the horizontal budget, or its altitude change
    plus 300 s of its vs change the vertical one (k_prep_cols).  So that only
    the event rebuilds: no resolver (an MVP manoeuvre is a velocity jump at every
    detect), a horizontal budget of 20 km (32 s at <= 300 m/s are < 10 km; the
    jump is 50 km), selalt rewritten with the values it holds (another target
    altitude makes the aircraft climb: a vs jump), and the event after 24 s of
    sim time at either simdt (at 0.05 s the list is still rebuilt at every
    detect 1.2 s into the sim: measured on the build before this file)."""
    got, exp, first, _ = run_event(ctx, simdt, EVENTS[name], reuse=(20000.0, 60.0), k=int(round(K / simdt)))
    same(got, exp)
    assert first['reuse']['builds'] == builds, first
