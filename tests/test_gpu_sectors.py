"""GPU: sector occupancy inside the resident step (bsa_sim_set_areas / _set_sectors / _sectors_poll)
against plugins/sectorcount.py's set arithmetic on tests/area_np.py masks of the state a sim WITHOUT
sectors reads back: masks, counts, arrived / left, the cumulative counters through a long batch, a
delete and a create between updates, the read-only property, and two ranks against one."""
import os

import numpy as np
import pytest

from bluesky_amd import dist, resident, synth
from tests import area_np, util
from tests.test_gpu_multirank import run_ranks

pytestmark = pytest.mark.gpu

N, EVERY, SIMDT = 2000, 4, 2.0
NAMES = ['BOXSWAP', 'CIRC', 'C', 'PENTAGRAM', 'SEAM']
# the plan: batches of EVERY, one of 3 * EVERY + 1, EVERY - 1 to the next update, then a delete and a create
BATCHES = [EVERY, EVERY, EVERY, 3 * EVERY + 1, EVERY - 1, 'change', EVERY, EVERY]
NEW = 40


@pytest.fixture(scope='module')
def areas():
    g = dict(np.load(os.path.join(util.GOLDEN, 'area_shapes.npz')))
    names = [str(x) for x in g['names']]
    shapes = area_np.load_shapes(g)
    return {k: shapes[names.index(k)] for k in NAMES}, dict(zip(names, area_np.named(shapes)))


def initial():
    return resident.initial_state(synth.box(N, 150.0, seed=11)), ['AC%04d' % k for k in range(N)]


def newcomers():
    st = resident.initial_state(synth.box(NEW, 120.0, seed=12))
    return st, ['NEW%03d' % k for k in range(NEW)]


def make_sim(ctx, rank=0, world=1, group=None):
    init, ids = initial()
    p = resident.params(simdt=SIMDT, reso=False)
    return resident.ResidentSim(init, p, ctx=ctx, rank=rank, world=world, group=group), ids


def deleted_indices(inside_any):
    """Some aircraft inside a sector and some outside, by index at the time of the change."""
    return np.sort(np.concatenate((np.flatnonzero(inside_any)[:25:2], np.flatnonzero(~inside_any)[:9:3])))


def truth_masks(shapes, st):
    return np.array([area_np.inside(*shapes[k], st['lat'], st['lon'], st['alt']) for k in NAMES])


@pytest.fixture(scope='module')
def truth(ctx, areas):
    """The sim without sectors, stepped update by update: per update the masks of its state and
    sectorcount.py's sets; its final state."""
    shapes, _ = areas
    sim, ids = make_sim(ctx)
    m = truth_masks(shapes, sim.read())
    prev = [set(np.array(ids)[m[k]]) for k in range(len(NAMES))]
    ups = [dict(step=0, masks=m, ids=list(ids), count=[len(s) for s in prev], arrived=[[] for _ in NAMES],
                left=[[] for _ in NAMES])]
    steps = 0
    total = sum(b for b in BATCHES if b != 'change')
    change_at = sum(b for b in BATCHES[:BATCHES.index('change')])
    assert change_at % EVERY == 0
    while steps < total:
        if steps == change_at:
            d = deleted_indices(ups[-1]['masks'].any(axis=0))
            sim.delete(d)
            ids = [x for k, x in enumerate(ids) if k not in set(d)]
            st, new_ids = newcomers()
            sim.create(st)
            ids = ids + new_ids
        sim.step(EVERY)
        steps += EVERY
        m = truth_masks(shapes, sim.read())
        u = dict(step=steps, masks=m, ids=list(ids), count=[], arrived=[], left=[])
        for k in range(len(NAMES)):
            now = set(np.array(ids)[m[k]])               # sectorcount.py:60-66
            u['arrived'].append(sorted(now - prev[k]))
            u['left'].append(sorted(prev[k] - now))
            u['count'].append(len(now))
            prev[k] = now
        ups.append(u)
    return dict(updates=ups, final=sim.read(), deleted=d)


def run_plan(sim, ids, shapes_named):
    """The plan on a sim with sectors: [(steps so far, sectors(masks=True), row ids)] per poll, the final state."""
    sim.set_areas(shapes_named)
    sim.set_sectors(NAMES, EVERY, ids=ids)
    polls = [(0, sim.sectors(masks=True), sim.row_ids())]
    steps = 0
    for b in BATCHES:
        if b == 'change':
            # every rank deletes the same aircraft: the truth's choice
            sim.delete(run_plan.deleted)
            st, new_ids = newcomers()
            sim.create(st, ids=new_ids)
            continue
        sim.step(b)
        steps += b
        polls.append((steps, sim.sectors(masks=True), sim.row_ids()))
    return polls, sim.read()


@pytest.fixture(scope='module')
def resident_run(ctx, areas, truth):
    run_plan.deleted = truth['deleted']
    sim, ids = make_sim(ctx)
    polls, final = run_plan(sim, ids, areas[1])
    return dict(polls=polls, final=final)


def update_of(truth, step):
    return truth['updates'][step // EVERY]


def test_masks_counts_and_lists_at_each_update(truth, resident_run):
    seen = 0
    for steps, sec, rows in resident_run['polls']:
        u = update_of(truth, steps)
        for k, name in enumerate(NAMES):
            s = sec[name]
            assert s['step'] == u['step'], (steps, name)
            assert s['count'] == u['count'][k], (steps, name)
            if steps % EVERY == 0:      # the state read back is the state of the update
                assert np.array_equal(s['inside'], u['masks'][k][rows]), (steps, name)
            if steps == u['step'] and steps > 0:
                assert s['arrived'] == u['arrived'][k], (steps, name)
                assert s['left'] == u['left'][k], (steps, name)
                seen += len(s['arrived']) + len(s['left'])
    assert seen > 20    # aircraft did cross sector borders


def test_cumulative_counters_cover_every_update(truth, resident_run):
    for steps, sec, rows in resident_run['polls']:
        done = [u for u in truth['updates'] if 0 < u['step'] <= steps]
        for k, name in enumerate(NAMES):
            assert sec[name]['arrived_total'] == sum(len(u['arrived'][k]) for u in done), (steps, name)
            assert sec[name]['left_total'] == sum(len(u['left'][k]) for u in done), (steps, name)
    long_batch = [u for u in truth['updates'] if 3 * EVERY < u['step'] <= 6 * EVERY]
    assert sum(len(a) + len(b) for u in long_batch for a, b in zip(u['arrived'], u['left'])) > 0


def test_deleted_inside_aircraft_leave_once_and_new_ones_arrive(truth, resident_run):
    change_at = sum(b for b in BATCHES[:BATCHES.index('change')])
    after = [p for p in resident_run['polls'] if p[0] > change_at]
    gone = set(update_of(truth, change_at)['ids'][i] for i in truth['deleted'])
    first = {x for name in NAMES for x in after[0][1][name]['left_deleted']}
    assert first and first <= gone
    for name in NAMES:
        assert set(after[0][1][name]['left_deleted']) <= set(after[0][1][name]['left'])
        assert not after[1][1][name]['left_deleted'] and not gone & set(after[1][1][name]['left'])
    arrived_new = [x for p in after for name in NAMES for x in p[1][name]['arrived'] if x.startswith('NEW')]
    assert arrived_new      # created aircraft start outside and can arrive at the next update


def test_pass_is_read_only(truth, resident_run):
    for k, v in truth['final'].items():
        assert np.array_equal(v, resident_run['final'][k]), k


def test_errors_and_off(ctx, areas):
    sim, ids = make_sim(ctx)
    with pytest.raises(ValueError):
        sim.sectors()
    sim.set_areas(areas[1])
    with pytest.raises(ValueError):
        sim.set_sectors(['NOSUCH'], 1)
    with pytest.raises(Exception, match='every'):
        sim.set_sectors(NAMES, 0)
    with pytest.raises(Exception, match='at most'):
        sim.ctx.sim_set_sectors([0] * 65, 1)
    with pytest.raises(Exception, match='names shape'):
        sim.ctx.sim_set_sectors([len(areas[1])], 1)
    sim.set_sectors(NAMES, 1)
    sim.step(2)
    assert sim.sectors()['C']['step'] == 2
    sim.set_areas(areas[1])        # a new table forgets the sectors
    with pytest.raises(ValueError):
        sim.sectors()
    sim.step(1)


@pytest.mark.parametrize('set_after', [0, 1])
def test_abort_in_mid_batch_is_exact(ctx, areas, set_after):
    """A candidate list far too small, CD every 4th step (as tests/test_gpu_turbulence.py forces it): the
    batch of steps 1-12 completes steps 1-3, aborts at step 4 and re-runs from there.  Cadence 2.  Sectors
    set before step 0: the passes of the batch follow steps 1 and 3 (completed), then 5, 7 .. (re-run).
    Set after step 0: they follow step 2 (completed), step 4 (the aborted step: its pass returned behind
    the sticky word and runs again in the re-run), then 6, 8 ..  Either way every update is counted once:
    the poll and the state equal those of a twin on its own context that never aborts."""
    from bluesky_amd import _lib
    init = resident.initial_state(synth.box(5000, 120.0, seed=149))
    p = resident.params(simdt=SIMDT, cd_every=4)

    def run(c, batches, small):
        sim = resident.ResidentSim(init, p, ctx=c)
        sim.set_areas(areas[1])
        n_conf = []
        for k, b in enumerate(batches):
            if k == set_after:
                sim.set_sectors(NAMES, 2)
            if small:
                c.set_candidate_capacity(16)
            sim.step(b)
            n_conf.append(sim.stats()['n_conf'])
        return sim.ctx.sim_sectors_poll(masks=True), sim.read(), sim.stats(), n_conf

    twin = _lib.Context(0)
    try:
        exp, exp_state, exp_stats, n_conf = run(twin, [1, 4, 8], False)
    finally:
        twin.close()
    # the CD step that ends the twin's second batch is step 4: a list of 16 candidates cannot hold it,
    # so the run below did abort there
    assert n_conf[1] > 16
    assert exp['updates'] == 6 and exp['step'] == 12      # 13 or 12 steps since set_sectors
    assert int(exp['arrived_total'].sum() + exp['left_total'].sum()) > 0     # aircraft did cross sector borders
    c = _lib.Context(0)
    try:
        got, state, stats, _ = run(c, [1, 12], True)
    finally:
        c.close()
    assert sorted(got) == sorted(exp)
    for k in exp:
        assert np.array_equal(got[k], exp[k]), k
    for k in exp_state:
        assert np.array_equal(state[k], exp_state[k]), k
    assert stats == exp_stats


def test_two_ranks_equal_one(areas, truth, resident_run):
    def fn(rank, c, group):
        sim, ids = make_sim(c, rank, 2, group)
        polls, _ = run_plan(sim, ids, areas[1])
        return [(steps, {n: {k: v for k, v in s.items() if not k.startswith('inside')} for n, s in sec.items()})
                for steps, sec, rows in polls]

    parts = run_ranks(2, fn)
    for q, (steps, sec, rows) in enumerate(resident_run['polls']):
        assert parts[0][q][0] == steps
        merged = dist.merge_sectors([parts[0][q][1], parts[1][q][1]])
        for name in NAMES:
            one = {k: v for k, v in sec[name].items() if not k.startswith('inside')}
            assert merged[name] == one, (steps, name)
