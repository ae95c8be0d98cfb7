"""Symmetric prefilter sweep: when rows and columns are the
same aircraft, K0d lists each unordered pair of 512-aircraft tiles once and the
sweep refines the stage-1 survivors of an off-diagonal item in both
orientations.  It only removes repeated stage-1 work, so every result is
BITWISE that of the sweep of both orders and of the unpruned detect.

N = 1 300 in a 60 NM box: three tiles, the last one partial (276 rows, a
20-row last slice) -- diagonal and upper tile pairs, the dropped lower ones and
the padding -- with thousands of conflict pairs."""
import os
import sys

import numpy as np
import pytest

from bluesky_amd import _lib, resident, statebased, synth
from tests.util import same

pytestmark = pytest.mark.gpu

RPZ, HPZ, TLA = synth.RPZ, synth.HPZ, synth.TLOOKAHEAD
N, L = 1300, 60.0
FIELDS = ('ci', 'cj', 'li', 'lj', 'inconf', 'tcpamax', 'qdr', 'dist', 'tcpa', 'tinconf')
TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')


@pytest.fixture(scope='module')
def traffic():
    return synth.box(N, L, seed=31)


def detect(ctx, own, intr, sym, **kw):
    """One drop-in detect with the symmetric sweep allowed or not: (results,
    whether its plan was symmetric, stage-1 blocks swept)."""
    ctx.set_symmetric_sweep(sym)
    try:
        o = statebased.detect_indices(own, intr, RPZ, HPZ, TLA, ctx=ctx, **kw)
        return o, ctx.symmetric_sweep_stats()['last'], ctx.last_tiles()[2]
    finally:
        ctx.set_symmetric_sweep(True)


def bitwise(a, b):
    for k in FIELDS:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == 'f'), k


def test_symmetric_equals_both_orders_equals_noprune(ctx, traffic):
    on, planned, g_on = detect(ctx, traffic, traffic, True)
    off, planned_off, g_off = detect(ctx, traffic, traffic, False)
    full, planned_np, _ = detect(ctx, traffic, traffic, True, noprune=True)
    assert planned and not planned_off and not planned_np
    assert len(on['ci']) > 2000 and len(on['li']) > 0
    bitwise(on, off)
    bitwise(on, full)
    assert 0 < g_on < g_off


def run_sim(ctx, init, p, batches, sym):
    ctx.set_symmetric_sweep(sym)
    try:
        sim = resident.ResidentSim(init, p, ctx=ctx)
        t0, s0 = ctx.tile_reuse_stats(), ctx.symmetric_sweep_stats()
        out = []
        for k in batches:
            sim.step(k)
            st = sim.stats()
            out.append((sim.read(), ctx.fetch_pairs(st['n_conf'], st['n_los'])))
        t, s = ctx.tile_reuse_stats(), ctx.symmetric_sweep_stats()
        return out, {k: t[k] - t0[k] for k in t}, s['detects'] - s0['detects']
    finally:
        ctx.set_symmetric_sweep(True)


def test_resident_steps_are_bitwise(ctx, traffic):
    """40 steps with MVP: state and pairs after each batch, over kept
    symmetric tile-pair lists and at least one rebuild of one."""
    init = resident.initial_state(traffic)
    p = resident.params(simdt=1.0, swresohoriz=False)   # 250 m per step: the list is rebuilt every few detects
    batches = [1, 9, 10, 20]
    exp, _, n_off = run_sim(ctx, init, p, batches, False)
    got, tile, n_on = run_sim(ctx, init, p, batches, True)
    print('tile-pair list: %r, symmetric detects %d / %d' % (tile, n_on, n_off))
    same(got, exp)
    assert sum(len(x[1]['ci']) for x in exp) > 0
    assert n_off == 0 and n_on >= 40
    assert tile['builds'] >= 2 and tile['detects'] - tile['builds'] >= 3, tile


@pytest.mark.parametrize('case', ['distinct', 'rows', 'kwik', 'stage1_t0'])
def test_fallbacks_keep_todays_sweep(ctx, traffic, case):
    intr, kw = traffic, {}
    if case == 'distinct':
        intr = synth.box(N, L, seed=37)
    elif case == 'rows':
        kw = dict(row_begin=70, row_end=1100)
    else:
        kw = {case: True}
    on, planned, g_on = detect(ctx, traffic, intr, True, **kw)
    off, planned_off, g_off = detect(ctx, traffic, intr, False, **kw)
    assert not planned and not planned_off
    bitwise(on, off)
    assert g_on == g_off
    assert len(on['ci']) > 0


def test_always_kept_inputs_under_the_mirror(ctx):
    """Aircraft the refine must keep whatever it computes -- NaN velocity,
    lat = 0, a latitude whose rho' < 0.05 (reach: infinite), faster than
    400 m/s -- spread over the box at the equator, so each meets aircraft of
    other tiles as the row and as the column of a mirrored item."""
    t = synth.box(N, L, seed=41, lat0=0.0, lon0=4.0)
    t.gs[100] = np.nan
    t.lat[500] = 0.0
    t.lat[700:704] = 87.6 + 0.02 * np.arange(4)     # cos(lat) = 0.042
    t.lon[700:704] = 4.0 + 0.3 * np.arange(4)
    t.alt[700:704] = t.alt[700]
    t.gs[900] = 450.0
    t.gs[1290] = 430.0                              # (the partial tile)
    on, planned, _ = detect(ctx, t, t, True)
    off, _, _ = detect(ctx, t, t, False)
    full, _, _ = detect(ctx, t, t, True, noprune=True)
    assert planned
    bitwise(on, full)
    bitwise(on, off)
    assert len(on['ci']) > 2000 and np.isnan(on['tcpamax']).any()
    for k in (500, 900, 1290):   # (finite ones: in conflict as a row and as a column)
        assert (on['ci'] == k).any() and (on['cj'] == k).any(), k


def test_work_count_matches_the_model(ctx, traffic):
    """`groups` (the 64 x 8 stage-1 blocks swept) with the symmetric sweep is the
    host model's diagonal + upper count, within the model's own slack against
    the device (fp64 records and keys there, fp32 here; measured: see below),
    and strictly below the count of both orders."""
    sys.path.insert(0, TOOLS)
    try:
        from sym_model import sym_model
    finally:
        sys.path.remove(TOOLS)
    m = sym_model(traffic)['blocks']
    _, planned, g_on = detect(ctx, traffic, traffic, True)
    _, _, g_off = detect(ctx, traffic, traffic, False)
    print('model: %r; device: symmetric %d, both orders %d' % (m, g_on, g_off))
    assert planned and g_on < g_off
    # the slack the model has against today's sweep bounds the symmetric one's
    # (MI355X: model 2 262 symmetric / 3 408 both orders, device 2 271 / 3 423 -- the device's
    # fp32 boxes keep 9 / 15 blocks more, 0.4 %)
    slack = abs(g_off - m['today'])
    assert slack <= 0.01 * m['today'], (g_off, m)
    assert abs(g_on - m['sym']) <= slack, (g_on, m, slack)


def test_overflow_regrows_and_reruns(traffic):
    """A candidate capacity far below the demand (a mirrored item emits up to
    twice the candidates per batch): the detect overflows, regrows the list and
    re-runs -- bitwise the run with ample capacity."""
    small, ample = _lib.Context(0), _lib.Context(0)
    try:
        small.set_candidate_capacity(256)
        got, planned, _ = detect(small, traffic, traffic, True)
        exp, _, _ = detect(ample, traffic, traffic, True)
        assert planned
        assert small.last_candidates() > 256
        bitwise(got, exp)
        again, _, _ = detect(small, traffic, traffic, True)   # (the grown list, no retry)
        bitwise(again, exp)
    finally:
        small.close()
        ample.close()
