"""Triangular sweep inside a diagonal tile pair (sweep level
2): slice q of tile t against column tile t skips the column sub-groups below
its own 64 columns -- the items of the slices below cover those pairs -- and
refines the survivors above them in both orientations.  It only removes
repeated stage-1 work, so every result is BITWISE that of level 1 (each
unordered tile pair once), of level 0 (both orders) and of the unpruned
detect.

Every test sets its level and leaves level 2 behind (the session's context
may arrive at level 1 from the symmetric-sweep tests)."""
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
# one-tile sizes and the box side [NM] of each (hundreds to thousands of
# conflict pairs by the oracle on the CPU: 224 at N = 64 / 8 NM, 938 at
# 128 / 10 NM, 6 309 at 512 / 20 NM): the last slice or sub-group has 1, 6 or
# 8 members -- slice, sub-group and tile boundaries; N <= 64: the mask is a no-op
SIZES = {64: 8.0, 65: 8.0, 70: 8.0, 128: 10.0, 129: 10.0, 512: 20.0, 513: 20.0, 520: 20.0}


@pytest.fixture(scope='module')
def traffic():
    return synth.box(N, L, seed=31)


def detect(ctx, t, level, **kw):
    """One drop-in detect of t against itself at a sweep level: (results, the
    level its plan took, stage-1 blocks swept)."""
    ctx.set_sweep_level(level)
    try:
        o = statebased.detect_indices(t, t, RPZ, HPZ, TLA, ctx=ctx, **kw)
        return o, ctx.symmetric_sweep_stats()['level'], ctx.last_tiles()[2]
    finally:
        ctx.set_sweep_level(2)


def bitwise(a, b):
    for k in FIELDS:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == 'f'), k


def test_three_tiles_every_level_and_noprune(ctx, traffic):
    """Three tiles, the last partial (276 rows, a 20-row last slice, a 4-column
    last sub-group)."""
    tri, l2, g2 = detect(ctx, traffic, 2)
    sym, l1, g1 = detect(ctx, traffic, 1)
    both, l0, g0 = detect(ctx, traffic, 0)
    full, lnp, _ = detect(ctx, traffic, 2, noprune=True)
    assert (l2, l1, l0, lnp) == (2, 1, 0, 0)
    s = ctx.symmetric_sweep_stats()
    assert s['last'] is False and s['level'] == 0       # (the unpruned detect)
    assert len(tri['ci']) > 2000 and len(tri['li']) > 0
    bitwise(tri, sym)
    bitwise(tri, both)
    bitwise(tri, full)
    assert 0 < g2 < g1 < g0


def test_one_tile_dense(ctx):
    """One tile: every pair goes through the triangular path (N = 500 in 20 NM:
    6 195 conflict pairs by the oracle)."""
    t = synth.box(500, 20.0, seed=43)
    tri, l2, _ = detect(ctx, t, 2)
    full, _, _ = detect(ctx, t, 2, noprune=True)
    assert l2 == 2 and len(tri['ci']) > 5000
    bitwise(tri, full)


@pytest.mark.parametrize('n', sorted(SIZES))
def test_slice_subgroup_and_tile_boundaries(ctx, n):
    t = synth.box(n, SIZES[n], seed=47)
    tri, l2, _ = detect(ctx, t, 2)
    full, _, _ = detect(ctx, t, 2, noprune=True)
    assert l2 == 2 and len(tri['ci']) > 200
    bitwise(tri, full)


def test_always_kept_inputs_inside_one_tile(ctx):
    """Aircraft the refine must keep whatever it computes -- NaN ground speed,
    lat = 0, four with cos(lat) < 0.05, two faster than 400 m/s -- in one
    tile at the equator: each meets the others as a row above, inside and
    below its own slice's columns."""
    t = synth.box(500, 30.0, seed=41, lat0=0.0, lon0=4.0)
    t.gs[100] = np.nan
    t.lat[200] = 0.0
    t.lat[300:304] = 87.6 + 0.02 * np.arange(4)     # cos(lat) = 0.042
    t.lon[300:304] = 4.0 + 0.3 * np.arange(4)
    t.alt[300:304] = t.alt[300]
    t.gs[400] = 450.0
    t.gs[450] = 430.0
    tri, l2, _ = detect(ctx, t, 2)
    full, _, _ = detect(ctx, t, 2, noprune=True)
    assert l2 == 2
    bitwise(tri, full)
    assert len(tri['ci']) > 2000 and np.isnan(tri['tcpamax']).any()
    for k in (200, 400, 450):   # (finite ones: in conflict as a row and as a column)
        assert (tri['ci'] == k).any() and (tri['cj'] == k).any(), k


def test_work_count_matches_the_model(ctx, traffic):
    """`groups` (the 64 x 8 stage-1 blocks swept) at level 2 is the host
    model's `tri` count within the slack the device shows against the model at
    level 0 (fp64 records and keys there, fp32 here), and strictly below level
    1's.  The model: 1 740 / 2 262 / 3 408 at levels 2 / 1 / 0."""
    sys.path.insert(0, TOOLS)
    try:
        from sym_model import sym_model
    finally:
        sys.path.remove(TOOLS)
    m = sym_model(traffic)['blocks']
    assert (m['tri'], m['sym'], m['today']) == (1740, 2262, 3408), m
    _, l2, g2 = detect(ctx, traffic, 2)
    _, _, g1 = detect(ctx, traffic, 1)
    _, _, g0 = detect(ctx, traffic, 0)
    print('model: %r; device: level 2 %d, level 1 %d, level 0 %d' % (m, g2, g1, g0))
    assert l2 == 2 and g2 < g1 < g0
    slack = abs(g0 - m['today'])
    assert slack <= 0.01 * m['today'], (g0, m)
    assert abs(g2 - m['tri']) <= slack, (g2, m, slack)


def run_sim(ctx, init, p, batches, levels):
    """The resident sim over `batches`, the sweep level set to levels[k] before
    batch k: [(state, pairs)] per batch, the tile-pair list's builds / detects
    of each batch, the symmetric detects."""
    try:
        ctx.set_sweep_level(levels[0])
        sim = resident.ResidentSim(init, p, ctx=ctx)
        s0 = ctx.symmetric_sweep_stats()
        out, tiles = [], []
        for q, (k, b) in enumerate(zip(levels, batches)):
            if q and k != levels[q - 1]:     # (the setter drops the kept list whatever the level)
                ctx.set_sweep_level(k)
            t0 = ctx.tile_reuse_stats()
            sim.step(b)
            st = sim.stats()
            out.append((sim.read(), ctx.fetch_pairs(st['n_conf'], st['n_los'])))
            t = ctx.tile_reuse_stats()
            tiles.append({f: t[f] - t0[f] for f in t})
            assert ctx.symmetric_sweep_stats()['level'] == k
        return out, tiles, ctx.symmetric_sweep_stats()['detects'] - s0['detects']
    finally:
        ctx.set_sweep_level(2)


def test_resident_steps_are_bitwise(ctx, traffic):
    """40 steps with MVP: state and pairs after each batch, over kept
    triangular tile-pair lists and at least one rebuild of one."""
    init = resident.initial_state(traffic)
    p = resident.params(simdt=1.0, swresohoriz=False)   # 250 m per step: the list is rebuilt every few detects
    batches = [1, 9, 10, 20]
    exp, _, n0 = run_sim(ctx, init, p, batches, [0] * 4)
    got, tiles, n2 = run_sim(ctx, init, p, batches, [2] * 4)
    builds, detects = sum(t['builds'] for t in tiles), sum(t['detects'] for t in tiles)
    print('tile-pair list: %r, symmetric detects %d / %d' % (tiles, n2, n0))
    same(got, exp)
    assert sum(len(x[1]['ci']) for x in exp) > 0
    assert n0 == 0 and n2 >= 40
    assert builds >= 2 and detects - builds >= 3, tiles


def test_level_switch_rebuilds_the_kept_list(traffic):
    """The level is part of the kept tile-pair list's key: a batch after a
    switch builds a new list, a batch without one keeps it (no resolution and
    12 m per step at the default simdt: every record stays within the list's
    budgets, no rebuild of its own), results bitwise level 0's.  A context of
    its own: the session's may carry other tests' reuse budgets."""
    init = resident.initial_state(traffic)
    p = resident.params(reso=False)
    batches, levels = [5, 5, 5, 5, 5], [2, 2, 1, 2, 2]
    own = _lib.Context(0)
    try:
        exp, _, _ = run_sim(own, init, p, batches, [0] * 5)
        got, tiles, _ = run_sim(own, init, p, batches, levels)
    finally:
        own.close()
    print('tile-pair list per batch: %r' % (tiles,))
    same(got, exp)
    assert sum(len(x[1]['ci']) for x in exp) > 0
    b = [t['builds'] for t in tiles]
    assert b[0] >= 1 and b[1] == 0 and b[2] >= 1 and b[3] >= 1 and b[4] == 0, tiles
    assert tiles[1]['detects'] > 0 and tiles[4]['detects'] > 0, tiles   # (kept lists swept)


def test_overflow_regrows_and_reruns(traffic):
    """A candidate capacity far below the demand: the level-2 detect
    overflows, regrows the list and re-runs -- bitwise the run with ample
    capacity."""
    small, ample = _lib.Context(0), _lib.Context(0)
    try:
        small.set_candidate_capacity(256)
        got, l2, _ = detect(small, traffic, 2)
        exp, _, _ = detect(ample, traffic, 2)
        assert l2 == 2
        assert small.last_candidates() > 256
        bitwise(got, exp)
        again, _, _ = detect(small, traffic, 2)   # (the grown list, no retry)
        bitwise(again, exp)
    finally:
        small.close()
        ample.close()


def test_a_fresh_context_is_at_level_two_and_refuses_others(traffic):
    c = _lib.Context(0)
    try:
        statebased.detect_indices(traffic, traffic, RPZ, HPZ, TLA, ctx=c)
        s = c.symmetric_sweep_stats()      # (detects: a first detect may regrow its lists and re-run)
        assert s['detects'] >= 1 and s['last'] is True and s['level'] == 2, s
        for bad in (3, -1):
            with pytest.raises(_lib.AccelError):
                c.set_sweep_level(bad)
        c.set_symmetric_sweep(True)               # (a bool maps to 0 / 1)
        statebased.detect_indices(traffic, traffic, RPZ, HPZ, TLA, ctx=c)
        assert c.symmetric_sweep_stats()['level'] == 1
    finally:
        c.close()
