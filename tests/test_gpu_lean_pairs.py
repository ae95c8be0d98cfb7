"""Lean pair placement of the resident step (StepPlan::lean): in one step() call every CD step
that a later CD step of the same call follows runs K2 + K4' without the block sums and without placing ci / cj /
out / li / lj / rowoff, and gates MVP with the detect's "any conflict" word instead of P.  The call's last CD
step places everything, so after the call every array is BITWISE what it is with the lean form off
(Context.set_lean_pairs(False)) and what single-step calls (always full) leave.

"Bitwise" here: every array of sim.read(), every array of fetch_pairs, and sim.stats().

N = 1 300 in a 60 NM box as in test_gpu_symmetric_sweep.py: three 512-row K2 blocks, the last one partial, MVP
on.  The far-apart sets are cliques of one (tests/clique_traffic.py: sites more than 100 NM apart)."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from bluesky_amd import _lib, resident, synth
from oracle import statebased as ocd
from tests import clique_traffic as ct

pytestmark = pytest.mark.gpu

RPZ, HPZ, TLA = synth.RPZ, synth.HPZ, synth.TLOOKAHEAD
N, L, SEED = 1300, 60.0, 31
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = ('ci', 'cj', 'qdr', 'dist', 'tcpa', 'tinconf', 'li', 'lj', 'inconf', 'tcpamax')


def snapshot(c, sim):
    st = sim.stats()
    return sim.read(), c.fetch_pairs(st['n_conf'], st['n_los']), st


def bitwise(a, b):
    (sa, pa, ta), (sb, pb, tb) = a, b
    assert ta == tb, (ta, tb)
    assert sorted(sa) == sorted(sb)
    for f in sa:
        assert np.asarray(sa[f]).tobytes() == np.asarray(sb[f]).tobytes(), f
    for f in PAIRS:
        assert np.asarray(pa[f]).tobytes() == np.asarray(pb[f]).tobytes(), f


def run(init, p, batches, lean, setup=None, width=None, capacity=None):
    """step(k) for every k of `batches` on a context of its own: (snapshot after the last call, lean / full CD
    step counts, aborts)."""
    c = _lib.Context(0)
    try:
        c.set_lean_pairs(lean)
        if width is not None:
            c.set_row_bucket(width)
        sim = resident.ResidentSim(init, p, ctx=c)
        if setup:
            setup(sim)
        for k in batches:
            if capacity is not None and k == batches[-1]:
                c.set_candidate_capacity(capacity)
            assert sim.step(k) == k
        return snapshot(c, sim), c.lean_pairs_stats(), sim.aborts()
    finally:
        c.close()


def home_block_of(init, p):
    """The K2 block (512 rows in home order) of every aircraft, from a scratch sim playing rank r of 3."""
    c = _lib.Context(0)
    try:
        resident.ResidentSim(init, p, ctx=c)
        blk = np.full(len(init['lat']), -1)
        for r in range(3):
            c.sim_probe_rank(r, 3)
            blk[c.sim_row_ids()] = r
        assert (blk >= 0).all()
        return blk
    finally:
        c.close()


@pytest.fixture(scope='module')
def box():
    t = synth.box(N, L, seed=SEED)
    r = ocd.detect_arrays(t, t, RPZ, HPZ, TLA)
    return t, resident.initial_state(t), r


def test_lean_equals_full_equals_single_steps(box):
    t, init, r = box
    p = resident.params(simdt=1.0, swresohoriz=False)
    blk = home_block_of(init, p)
    assert len(np.unique(blk[r['ci']])) >= 2 and len(r['li']) >= 1     # (the oracle: conflicts in >= 2 blocks, LoS)
    lean, n_lean, _ = run(init, p, [12], True)
    full, n_full, _ = run(init, p, [12], False)
    ones, n_ones, _ = run(init, p, [1] * 12, True)
    assert n_lean == dict(lean=11, full=1) and n_full == dict(lean=0, full=12) and n_ones == dict(lean=0, full=12)
    assert len(lean[1]['ci']) > 0 and len(lean[1]['li']) > 0
    bitwise(lean, full)
    bitwise(lean, ones)


def test_lean_with_cd_every_two_keeps_the_last_detect_full(box):
    """cd_every = 2, 6 steps: CD steps 0, 2, 4 -- the last one is not the call's last step, and is full."""
    _, init, _ = box
    p = resident.params(simdt=1.0, cd_every=2)
    lean, n_lean, _ = run(init, p, [6], True)
    full, _, _ = run(init, p, [6], False)
    assert n_lean == dict(lean=2, full=1)
    bitwise(lean, full)


def test_gate_closed():
    t = ct.cliques([1] * 600, 211)
    r = ocd.detect_arrays(t, t, RPZ, HPZ, TLA)
    assert len(r['ci']) == 0 and len(r['li']) == 0
    init = resident.initial_state(t)
    p = resident.params(simdt=1.0)
    lean, n_lean, _ = run(init, p, [6], True)
    full, _, _ = run(init, p, [6], False)
    assert n_lean == dict(lean=5, full=1)
    bitwise(lean, full)
    s = lean[0]
    assert lean[2]['n_conf'] == 0 and not s['active'].any()
    assert np.array_equal(s['asas_trk'], init['trk']) and np.array_equal(s['asas_tas'], init['tas'])
    assert not s['asas_vs'].any() and np.array_equal(s['asas_alt'], init['asas_alt'])


def test_gate_opened_by_one_block():
    """1 100 aircraft far apart and one pair in conflict: every conflict row lies in one K2 block, the rows of the
    two other blocks resolve (asas targets written) only because that block's evaluation opened the gate."""
    t = ct.cliques([1] * 1100 + [2], 223)
    r = ocd.detect_arrays(t, t, RPZ, HPZ, TLA)
    assert sorted(r['ci'].tolist()) == sorted(np.flatnonzero(t.clique == 1100).tolist())
    init = resident.initial_state(t)
    p = resident.params(simdt=1.0)
    blk = home_block_of(init, p)
    assert len(np.unique(blk)) == 3 and len(np.unique(blk[r['ci']])) == 1
    lean, n_lean, _ = run(init, p, [6], True)
    full, _, _ = run(init, p, [6], False)
    assert n_lean == dict(lean=5, full=1)
    bitwise(lean, full)
    assert lean[0]['active'].sum() == 2


def test_fold_spill_and_bucket_growth():
    """Case f of the K2 path tests (129 cliques of 10, 9 pairs per row): width 8 overflows in the call's first,
    lean step, which re-runs at 16; every full block then holds ~4 600 conflict pairs > kRankLds = 1 536 and folds
    through its slice of pdv / pfl."""
    t = ct.case('f')
    init = resident.initial_state(t)
    p = resident.params(simdt=1.0, swresohoriz=False)
    lean, n_lean, ab = run(init, p, [4], True, width=8)
    full, _, _ = run(init, p, [4], False, width=8)
    assert ab >= 1 and n_lean == dict(lean=3, full=1)
    assert len(lean[1]['ci']) == 129 * 90
    bitwise(lean, full)


def _condition(sim):     # armed, never met: an altitude no aircraft reaches
    sim.set_conditions(idx=[3], condtype=[0], target=[1e6], lastdif=[1.0])


def _exparea(sim):       # a circle around everything: the pass runs, nobody leaves
    sim.set_areas({'ALL': ('CIRCLE', [52.0, 4.0, 5000.0], 1e9, -1e9)})
    sim.set_exparea('ALL', dt=1.0, every=1)


@pytest.mark.parametrize('case', ['resume_nav', 'condition', 'exparea', 'one_step'])
def test_plan_rule_keeps_these_full(box, case):
    _, init, _ = box
    p = resident.params(simdt=1.0, resume_nav=case == 'resume_nav')
    setup = {'condition': _condition, 'exparea': _exparea}.get(case)
    batches = [1] if case == 'one_step' else [6]
    on, n_on, _ = run(init, p, batches, True, setup)
    off, _, _ = run(init, p, batches, False, setup)
    assert n_on == dict(lean=0, full=batches[0])
    bitwise(on, off)


def test_plan_rule_world_two(box):
    from tests.test_gpu_multirank import run_ranks
    _, init, _ = box
    p = resident.params(simdt=1.0)
    exp, _, _ = run(init, p, [6], False)

    def rank(r, c, g):
        c.set_lean_pairs(True)
        sim = resident.ResidentSim(init, p, ctx=c, rank=r, world=2, group=g)
        sim.step(6)
        return sim.read(), sim.gather_pairs(root=0), c.lean_pairs_stats()

    res = run_ranks(2, rank)
    for state, _, n in res:
        assert n == dict(lean=0, full=6)
        for f, v in exp[0].items():
            assert np.asarray(state[f]).tobytes() == np.asarray(v).tobytes(), f
    for f in PAIRS:
        assert np.asarray(res[0][1][f]).tobytes() == np.asarray(exp[1][f]).tobytes(), f


def digest(snap):
    h = hashlib.sha256()
    for f in sorted(snap[0]):
        h.update(np.ascontiguousarray(snap[0][f]).tobytes())
    for f in PAIRS:
        h.update(np.ascontiguousarray(snap[1][f]).tobytes())
    return h.hexdigest()


CHILD = """
import sys
sys.path.insert(0, %r)
from bluesky_amd import _lib, resident, synth
from tests.test_gpu_lean_pairs import N, L, SEED, run, digest
init = resident.initial_state(synth.box(N, L, seed=SEED))
snap, n, _ = run(init, resident.params(simdt=1.0), [6], True)
print('RESULT', n['lean'], n['full'], digest(snap))
"""


def test_plan_rule_k24_off(box):
    """BSA_K24=0 (read once per process: a child process): K2 and K4' are two launches, no step is lean."""
    _, init, _ = box
    exp, _, _ = run(init, resident.params(simdt=1.0), [6], False)
    env = dict(os.environ, BSA_K24='0')
    r = subprocess.run([sys.executable, '-c', CHILD % REPO], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [x for x in r.stdout.splitlines() if x.startswith('RESULT')][0].split()
    assert line[1:3] == ['0', '6'] and line[3] == digest(exp)


def test_listing_after_a_lean_step(monkeypatch):
    """BSA_PF_HEAVY_US=0 lists every slot of the kept tile-pair list for the next detect: the same slots from the
    extra workgroups of a lean K2 + K4' as from k_rowblk in front of a full one, from the same state.  (Level 2 of
    set_lean_pairs makes the call's last CD step lean, so that the host can look at what it listed.)"""
    monkeypatch.setenv('BSA_PF_HEAVY_US', '0')
    init = resident.initial_state(synth.box(20000, 300.0, seed=109))
    p = resident.params(simdt=0.5, swresohoriz=False)
    got = {}
    for last in (2, 0):
        c = _lib.Context(0)
        try:
            sim = resident.ResidentSim(init, p, ctx=c)
            sim.step(4)     # (the listing rides on detects of a kept list: not the first ones)
            n0 = c.lean_pairs_stats()
            c.set_lean_pairs(last)
            sim.step(1)
            n = c.lean_pairs_stats()
            got[last] = (c.listed_items(0), c.listed_items(1), n['lean'] - n0['lean'], sim.read())
        finally:
            c.close()
    assert got[2][2] == 1 and got[0][2] == 0
    assert len(got[2][0]) + len(got[2][1]) > 0
    assert np.array_equal(got[2][0], got[0][0]) and np.array_equal(got[2][1], got[0][1])
    for f, v in got[0][3].items():
        assert np.asarray(got[2][3][f]).tobytes() == np.asarray(v).tobytes(), f


def test_candidate_overflow_in_a_lean_batch(box):
    """The 256-candidate list of the sweep tests, set before the second call: its first, lean step overflows,
    the list regrows, the call re-runs from that step under the same rule and ends bitwise the full run."""
    _, init, _ = box
    p = resident.params(simdt=1.0, swresohoriz=False)
    lean, n_lean, ab = run(init, p, [3, 6], True, capacity=256)
    full, _, ab_full = run(init, p, [3, 6], False, capacity=256)
    assert ab >= 1 and ab_full >= 1
    assert n_lean == dict(lean=2 + 5, full=2)
    bitwise(lean, full)
