"""Every K2 placement and fold path of the detect and the resident step against
the oracle ("K2 paths"), on traffic whose per-row pair counts are
known in advance (tests/clique_traffic.py; the counts themselves are checked
on the CPU by tests/test_clique_traffic.py and again here, from the oracle
result each test already has).

Which path a detect takes depends on the bucket width B (8: the whole bucket
in one go; 16 / 32 / 64: the generic loop; 0: scan + k_scatter + k_rank, MVP's
fold and K4' as launches of their own), on whether a 512-row block's conflict
pairs fit LDS (tc <= kRankLds = 1536: MVP folded from LDS, else through global
memory) and on the launch form (K2 fused with K4' or not, K4' preparing the
next detect or not).  Every test opens a context of its own and sets its bucket
width, so no path is inherited from an earlier test:

  case  traffic                          width   path
  a     430 cliques of 3                 8       B == 8, every block LDS (1024 per full block)
  b     320 cliques of 4                 8       full blocks hold exactly 1536 pairs: tc == kRankLds
  c     320 cliques of 4, one of 5       8       a block just over 1536 next to blocks that are not
  d     258 cliques of 5                 8       B == 8, global fold in the full blocks, LDS in the partial one
  e     144 cliques of 9                 8       every bucket exactly full (8 of 8), no retry
  f     129 cliques of 10                8, 16   9 per row: 8 overflows and re-runs at 16; equal to 16 set directly
  g     20 cliques of 65                 64      every bucket exactly full at the widest width
  h     20 cliques of 66                 64, 0   65 per row: scatter, by growth from 64 and set directly
  i     box + cliques of 30 and 70       8       growth 8 -> scatter in one detect on mixed density
  j     box + clique of 12               8       growth to 16: the generic bucket loop with the LDS fold

Tolerance: the project's bar unchanged (tests/util.py RTOL, tests/test_gpu_sim.py
SCALES).  Clique pairs are close (down to 4 m) and MVP divides by small
distances, so the oracle's own conditioning was measured on the CPU: three
oracle steps per case (horizontal, and horizontal + vertical resolution), each
repeated with every input moved one ulp by np.nextafter, up or down by a hash
of the value's own bits.  Equal values so stay equal and an exact 0 stays 0:
MVP branches on vs1 == vs2 (MVP.py:200-215), ties that the
device and the oracle see alike because every step starts from the same state;
moved independently, the level members of a clique (equal vs in every step)
change branch and asas.vs by tens of m/s, which says nothing about rounding.
Pair lists, active and n_conf never changed between the two runs.  The largest
difference in units of util.close's tolerance is in ORACLE_NUDGE below (1 =
1e-9 relative), with the final seeds of tests/clique_traffic.py CASES: 101-107,
109, 110 at the first try; case h at seed 108 reached 1.92 on asas.vs with
vertical resolution (2.99 on asas.trk at 0.5 NM jitter), so g and h use 1 NM
jitter and h seed 408 (seeds 208: 0.40, 308: 6.4).  Every figure is below 1."""
import contextlib
import functools

import numpy as np
import pytest

from bluesky_amd import _lib, resident, statebased, synth
from oracle import statebased as ocd
from oracle import step as ostep
from tests import clique_traffic as ct
from tests import util
from tests.test_gpu_sim import compare, full_state, oracle_params

pytestmark = pytest.mark.gpu

RPZ, HPZ, TLA = synth.RPZ, synth.HPZ, synth.TLOOKAHEAD
RANK_ROWS, RANK_LDS = 512, 1536     # kRankRows, kRankLds (bsa_cd_args.h)
ALL = sorted(ct.CASES)
PAIR_FIELDS = ('ci', 'cj', 'qdr', 'dist', 'tcpa', 'tinconf', 'li', 'lj', 'inconf', 'tcpamax')

# oracle vs oracle with one-ulp inputs, worst |difference| / util.close tolerance over
# 3 steps: (horizontal resolution incl. the detect's reals, horizontal + vertical)
ORACLE_NUDGE = {
    'a': (0.016, 0.016), 'b': (0.028, 0.027), 'c': (0.17, 0.14), 'd': (0.039, 0.039), 'e': (0.15, 0.15),
    'f': (0.29, 0.44), 'g': (0.32, 0.29), 'h': (0.30, 0.30), 'i': (0.15, 0.15), 'j': (0.025, 0.025),
}


@functools.lru_cache(maxsize=None)
def traffic(name):
    return ct.case(name)


@functools.lru_cache(maxsize=None)
def oracle0(name):
    """The oracle detect of the case's initial traffic: computed once, shared, read-only."""
    t = traffic(name)
    r = ocd.detect_arrays(t, t, RPZ, HPZ, TLA, want_dcpa=True)
    for v in r.values():
        v.setflags(write=False)
    ct.check_clique_counts(t, r)
    return r


@contextlib.contextmanager
def fresh(width):
    """A context of its own with a known bucket width."""
    c = _lib.Context(0)
    try:
        c.set_row_bucket(width)
        yield c
    finally:
        c.close()


def block_sums(counts, order):
    c = counts[order]
    return [int(c[k:k + RANK_ROWS].sum()) for k in range(0, len(c), RANK_ROWS)]


@functools.lru_cache(maxsize=None)
def home_blocks(name):
    """The conflict pairs of each 512-row K2 block of the resident step, whose rows
    are in home order: a scratch sim playing rank r of 3 names the aircraft of
    homes [512 r, 512 (r + 1)); their rows' counts are the oracle's."""
    t = traffic(name)
    nc, _ = ct.row_counts(oracle0(name), t.ntraf)
    with fresh(8) as c:
        resident.ResidentSim(resident.initial_state(t), resident.params(), ctx=c)
        ids = []
        for r in range(3):
            c.sim_probe_rank(r, 3)
            ids.append(c.sim_row_ids())
    assert [len(i) for i in ids[:2]] == [RANK_ROWS, RANK_ROWS] and 0 < len(ids[2]) < RANK_ROWS
    assert np.array_equal(np.sort(np.concatenate(ids)), np.arange(t.ntraf))
    return [int(nc[i].sum()) for i in ids]


def check_fold_mix(name, blocks):
    """The LDS / global fold mix the case promises, for the given block sums."""
    if name == 'a':
        assert blocks[:2] == [1024, 1024] and blocks[2] <= RANK_LDS, blocks
    if name == 'b':
        assert blocks[:2] == [RANK_LDS, RANK_LDS], blocks
    if name == 'c':
        assert RANK_LDS < max(blocks) <= RANK_LDS + 5 and min(blocks[:2]) >= RANK_LDS, blocks
        assert sum(b <= RANK_LDS for b in blocks) >= 1, blocks
    if name == 'd':
        assert min(blocks[:2]) > RANK_LDS and blocks[2] <= RANK_LDS, blocks
    if name == 'j':
        assert max(blocks) <= RANK_LDS, blocks


def initial(name):
    t = traffic(name)
    init = resident.initial_state(t)
    prev = dict(init)
    prev.update(asas_trk=init['trk'].copy(), asas_tas=init['tas'].copy(),
                asas_vs=np.zeros(t.ntraf), active=np.zeros(t.ntraf, bool))
    return t, init, prev


def oracle_detect(name, k, prev, p):
    """Step 0 detects the initial traffic (the shared result); later steps their own state."""
    if k == 0:
        return oracle0(name)
    traf = {f: prev[f] for f in ('lat', 'lon', 'trk', 'gs', 'alt', 'vs')}
    return ocd.detect_arrays(traf, traf, p.rpz, p.hpz, p.tla)


def fetched(c, sim):
    st = sim.stats()
    return c.fetch_pairs(st['n_conf'], st['n_los'])


# ---------------------------------------------------------------- stand-alone detect
@pytest.mark.parametrize('name', ALL)
def test_standalone_detect_matches_oracle(name):
    """bsa_detect (rows in aircraft-index order) at each width of the case: pair
    order and inconf exact, reals and tcpamax within RTOL, also with dcpa; the
    first detect of a too narrow width is the retried one, the second runs at
    the grown width directly; the case's widths agree bitwise."""
    t, exp = traffic(name), oracle0(name)
    nc, _ = ct.row_counts(exp, t.ntraf)
    check_fold_mix(name, block_sums(nc, np.arange(t.ntraf)))
    runs = []
    for w in ct.CASES[name]['widths']:
        with fresh(w) as c:
            got = statebased.detect_indices(t, t, RPZ, HPZ, TLA, ctx=c)
            util.assert_detect_equal(got, exp, RPZ, TLA)
            again = statebased.detect_indices(t, t, RPZ, HPZ, TLA, ctx=c, with_dcpa=True)
            util.assert_detect_equal(again, exp, RPZ, TLA)
            ok, msg = util.close(again['dcpa'], exp['dcpa'], RPZ)
            assert ok, 'dcpa: %s' % msg
            for f in PAIR_FIELDS:
                assert np.array_equal(got[f], again[f]), f
            runs.append(again)
    for other in runs[1:]:
        for f in PAIR_FIELDS + ('dcpa',):
            assert np.array_equal(other[f], runs[0][f]), f


# ---------------------------------------------------------------- resident step
VARIANTS = {'cd1': dict(cd_every=1), 'cd2': dict(cd_every=2), 'hv': dict(cd_every=1, swresohoriz=False)}


@pytest.mark.parametrize('variant', sorted(VARIANTS))
@pytest.mark.parametrize('name', ALL)
def test_resident_steps_match_oracle(name, variant):
    """Three re-anchored steps (rows in home order) against oracle/step.py: CD
    every step (K2 fused with K4', K4' preparing the next detect), every second
    step (non-CD steps, K4' with and without the preparation) and with vertical
    resolution acting; the pair list of every CD step against the oracle detect
    of the same state."""
    t, init, prev = initial(name)
    check_fold_mix(name, home_blocks(name))
    p = resident.params(**VARIANTS[variant])
    op = oracle_params(p)
    with fresh(ct.CASES[name]['widths'][0]) as c:
        sim = resident.ResidentSim(init, p, ctx=c)
        for k in range(3):
            cd = k % p.cd_every == 0
            r = oracle_detect(name, k, prev, p) if cd else None
            exp = ostep.sim_step(prev, op, do_cd=cd, cd=r)
            sim.step(1)
            got = full_state(init, sim.read())
            compare(got, exp, k)
            if cd:
                assert sim.stats()['n_conf'] == exp['n_conf'] == len(r['ci']) > 0
                util.assert_detect_equal(fetched(c, sim), r, p.rpz, p.tla)
            prev = got
        assert sim.stats()['steps'] == 3 and sim.stats()['cd_calls'] == (3 + p.cd_every - 1) // p.cd_every


@pytest.mark.parametrize('name', ['a', 'd', 'h', 'i'])
def test_resident_resume_nav_matches_oracle(name):
    """resume_nav (K2 and K4' never fused, the bookkeeping on) against
    oracle/asas.py composed into the step; the cliques are in LoS, so every
    resopair persists."""
    from oracle import asas as oasas
    t, init, prev = initial(name)
    p = resident.params(cd_every=1, resume_nav=True)
    op = oracle_params(p)
    bk = oasas.Bookkeeping(t.ntraf)
    with fresh(ct.CASES[name]['widths'][0]) as c:
        sim = resident.ResidentSim(init, p, ctx=c)
        for k in range(3):
            r = oracle_detect(name, k, prev, p)
            exp = ostep.sim_step(prev, op, do_cd=True, bk=bk, cd=r)
            sim.step(1)
            got = full_state(init, sim.read())
            compare(got, exp, k)
            i, j = sim.resopairs()
            assert list(zip(i.tolist(), j.tolist())) == sorted(bk.resopairs), 'step %d resopairs' % k
            assert sim.asas_stats() == dict(
                resopairs=len(bk.resopairs), confpairs_unique=len(bk.confpairs_unique),
                lospairs_unique=len(bk.lospairs_unique), confpairs_all=bk.confpairs_all,
                lospairs_all=bk.lospairs_all, active=int(exp['active'].sum())), k
            util.assert_detect_equal(fetched(c, sim), r, p.rpz, p.tla)
            prev = got
    assert len(bk.resopairs) >= len(oracle0(name)['ci']) > 0


def run_world1(name, width, p, steps=3):
    """[(state, fetched pairs)] per step of a one-rank run on a fresh context."""
    _, init, _ = initial(name)
    out = []
    with fresh(width) as c:
        sim = resident.ResidentSim(init, p, ctx=c)
        for _ in range(steps):
            sim.step(1)
            out.append((sim.read(), fetched(c, sim)))
    return out


@pytest.mark.parametrize('name', ['f', 'h'])
def test_resident_widths_agree_bitwise(name):
    """The step that overflows its buckets and re-runs wider (f: 8 -> 16; h: 64 ->
    scatter) against the one set to the final width from the start."""
    p = resident.params(cd_every=1, swresohoriz=False)
    w0, w1 = ct.CASES[name]['widths']
    a, b = run_world1(name, w0, p), run_world1(name, w1, p)
    util.same(a, b)
    assert len(a[-1][1]['ci']) == len(oracle0(name)['ci'])


@pytest.mark.parametrize('world', [2, 3])
@pytest.mark.parametrize('name', ['a', 'd', 'h'])
def test_sharded_steps_equal_world1(name, world):
    """In-process ranks (rows are a slice of the columns: rb > 0 on every rank but
    the first; K2 and K4' never fused): state and gathered pair lists bitwise
    those of one rank."""
    from tests.test_gpu_multirank import run_ranks
    _, init, _ = initial(name)
    p = resident.params(cd_every=1, swresohoriz=False)
    width = ct.CASES[name]['widths'][0]
    exp = run_world1(name, width, p)

    def rank(r, c, g):
        c.set_row_bucket(width)
        sim = resident.ResidentSim(init, p, ctx=c, rank=r, world=world, group=g)
        out = []
        for _ in range(3):
            sim.step(1)
            out.append((sim.read(), sim.gather_pairs(root=0)))
        return out, sim.stats()

    res = run_ranks(world, rank)
    util.same(res[0][0], exp)
    for got, _ in res[1:]:
        for k, (state, pairs) in enumerate(got):
            assert pairs is None
            for f, v in exp[k][0].items():
                assert np.array_equal(state[f], v), 'step %d %s' % (k, f)
    begins = [st['row_begin'] for _, st in res]
    assert begins[0] == 0 and all(b > 0 and b % RANK_ROWS == 0 for b in begins[1:]), begins
    assert sum(st['n_conf'] for _, st in res) == len(exp[-1][1]['ci']) > 0


@pytest.mark.parametrize('name', ['d', 'i'])
def test_sweep_levels_and_noprune_agree_bitwise(name):
    """Dense rows inside one tile (the sweep tests' uniform boxes have none): the
    detect at sweep levels 0, 1, 2 and unpruned, bitwise equal (level 2 is the
    one test_standalone_detect_matches_oracle compares with the oracle)."""
    t = traffic(name)
    runs = []
    for level, noprune in ((2, False), (1, False), (0, False), (2, True)):
        with fresh(ct.CASES[name]['widths'][0]) as c:
            c.set_sweep_level(level)
            runs.append(statebased.detect_indices(t, t, RPZ, HPZ, TLA, ctx=c, noprune=noprune, with_dcpa=True))
            if not noprune:
                assert c.symmetric_sweep_stats()['level'] == level
    assert np.array_equal(runs[0]['ci'], oracle0(name)['ci'])
    for other in runs[1:]:
        for f in PAIR_FIELDS + ('dcpa',):
            assert np.array_equal(other[f], runs[0][f]), f
