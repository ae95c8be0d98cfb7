"""GPU: every optional stage of the resident step on at once -- ResumeNav's bookkeeping, OpenAP perf
and forces, FMS guidance with waypoint recovery, geovectors, turbulence, sector occupancy -- through one
aborted batch, bitwise against a twin on its own context that never aborts.  The per-stage abort tests
(test_gpu_fms, _recover, _geovector, _perf_forces, _turbulence, _sectors) each switch one stage on; here
the host clocks of all of them are replayed together and both undo sets are put back in one rollback.
Tables, routes and areas are those of the per-stage tests."""
import os

import numpy as np
import pytest

from bluesky_amd import _lib, fms, resident
from tests import geovec_np, util
from tests.test_gpu_geovector import GEOVECS, SIM_AREAS
from tests.test_gpu_perf_forces import traffic as forces_traffic

pytestmark = pytest.mark.gpu

N, SEED, SPREAD = 5000, 149, 120.0
SD, TURB_SEED = (1.0, 2.0, 0.5), 20261020
ABORTED = 4      # CD every 4th step, a batch of steps 1-12: steps 1-3 complete, step 4 aborts


@pytest.fixture(scope='module')
def case():
    """synth.box(5000, 120.0, seed=149) as tests/test_gpu_perf_forces.py dresses it (types over every
    flight phase, both tables, masses), tests/test_gpu_fms.py's routes for it and
    tests/test_gpu_geovector.py's areas (built once, left unchanged)."""
    tr = forces_traffic(N, SEED, SPREAD)
    tr['routes'] = fms.synthetic_routes(tr['init'], seed=SEED)
    areas = geovec_np.load_areas(dict(np.load(os.path.join(util.GOLDEN, 'geovec_apply.npz'))))
    tr['areas'] = {k: areas[k] for k in SIM_AREAS}
    return tr


def all_on(case, c, simt0, gv_every, sect_every):
    p = resident.params(cd_every=4, resume_nav=True)
    sim = resident.ResidentSim(case['init'], p, ctx=c)
    sim.set_perf(case['table'], case['tidx'])
    sim.set_forces(case['ftable'], case['mass'])
    sim.set_fms(*case['routes'], simt=simt0)
    sim.set_recovery()
    sim.set_areas(case['areas'])
    sim.set_geovectors(GEOVECS, gv_every)
    sim.set_turbulence(True, SD, TURB_SEED)
    sim.set_sectors(list(SIM_AREAS), sect_every)
    return sim


def read_everything(sim):
    return dict(state=sim.read(), fms=sim.read_fms(), forces=sim.read_forces(), drops=sim.read_dropcount(),
                geovec=sim.geovector_stats(), sectors=sim.ctx.sim_sectors_poll(masks=True), turb_call=sim.turb_call(),
                stats=sim.stats())


def assert_same(got, exp, what=''):
    if isinstance(exp, dict):
        assert sorted(got) == sorted(exp), what
        for k in exp:
            assert_same(got[k], exp[k], '%s.%s' % (what, k))
    else:
        assert np.array_equal(np.asarray(got), np.asarray(exp), equal_nan=True), what


@pytest.mark.parametrize('simt0,gv_every,sect_every,both', [(0.0, 4, 5, True), (0.9, 3, 2, False)])
def test_abort_with_every_stage_on_is_exact(case, simt0, gv_every, sect_every, both):
    """A candidate list far too small (as tests/test_gpu_turbulence.py forces it): the batch of steps 1-12
    aborts at step 4 and re-runs from there.  both: from simt 0 step 4 is an FMS tick, and with a geovector
    cadence of 4 it applies -- the FMS undo set, then the geovector one, are put back -- and with a sector
    cadence of 5 its pass falls on the aborted step.  Neither: from simt 0.9 steps 0-2 tick and step 4 does
    not, the geovectors applied in step 3 (cadence 3) and the sectors were counted after it (cadence 2):
    both undo sets hold an earlier step's start and must be left alone."""
    sched = fms.tick_schedule(simt0, 0.05, ABORTED + 1)[0]
    assert bool(sched[ABORTED]) == both and (ABORTED % gv_every == 0) == both
    assert ((ABORTED + 1) % sect_every == 0) == both
    twin = _lib.Context(0)
    try:
        ref = all_on(case, twin, simt0, gv_every, sect_every)
        ref.step(1)
        ref.step(ABORTED)
        # the last CD step so far is step 4: a list of 16 candidates cannot hold it, so the run below aborts there
        assert ref.stats()['n_conf'] > 16
        ref.step(12 - ABORTED)
        exp = read_everything(ref)
    finally:
        twin.close()
    assert exp['turb_call'] == 13 and exp['stats']['steps'] == 13 and exp['stats']['cd_calls'] == 4
    assert exp['geovec']['applies'] == 12 // gv_every and exp['sectors']['updates'] == 13 // sect_every
    assert exp['forces']['fuel_used'].max() > 0 and sum(exp['geovec']['changed'].values()) > 0
    c = _lib.Context(0)
    try:
        sim = all_on(case, c, simt0, gv_every, sect_every)
        c.set_candidate_capacity(16)
        sim.step(1)
        c.set_candidate_capacity(16)
        sim.step(12)
        got = read_everything(sim)
    finally:
        c.close()
    assert_same(got, exp, 'after the re-run')
