"""GPU parity of the 3-D wind field (winddim 3, bsa_set_windfield3d):
Windfield.getdata's altitude branch (windfield.py:158-202) per aircraft.

The pin is the reference's own getdata called once per position
(tests/golden/wind3d_*.npz, kin3d_wind1500.npz; tools/make_golden.py
--wind3d-only) and tests/wind3d_np.py, asserted bitwise equal to it at capture.
Tolerance: tests/util.close with the scales of the neighbouring tests."""
import numpy as np
import pytest

from bluesky_amd import _lib, resident, synth
from oracle import kinematics as okin
from oracle import step as ostep
from tests import util, wind3d_np
from tests.test_gpu_multirank import run_ranks
from tests.test_gpu_sim import compare, full_state, oracle_params

pytestmark = pytest.mark.gpu

WIND = 300.0   # scale of a wind component [m/s], as gseast / gsnorth in the kinematic tests
CASES = util.golden('wind3d_*.npz')


def upload(ctx, z):
    ctx.set_windfield3d(z['wlat'], z['wlon'], z['wvnorth'], z['wveast'], float(z['altstep']))


def field5():
    """The 5-point field of kin3d_wind1500 as ResidentSim's dict."""
    z = np.load(util.golden('kin3d_wind1500.npz')[0])
    return dict(lat=z['wlat'], lon=z['wlon'], vnorth=z['wvnorth'], veast=z['wveast'], altstep=float(z['altstep']))


def other_field(f):
    """A second field on the same points: the first one turned and scaled (a weather reload)."""
    return dict(f, vnorth=-0.5 * f['veast'] + 3.0, veast=1.5 * f['vnorth'] - 2.0)


def helper_wind(f, st):
    return wind3d_np.getdata(st['lat'], st['lon'], st['alt'], f['lat'], f['lon'], f['vnorth'], f['veast'],
                             f['altstep'])


@pytest.fixture
def clean(ctx):
    yield ctx
    ctx.set_windfield3d()
    ctx.set_windfield()


@pytest.mark.parametrize('path', CASES, ids=[util.case_name(p) for p in CASES])
def test_getdata_matches_reference_golden(clean, path):
    z = np.load(path)
    upload(clean, z)
    vn, ve = clean.wind_getdata(3, z['lat'], z['lon'], z['alt'])
    for got, exp in ((vn, z['vnorth']), (ve, z['veast'])):
        ok, msg = util.close(got, exp, WIND)
        assert ok, msg
    assert np.ptp(z['vnorth']) > 1.0


@pytest.mark.parametrize('path', CASES, ids=[util.case_name(p) for p in CASES])
def test_getdata_build_defined_altitudes(clean, path):
    """alt at and above the top level: the top level's wind; a NaN altitude: NaN
    (ialt clamped before the table read).  Against the helper."""
    z = np.load(path)
    upload(clean, z)
    nalt, st = z['wvnorth'].shape[0], float(z['altstep'])
    top = (nalt - 1) * st
    lat, lon = z['lat'][:12].copy(), z['lon'][:12].copy()
    alt = np.array([top, top + 300.0, np.nan, np.inf, -np.inf, top - 1e-9] * 2)
    vn, ve = clean.wind_getdata(3, lat, lon, alt)
    en, ee = wind3d_np.getdata(lat, lon, alt, **wind3d_np.field_of(z))
    assert util.close(vn, en, WIND)[0] and util.close(ve, ee, WIND)[0], (vn, en)
    assert np.isnan(vn[2]) and np.isnan(ve[2]) and np.isfinite(np.delete(vn, [2, 8])).all()
    # the top level's value: the same position far above the axis reads the same two rows
    far, _ = clean.wind_getdata(3, lat[:2], lon[:2], np.array([top, 1e9]))
    assert far[0] == vn[0] and np.isfinite(far).all()


def test_getdata_winddim_1_and_2(clean):
    t = synth.box(300, 60.0, seed=5)
    f = dict(lat=np.array([52.0, 52.6, 51.5]), lon=np.array([4.0, 3.2, 4.9]),
             vnorth=np.array([-12.0, 3.5, 20.0]), veast=np.array([5.0, -15.0, 2.0]))
    clean.set_windfield(f['lat'], f['lon'], f['vnorth'], f['veast'])
    vn, ve = clean.wind_getdata(2, t.lat, t.lon)
    en, ee = okin.windfield_2d(t.lat, t.lon, f['lat'], f['lon'], f['vnorth'], f['veast'])
    assert util.close(vn, en, WIND)[0] and util.close(ve, ee, WIND)[0]
    vn, ve = clean.wind_getdata(1, t.lat, t.lon)    # windfield.py:150-152: the first point everywhere
    assert np.array_equal(vn, np.ones(300) * -12.0) and np.array_equal(ve, np.ones(300) * 5.0)


def test_kinematics_matches_reference_golden(clean):
    z = dict(np.load(util.golden('kin3d_wind1500.npz')[0], allow_pickle=False))
    state = {k: np.ascontiguousarray(z[k], dtype=np.float64).copy()
             for k in ('tas', 'hdg', 'alt', 'vs', 'lat', 'lon')}
    inputs = {k: z[k] for k in ('ptas', 'phdg', 'palt', 'pvs', 'bank', 'eps', 'accel')}
    upload(clean, z)
    o = clean.kinematics(float(z['dt']), state, inputs, 3, 0.0, 0.0)
    o.update(state)
    o['M'] = o.pop('mach')
    scales = dict(ax=1.0, delspd=100.0, tas=300.0, cas=300.0, M=1.0, hdg=360.0, az=1.0, vs=20.0,
                  gsnorth=300.0, gseast=300.0, gs=300.0, trk=360.0, alt=1e4, lat=90.0, lon=180.0,
                  coslat=1.0)
    for k, s in scales.items():
        ok, msg = util.close(o[k], z['out_' + k], s)
        assert ok, '%s: %s' % (k, msg)
    for k in ('swhdgsel', 'swaltsel'):
        assert np.array_equal(o[k], z['out_' + k].astype(bool)), k


def start(t):
    init = resident.initial_state(t)
    prev = dict(init)
    prev.update(asas_trk=init['trk'].copy(), asas_tas=init['tas'].copy(),
                asas_vs=np.zeros(t.ntraf), active=np.zeros(t.ntraf, bool))
    return init, prev


def oracle_steps(sim, init, prev, op, fields, bk=None):
    """One GPU step per entry of ``fields`` (the field of that step; a change is
    uploaded first), each against one oracle step from the GPU's previous state."""
    out = []
    for k, f in enumerate(fields):
        if k and f is not fields[k - 1]:
            sim.set_windfield3d(**f)
        op['wind'] = helper_wind(f, prev)
        exp = ostep.sim_step(prev, op, do_cd=True, bk=bk) if bk is not None else ostep.sim_step(prev, op, do_cd=True)
        sim.step(1)
        got = full_state(init, sim.read())
        compare(got, exp, k)
        st = sim.stats()
        out.append((sim.read(), sim.ctx.fetch_pairs(st['n_conf'], st['n_los'])))
        prev = got
    return out


@pytest.mark.parametrize('resume_nav', [False, True], ids=['fused_k2_k4', 'standalone_k4'])
def test_resident_steps_match_oracle(clean, resume_nav):
    """MVP on, CD every step.  Without ResumeNav one rank runs K2 + K4' as one
    launch; with it the bookkeeping sits between K3 and a K4' of its own."""
    from oracle import asas as oasas
    t = synth.box(1500, 60.0, seed=23)
    init, prev = start(t)
    f = field5()
    p = resident.params(cd_every=1, windfield3d=True, resume_nav=resume_nav)
    assert p.winddim == 3
    sim = resident.ResidentSim(init, p, ctx=clean, windfield3d=f)
    bk = oasas.Bookkeeping(t.ntraf) if resume_nav else None
    oracle_steps(sim, init, prev, oracle_params(p), [f] * 4, bk)
    vn, _ = helper_wind(f, prev)
    assert np.ptp(vn) > 1.0      # the field actually varies over the traffic


def test_field_replaced_between_steps():
    """set_windfield3d after step 2: steps 3-4 follow the new field, and the run
    is bitwise the run without tile-pair and candidate reuse (no kept detect
    state depends on the field)."""
    t = synth.box(1500, 60.0, seed=23)
    f = field5()
    g = other_field(f)
    runs = []
    for reuse in (True, False):
        c = _lib.Context(0)
        try:
            c.set_tile_reuse(reuse)
            c.set_candidate_reuse(reuse)
            init, prev = start(t)
            p = resident.params(cd_every=1, windfield3d=True)
            sim = resident.ResidentSim(init, p, ctx=c, windfield3d=f)
            runs.append(oracle_steps(sim, init, prev, oracle_params(p), [f, f, g, g]))
        finally:
            c.close()
    util.same(runs[0], runs[1])
    assert not np.array_equal(helper_wind(f, runs[0][1][0])[0], helper_wind(g, runs[0][1][0])[0])


def test_sharded_equals_one_rank(ctx):
    """World 2 over the in-process group: every state array bitwise the one-rank run's."""
    t = synth.box(1500, 60.0, seed=23)
    init, _ = start(t)
    f = field5()
    p = resident.params(cd_every=1, windfield3d=True)
    steps = 3

    def run(sim):
        out = []
        for _ in range(steps):
            sim.step(1)
            out.append(sim.read())
        return out

    c = _lib.Context(0)
    try:
        exp = run(resident.ResidentSim(init, p, ctx=c, windfield3d=f))
    finally:
        c.close()
    res = run_ranks(2, lambda r, cr, grp: run(resident.ResidentSim(init, p, ctx=cr, rank=r, world=2, group=grp,
                                                                    windfield3d=f)))
    for r in range(2):
        for k in range(steps):
            for name, v in exp[k].items():
                assert np.array_equal(res[r][k][name], v), 'rank %d step %d %s' % (r, k, name)


def test_missing_field_fails_by_name(clean):
    """winddim 3 without a 3-D field: refused before any kernel is launched (the state stays)."""
    clean.set_windfield3d()
    z = dict(np.load(util.golden('kin3d_wind1500.npz')[0], allow_pickle=False))
    state = {k: np.ascontiguousarray(z[k], dtype=np.float64).copy()
             for k in ('tas', 'hdg', 'alt', 'vs', 'lat', 'lon')}
    before = {k: v.copy() for k, v in state.items()}
    inputs = {k: z[k] for k in ('ptas', 'phdg', 'palt', 'pvs', 'bank', 'eps', 'accel')}
    with pytest.raises(Exception, match='bsa_set_windfield3d'):
        clean.kinematics(float(z['dt']), state, inputs, 3, 0.0, 0.0)
    assert all(np.array_equal(state[k], before[k]) for k in state)
    with pytest.raises(Exception, match='bsa_set_windfield3d'):
        clean.wind_getdata(3, z['lat'], z['lon'], z['alt'])
    t = synth.box(600, 60.0, seed=7)
    init, _ = start(t)
    sim = resident.ResidentSim(init, resident.params(windfield3d=True), ctx=clean)
    with pytest.raises(Exception, match='bsa_set_windfield3d'):
        sim.step(1)
    assert sim.stats()['steps'] == 0
