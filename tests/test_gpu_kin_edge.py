"""GPU: the kinematic step and the pilot's wind correction on their thresholds
and edges (tests/golden/kin_edge_*.npz, hand-made rows captured from the
reference by tools/make_golden.py --kin-edge-only; tests/test_golden_census.py
counts what they reach).

test_gpu_mvp_kin.py already compares bsa_kinematics with these fixtures under
util.RTOL (they match its kin_*.npz pattern).  Here: the signs of zero that
util.close cannot see, the rows set aside as ill-conditioned
(kinx_edge_illcond.npz) and the same rows through the resident
step's fused pilot + kinematics kernel against oracle/step.py."""
import numpy as np
import pytest

from bluesky_amd import resident
from oracle import step as ostep
from tests import util
from tests.test_gpu_sim import compare, full_state, oracle_params

pytestmark = pytest.mark.gpu

KIN_EDGE = util.golden('kin_edge_*.npz')
KIN_ILLCOND = util.golden('kinx_edge_illcond.npz')
KIN_OUT = tuple(util.KIN_SCALES)


def test_edge_fixtures_present():
    assert len(KIN_EDGE) == 5 and len(KIN_ILLCOND) == 1


def assert_zero_signs(got, exp, fields, what):
    """Where the reference value is exactly 0 the device's zero has its sign."""
    for k in fields:
        z0 = np.asarray(exp[k]) == 0
        bad = np.flatnonzero(z0 & (np.signbit(got[k]) != np.signbit(exp[k])))
        assert len(bad) == 0, '%s %s: sign of zero differs at rows %s' % (what, k, bad.tolist())


@pytest.mark.parametrize('path', KIN_EDGE, ids=[util.case_name(p) for p in KIN_EDGE])
def test_kinematics_edge_rows_signs_of_zero(ctx, path):
    """-0.0 against +0.0 in ax, az, vs, hdg and trk (need_ax * sign * accel, the
    copysign of nprem, swaltsel * sign * |pvs|): the fixture holds rows whose
    reference value is -0.0 (ax, az, vs) and +0.0 from a negative operand (hdg, trk)."""
    z = dict(np.load(path, allow_pickle=False))
    o = util.run_kinematics(ctx, z)
    exp = {k: z['out_' + k] for k in KIN_OUT}
    for k in ('ax', 'az', 'vs'):
        assert np.any((exp[k] == 0) & np.signbit(exp[k])), k
    assert np.any(exp['hdg'] == 0)
    assert_zero_signs(o, exp, ('ax', 'az', 'vs', 'hdg', 'trk'), util.case_name(path))


def test_kinematics_illconditioned_rows(ctx):
    """tas = +-1e200 (tas^2 overflows): cas, gs and the position leave every
    range, coslat = cos(radians(~1e192)) and lon = ... / coslat turn one ulp of
    lat into any value at all -- those two are compared for their non-finite
    pattern only, the flags exactly and every other field under util.RTOL."""
    z = dict(np.load(KIN_ILLCOND[0], allow_pickle=False))
    o = util.run_kinematics(ctx, z)
    for k in util.KIN_FLAGS:
        assert np.array_equal(o[k], z['out_' + k].astype(bool)), k
    for k in KIN_OUT:
        exp = z['out_' + k]
        assert np.array_equal(np.isnan(o[k]), np.isnan(exp)), k
        assert np.array_equal(np.isinf(o[k]) * np.sign(o[k]), np.isinf(exp) * np.sign(exp)), k
        if k not in ('coslat', 'lon'):
            ok, msg = util.close(o[k], exp, util.KIN_SCALES[k])
            assert ok, '%s: %s' % (k, msg)
    assert np.isinf(z['out_cas']).all() and np.all(np.abs(z['out_lat']) > 1e190)


def spread(n, lat0=20.0, lon0=-40.0):
    """n positions 2 deg of latitude / 3 deg of longitude apart: more than 200 km,
    beyond what two aircraft close within the look-ahead time."""
    k = np.arange(n)
    return lat0 + 2.0 * (k // 12), lon0 + 3.0 * (k % 12)


def edge_sim_state(z):
    """resident.initial_state's fields from the fixture's finite rows: the pilot
    targets become the autopilot's (ap_tas = ptas, ap_trk = phdg, ap_alt = palt,
    ap_vs = pvs).  Rows on the base position move onto a grid; the rows whose
    position is the edge keep it and fly 700 m above each other."""
    keep = np.all([np.isfinite(z[k]) for k in util.KIN_INPUTS], axis=0)
    keep &= np.all([np.isfinite(z['out_' + k]) for k in KIN_OUT], axis=0)
    s = {k: z[k][keep].copy() for k in util.KIN_INPUTS}
    n = int(keep.sum())
    base = (s['lat'] == 52.0) & (s['lon'] == 4.0)
    s['lat'][base], s['lon'][base] = spread(int(base.sum()))
    stack = 1000.0 + 700.0 * np.arange(int((~base).sum()))
    assert np.all(s['alt'][~base] == 8000.0) and np.all(s['palt'][~base] == 8000.0)
    s['alt'][~base] = s['palt'][~base] = stack
    init = dict(lat=s['lat'], lon=s['lon'], alt=s['alt'], tas=s['tas'], hdg=s['hdg'], vs=s['vs'],
                gs=s['tas'].copy(), trk=s['hdg'].copy(), gseast=s['tas'] * np.sin(np.radians(s['hdg'])),
                gsnorth=s['tas'] * np.cos(np.radians(s['hdg'])), ap_trk=s['phdg'], ap_tas=s['ptas'],
                ap_alt=s['palt'], ap_vs=s['pvs'], selalt=s['palt'].copy(), bank=s['bank'], eps=s['eps'],
                accel=s['accel'], asas_alt=s['alt'].copy())
    return init, n, z['row_name'][keep]


def one_resident_step(ctx, init, wind):
    n = len(init['lat'])
    p = resident.params(cd_every=1, wind=wind)
    sim = resident.ResidentSim(init, p, ctx=ctx)
    prev = dict(init)
    prev.update(asas_trk=init['trk'].copy(), asas_tas=init['tas'].copy(), asas_vs=np.zeros(n),
                active=np.zeros(n, bool))
    with np.errstate(all='ignore'):
        exp = ostep.sim_step(prev, oracle_params(p), do_cd=True)
    assert sim.step(1) == 1
    got = full_state(init, sim.read())
    assert exp['n_conf'] == 0 and sim.stats()['n_conf'] == 0    # no pair in conflict: the pilot flies the autopilot's targets
    assert sim.stats()['steps'] == 1
    return got, exp


@pytest.mark.parametrize('wind', [None, (-7.5, 12.0)], ids=['nowind', 'wind'])
def test_resident_step_edge_rows(ctx, wind):
    """The finite edge rows through the resident step's fused pilot + kinematics
    kernel (pilot_kin_row, bsa_sim_row.h): one step against oracle/step.py under
    the resident tests' compare() and SCALES, and the signs of zero of vs, hdg
    and trk (ax and az do not leave the resident step; the test above has them)."""
    z = dict(np.load(util.golden('kin_edge_nowind.npz' if wind is None else 'kin_edge_wind.npz')[0],
                     allow_pickle=False))
    init, n, names = edge_sim_state(z)
    assert n >= 60
    got, exp = one_resident_step(ctx, init, wind)
    for k in ('lat', 'lon', 'alt', 'tas', 'hdg', 'vs', 'gs', 'trk', 'gseast', 'gsnorth'):
        assert np.isfinite(exp[k]).all(), k
    compare(got, exp, 0)
    assert_zero_signs(got, exp, ('vs', 'hdg', 'trk'), 'resident step')
    assert np.any((exp['vs'] == 0) & np.signbit(exp['vs']))


WINDS = {'crosswind': (-7.5, 12.0), 'zero': (0.0, 0.0), 'tiny': (1e-6, -2e-6)}


@pytest.mark.parametrize('wind', sorted(WINDS))
def test_resident_pilot_wind_correction_edges(ctx, wind):
    """Pilot.APorASAS' wind correction (pilot.py:51-61) as oracle/step.py restates it,
    arcsin(clamp(Vw sin(drift) / max(0.001, tas))): tas below, on and above the
    0.001 floor and 0; a crosswind faster than tas, so that the arcsin's argument
    clamps at +1 and at -1; a zero wind vector with winddim 1 (arctan2(0, 0)); a
    wind so small that the floor decides without the clamp; ap_trk = 360 and -0.0."""
    vn, ve = WINDS[wind]
    winddir = np.degrees(np.arctan2(ve, vn))
    tas = np.array([0.0005, 0.001, float(np.nextafter(0.001, 1.0)), 0.0, 10.0, 200.0])
    trk = np.array([(winddir + 90.0) % 360.0, (winddir - 90.0) % 360.0, 360.0, -0.0, 45.0, winddir % 360.0])
    tas, trk = [a.ravel() for a in np.meshgrid(tas, trk)]
    n = len(tas)
    lat, lon = spread(n)
    hdg = trk % 360.0
    init = dict(lat=lat, lon=lon, alt=np.full(n, 8000.0), tas=tas, hdg=hdg, vs=np.zeros(n), gs=tas.copy(),
                trk=hdg.copy(), gseast=tas * np.sin(np.radians(hdg)), gsnorth=tas * np.cos(np.radians(hdg)),
                ap_trk=trk, ap_tas=tas.copy(), ap_alt=np.full(n, 8000.0), ap_vs=np.zeros(n), selalt=np.full(n, 8000.0),
                bank=np.full(n, np.radians(25.0)), eps=np.full(n, 0.01), accel=np.full(n, 0.5),
                asas_alt=np.full(n, 8000.0))
    # the arcsin argument of every row, as the oracle forms it
    Vw = np.sqrt(vn * vn + ve * ve)
    arg = Vw * np.sin(np.radians(trk) - np.arctan2(ve, vn)) / np.maximum(0.001, tas)
    if wind == 'crosswind':
        assert (arg > 1.0).any() and (arg < -1.0).any() and (np.abs(arg) < 1.0).any()
    elif wind == 'tiny':
        assert (np.abs(arg) < 1.0).all() and (np.abs(arg[tas < 0.001]) > 1e-4).any()
    else:
        assert (arg == 0).all()
    got, exp = one_resident_step(ctx, init, (vn, ve))
    compare(got, exp, 0)
    assert_zero_signs(got, exp, ('vs', 'hdg', 'trk'), 'pilot wind correction')
