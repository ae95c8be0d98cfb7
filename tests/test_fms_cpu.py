"""CPU: Autopilot.update's numpy restatement (tests/fms_np.py) and the host-side
route table (bluesky_amd.fms.route_table) against tests/golden/fms_update2000.npz,
captured from the reference's own Autopilot / ActiveWaypoint / Route objects
(tools/make_golden.py run_fms), and the FMS tick rule (autopilot.py:61-62)."""
import types

import numpy as np
import pytest

from bluesky_amd import fms
from tests import fms_np
from tests import util
from tests.fms_cases import FLIGHT_TRAFFIC, INPUTS, compare, flight_state, flight_step, load, load_flight


def test_helper_reproduces_reference():
    """Bitwise where this numpy is the capture's (its sin / cos / arctan2 / pow
    loops), else within the 1e-9 rule."""
    g, st = load()
    got = fms_np.update(st, g['route_rows'], g['rt_off'], g['rt_n'])
    compare(got, g, exact=str(g['numpy_version']) == np.__version__)
    for k in INPUTS:                                    # the inputs stay as they were
        assert np.array_equal(st[k], g[k], equal_nan=True), k


def test_golden_covers_the_cases():
    g, st = load()
    info = {}
    fms_np.update(st, g['route_rows'], g['rt_off'], g['rt_n'], info=info)
    assert np.array_equal(info['reached'], g['reached']) and np.array_equal(info['vnav'], g['vnav_path'])
    h = slice(0, 257)
    assert set(np.unique(g['vnav_path'][h])) == {0, 1, 2, 3, 4, 5, 6}
    assert {0, 1, 2} <= set(g['rt_n'][h].tolist()) and g['rt_n'].max() == 40
    re_ = g['reached'][h]
    assert (re_ & info['bydist'][h]).any() and (re_ & info['circling'][h] & ~info['bydist'][h]).any()
    assert (re_ & g['swvnav'][h] & ~g['out_swlnav'][h] & ~g['out_swvnav'][h]).any()         # end of route
    assert (g['out_iactwp'][h][re_] >= g['iactwp'][h][re_]).all()
    assert (~g['swlnav'][h] & g['swvnav'][h] & (g['out_swvnavvs'][h] == 1.0)).any()          # LNAV off, VNAV on
    assert info['usespdcon'][h].any() and (~info['usespdcon'][h]).any()
    assert not g['near_threshold'].any()
    assert np.array_equal(g['near_threshold'], fms_np.near_threshold(st, g['route_rows'], g['rt_off'], g['rt_n']))
    # an aircraft without a route never has LNAV on
    assert not g['swlnav'][g['rt_n'] == 0].any()


def test_non_tick_is_ap_tas_only():
    g, st = load()
    got = fms_np.update(st, g['route_rows'], g['rt_off'], g['rt_n'], tick=False)
    for k in fms_np.OUTPUTS:
        if k != 'ap_tas':
            assert np.array_equal(got[k], st[k], equal_nan=True), k
    assert np.array_equal(got['ap_tas'], fms_np.vcasormach2tas(st['selspd'], st['alt']))


def route(lat, lon, alt, spd=None, flyby=None, wptype=None, iactwp=0, **kw):
    n = len(lat)
    return types.SimpleNamespace(wplat=list(lat), wplon=list(lon), wpalt=list(alt), wpspd=list(spd or [-999.] * n),
                                 wpflyby=list(flyby or [True] * n), wptype=list(wptype or [0] * n), iactwp=iactwp,
                                 nwp=n, **kw)


def test_route_table_of_hand_made_routes():
    a = route([52.0, 52.5, 53.0, 53.5], [4.0, 4.0, 4.0, 4.0], [-999., -999., 3000., -999.], flyby=[True, False, True, True],
              iactwp=1)
    b = route([], [], [], iactwp=-1)
    c = route([10.0, 10.0], [20.0, 21.0], [-999., -999.], spd=[150., 0.78], wptype=[0, fms.WP_DEST])
    rows, off, n, act = fms.route_table([a, b, c])
    assert rows.shape == (6, 8) and rows.dtype == np.float64
    assert off.tolist() == [0, 4, 4] and n.tolist() == [4, 0, 2] and act.tolist() == [1, -1, 0]
    assert off.dtype == n.dtype == act.dtype == np.int32
    # nextqdr: due north along a meridian, -999 for each route's last waypoint
    assert np.allclose(rows[:3, 7], 0.0, atol=1e-9) and rows[3, 7] == -999. and rows[5, 7] == -999.
    assert abs(rows[4, 7] - 90.0) < 0.1
    assert rows[:4, 6].tolist() == [1.0, 0.0, 1.0, 1.0]
    # toalt / xtoalt (route.py:1016-1041): the constraint at waypoint 2 seen from 0 and 1, the
    # distance accumulated over the legs without one; nothing after it
    d01 = fms.qdrdist(np.float64(52.0), np.float64(4.0), np.float64(52.5), np.float64(4.0))[1] * fms.NM
    d12 = fms.qdrdist(np.float64(52.5), np.float64(4.0), np.float64(53.0), np.float64(4.0))[1] * fms.NM
    assert rows[:4, 5].tolist() == [3000., 3000., 3000., -999.]
    assert rows[2, 4] == 0.0 and rows[1, 4] == d12 and rows[0, 4] == d12 + d01 and rows[3, 4] == 0.0
    assert 55000. < d01 < 56000.
    # a destination counts as altitude 0 there
    assert rows[4:, 5].tolist() == [0., 0.] and rows[5, 4] == 0.0 and rows[4, 4] > 100000.
    assert rows[4:, 3].tolist() == [150., 0.78]
    # a route that carries its own calcfp results keeps them
    a2 = route([52.0, 52.5], [4.0, 4.0], [-999., -999.], wpxtoalt=[7.0, 8.0], wptoalt=[9.0, 10.0])
    r2 = fms.route_table([a2])[0]
    assert r2[:, 4].tolist() == [7.0, 8.0] and r2[:, 5].tolist() == [9.0, 10.0]


def test_route_table_of_the_golden():
    """The golden's table was built from the reference's Route objects after
    calcfp(); rebuilt here from its raw columns alone."""
    g, _ = load()
    routes = []
    for o, m, i in zip(g['rt_off'], g['rt_n'], g['iactwp']):
        q = slice(o, o + m)
        routes.append(route(g['route_rows'][q, 0], g['route_rows'][q, 1], g['route_rows'][q, 2],
                            spd=list(g['route_rows'][q, 3]), flyby=list(g['route_rows'][q, 6] != 0),
                            wptype=list(g['wp_type'][q]), iactwp=int(i) if m else -1))
    rows, off, n, act = fms.route_table(routes, g['swlnav'])
    assert np.array_equal(off, g['rt_off']) and np.array_equal(n, g['rt_n'])
    assert np.array_equal(act[n > 0], g['iactwp'][n > 0])
    if str(g['numpy_version']) == np.__version__:
        assert np.array_equal(rows, g['route_rows'])
    else:
        for col in range(8):
            ok, msg = util.close(rows[:, col], g['route_rows'][:, col], np.abs(g['route_rows'][:, col]).max())
            assert ok, '%s: %s' % (fms.COLS[col], msg)


def test_route_table_refusals():
    ok = route([52.0, 52.5], [4.0, 4.0], [-999., -999.])
    with pytest.raises(ValueError):
        fms.route_table([route([52.0, 52.5], [4.0, 4.0], [-999., -999.], wptype=[0, fms.WP_RUNWAY])])
    with pytest.raises(ValueError):
        fms.route_table([ok, route([52.0], [4.0], [-999.], iactwp=1)])
    with pytest.raises(ValueError):
        fms.route_table([ok, route([52.0], [4.0], [-999.], iactwp=-1)])
    with pytest.raises(ValueError):
        fms.route_table([ok, route([], [], [], iactwp=-1)], swlnav=[True, True])       # LNAV on an empty route
    with pytest.raises(ValueError):
        fms.route_table([route([52.0, 52.5], [4.0], [-999., -999.])])                  # a short column
    fms.route_table([ok, route([], [], [], iactwp=-1)], swlnav=[True, False])


@pytest.mark.parametrize('simdt', [0.05, 0.1, 1.0])
def test_tick_schedule_is_the_reference_condition(simdt):
    """200 steps from simt 0: the schedule against a replay of Autopilot.update's
    own scheduling lines on an object with its t0 / dt."""
    ap = types.SimpleNamespace(t0=-999., dt=1.01)
    simt, exp = 0.0, []
    for _ in range(200):
        ticked = False
        assert fms_np.ticks(simt, ap.t0) == (ap.t0 + ap.dt < simt or simt < ap.t0 or simt < ap.dt)
        if ap.t0 + ap.dt < simt or simt < ap.t0 or simt < ap.dt:      # autopilot.py:61
            ap.t0 = simt                                               # autopilot.py:62
            ticked = True
        exp.append(ticked)
        simt += simdt                                                  # simulation.py:119
    got, simt1, t01 = fms.tick_schedule(0.0, simdt, 200)
    assert got.tolist() == exp and simt1 == simt and t01 == ap.t0
    # in two batches: the same
    a, s, t = fms.tick_schedule(0.0, simdt, 77)
    b, s, t = fms.tick_schedule(s, simdt, 123, t0=t)
    assert np.concatenate([a, b]).tolist() == exp and (s, t) == (simt1, t01)
    if simdt == 0.05:
        assert got[:21].all() and not got[21:41].any() and got[41] and not got[42:62].any()
    # a time that runs backwards (a reset) ticks at once
    assert fms.tick_schedule(3.0, simdt, 1, t0=50.0)[0][0]


def test_helper_flies_the_reference_flight():
    """fms_np.update + oracle/step.py from the flight golden's initial state over
    its 2400 steps: every 40-step sample (traffic, FMS state, simt, t0), every
    waypoint switch at its recorded step, the tick count.  Bitwise where this
    numpy is the capture's, else the 1e-9 rule on the reals and the flags /
    iactwp exactly.  This pins the helper's non-tick path and its behaviour
    over many steps to the reference."""
    g = load_flight()
    exact = str(g['numpy_version']) == np.__version__
    every, nsteps = int(g['every']), int(g['nsteps'])
    st, simt, t0 = flight_state(g, 0)
    sw, nticks = [], 0
    for step in range(nsteps + 1):
        if step % every == 0:
            s = step // every
            compare(st, {'out_' + k: g['s_' + k][s] for k in fms_np.OUTPUTS}, exact=exact, what='sample %d ' % s)
            for k in FLIGHT_TRAFFIC:
                if exact:
                    assert np.array_equal(st[k], g['s_' + k][s]), 'sample %d %s' % (s, k)
                else:
                    ok, msg = util.close(st[k], g['s_' + k][s], max(np.abs(g['s_' + k][s]).max(), 1.0))
                    assert ok, 'sample %d %s: %s' % (s, k, msg)
            assert (simt, t0) == (g['s_simt'][s], g['s_t0'][s])
        if step == nsteps:
            break
        before = st['iactwp'].copy()
        simt, t0, tick = flight_step(st, g, simt, t0)
        nticks += tick
        sw += [(k, step) for k in np.flatnonzero(st['iactwp'] != before)]
    assert nticks == int(g['nticks'])
    assert sw == list(zip(g['sw_ac'].tolist(), g['sw_step'].tolist()))


def test_flight_golden_holds_what_it_should():
    g = load_flight()
    assert g['init_lat'].shape == (64,) and int(g['nsteps']) == 2400 and int(g['every']) == 40
    assert g['s_lat'].shape == (61, 64) and float(g['simdt']) == 0.05 and g['s_simt'][0] == 0.0
    assert len(np.unique(g['sw_ac'])) == 64                      # every aircraft passes a waypoint
    ended = ~g['s_swlnav'][-1]
    assert ended.any() and not ended.all()                       # some finish their route
    assert not g['s_swvnav'][-1][ended].any()                    # ... and VNAV follows LNAV off
    assert (g['init_tas'] >= 100.).all() and (g['init_tas'] <= 150.).all()
    assert float(g['margin_rel']) == 1e-6
    # at no tick of the flight a comparison lies within 1e-6 of equality (asserted at capture; here on the samples' ticks)
    for s in range(0, 61, 10):
        st, simt, t0 = flight_state(g, s)
        assert not fms_np.near_threshold(st, g['route_rows'], g['rt_off'], g['rt_n'], rel=1e-6).any()
