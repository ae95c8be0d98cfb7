"""CPU: tests/recover_np.py (Route.findact + Route.direct restated) against the
goldens captured from the reference's own Route / Autopilot objects, and
``fms.from_bluesky(unique_names=True)``."""
import types

import numpy as np
import pytest

from bluesky_amd import fms
from tests import recover_np
from tests.recover_cases import load


def test_helper_reproduces_the_standalone_golden_bitwise():
    g, st = load()
    with np.errstate(all='ignore'):
        got = recover_np.recover(st, g['route_rows'], g['rt_off'], g['rt_n'], g['count'])
    for k in recover_np.OUTPUTS:
        e = g['out_' + k]
        assert np.array_equal(np.asarray(got[k]).astype(e.dtype), e, equal_nan=True), k
    for k in recover_np.UNTOUCHED:                         # direct sets none of these
        if k in st:
            assert np.array_equal(got[k], st[k], equal_nan=True), k
    idle = (g['count'] == 0) | (g['rt_n'] == 0)            # no dropped pair, or findact's -1: nothing at all
    assert idle.any() and (g['rt_n'][g['count'] > 0] == 0).any()
    for k in recover_np.OUTPUTS:
        assert np.array_equal(g['out_' + k][idle], np.asarray(st[k])[idle].astype(g['out_' + k].dtype), equal_nan=True), k
    with np.errstate(all='ignore'):
        assert not recover_np.near_threshold(st, g['route_rows'], g['rt_off'], g['rt_n'], g['count']).any()
    assert (g['out_iactwp'] != g['iactwp']).sum() > 100 and (g['out_swlnav'] & ~g['swlnav']).any()


def test_applications_are_sequential():
    """count 2 is two applications, not one: rows exist where it differs."""
    g, st = load()
    two = g['count'] >= 2
    with np.errstate(all='ignore'):
        once = recover_np.recover(st, g['route_rows'], g['rt_off'], g['rt_n'], np.minimum(g['count'], 1))
    differs = np.zeros(len(two), bool)
    for k in recover_np.OUTPUTS:
        differs |= ~((once[k] == g['out_' + k]) | ((once[k] != once[k]) & (g['out_' + k] != g['out_' + k])))
    assert (differs & two).any() and not (differs & ~two).any()
    assert ((once['iactwp'] != g['out_iactwp']) & two).any()


def stub_traffic(names):
    n = len(names)
    route = types.SimpleNamespace(wpname=list(names), wplat=[52.0 + 0.1 * i for i in range(n)],
                                  wplon=[4.0] * n, wpalt=[-999.] * n, wpspd=[-999.] * n, wpflyby=[True] * n,
                                  wptype=[0] * n, iactwp=0, nwp=n)
    one = np.zeros(1)
    wp = types.SimpleNamespace(lat=one, lon=one, nextaltco=one, xtoalt=one, spd=one, vs=one, turndist=one,
                               flyby=one, next_qdr=one)
    ap = types.SimpleNamespace(route=[route], dist2vs=one, vnavvs=one, swvnavvs=one, trk=one, tas=one, alt=one, vs=one)
    return types.SimpleNamespace(ap=ap, actwp=wp, swlnav=np.ones(1, bool), swvnav=np.zeros(1, bool),
                                 abco=np.zeros(1, bool), belco=np.ones(1, bool), selspd=one, selvs=one, apvsdef=one,
                                 selalt=one, **{k: one for k in fms.TRAFFIC})


def test_from_bluesky_refuses_a_repeated_name_on_request():
    rows, off, cnt, st = fms.from_bluesky(stub_traffic(['A', 'B', 'C']), unique_names=True)
    assert len(rows) == 3 and cnt[0] == 3
    twice = stub_traffic(['A', 'B', ' a '])                 # direct's lookup upper()s and strip()s the name
    with pytest.raises(ValueError, match='more than once'):
        fms.from_bluesky(twice, unique_names=True)
    rows, off, cnt, st = fms.from_bluesky(twice)            # off by default
    assert len(rows) == 3


def test_helper_reproduces_the_flight_goldens_events():
    """The closed loop of the reference with ASAS (real Autopilot.update ->
    ASAS.update with ResumeNav's findact / direct -> Pilot -> kinematics): the
    helper composition from the initial state gives the recorded recovery events,
    waypoint switches and every sample bitwise."""
    from tests.recover_cases import flight_run, load_flight
    from tests import fms_np
    g = load_flight()
    samples, events, switches = flight_run(g, int(g['nsteps']))
    assert events == list(zip(g['ev_cd'].tolist(), g['ev_ac'].tolist(), g['ev_count'].tolist(), g['ev_iactwp'].tolist()))
    assert switches == list(zip(g['sw_ac'].tolist(), g['sw_step'].tolist()))
    assert len(set(g['ev_ac'].tolist())) >= 8 and (g['ev_count'] >= 2).any()
    for s, st in enumerate(samples):
        for k in ('lat', 'lon', 'alt', 'tas', 'hdg', 'vs') + fms_np.OUTPUTS + ('active', 'asas_trk', 'asas_alt'):
            e = g['s_' + k][s]
            assert np.array_equal(np.asarray(st[k]).astype(e.dtype), e, equal_nan=True), 'sample %d %s' % (s, k)
    # never recovering is another flight: the feature's effect, on the reference's own scenario
    _, ev0, sw0 = flight_run(g, int(g['nsteps']), recovery=False)
    assert sw0 != switches
