"""Shared by the route-edit tests (CPU and GPU): the loader of the captured
fixtures tests/golden/route_edit_*.npz (tools/make_golden.py --route-edit: the
reference's own Route.addwpt / delwpt / direct on real Route / Autopilot objects;
the capture rules for deletes stand in DESIGN.md 7) and their comparison."""
import numpy as np

from bluesky_amd import _lib, fms
from tests import recover_np, route_np, util
from tests.recover_cases import compare

FIXTURES = sorted(util.golden('route_edit_*.npz'))
STATE = recover_np.TRAFFIC + tuple(_lib.FMS_REALS) + tuple(_lib.FMS_FLAGS) + ('ap_trk', 'ap_tas', 'ap_alt', 'ap_vs', 'selalt',
                                                                            'iactwp')


def load(path):
    """(fixture dict, state before, records as stored, expected table, expected state)."""
    g = dict(np.load(path))
    st = {k: g[k] for k in STATE}
    recs = np.zeros(len(g['rec_op']), _lib.ROUTE_REC_DTYPE)
    for f in _lib.ROUTE_REC_DTYPE.names:
        recs[f] = g['rec_' + f]
    table = (g['out_route_rows'], g['out_rt_off'], g['out_rt_n'], g['out_wptype'])
    exp = {k[4:]: g[k] for k in g if k.startswith('out_') and k[4:] in STATE}
    return g, st, recs, table, exp


def names_of(g):
    """The routes' waypoint names and types before the commands, per aircraft."""
    off, n = g['rt_off'], g['rt_n']
    return ([[str(x) for x in g['names'][off[k]:off[k] + n[k]]] for k in range(len(n))],
            [[int(t) for t in g['wptype'][off[k]:off[k] + n[k]]] for k in range(len(n))])


def resolve(g):
    """The fixture's command sequence through fms.RouteNames: (records, RouteNames after)."""
    rn = fms.RouteNames(*names_of(g))
    recs = []
    for q in range(len(g['cmd_kind'])):
        k, nam, kind = int(g['cmd_aircraft'][q]), str(g['cmd_name'][q]), str(g['cmd_kind'][q])
        if kind == 'add':
            r = rn.addwpt(k, nam, int(g['cmd_wptype'][q]), float(g['cmd_lat'][q]), float(g['cmd_lon'][q]),
                          float(g['cmd_alt'][q]), float(g['cmd_spd'][q]), afterwp=str(g['cmd_after'][q]),
                          beforewp=str(g['cmd_before'][q]), flyby=bool(g['cmd_flyby'][q]))
        else:
            r = rn.delwpt(k, nam) if kind == 'del' else rn.direct(k, nam)
        assert len(r) == g['cmd_records'][q]
        recs += r
    return _lib.route_records(recs), rn


def compare_state(got, st, exp, skip=None, exact=False):
    """Every output of an edit as tests/test_recover_np.py compares a recovery's, actwp.next_qdr
    with them, and what an edit does not touch bitwise against the state before."""
    compare(got, exp, skip=skip, exact=exact)
    a, e = np.asarray(got['actwp_next_qdr']), exp['actwp_next_qdr']
    if skip is not None:
        a, e = a[~skip], e[~skip]
    if exact:
        assert np.array_equal(a, e)
    else:
        ok, msg = util.close(a, e, 360.)
        assert ok, msg
    for k in route_np.UNTOUCHED:
        if k in got:
            assert np.array_equal(got[k], st[k], equal_nan=True), k
            if k in exp:
                assert np.array_equal(exp[k], st[k], equal_nan=True), k
