"""numpy restatement of plugins/geovector.py:76-128 (applygeovec) on tests/area_np.py's inside
tests and oracle/kinematics.py's vtas2cas.  Pinned bitwise to the reference plugin by
tests/golden/geovec_apply.npz (tools/make_golden_geovec.py asserts it at capture,
tests/test_geovec_np.py afterwards)."""
import numpy as np

from oracle import kinematics as okin
from tests import area_np

FT = 0.3048
TARGETS = ('selspd', 'ap_trk', 'selvs', 'selalt')
LIMITS = ('gsmin', 'gsmax', 'trkmin', 'trkmax', 'vsmin', 'vsmax')


def degto180(a):
    """tools/misc.py:102-104"""
    return (a + 180.) % 360 - 180.


def apply(geovecs, areas, st):
    """``geovecs``: [[area, gsmin, gsmax, trkmin, trkmax, vsmin, vsmax]]; ``areas``: name ->
    (type number or name, coordinates, top, bottom); ``st``: dict of lat lon alt trk vs and the
    four TARGETS.  Returns the four TARGETS after the call (copies)."""
    lat, lon, alt, trk, vs = (np.asarray(st[k], dtype=np.float64) for k in ('lat', 'lon', 'alt', 'trk', 'vs'))
    selspd, ap_trk, selvs, selalt = (np.array(st[k], dtype=np.float64) for k in TARGETS)
    n = len(lat)
    with np.errstate(invalid='ignore'):
        for area, gsmin, gsmax, trkmin, trkmax, vsmin, vsmax in geovecs:
            if area not in areas:
                continue
            typ, co, top, bottom = areas[area]
            typ = area_np.TYPE_NAMES.index(typ) if isinstance(typ, str) else typ
            inside = area_np.inside(typ, co, top, bottom, lat, lon, alt)
            if gsmin:
                casmin = okin.vtas2cas(np.ones(n) * gsmin, alt)
                use = inside & (selspd < casmin)
                selspd[use] = casmin[use]
            if gsmax:
                casmax = okin.vtas2cas(np.ones(n) * gsmax, alt)
                use = inside & (selspd > casmax)
                selspd[use] = casmax[use]
            if trkmin and trkmax:
                usemin = inside & (degto180(trk - trkmin) < 0)
                usemax = inside & (degto180(trk - trkmax) > 0)
                ap_trk[usemin] = trkmin
                ap_trk[usemax] = trkmax
            if vsmin:
                use = inside & (vs < vsmin)
                selvs[use] = vsmin
                selalt[use] = alt[use] + np.sign(vsmin) * 200. * FT
            if vsmax:
                use = inside & (vs > vsmax)
                selvs[use] = vsmax
                selalt[use] = alt[use] + np.sign(vsmax) * 200. * FT
    return dict(zip(TARGETS, (selspd, ap_trk, selvs, selalt)))


def changed(before, after):
    """Aircraft whose value differs bitwise, per target: (4,) counts and a dict of masks."""
    m = {k: np.asarray(before[k], dtype=np.float64).view(np.uint64) != np.asarray(after[k], dtype=np.float64).view(np.uint64)
         for k in TARGETS}
    return np.array([m[k].sum() for k in TARGETS], dtype=np.uint64), m


# ---- the golden file's layout (tools/make_golden_geovec.py)
def load_lists(g):
    """{list name: [[area, gsmin, ...]]} of a golden: limits stored as NaN plus a mask for None."""
    names = [str(x) for x in g['list_names']]
    off = g['list_off']
    out = {}
    for k, name in enumerate(names):
        rows = []
        for r in range(off[k], off[k + 1]):
            lim = [None if g['gv_none'][r, q] else float(g['gv_limits'][r, q]) for q in range(6)]
            rows.append([str(g['gv_area'][r])] + lim)
        out[name] = rows
    return out


def load_areas(g):
    """name -> (type name, coordinates, top, bottom), in the golden's order."""
    shapes = area_np.named(area_np.load_shapes(g))
    return dict(zip([str(x) for x in g['names']], shapes))


def load_state(g, n=None):
    return {k: g[k][:n].copy() for k in ('lat', 'lon', 'alt', 'trk', 'vs') + TARGETS}
