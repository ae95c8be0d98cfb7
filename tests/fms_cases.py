"""Shared by the FMS tests (CPU and GPU): the golden's loader and the comparison rule."""
import numpy as np

from tests import fms_np
from tests import util

INPUTS = fms_np.TRAFFIC + fms_np.REALS + fms_np.FLAGS + fms_np.TARGETS + ('iactwp',)


def load():
    """(golden dict, state dict of its inputs)."""
    g = dict(np.load(util.golden('fms_update2000.npz')[0]))
    return g, {k: g[k] for k in INPUTS}


def compare(got, g, n=None, skip=None, exact=False, what=''):
    """Flags and iactwp exactly; reals bitwise (``exact``) or within util.close's
    1e-9 rule with the field's largest finite magnitude as scale, NaN positions equal."""
    for k in fms_np.OUTPUTS:
        a, e = np.asarray(got[k]), np.asarray(g['out_' + k])[:n]
        if skip is not None:
            a, e = a[~skip], e[~skip]
        if e.dtype != np.float64 or exact:
            assert np.array_equal(a.astype(e.dtype), e, equal_nan=True), what + k
            continue
        assert np.array_equal(np.isnan(a), np.isnan(e)), '%s%s: NaN positions' % (what, k)
        fin = np.abs(e[np.isfinite(e)])
        ok, msg = util.close(a, e, fin.max() if len(fin) and fin.max() > 0 else 1.0)
        assert ok, '%s%s: %s' % (what, k, msg)


# ---------------------------------------------------------------- the closed-loop flight golden
FLIGHT_TRAFFIC = ('lat', 'lon', 'alt', 'tas', 'hdg', 'vs', 'ax')
STEP_KEYS = ('tas', 'hdg', 'alt', 'vs', 'lat', 'lon', 'gs', 'trk', 'gseast', 'gsnorth', 'ax')
FMS_KEYS = fms_np.REALS + fms_np.FLAGS + ('iactwp',)


def load_flight():
    return dict(np.load(util.golden('fms_flight64.npz')[0]))


def flight_state(g, s):
    """The full state (oracle/step.py's keys + fms_np's) at sample ``s`` of the flight golden."""
    st = {k[5:]: np.array(v) for k, v in g.items() if k.startswith('init_')}
    for k in FLIGHT_TRAFFIC + fms_np.OUTPUTS:
        st[k] = np.array(g['s_' + k][s])
    st['gs'], st['trk'] = st['tas'].copy(), st['hdg'].copy()
    st['gseast'] = st['tas'] * np.sin(np.radians(st['hdg']))
    st['gsnorth'] = st['tas'] * np.cos(np.radians(st['hdg']))
    return st, float(g['s_simt'][s]), float(g['s_t0'][s])


def flight_step(st, g, simt, t0):
    """One step of fms_np.update then oracle/step.py (ASAS inactive, no wind), in place.
    Returns (simt, t0, ticked)."""
    from oracle import step as ostep
    tick = fms_np.ticks(simt, t0)
    new = fms_np.update(st, g['route_rows'], g['rt_off'], g['rt_n'], tick=tick)
    st.update({k: new[k] for k in fms_np.OUTPUTS})
    op = dict(simdt=float(g['simdt']), rpz=1.0, hpz=1.0, tla=1.0, reso=False, wind=None, mvp=None)
    nxt = ostep.sim_step({k: v for k, v in st.items() if k not in FMS_KEYS}, op, do_cd=False)
    st.update({k: nxt[k] for k in STEP_KEYS})
    return simt + float(g['simdt']), (simt if tick else t0), tick
