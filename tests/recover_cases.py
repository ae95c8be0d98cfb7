"""Shared by the waypoint-recovery tests (CPU and GPU): the goldens' loaders and
the comparison rule."""
import numpy as np

from tests import fms_np, recover_np
from tests import util

INPUTS = recover_np.TRAFFIC + fms_np.REALS + fms_np.FLAGS + ('ap_alt', 'iactwp')


def load():
    """(golden dict, state dict of its inputs) of the standalone golden."""
    g = dict(np.load(util.golden('fms_recover2000.npz')[0]))
    return g, {k: g[k] for k in INPUTS}


def compare(got, exp, n=None, skip=None, exact=False, what=''):
    """``got`` against ``exp[k][:n]`` for every output of a recovery: flags and
    iactwp exactly; reals bitwise (``exact``) or within util.close's 1e-9 rule with
    the field's largest finite magnitude as scale, NaN positions equal."""
    for k in recover_np.OUTPUTS:
        a, e = np.asarray(got[k]), np.asarray(exp[k])[:n]
        if skip is not None:
            a, e = a[~skip], e[~skip]
        if e.dtype != np.float64 or exact:
            assert np.array_equal(a.astype(e.dtype), e, equal_nan=True), what + k
            continue
        assert np.array_equal(np.isnan(a), np.isnan(e)), '%s%s: NaN positions' % (what, k)
        fin = np.abs(e[np.isfinite(e)])
        ok, msg = util.close(a, e, fin.max() if len(fin) and fin.max() > 0 else 1.0)
        assert ok, '%s%s: %s' % (what, k, msg)


# ---------------------------------------------------------------- the resident step
FMS_KEYS = fms_np.REALS + fms_np.FLAGS + ('iactwp',)


def drop_counts(bk, n):
    """Resopairs the last ``Bookkeeping.update`` dropped, per ownship."""
    count = np.zeros(n, dtype=np.int32)
    for (i, _), kept in bk.last_keep.items():
        if not kept:
            count[i] += 1
    return count


def recover_step(st, rows, off, cnt, op, bk, tick, do_cd, recovery=True):
    """One step of Traffic.update's ap -> asas -> pilot chain on the full state dict
    ``st`` (oracle/step.py's keys + fms_np's): ``fms_np.update`` (Autopilot.update),
    on a CD step oracle/step.py's detect + MVP + ``bk``'s ResumeNav, then
    ``recover_np.recover`` with the pairs it dropped per ownship (asas.py:459-465;
    ``recovery`` False: never), then Pilot.APorASAS and the kinematics on the
    recovered ``ap_alt``.  Returns (new state, drop counts)."""
    from oracle import step as ostep
    n = len(st['lat'])
    new = fms_np.update(st, rows, off, cnt, tick=tick)
    st = dict(st, **{k: new[k] for k in fms_np.OUTPUTS})
    count = np.zeros(n, dtype=np.int32)
    if do_cd:
        a = ostep.sim_step({k: v for k, v in st.items() if k not in FMS_KEYS}, op, do_cd=True, bk=bk)
        st = dict(st, **{k: a[k] for k in ('asas_trk', 'asas_tas', 'asas_vs', 'asas_alt', 'active')})
        count = drop_counts(bk, n)
        if recovery and count.any():
            with np.errstate(all='ignore'):
                rec = recover_np.recover(st, rows, off, cnt, count)
            st = dict(st, **{k: rec[k] for k in recover_np.OUTPUTS})
    nxt = ostep.sim_step({k: v for k, v in st.items() if k not in FMS_KEYS}, op, do_cd=False)
    st = dict(st, **{k: nxt[k] for k in ('tas', 'hdg', 'alt', 'vs', 'lat', 'lon', 'gs', 'trk', 'gseast', 'gsnorth', 'ax')})
    return st, count


# ---------------------------------------------------------------- the closed-loop golden with ASAS
def load_flight():
    return dict(np.load(util.golden('fms_recover_flight.npz')[0]))


def flight_params(g):
    from oracle import mvp as omvp
    return dict(simdt=float(g['simdt']), rpz=float(g['rpz']), hpz=float(g['hpz']), tla=float(g['tla']), reso=True,
                wind=None, mvp=omvp.params_from_settings(float(g['rpz']), float(g['hpz']), float(g['tla']), float(g['mar'])))


def flight_run(g, nsteps, recovery=True, keep=None):
    """The helper composition from the golden's initial state: (samples every
    ``every`` steps as a list of state dicts, events as (CD call, aircraft, count,
    iactwp after), switches as (aircraft, step)); with ``keep``, a set of steps,
    also a dict step -> (state before, simt, t0, state after, drop counts)."""
    from oracle import asas as oasas
    st = {k[5:]: np.array(v) for k, v in g.items() if k.startswith('init_')}
    st['ax'] = np.zeros(len(st['lat'])) if 'ax' not in st else st['ax']
    rows, off, cnt = g['route_rows'], g['rt_off'], g['rt_n']
    op, bk = flight_params(g), oasas.Bookkeeping(len(st['lat']))
    every, cd_every, simdt = int(g['every']), int(g['cd_every']), float(g['simdt'])
    simt, t0, ncd = 0.0, -999., 0
    samples, events, switches, kept = [], [], [], {}
    with np.errstate(all='ignore'):
        for step in range(nsteps):
            if step % every == 0:
                samples.append(st)
            tick = fms_np.ticks(simt, t0)
            t0_was, t0 = t0, (simt if tick else t0)
            do_cd = step % cd_every == 0
            before, was = st['iactwp'], st
            st, count = recover_step(st, rows, off, cnt, op, bk, tick, do_cd, recovery=recovery)
            if keep is not None and step in keep:
                kept[step] = (was, simt, t0_was, st, count)
            if do_cd:
                events += [(ncd, int(k), int(count[k]), int(st['iactwp'][k])) for k in np.flatnonzero(count)]
                ncd += 1
            switches += [(int(k), step) for k in np.flatnonzero(st['iactwp'] != before)]
            simt += simdt
    samples.append(st)
    if keep is not None:
        return samples, events, switches, kept
    return samples, events, switches
