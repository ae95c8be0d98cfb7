"""Drop-in kinematic integration on MI355X.

Replaces ``Traffic.UpdateAirSpeed`` + ``UpdateGroundSpeed`` +
``UpdatePosition`` (bluesky/traffic/traffic.py:425-483), which
``Traffic.update`` calls back to back (traffic.py:407-409), by ONE fused HIP
kernel.  BlueSky has no plugin API for kinematics, so
``install(traf)`` rebinds the three methods on the instance: the fused step
runs in ``UpdateAirSpeed`` and the other two become no-ops.

Supports winddim 0 (no wind), 1 (constant wind) and 2 (2-D field: the
inverse-distance-squared interpolation of windfield.py:158-179, per aircraft
on the device, bsa_set_windfield).  winddim 3 (altitude profiles) raises
ValueError by default, as the reference's own getdata does for array positions
(windfield.py:177 compares an ndarray with None in a boolean context).  The
reference raises for arrays only: called with one position at a time its 3-D
branch (windfield.py:181-202) runs, and ``wind3d=True`` opts in to exactly that
per-aircraft result, evaluated on the device (bsa_set_windfield3d).  The
tables (``Windfield.vnorth`` / ``veast``, nalt x nvec) are uploaded only when
``traf.wind`` holds other array objects than at the last upload -- addpoint,
remove and clear all rebind them; ``reload_wind3d(ctx)`` forces the next
upload (after an in-place edit of the tables).
"""
import types

import numpy as np

from . import _lib

KTS = 0.514444


def _upload_wind3d(ctx, w):
    """The 3-D field of Windfield ``w`` on ``ctx``, unless it holds the arrays uploaded last."""
    arrs = (w.lat, w.lon, w.vnorth, w.veast)
    last = getattr(ctx, '_wind3d_uploaded', None)
    if last is not None and len(last) == 5 and all(a is b for a, b in zip(last, arrs)) \
            and last[4] == float(w.altstep):
        return
    ctx.set_windfield3d(w.lat, w.lon, w.vnorth, w.veast, float(w.altstep))
    ctx._wind3d_uploaded = arrs + (float(w.altstep),)   # (keeps the arrays alive: ``is`` stays meaningful)


def reload_wind3d(ctx=None):
    """Force the next ``step(..., wind3d=True)`` on ``ctx`` to upload the 3-D field again."""
    ctx = ctx or _lib.default_context()
    ctx._wind3d_uploaded = None


def step(traf, simdt, ctx=None, wind3d=False):
    """One fused UpdateAirSpeed/GroundSpeed/Position on ``traf`` (bs.traf-like).
    ``wind3d``: run a 3-D wind field (winddim 3) on the device instead of raising."""
    ctx = ctx or _lib.default_context()
    winddim = int(getattr(traf.wind, 'winddim', 0)) if hasattr(traf, 'wind') else 0
    vn = ve = 0.0
    if winddim == 1:
        vn = float(traf.wind.vnorth[0, 0])   # windfield.py:150-152
        ve = float(traf.wind.veast[0, 0])
    elif winddim == 2:
        w = traf.wind                         # Windfield.lat / lon / vnorth[0, :] / veast[0, :]
        ctx.set_windfield(w.lat, w.lon, np.asarray(w.vnorth)[0, :], np.asarray(w.veast)[0, :])
    elif winddim == 3 and wind3d:
        _upload_wind3d(ctx, traf.wind)
    elif winddim > 2:
        raise ValueError('winddim %d: the reference\'s 3-D wind interpolation fails for array '
                         'positions (windfield.py:177)' % winddim)
    state = {k: np.array(getattr(traf, k), dtype=np.float64, copy=True)
             for k in ('tas', 'hdg', 'alt', 'vs', 'lat', 'lon')}
    inputs = dict(ptas=traf.pilot.tas, phdg=traf.pilot.hdg, palt=traf.pilot.alt, pvs=traf.pilot.vs,
                  bank=traf.bank, eps=traf.eps, accel=traf.perf.acceleration())
    o = ctx.kinematics(simdt, state, inputs, winddim, vn, ve)
    # traffic.py:428-454
    traf.ax, traf.delspd = o['ax'], o['delspd']
    traf.tas, traf.cas, traf.M = state['tas'], o['cas'], o['mach']
    traf.swhdgsel, traf.hdg = o['swhdgsel'], state['hdg']
    traf.swaltsel, traf.az, traf.vs = o['swaltsel'], o['az'], state['vs']
    # traffic.py:458-476
    traf.gsnorth, traf.gseast, traf.gs, traf.trk = o['gsnorth'], o['gseast'], o['gs'], o['trk']
    # traffic.py:480-483
    traf.alt, traf.lat, traf.coslat, traf.lon = state['alt'], state['lat'], o['coslat'], state['lon']


def install(traf, ctx=None, wind3d=False):
    """Rebind the three Update* methods of a Traffic instance to the fused kernel.
    ``wind3d``: as in ``step``."""
    def _air(self, simdt, simt=None):
        step(self, simdt, ctx, wind3d)

    def _noop(self, simdt):
        return None

    traf.UpdateAirSpeed = types.MethodType(_air, traf)
    traf.UpdateGroundSpeed = types.MethodType(_noop, traf)
    traf.UpdatePosition = types.MethodType(_noop, traf)
    return traf
