"""Turbulence.Woosh on the device (bsa_turb_apply): a drop-in for
``bluesky.traffic.turbulence.Turbulence``, installable as ``traf.turbulence``.

The reference draws its three normal arrays from numpy's global Mersenne
state.  Here the draws are build-defined: aircraft ``i`` of
call number ``c`` owns the Philox4x64-10 block of counter ``{i, c, 0, 0}`` and
key ``{seed, 0}``; ``draws`` returns that stream.  Same statistics, another
sequence: a run repeats bitwise from ``seed``, whatever numpy's state.
"""
import numpy as np

from . import _lib


def draws(n, seed=0, call=0, first_index=0, ctx=None, raw=False):
    """Unit normals ``(n, 3)`` -- flight direction, wing direction, vertical -- of
    the aircraft indices ``first_index .. first_index + n - 1`` of call ``call``
    (bsa_turb_draws); with ``raw`` also the Philox words ``(n, 4)`` uint64, first."""
    ctx = ctx or _lib.default_context()
    words, z = ctx.turb_draws(n, seed, call, first_index, raw=raw)
    return (words, z) if raw else z


class Turbulence:
    """``reset / SetNoise / SetStandards / Woosh(dt)`` of turbulence.py:7-46 on ``traf``
    (``lat lon alt trk coslat ntraf``); ``seed`` and ``call``, the number of Wooshes
    that drew so far, define the draws."""

    def __init__(self, traf, seed=0, ctx=None):
        self.traf = traf
        self.ctx = ctx
        self.seed = int(seed)
        self.reset()

    def reset(self):
        self.active = False
        self.call = 0
        self.SetStandards([0, 0.1, 0.1])

    def SetNoise(self, n):
        self.active = n

    def SetStandards(self, s):
        sd = np.array(s, dtype=np.float64)
        if sd.shape != (3,) or not np.isfinite(sd).all() or (sd < 0).any():
            raise ValueError('turbulence standards: three finite values >= 0')
        self.sd = np.where(sd > 1e-6, sd, 1e-6)

    def Woosh(self, dt):
        if not self.active:
            return
        traf = self.traf
        ctx = self.ctx or _lib.default_context()
        if traf.ntraf > 0:
            traf.lat, traf.lon, traf.alt = ctx.turb_apply(dt, self.sd, traf.trk, traf.coslat, traf.lat, traf.lon,
                                                          traf.alt, seed=self.seed, call=self.call)
        self.call += 1


def install(traf, seed=0, ctx=None):
    """Replace ``traf.turbulence`` by the device version, keeping its ``active`` and ``sd``."""
    old = getattr(traf, 'turbulence', None)
    new = Turbulence(traf, seed=seed, ctx=ctx)
    if old is not None:
        new.SetStandards(old.sd)
        new.SetNoise(old.active)
    traf.turbulence = new
    return new
