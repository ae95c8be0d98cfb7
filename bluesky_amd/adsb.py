"""The ADS-B model on the device (bsa_adsb_update): a drop-in for
``bluesky.traffic.adsbmodel.ADSB``, installable as ``traf.adsb`` -- the truncated,
noisy broadcast picture ``detect(traf, traf.adsb, ...)`` can take as intruder.

The reference draws its normals from numpy's global Mersenne state.  Here they
are build-defined: the Philox4x64-10 block of counter
``{index, call, stream, 0}`` and key ``{seed, 0}``; stream 1 the update's three
normals, stream 2 ``create``'s uniform.  The reference draws ONE normal per
quantity per call (its ``nup = len(np.where(...))`` is 1), shared by every
updated aircraft: ``draws='shared'``, the default, restates that with index 0;
``draws='per_aircraft'`` gives every aircraft its own three.
"""
import numpy as np

from . import _lib

FT = 0.3048
FIELDS = _lib.ADSB_FIELDS
ARRAYS = ('lastupdate',) + FIELDS


def draws(n, seed=0, call=0, first_index=0, ctx=None, raw=False):
    """Unit normals ``(n, 3)`` -- lat, lon, alt -- of the aircraft indices ``first_index ..
    first_index + n - 1`` of call ``call`` (bsa_adsb_draws, stream 1); the shared draw is
    ``draws(1, seed, call)[0]``.  With ``raw`` also the Philox words ``(n, 4)`` uint64, first."""
    ctx = ctx or _lib.default_context()
    words, z, _ = ctx.adsb_draws(n, seed, call, first_index, stream=1, raw=raw)
    return (words, z) if raw else z


def create_uniforms(n, seed=0, call=0, first_index=0, ctx=None):
    """``create``'s uniforms in (0, 1] of the same indices (bsa_adsb_draws, stream 2)."""
    ctx = ctx or _lib.default_context()
    return ctx.adsb_draws(n, seed, call, first_index, stream=2, raw=False)[2]


class ADSB:
    """``SetNoise / create / delete / reset / update(time)`` of adsbmodel.py:8-59 on ``traf`` (``lat lon
    alt trk tas gs vs``); ``seed``, ``draws`` and ``call``, the number of updates that ran with noise
    on, define the draws.  It is a leaf of the reference's TrafficArrays tree
    (tools/trafficarrays.py): it carries ``parent`` and ``children`` and answers ``create_children`` and
    ``reparent``, because ``Traffic.create``, ``delete`` and ``reset`` reach the ADS-B object only
    through ``traf.children`` -- ``install`` puts it there."""

    def __init__(self, traf, seed=0, draws='shared', ctx=None):
        if draws not in _lib.ADSB_DRAWS:
            raise ValueError("draws: 'shared' or 'per_aircraft'")
        self.traf = traf
        self.ctx = ctx
        self.seed = int(seed)
        self.draws = draws
        self.call = 0
        self.parent = None
        self.children = []
        for k in ARRAYS:
            setattr(self, k, np.array([]))
        self.SetNoise(False)

    # ---- the TrafficArrays protocol (trafficarrays.py:58-62, 107-138) of an object without children
    def reparent(self, newparent):
        if self.parent is not None and self in self.parent.children:
            self.parent.children.remove(self)
        newparent.children.append(self)
        self.parent = newparent

    def create_children(self, n=1):
        pass

    def SetNoise(self, n):
        self.transnoise = n
        self.truncated = n
        self.transerror = [1e-4, 100 * FT]   # [degree, m] standard lat / lon distance, altitude error
        self.trunctime = 0                   # [s]

    def reset(self):
        for k in ARRAYS:
            setattr(self, k, np.array([]))

    def create(self, n=1):
        """adsbmodel.py:33-42: lastupdate = -trunctime * u, the picture from the new aircraft's state, vs 0."""
        first = len(self.lastupdate)
        for k in ARRAYS:
            setattr(self, k, np.append(getattr(self, k), np.zeros(n)))
        # (u lies in (0, 1]: with trunctime 0 the product is a zero whatever u, and no device is asked)
        u = create_uniforms(n, self.seed, self.call, first, ctx=self.ctx) if self.trunctime else np.ones(n)
        self.lastupdate[-n:] = -self.trunctime * u
        for k in FIELDS[:-1]:
            getattr(self, k)[-n:] = np.asarray(getattr(self.traf, k))[-n:]

    def delete(self, idx):
        for k in ARRAYS:
            setattr(self, k, np.delete(getattr(self, k), idx))

    def update(self, time, given=None):
        """adsbmodel.py:44-59 on the device.  ``given``: unit normals to apply instead of the object's own
        (three values, or (3, n) with per-aircraft draws) -- the replay of a recorded reference run."""
        if len(self.lastupdate) == 0:
            if self.transnoise:
                self.call += 1
            return
        ctx = self.ctx or _lib.default_context()
        out = ctx.adsb_update(time, {k: getattr(self.traf, k) for k in FIELDS}, {k: getattr(self, k) for k in ARRAYS},
                              trunctime=self.trunctime, noise=self.transnoise, transerror=self.transerror,
                              draws=self.draws, given=given if self.transnoise else None, seed=self.seed, call=self.call)
        for k in ARRAYS:
            setattr(self, k, out[k])
        if self.transnoise:
            self.call += 1


def install(traf, seed=0, draws='shared', ctx=None):
    """Replace ``traf.adsb`` by the device version, keeping its settings and arrays, and give it the old
    object's place among ``traf.children``: the reference's ``Traffic.create`` / ``delete`` / ``reset`` walk
    that list (``create_children``, trafficarrays.py:107-135) and name ``self.adsb`` only for ``update`` and
    ``SetNoise``.  A ``traf`` without ``children`` (a stand-in) only gets the attribute."""
    old = getattr(traf, 'adsb', None)
    new = ADSB(traf, seed=seed, draws=draws, ctx=ctx)
    if old is not None:
        new.transnoise, new.truncated = old.transnoise, old.truncated
        new.transerror, new.trunctime = list(old.transerror), old.trunctime
        for k in ARRAYS:
            setattr(new, k, np.array(getattr(old, k), dtype=np.float64))
    kids = getattr(traf, 'children', None)
    if kids is not None:
        at = [q for q, k in enumerate(kids) if k is old]
        if at:
            kids[at[0]] = new                # the same place: the children are created and deleted in list order
            old.parent = None
        else:
            kids.append(new)
        new.parent = traf
    traf.adsb = new
    return new
