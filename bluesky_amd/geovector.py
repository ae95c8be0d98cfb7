"""Geovectoring on the device (bsa_geovec_apply): a drop-in for ``plugins/geovector.py``
with the plugin's names and return values -- ``geovecs``, ``reset``, ``defgeovec``,
``delgeovec``, ``applygeovec`` -- without its ``bluesky.traf`` / stack dependency: the
traffic object is an argument.

A geovector is ``[area, gsmin, gsmax, trkmin, trkmax, vsmin, vsmax]`` in m/s, deg and m/s
(the stack command's unit conversions are the caller's).  A limit is on by Python truth,
as in the plugin: ``None`` or ``0`` is off, the track limit needs both bounds, so a track
bound of exactly 0 deg switches track limiting off.  Inside a resident run
the same list goes to ``ResidentSim.set_geovectors``.
"""
from . import _lib, areafilter

geovecs = []   # [[area, gsmin, gsmax, trkmin, trkmax, vsmin, vsmax]], applied in this order


def reset():
    """Forget every geovector."""
    global geovecs
    geovecs = []


def _find(area):
    return [k for k, vec in enumerate(geovecs) if vec[0].upper() == area.upper()]


def _sorted_pair(lo, hi):
    """min / max in the right order when both are on (not for the track: 355, 10 is a valid interval)."""
    return (min(lo, hi), max(lo, hi)) if (lo and hi) else (lo, hi)


def defgeovec(area="", spdmin=None, spdmax=None, trkmin=None, trkmax=None, vspdmin=None, vspdmax=None):
    """Define the geovector of ``area`` (replacing an older one of that name, compared
    upper-case); without any limit, report the one it has."""
    if area == "":
        return False, "We need an area"
    if not (spdmin or spdmax or (trkmin and trkmax) or vspdmin or vspdmax):
        hit = _find(area)
        if hit:
            return True, area + " uses " + str(geovecs[hit[0]][1:]) + " gs[m/s], trk[deg], vs[m/s]"
        return False, "No geovector found for " + area
    geovecs[:] = [vec for vec in geovecs if vec[0].upper() != area.upper()]
    gsmin, gsmax = _sorted_pair(spdmin, spdmax)
    vsmin, vsmax = _sorted_pair(vspdmin, vspdmax)
    geovecs.append([area, gsmin, gsmax, trkmin, trkmax, vsmin, vsmax])
    return True


def delgeovec(area=""):
    """Remove the geovector of ``area``."""
    if not _find(area):
        return False, "No geovector found for " + area
    geovecs[:] = [vec for vec in geovecs if vec[0].upper() != area.upper()]
    return True


def table(geovecs, areanames):
    """The ``bsa_geovec`` rows of a geovector list over the shape table whose names are
    ``areanames``: ``(rows, kept)``, ``rows`` a list of ``(shape, given, gsmin, gsmax, trkmin,
    trkmax, vsmin, vsmax)`` as ``_lib.geovec_rows`` takes it, ``kept`` the positions in
    ``geovecs`` they came from.  The ``given`` bits are set by Python truth; a bound that is
    off is stored as 0; a geovector whose area is not in ``areanames`` is skipped, as
    ``applygeovec`` skips it."""
    names = list(areanames)
    rows, kept = [], []
    for k, (area, gsmin, gsmax, trkmin, trkmax, vsmin, vsmax) in enumerate(geovecs):
        if area not in names:
            continue
        trk = bool(trkmin and trkmax)
        given = (_lib.GEOVEC_GSMIN if gsmin else 0) | (_lib.GEOVEC_GSMAX if gsmax else 0) | \
                (_lib.GEOVEC_TRK if trk else 0) | (_lib.GEOVEC_VSMIN if vsmin else 0) | \
                (_lib.GEOVEC_VSMAX if vsmax else 0)
        rows.append((names.index(area), given, float(gsmin or 0.), float(gsmax or 0.), float(trkmin) if trk else 0.,
                     float(trkmax) if trk else 0., float(vsmin or 0.), float(vsmax or 0.)))
        kept.append(k)
    return rows, kept


def apply_arrays(geovecs, areas, lat, lon, alt, trk, vs, selspd, ap_trk, selvs, selalt, ctx=None, nocull=False):
    """One application of ``geovecs`` over the areas ``areas`` (name -> (type, coordinates,
    top, bottom)) in one launch: (dict of selspd / ap_trk / selvs / selalt after it, new
    arrays; changed (4,) uint64 -- aircraft changed per array)."""
    names = list(areas)
    rows, _ = table(geovecs, names)
    ctx = ctx or _lib.default_context()
    return ctx.geovec_apply([areas[k] for k in names], rows, lat, lon, alt, trk, vs, selspd, ap_trk, selvs, selalt,
                            nocull=nocull)


def applygeovec(traf, ctx=None):
    """Apply every geovector to ``traf`` (``lat lon alt trk vs selspd selvs selalt ap.trk``):
    ``traf.selspd``, ``traf.ap.trk``, ``traf.selvs`` and ``traf.selalt`` are written in place.
    The areas are ``bluesky_amd.areafilter.areas``."""
    if not geovecs or traf.ntraf == 0:
        return
    out, _ = apply_arrays(geovecs, areafilter.areas, traf.lat, traf.lon, traf.alt, traf.trk, traf.vs, traf.selspd,
                          traf.ap.trk, traf.selvs, traf.selalt, ctx=ctx)
    traf.selspd[:] = out['selspd']
    traf.ap.trk[:] = out['ap_trk']
    traf.selvs[:] = out['selvs']
    traf.selalt[:] = out['selalt']
