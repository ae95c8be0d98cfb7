"""The area filter on the device (bsa_area_inside): a drop-in for
``bluesky.tools.areafilter`` with the same names and signatures, without its
``bs.scr`` dependency (nothing is drawn).

``checkInside`` returns what the reference's Box / Circle / Poly / Line return
(areafilter.py:52-104; the polygon rule is matplotlib's even-odd crossing count
on (lat, lon)); ``checkInsideAll`` tests any number of areas in
one launch.
"""
import numpy as np

from . import _lib

areas = dict()   # name -> (type, coordinates, top, bottom), as area_table takes them
_NOWHERE = ('LINE', (), 1e9, -1e9)


def hasArea(areaname):
    """Check if area with name 'areaname' exists."""
    return areaname in areas


def defineArea(areaname, areatype, coordinates, top=1e9, bottom=-1e9):
    """Define a new area: BOX, CIRCLE, POLY* or LINE; any other type defines nothing
    (areafilter.py:15-24)."""
    t = 'POLY' if areatype[:4] == 'POLY' else areatype
    if t not in _lib.AREA_TYPES:
        return
    coords = np.array(coordinates, dtype=np.float64).ravel()
    if t == 'POLY' and len(coords) < 2:
        raise ValueError('a polygon needs at least one (lat, lon) vertex')
    _lib.area_table([(t, coords, top, bottom)])   # (the coordinate counts, now)
    areas[areaname] = (t, coords, float(top), float(bottom))


def checkInside(areaname, lat, lon, alt, ctx=None):
    """Are the points lat, lon, alt inside area 'areaname'?  An array of booleans,
    all False for a LINE or an unknown name."""
    return checkInsideAll([areaname], lat, lon, alt, ctx=ctx)[0]


def checkInsideAll(areanames, lat, lon, alt, ctx=None):
    """``checkInside`` for every name of ``areanames`` in one launch: a
    ``(len(areanames), n)`` bool array."""
    lat = np.atleast_1d(lat)
    if len(areanames) == 0 or len(lat) == 0:
        return np.zeros((len(areanames), len(lat)), dtype=bool)
    ctx = ctx or _lib.default_context()
    return ctx.area_inside([areas.get(k, _NOWHERE) for k in areanames], lat, np.atleast_1d(lon),
                           np.atleast_1d(alt))[0]


def deleteArea(areaname):
    """ Delete area with name 'areaname'. """
    areas.pop(areaname, None)


def reset():
    """ Clear all data. """
    areas.clear()
