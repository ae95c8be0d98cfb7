"""numpy restatement of the area filter's inside tests (bluesky/tools/areafilter.py:61-104,
geo.py:288-305, and matplotlib's Path.contains_points as the even-odd rule of DESIGN.md 3.26).
Pinned bitwise to the reference by tests/golden/area_shapes.npz (test_area_np.py)."""
import numpy as np

NM = 1852.0
RE = 6371000.0
LINE, BOX, CIRCLE, POLY = 0, 1, 2, 3
TYPE_NAMES = ('LINE', 'BOX', 'CIRCLE', 'POLY')


def levels(top, bottom, alt):
    hi, lo = np.maximum(bottom, top), np.minimum(bottom, top)
    return (lo <= alt) & (alt <= hi)


def box(c, lat, lon):
    lat0, lat1 = min(c[0], c[2]), max(c[0], c[2])
    lon0, lon1 = min(c[1], c[3]), max(c[1], c[3])
    return ((lat0 <= lat) & (lat <= lat1)) & ((lon0 <= lon) & (lon <= lon1))


def kwikdist(lata, lona, latb, lonb):
    dlat = np.radians(latb - lata)
    dlon = np.radians(lonb - lona)
    cavelat = np.cos(np.radians(lata + latb) * 0.5)
    return RE * np.sqrt(dlat * dlat + dlon * dlon * cavelat * cavelat) / NM


def circle(c, lat, lon):
    return kwikdist(c[0], c[1], lat, lon) <= c[2]


def poly(c, lat, lon):
    """Even-odd crossing count over the closed ring, x = lat, y = lon."""
    v = np.asarray(c, dtype=np.float64)
    v = v[:2 * (len(v) // 2)].reshape(-1, 2)
    x, y = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    inside = np.zeros(x.shape, dtype=bool)
    if len(v) < 3:
        return inside
    with np.errstate(invalid='ignore'):
        for k in range(len(v)):
            x0, y0 = v[k - 1]
            x1, y1 = v[k]
            f0, f1 = y0 >= y, y1 >= y
            inside ^= (f0 != f1) & (((y1 - y) * (x0 - x1) >= (x1 - x) * (y0 - y1)) == f1)
    return inside & np.isfinite(x) & np.isfinite(y)


def inside(typ, coords, top, bottom, lat, lon, alt):
    lat, lon, alt = (np.asarray(a, dtype=np.float64) for a in (lat, lon, alt))
    with np.errstate(invalid='ignore'):
        if typ == BOX:
            hor = box(coords, lat, lon)
        elif typ == CIRCLE:
            hor = circle(coords, lat, lon)
        elif typ == POLY:
            hor = poly(coords, lat, lon)
        else:
            return np.zeros(lat.shape, dtype=bool)
        return hor & levels(top, bottom, alt)


def load_shapes(g):
    """[(type, coordinates, top, bottom)] of a golden file's shape arrays."""
    off = g['coord_off']
    return [(int(g['types'][k]), g['coords'][off[k]:off[k + 1]].copy(), float(g['top'][k]), float(g['bottom'][k]))
            for k in range(len(g['types']))]


def named(shapes):
    """The same list with type names, as bluesky_amd takes it."""
    return [(TYPE_NAMES[t], c, top, bottom) for t, c, top, bottom in shapes]
