#!/usr/bin/env python3
"""Capture tests/golden/area_shapes.npz from the REFERENCE area filter (build container only).

Runs the reference's own ``Box`` / ``Circle`` / ``Poly`` / ``Line`` objects
(bluesky/tools/areafilter.py:52-104; ``defineArea`` needs ``bs.scr``, so the
shapes are constructed directly) on fixed shapes and points and stores the
shapes, the points and the reference's masks -- arrays only.  The numpy
restatement tests/area_np.py is asserted equal at capture.

It also ASSERTS, and records, the margins that make every comparison of the
tests exact equality: no random point within 1e-9 deg of a polygon edge or a
box face, none within 1e-9 relative of the circle's rim.  If an assertion
fires, change the seed, not the margin.

Usage:  python tools/make_golden_area.py
"""
import os
import sys

import numpy as np

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT = os.path.join(REPO, 'tests', 'golden', 'area_shapes.npz')

# numpy-2 shims for the 2019 reference
np.mat = np.asmatrix
np.int = int
np.float = float
np.object = object
np.str = str
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, REPO)

from bluesky.tools import areafilter as ref      # noqa: E402
from tests import area_np                         # noqa: E402

FT = 0.3048
SEED = 20261020
MARGIN = 1e-9
CHUNK = 64          # bsa_area.hip: kAreaChunk
CLAT, CLON = 52.0, 4.0


def ring(n, r0, wobble, phase=0.0, seed=0):
    """n vertices around (CLAT, CLON), radius r0 deg modulated by +/- wobble."""
    rng = np.random.RandomState(seed)
    th = phase + 2 * np.pi * np.arange(n) / n
    r = r0 * (1.0 + wobble * rng.uniform(-1, 1, n))
    return np.column_stack((CLAT + r * np.cos(th), CLON + 1.6 * r * np.sin(th))).ravel()


def shapes():
    star = [CLAT + 0.9 * np.cos(2 * np.pi * k * 2 / 5 + 0.3) for k in range(5)]
    star_lon = [CLON + 1.4 * np.sin(2 * np.pi * k * 2 / 5 + 0.3) for k in range(5)]
    pentagram = np.column_stack((star, star_lon)).ravel()
    c_shape = np.array([51.2, 2.5, 52.8, 2.5, 52.8, 5.0, 52.4, 5.0, 52.4, 3.2, 51.6, 3.2, 51.6, 5.0, 51.2, 5.0])
    out = [
        # name,      type,     coordinates,                               top,          bottom
        ('BOXSWAP', 'BOX', np.array([52.6, 5.1, 51.4, 2.9]), 5000 * FT, 30000 * FT),   # corners and levels swapped
        ('CIRC', 'CIRCLE', np.array([52.1, 3.9, 45.0]), 40000 * FT, 10000 * FT),
        ('TRI', 'POLY', np.array([51.0, 2.0, 53.0, 3.5, 51.5, 6.0]), 1e9, -1e9),
        ('C', 'POLY', c_shape, 35000 * FT, 0.0),
        ('PENTAGRAM', 'POLY', pentagram, 1e9, -1e9),
        ('P37', 'POLY', ring(37, 0.8, 0.35, 0.1, seed=1), 45000 * FT, 2000 * FT),
        ('SEAM', 'POLYALT', ring(CHUNK + 1, 1.0, 0.3, 0.7, seed=2), 20000 * FT, 44000 * FT),   # one vertex past a chunk
        ('REPEAT', 'POLY', np.array([51.5, 3.0, 52.5, 3.0, 52.5, 3.0, 52.5, 5.0, 51.5, 5.0, 51.5, 5.0]), 1e9, -1e9),
        ('TWO', 'POLY', np.array([51.0, 2.0, 53.0, 6.0]), 1e9, -1e9),
        ('LINE', 'LINE', np.array([51.0, 2.0, 53.0, 6.0]), 1e9, -1e9),
    ]
    return out


def ref_object(name, typ, coords, top, bottom):
    if typ == 'BOX':
        return ref.Box(name, coords, top, bottom)
    if typ == 'CIRCLE':
        return ref.Circle(name, coords, top, bottom)
    if typ[:4] == 'POLY':
        return ref.Poly(name, coords, top, bottom)
    return ref.Line(name, coords)


def seg_dist(px, py, ax, ay, bx, by):
    """Planar distance [deg] of points to the segment a-b."""
    dx, dy = bx - ax, by - ay
    L2 = dx * dx + dy * dy
    t = np.zeros_like(px) if L2 == 0 else np.clip(((px - ax) * dx + (py - ay) * dy) / L2, 0, 1)
    return np.hypot(px - (ax + t * dx), py - (ay + t * dy))


def main():
    rng = np.random.RandomState(SEED)
    sh = shapes()
    nrand = 3000
    lat = rng.uniform(CLAT - 1.5, CLAT + 1.5, nrand)
    lon = rng.uniform(CLON - 2.5, CLON + 2.5, nrand)
    alt = rng.uniform(0.0, 45000 * FT, nrand)

    # the margins of the random points
    m_edge, m_face, m_rim, m_level = np.inf, np.inf, np.inf, np.inf
    for name, typ, co, top, bottom in sh:
        if typ != 'LINE':
            m_level = min(m_level, np.abs(alt - top).min(), np.abs(alt - bottom).min())
        if typ == 'BOX':
            m_face = min(m_face, np.abs(lat - co[0]).min(), np.abs(lat - co[2]).min(),
                         np.abs(lon - co[1]).min(), np.abs(lon - co[3]).min())
        elif typ == 'CIRCLE':
            d = ref.kwikdist(co[0], co[1], lat, lon)
            m_rim = min(m_rim, (np.abs(d - co[2]) / co[2]).min())
        elif typ[:4] == 'POLY':
            v = co.reshape(-1, 2)
            for k in range(len(v)):
                m_edge = min(m_edge, seg_dist(lat, lon, v[k - 1, 0], v[k - 1, 1], v[k, 0], v[k, 1]).min())
    assert m_edge >= MARGIN, 'a random point within %g deg of a polygon edge (%g): change SEED' % (MARGIN, m_edge)
    assert m_face >= MARGIN, 'a random point within %g deg of a box face (%g): change SEED' % (MARGIN, m_face)
    assert m_rim >= MARGIN, 'a random point within %g relative of the rim (%g): change SEED' % (MARGIN, m_rim)
    assert m_level >= MARGIN, 'a random altitude within %g m of a level (%g): change SEED' % (MARGIN, m_level)

    # on-border points (boxes and polygons only: comparisons and products) and non-finite ones
    bl, bo = [], []
    for name, typ, co, top, bottom in sh:
        if typ[:4] == 'POLY':
            v = co.reshape(-1, 2)
            bl += list(v[:, 0]) + list(0.5 * (v[:, 0] + np.roll(v[:, 0], -1)))
            bo += list(v[:, 1]) + list(0.5 * (v[:, 1] + np.roll(v[:, 1], -1)))
        elif typ == 'BOX':
            bl += [co[0], co[0], co[2], co[2]]
            bo += [co[1], co[3], co[1], co[3]]
    nborder = len(bl)
    nf = np.array([[np.nan, 4.0, 6000.0], [52.0, np.nan, 6000.0], [52.0, 4.0, np.nan],
                   [np.inf, 4.0, 6000.0], [52.0, -np.inf, 6000.0], [52.0, 4.0, np.inf]])
    lat = np.concatenate((lat, bl, nf[:, 0]))
    lon = np.concatenate((lon, bo, nf[:, 1]))
    alt = np.concatenate((alt, np.full(nborder, 6000.0), nf[:, 2]))

    masks = np.zeros((len(sh), len(lat)), dtype=bool)
    for k, (name, typ, co, top, bottom) in enumerate(sh):
        with np.errstate(invalid='ignore'):
            masks[k] = ref_object(name, typ, co, top, bottom).checkInside(lat, lon, alt)
        mine = area_np.inside(area_np.TYPE_NAMES.index(typ[:4] if typ[:4] == 'POLY' else typ), co, top, bottom,
                              lat, lon, alt)
        assert np.array_equal(mine, masks[k]), (name, np.flatnonzero(mine != masks[k]))
        print('%-10s %-7s %3d vertices  inside %4d of %d' % (name, typ, len(co) // 2 if typ[:4] == 'POLY' else 0,
                                                            masks[k].sum(), len(lat)))
    off = np.concatenate(([0], np.cumsum([len(s[2]) for s in sh])))
    np.savez_compressed(
        OUT, names=np.array([s[0] for s in sh]),
        types=np.array([area_np.TYPE_NAMES.index('POLY' if s[1][:4] == 'POLY' else s[1]) for s in sh], dtype=np.int32),
        coords=np.concatenate([s[2] for s in sh]), coord_off=off.astype(np.int64),
        top=np.array([s[3] for s in sh]), bottom=np.array([s[4] for s in sh]),
        lat=lat, lon=lon, alt=alt, masks=masks, nrandom=np.int64(nrand), nborder=np.int64(nborder),
        nnonfinite=np.int64(len(nf)), margin=np.float64(MARGIN),
        margins=np.array([m_edge, m_face, m_rim, m_level]), chunk=np.int64(CHUNK), seed=np.int64(SEED))
    print('margins: edge %.3g deg, box face %.3g deg, rim %.3g rel, level %.3g m' % (m_edge, m_face, m_rim, m_level))
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
