"""GPU: the area filter's inside tests (bsa_area_inside, bluesky_amd.areafilter) against the
reference's masks (tests/golden/area_shapes.npz): exact equality at the wave and word seams,
cull on equal to cull off, counts equal to the masks' popcounts, argument errors reported."""
import ctypes
import os

import numpy as np
import pytest

from bluesky_amd import _lib, areafilter
from tests import area_np, util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    g = dict(np.load(os.path.join(util.GOLDEN, 'area_shapes.npz')))
    g['shapes'] = area_np.named(area_np.load_shapes(g))
    g['names'] = [str(x) for x in g['names']]
    return g


@pytest.fixture()
def defined(golden):
    areafilter.reset()
    for name, (typ, co, top, bottom) in zip(golden['names'], golden['shapes']):
        areafilter.defineArea(name, 'POLYALT' if name == 'SEAM' else typ, list(co), top, bottom)
    yield golden
    areafilter.reset()


def points(g, n):
    """n points of the golden set: the whole set, or a slice that ends with the on-border and
    non-finite points (the random ones in front are dropped first)."""
    k = len(g['lat']) - n if n < 300 else 0
    return slice(k, k + n)


@pytest.mark.parametrize('n', [1, 63, 64, 65, 3000])
def test_check_inside_equals_reference(ctx, defined, n):
    g = defined
    for sl in (points(g, n), slice(0, n)):
        lat, lon, alt = g['lat'][sl], g['lon'][sl], g['alt'][sl]
        every = areafilter.checkInsideAll(g['names'], lat, lon, alt, ctx=ctx)
        assert every.shape == (len(g['names']), n) and every.dtype == bool
        assert np.array_equal(every, g['masks'][:, sl])
        for k, name in enumerate(g['names']):
            assert np.array_equal(areafilter.checkInside(name, lat, lon, alt, ctx=ctx), g['masks'][k, sl]), name


def test_whole_golden_set(ctx, defined):
    g = defined
    assert np.array_equal(areafilter.checkInsideAll(g['names'], g['lat'], g['lon'], g['alt'], ctx=ctx), g['masks'])


def test_dropin_names(ctx, defined):
    g = defined
    assert areafilter.hasArea('C') and not areafilter.hasArea('NOSUCH')
    lat, lon, alt = g['lat'][:100], g['lon'][:100], g['alt'][:100]
    assert not areafilter.checkInside('NOSUCH', lat, lon, alt, ctx=ctx).any()
    assert not areafilter.checkInside('LINE', lat, lon, alt, ctx=ctx).any()
    got = areafilter.checkInsideAll(['NOSUCH', 'C', 'LINE'], lat, lon, alt, ctx=ctx)
    assert not got[0].any() and not got[2].any() and np.array_equal(got[1], g['masks'][g['names'].index('C'), :100])
    areafilter.deleteArea('C')
    assert not areafilter.hasArea('C') and not areafilter.checkInside('C', lat, lon, alt, ctx=ctx).any()
    areafilter.deleteArea('C')
    assert areafilter.checkInsideAll([], lat, lon, alt, ctx=ctx).shape == (0, 100)
    assert areafilter.checkInside('TRI', [], [], [], ctx=ctx).shape == (0,)


@pytest.mark.parametrize('ns', [1, 64, 65])
@pytest.mark.parametrize('n', [65, 3000])
def test_word_seam_cull_and_counts(ctx, golden, ns, n):
    g = golden
    # golden shapes repeated, starting at the long polygon: shape s is golden shape order[s]
    order = (np.arange(ns) + g['names'].index('SEAM')) % len(g['shapes'])
    shapes = [g['shapes'][k] for k in order]
    sl = points(g, n)
    lat, lon, alt = g['lat'][sl], g['lon'][sl], g['alt'][sl]
    inside, counts = ctx.area_inside(shapes, lat, lon, alt)
    assert np.array_equal(inside, g['masks'][order][:, sl])
    assert np.array_equal(counts, inside.sum(axis=1).astype(np.uint64))
    inside0, counts0 = ctx.area_inside(shapes, lat, lon, alt, nocull=True)
    assert np.array_equal(inside0, inside) and np.array_equal(counts0, counts)


def test_cull_skips_nothing_it_should_keep(ctx, golden):
    """Sorted points (compact waves, as the resident step's home order gives them): most waves skip
    most shapes, and the result is that of the unculled run."""
    g = golden
    o = np.lexsort((g['lon'], np.round(g['lat'] * 4), np.round(g['alt'] / 3000.0)))
    lat, lon, alt = g['lat'][o], g['lon'][o], g['alt'][o]
    inside, counts = ctx.area_inside(g['shapes'], lat, lon, alt)
    inside0, counts0 = ctx.area_inside(g['shapes'], lat, lon, alt, nocull=True)
    assert np.array_equal(inside, g['masks'][:, o])
    assert np.array_equal(inside0, inside) and np.array_equal(counts0, counts)


def raw_call(ctx, n, lat, lon, alt, ns, tab, nv, verts, flags=0, out=True):
    W = max(1, (max(ns, 0) + 63) // 64)
    words = np.zeros((W, max(n, 1)), dtype=np.uint64)
    counts = np.zeros(max(ns, 1), dtype=np.uint64)
    rc = ctx.lib.bsa_area_inside(ctx.h, n, _lib.ptr(lat), _lib.ptr(lon), _lib.ptr(alt), ns, tab, nv, _lib.ptr(verts),
                                 flags, _lib.ptr(words, _lib._c_u64p) if out else None,
                                 _lib.ptr(counts, _lib._c_u64p))
    return rc, ctx.lib.bsa_last_error(ctx.h).decode()


def test_argument_errors_are_reported(ctx, golden):
    g = golden
    tab, verts = _lib.area_table(g['shapes'])
    ns, nv = len(g['shapes']), len(verts)
    lat, lon, alt = (np.ascontiguousarray(g[k][:10]) for k in ('lat', 'lon', 'alt'))
    assert raw_call(ctx, 10, lat, lon, alt, ns, tab, nv, verts)[0] == 0
    for bad in [dict(lat=None), dict(lon=None), dict(alt=None), dict(tab=None), dict(verts=None), dict(out=False),
                dict(n=-1), dict(ns=-1), dict(ns=_lib.AREA_SHAPES_MAX + 1), dict(nv=_lib.AREA_VERTS_MAX + 1),
                dict(nv=-1), dict(flags=2)]:
        a = dict(n=10, lat=lat, lon=lon, alt=alt, ns=ns, tab=tab, nv=nv, verts=verts, flags=0, out=True)
        a.update(bad)
        rc, msg = raw_call(ctx, a['n'], a['lat'], a['lon'], a['alt'], a['ns'], a['tab'], a['nv'], a['verts'],
                           a['flags'], a['out'])
        assert rc != 0 and 'bsa_area_inside' in msg, (bad, msg)
    k = g['names'].index('TRI')
    for field, value, word in [('nvert', 0, 'polygon'), ('nvert', -3, 'polygon'), ('voff', nv - 2, 'outside'),
                               ('voff', -1, 'outside'), ('nvert', nv + 1, 'outside'), ('type', 7, 'unknown type')]:
        t2, _ = _lib.area_table(g['shapes'])
        setattr(t2[k], field, value)
        rc, msg = raw_call(ctx, 10, lat, lon, alt, ns, t2, nv, verts)
        assert rc != 0 and word in msg, (field, value, msg)
    v2 = verts.copy()
    v2[tab[k].voff, 1] = np.nan
    rc, msg = raw_call(ctx, 10, lat, lon, alt, ns, tab, nv, v2)
    assert rc != 0 and 'not finite' in msg
    # and the context still works
    assert raw_call(ctx, 10, lat, lon, alt, ns, tab, nv, verts)[0] == 0
    assert raw_call(ctx, 0, None, None, None, ns, tab, nv, verts)[0] == 0     # no points: nothing to do
    with pytest.raises(ValueError):
        ctx.area_inside(g['shapes'], lat, lon[:5], alt)
    assert ctypes.sizeof(_lib.AreaShape) == 96
