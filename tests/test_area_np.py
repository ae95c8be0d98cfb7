"""CPU: the numpy restatement of the area filter (tests/area_np.py) against the reference's
masks (tests/golden/area_shapes.npz): exact equality, on-border and non-finite points included."""
import os

import numpy as np
import pytest

from tests import area_np
from tests.util import GOLDEN


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(os.path.join(GOLDEN, 'area_shapes.npz')))


def test_restatement_equals_reference(golden):
    g = golden
    shapes = area_np.load_shapes(g)
    assert len(shapes) == 10 and g['masks'].shape == (10, len(g['lat']))
    for k, (typ, co, top, bottom) in enumerate(shapes):
        got = area_np.inside(typ, co, top, bottom, g['lat'], g['lon'], g['alt'])
        assert np.array_equal(got, g['masks'][k]), (str(g['names'][k]), np.flatnonzero(got != g['masks'][k])[:8])


def test_golden_margins_and_cases(golden):
    g = golden
    assert (g['margins'] >= g['margin']).all() and g['margin'] == 1e-9
    assert int(g['nrandom']) + int(g['nborder']) + int(g['nnonfinite']) == len(g['lat'])
    names = [str(x) for x in g['names']]
    nv = np.diff(g['coord_off']) // 2
    assert nv[names.index('SEAM')] == int(g['chunk']) + 1 and nv[names.index('P37')] == 37 and nv[names.index('TWO')] == 2
    m = g['masks']
    assert not m[:, -int(g['nnonfinite']):].any()              # a non-finite coordinate is never inside
    assert not m[names.index('TWO')].any() and not m[names.index('LINE')].any()
    assert g['top'][0] < g['bottom'][0] and m[0].any()         # the box given upside down still holds points
    border = slice(int(g['nrandom']), int(g['nrandom']) + int(g['nborder']))
    assert m[:, border].any() and not m[:, border].all()       # on-border points fall on both sides


def test_pentagram_centre_is_outside(golden):
    g = golden
    k = [str(x) for x in g['names']].index('PENTAGRAM')
    typ, co, top, bottom = area_np.load_shapes(g)[k]
    v = co.reshape(-1, 2)
    c = v.mean(axis=0)
    assert not area_np.inside(typ, co, top, bottom, [c[0]], [c[1]], [0.0])[0]      # even-odd, not winding
    tip = 0.9 * v[0] + 0.1 * c
    assert area_np.inside(typ, co, top, bottom, [tip[0]], [tip[1]], [0.0])[0]
