"""CPU: tests/geovec_np.py, the numpy restatement of plugins/geovector.py:76-128, against the
reference plugin's own results in tests/golden/geovec_apply.npz (tools/make_golden_geovec.py).
ap_trk, selvs and selalt are copies of bounds or one addition: bitwise.  selspd is vtas2cas, two
pow calls, and this numpy's pow may differ from the capture's in the last bits: which aircraft
changed is exact (the capture keeps every random selspd 1e-6 relative away from a clamp value),
the values within util.close's 1e-9 rule."""
import os

import numpy as np
import pytest

from tests import geovec_np, util


@pytest.fixture(scope='module')
def golden():
    g = dict(np.load(os.path.join(util.GOLDEN, 'geovec_apply.npz')))
    return g, geovec_np.load_lists(g), geovec_np.load_areas(g), geovec_np.load_state(g)


def test_every_list_matches_the_reference(golden):
    g, lists, areas, st = golden
    assert len(lists) == len(g['list_names']) >= 9
    for q, name in enumerate(str(x) for x in g['list_names']):
        got = geovec_np.apply(lists[name], areas, st)
        exp = {k: g['out_' + k][q] for k in geovec_np.TARGETS}
        for k in ('ap_trk', 'selvs', 'selalt'):
            assert np.array_equal(got[k].view(np.uint64), exp[k].view(np.uint64)), (name, k)
        cnt, m = geovec_np.changed(st, got)
        _, me = geovec_np.changed(st, exp)
        assert np.array_equal(m['selspd'], me['selspd']), name
        ok, msg = util.close(got['selspd'], exp['selspd'], 100.0)
        assert ok, '%s selspd: %s' % (name, msg)
        assert np.array_equal(cnt, g['changed'][q]), name


def test_golden_holds_what_the_tests_rely_on(golden):
    g, lists, areas, st = golden
    names = [str(x) for x in g['list_names']]
    assert (g['margins'][:4] >= 1e-9).all() and g['margins'][4] >= 1e-6 and (g['margins'][5:] >= 1e-9).all()
    ab, ba = names.index('overlap_ab'), names.index('overlap_ba')
    assert not np.array_equal(g['out_selspd'][ab], g['out_selspd'][ba])          # the order of the list matters
    assert g['changed'][names.index('line_and_missing')].sum() == 0
    z = names.index('zero_is_off')
    assert lists['zero_is_off'][0][3] == 0.0 and lists['zero_is_off'][0][6] == 0.0
    assert g['changed'][z][1] == 0 and g['changed'][z][0] > 0                    # trkmin = 0 switches the track limit off
    assert lists['box_all'][0][1:] == [150., 210., 100., 200., -5., 5.]          # defgeovec swapped speed and V/S
    assert lists['circle_wrap'][0][3:5] == [350., 30.]                           # ... and never the track
    seam = areas['SEAM']
    assert seam[0] == 'POLY' and len(seam[1]) // 2 == 65
    assert np.isnan(st['lat'][:64]).any() and np.isnan(st['alt'][:64]).any() and np.isnan(st['vs'][:64]).any() \
        and np.isnan(st['trk'][:64]).any()
    assert (g['changed'][names.index('box_all')] >= 20).all()


def test_untouched_aircraft_keep_their_bits(golden):
    g, lists, areas, st = golden
    got = geovec_np.apply(lists['three_areas'], areas, st)
    _, m = geovec_np.changed(st, got)
    inside_any = np.zeros(len(st['lat']), bool)
    for name in ('C', 'SEAM', 'CIRC'):
        typ, co, top, bottom = areas[name]
        inside_any |= geovec_np.area_np.inside(geovec_np.area_np.TYPE_NAMES.index(typ), co, top, bottom, st['lat'], st['lon'],
                                               st['alt'])
    for k in geovec_np.TARGETS:
        assert not m[k][~inside_any].any(), k
    assert (~inside_any).sum() > 100 and inside_any.sum() > 100
