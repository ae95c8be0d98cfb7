"""CPU: tests/wind3d_np.py against the reference's per-position getdata
(tests/golden/wind3d_*.npz, kin3d_wind1500.npz), compared the way
test_oracle_golden.py compares kin_windfield1500."""
import numpy as np
import pytest

from oracle import kinematics as okin
from tests import util, wind3d_np

CASES = util.golden('wind3d_*.npz')


def test_fixtures_present():
    assert [util.case_name(p) for p in CASES] == ['wind3d_n1', 'wind3d_n5', 'wind3d_n67']


@pytest.mark.parametrize('path', CASES, ids=[util.case_name(p) for p in CASES])
def test_helper_matches_reference(path):
    z = np.load(path)
    vn, ve = wind3d_np.getdata(z['lat'], z['lon'], z['alt'], **wind3d_np.field_of(z))
    assert util.close(vn, z['vnorth'], 1.0, rtol=1e-12)[0] and util.close(ve, z['veast'], 1.0, rtol=1e-12)[0]
    assert z['wvnorth'].shape == (451, len(z['wlat']))          # Windfield's axis: 0 .. 45000 ft by 100 ft
    # the edge positions the capture plants: below and at the ground, on a level, just under the top
    st = float(z['altstep'])
    assert list(z['alt'][:4]) == [-10.0, 0.0, 7 * st, 13715.9]
    assert z['lat'][8] == z['wlat'][0] and z['lon'][8] == z['wlon'][0]
    assert (z['lat'][9:12] < 0).all()


def test_level_edges():
    st, nalt = 30.48, 451
    top = (nalt - 1) * st
    alt = np.array([-10.0, 0.0, 7 * st, 13715.9, top, top + 300.0, np.inf, -np.inf, np.nan])
    ialt, falt = wind3d_np.level(alt, nalt, st)
    assert list(ialt) == [0, 0, 7, 449, 449, 449, 449, 0, 0]
    assert list(falt[:3]) == [0.0, 0.0, 0.0] and 0.99 < falt[3] < 1.0
    assert list(falt[4:8]) == [1.0, 1.0, 1.0, 0.0] and np.isnan(falt[8])


def test_top_level_and_nan_altitude():
    """Build-defined: at and above the top level the top level's wind, NaN carried through."""
    z = np.load(CASES[1])
    f = wind3d_np.field_of(z)
    top = (z['wvnorth'].shape[0] - 1) * f['altstep']
    lat, lon = z['lat'][:3], z['lon'][:3]
    vn, ve = wind3d_np.getdata(lat, lon, np.array([top, top + 300.0, np.nan]), **f)
    flat = dict(f, wvnorth=np.repeat(z['wvnorth'][-1:], 451, axis=0), wveast=np.repeat(z['wveast'][-1:], 451, axis=0))
    en, ee = wind3d_np.getdata(lat, lon, np.array([100.0, 100.0, 100.0]), **flat)
    assert util.close(vn[:2], en[:2], 1.0, rtol=1e-12)[0] and util.close(ve[:2], ee[:2], 1.0, rtol=1e-12)[0]
    assert np.isnan(vn[2]) and np.isnan(ve[2])


def test_helper_with_oracle_kinematics_matches_reference():
    z = dict(np.load(util.golden('kin3d_wind1500.npz')[0], allow_pickle=False))
    assert int(z['winddim']) == 3
    s = {k: z[k] for k in ('lat', 'lon', 'alt', 'tas', 'hdg', 'vs', 'ptas', 'phdg', 'palt', 'pvs',
                           'bank', 'eps', 'accel')}
    vn, ve = wind3d_np.getdata(z['lat'], z['lon'], z['alt'], **wind3d_np.field_of(z))
    assert util.close(vn, z['windnorth'], 1.0, rtol=1e-12)[0] and util.close(ve, z['windeast'], 1.0, rtol=1e-12)[0]
    o = okin.step(s, float(z['dt']), 1, vn, ve)
    for k in ('ax', 'delspd', 'tas', 'cas', 'M', 'hdg', 'swhdgsel', 'swaltsel', 'az', 'vs',
              'gsnorth', 'gseast', 'gs', 'trk', 'alt', 'lat', 'lon', 'coslat'):
        ok, msg = util.close(np.asarray(o[k], dtype=np.float64),
                             np.asarray(z['out_' + k], dtype=np.float64), 1.0, rtol=1e-12)
        assert ok, '%s: %s' % (k, msg)
