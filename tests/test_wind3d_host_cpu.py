"""CPU: the opt-in 3-D wind path of bluesky_amd.kinematics on a fake context
(what is handed to the library, and when), and the bindings of its two calls."""
import ctypes
import types

import numpy as np
import pytest

from bluesky_amd import _lib, kinematics, resident


class FakeCtx:
    def __init__(self):
        self.uploads, self.calls = [], []

    def set_windfield3d(self, lat, lon, vnorth, veast, altstep):
        self.uploads.append((lat, lon, vnorth, veast, altstep))

    def kinematics(self, simdt, state, inputs, winddim, vn, ve):
        self.calls.append((winddim, vn, ve))
        z = np.zeros(2)
        return dict(ax=z, delspd=z, cas=z, mach=z, gsnorth=z, gseast=z, gs=z, trk=z, coslat=z, az=z,
                    swhdgsel=z, swaltsel=z)


def make_traf():
    w = types.SimpleNamespace(winddim=3, altstep=30.48, lat=np.array([1.0, 2.0, 3.0]), lon=np.array([4.0, 5.0, 6.0]),
                              vnorth=np.arange(451 * 3, dtype=float).reshape(451, 3),
                              veast=-np.arange(451 * 3, dtype=float).reshape(451, 3))
    z = np.zeros(2)
    return types.SimpleNamespace(wind=w, tas=z, hdg=z, alt=z, vs=z, lat=z, lon=z, bank=z, eps=z,
                                 pilot=types.SimpleNamespace(tas=z, hdg=z, alt=z, vs=z),
                                 perf=types.SimpleNamespace(acceleration=lambda: z))


def test_opt_in_hands_over_the_full_tables():
    c, traf = FakeCtx(), make_traf()
    kinematics.step(traf, 0.05, c, wind3d=True)
    assert c.calls == [(3, 0.0, 0.0)]
    (lat, lon, vn, ve, altstep), = c.uploads
    w = traf.wind
    assert lat is w.lat and lon is w.lon and vn is w.vnorth and ve is w.veast
    assert vn.shape == (451, 3) and altstep == 30.48


def test_default_still_raises():
    with pytest.raises(ValueError, match='windfield.py:177'):
        kinematics.step(make_traf(), 0.05, FakeCtx())


def test_uploads_again_only_after_a_rebind():
    c, traf = FakeCtx(), make_traf()
    for _ in range(3):
        kinematics.step(traf, 0.05, c, wind3d=True)
    assert len(c.uploads) == 1 and len(c.calls) == 3
    traf.wind.vnorth = traf.wind.vnorth.copy()            # addpoint / remove / clear rebind the arrays
    kinematics.step(traf, 0.05, c, wind3d=True)
    kinematics.step(traf, 0.05, c, wind3d=True)
    assert len(c.uploads) == 2 and c.uploads[1][2] is traf.wind.vnorth
    traf.wind.lat = np.append(traf.wind.lat[:2], 9.0)
    kinematics.step(traf, 0.05, c, wind3d=True)
    assert len(c.uploads) == 3
    traf.wind.veast[7, 1] = 99.0                          # an edit in place is not seen ...
    kinematics.step(traf, 0.05, c, wind3d=True)
    assert len(c.uploads) == 3
    kinematics.reload_wind3d(c)                           # ... until the upload is forced
    kinematics.step(traf, 0.05, c, wind3d=True)
    assert len(c.uploads) == 4
    other = FakeCtx()                                     # the record is per context
    kinematics.step(traf, 0.05, other, wind3d=True)
    assert len(other.uploads) == 1


def test_install_passes_the_opt_in_on():
    c, traf = FakeCtx(), make_traf()
    kinematics.install(traf, c, wind3d=True)
    traf.UpdateAirSpeed(0.05, 0.0)
    assert c.calls == [(3, 0.0, 0.0)] and len(c.uploads) == 1
    with pytest.raises(ValueError, match='windfield.py:177'):
        kinematics.install(make_traf(), FakeCtx()).UpdateAirSpeed(0.05, 0.0)


def test_params_select_winddim_3():
    assert resident.params(windfield3d=True).winddim == 3
    assert resident.params(windfield=True).winddim == 2 and resident.params().winddim == 0


def test_bindings_of_the_two_calls():
    dp, i64 = ctypes.POINTER(ctypes.c_double), ctypes.c_int64
    assert _lib.ABI_VERSION == 2
    assert _lib.SIGNATURES['bsa_set_windfield3d'] == (ctypes.c_int, [ctypes.c_void_p, i64, i64, ctypes.c_double,
                                                                     dp, dp, dp, dp])
    assert _lib.SIGNATURES['bsa_wind_getdata'] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, i64,
                                                                  dp, dp, dp, dp, dp])


def test_context_checks_the_table_shape():
    c = _lib.Context.__new__(_lib.Context)    # no device: the shape is checked before the library is called
    with pytest.raises(ValueError, match='nalt, nvec'):
        c.set_windfield3d(np.zeros(3), np.zeros(3), np.zeros((451, 2)), np.zeros((451, 2)), 30.48)
    with pytest.raises(ValueError, match='altstep'):
        c.set_windfield3d(np.zeros(3), np.zeros(3), np.zeros((451, 3)), np.zeros((451, 3)))
