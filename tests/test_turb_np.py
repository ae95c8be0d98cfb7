"""CPU: the numpy restatement of the device turbulence (tests/turb_np.py) against its pins --
numpy's own Philox4x64-10 words, the reference's Turbulence.Woosh -- and the statistics of
its stream at the seed the GPU test uses."""
import os

import numpy as np
import pytest

from tests import turb_np
from tests.util import GOLDEN

STAT_N, STAT_SEED, STAT_CALL, STAT_DT = 4096, 0, 0, 0.05
STAT_SD = (1.0, 2.0, 0.5)


def stat_check(z, sd=STAT_SD, dt=STAT_DT):
    """The issue's bounds on the three scaled components of one call; returns the figures."""
    n = len(z)
    out = []
    for k in range(3):
        s = sd[k] * np.sqrt(dt)
        x = s * z[:, k]
        mean, ratio = x.mean(), x.var() / (s * s)
        out.append((mean, ratio))
        assert abs(mean) < 5 * s / np.sqrt(n), (k, mean)
        assert abs(ratio - 1.0) < 5 * np.sqrt(2.0 / n), (k, ratio)
    return out


def test_philox_matches_numpy_fixture():
    z = np.load(os.path.join(GOLDEN, 'philox_raw.npz'))
    ctr, key, raw = z['counter'], z['key'], z['raw']
    assert len(ctr) == 64
    assert any(int(c[0]) == 2 ** 64 - 1 for c in ctr)   # a carry into the second word
    for c, k, r in zip(ctr, key, raw):
        c1 = turb_np.numpy_counter(c)
        assert list(r[:4]) == list(turb_np.philox4x64_10(c1, k))
        assert list(r[4:]) == list(turb_np.philox4x64_10(turb_np.numpy_counter(c1), k))


def test_philox_matches_installed_numpy():
    """The same against the numpy at hand (the fixture pins the numpy of the capture)."""
    c, k = np.array([2 ** 64 - 1, 11, 0, 0], dtype=np.uint64), np.array([5, 0], dtype=np.uint64)
    r = np.random.Philox(counter=c, key=k).random_raw(4)
    assert list(r) == list(turb_np.philox4x64_10(turb_np.numpy_counter(c), k))


def test_known_answer():
    # Random123's kat_vectors: philox4x64 10 rounds, zero counter and key
    assert turb_np.philox4x64_10((0, 0, 0, 0), (0, 0)) == (0x16554d9eca36314c, 0xdb20fe9d672d0fdc,
                                                           0xd7e772cee186176b, 0x7e68b68aec7ba23b)


def test_uniforms_never_zero():
    w = np.array([[0, 2 ** 64 - 1, 2 ** 11 - 1, 2 ** 11]], dtype=np.uint64)
    u = turb_np.uniforms(w)[0]
    assert u[0] == 2.0 ** -54 and u[2] == u[0] and u[3] == 1.5 * 2.0 ** -53
    assert u[1] == 1.0   # above 2^52 the + 0.5 rounds to even: u lies in (0, 1], log(u) stays finite


@pytest.mark.parametrize('q', [0, 1])
def test_woosh_apply_matches_reference(q):
    z = np.load(os.path.join(GOLDEN, 'turb_woosh300.npz'))
    assert z['trk'][2] == 0.0 and abs(z['lat']).max() == 80.0
    lat, lon, alt = turb_np.woosh_apply(z['z%d' % q], float(z['dt']), z['sd%d' % q], z['trk'], z['coslat'],
                                        z['lat'], z['lon'], z['alt'])
    assert np.array_equal(lat, z['out_lat%d' % q])
    assert np.array_equal(lon, z['out_lon%d' % q])
    assert np.array_equal(alt, z['out_alt%d' % q])
    if q == 0:   # sd[0] = 0 clamps to 1e-6: the flight-direction draw still moves the aircraft
        assert not np.array_equal(lat[2], z['lat'][2])


def test_stream_statistics():
    stat_check(turb_np.draws(STAT_N, STAT_SEED, STAT_CALL))


def test_draws_are_keyed_by_seed_call_index():
    a = turb_np.raw_words(70, seed=3, call=5)
    assert np.array_equal(a[10:20], turb_np.raw_words(10, seed=3, call=5, first_index=10))
    assert not np.array_equal(a, turb_np.raw_words(70, seed=4, call=5))
    assert not np.array_equal(a, turb_np.raw_words(70, seed=3, call=6))
