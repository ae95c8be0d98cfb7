"""CPU: tests/adsb_np.py against the reference's recorded ADS-B results (adsb_update.npz, adsb_flight64.npz),
a census of the update rule's sides in those fixtures, and the build-defined draws: their streams and statistics."""
import os

import numpy as np
import pytest

from tests import adsb_np, turb_np, util
from tests.test_turb_np import STAT_CALL, STAT_N, STAT_SEED, stat_check

NS = (1, 63, 64, 65, 257)


@pytest.fixture(scope='module')
def upd():
    return dict(np.load(os.path.join(util.GOLDEN, 'adsb_update.npz')))


@pytest.fixture(scope='module')
def flight():
    return dict(np.load(os.path.join(util.GOLDEN, 'adsb_flight64.npz')))


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        a[~np.isnan(a)].tobytes() == b[~np.isnan(b)].tobytes()


def case_of(g, name):
    """(traf, the arrays before, the arrays after, unit normals, trunctime, noise) of a recorded update."""
    return ({k: g['%s_traf_%s' % (name, k)] for k in adsb_np.FIELDS}, {k: g['%s_in_%s' % (name, k)] for k in adsb_np.ARRAYS},
            {k: g['%s_out_%s' % (name, k)] for k in adsb_np.ARRAYS}, g[name + '_z'], float(g[name + '_trunctime']),
            '_noise1_' in name)


def names_of(g, n):
    return [str(x) for x in g['names'] if str(x).startswith('n%d_' % n)]


@pytest.mark.parametrize('n', NS)
def test_restatement_equals_the_update_golden(upd, n):
    names = names_of(upd, n)
    assert len(names) == 4
    moved = 0
    for name in names:
        traf, st, exp, z, trunctime, noise = case_of(upd, name)
        got = adsb_np.update(st, traf, float(upd['time']), trunctime, noise, adsb_np.TRANSERROR, z)
        for k in adsb_np.ARRAYS:
            assert same(got[k], exp[k]), (name, k)
        moved += int(not same(exp['trk'], st['trk']))
        if noise and not same(exp['trk'], st['trk']):          # noise on: the position is not a copy
            up = adsb_np.due(st['lastupdate'], trunctime, float(upd['time']))
            ok = ~np.isnan(traf['lat'][up])
            assert not np.any(exp['lat'][up][ok] == traf['lat'][up][ok]) and same(exp['gs'][up], traf['gs'][up])
    assert moved == 4


def test_restatement_equals_zero_time_create_and_setnoise(upd):
    g = upd
    traf = {k: g['zero_traf_' + k] for k in adsb_np.FIELDS}
    st = {k: g['zero_in_' + k] for k in adsb_np.ARRAYS}
    assert not st['lastupdate'].any()
    got = adsb_np.update(st, traf, 0.0, 0, True, adsb_np.TRANSERROR, g['zero_z'])     # time 0: nobody updates
    assert all(same(got[k], st[k]) for k in adsb_np.ARRAYS)
    traf = {k: g['create_traf_' + k] for k in adsb_np.FIELDS}
    st = {k: g['create_in_' + k] for k in adsb_np.ARRAYS}
    got = adsb_np.create(st, traf, 3, float(g['create_trunctime']), g['create_u'])
    for k in adsb_np.ARRAYS:
        assert same(got[k], g['create_out_' + k]), k
        assert same(got[k][:-3], st[k])
    assert not got['vs'][-3:].any() and same(got['gs'][-3:], traf['gs'][-3:])
    assert np.all((got['lastupdate'][-3:] < 0) & (got['lastupdate'][-3:] > -5.0))
    for row, flag in zip(g['setnoise'], (True, False)):
        tn, tr, te, tt = adsb_np.set_noise(flag)
        assert list(row) == [float(tn), float(tr), te[0], te[1], float(tt)]


@pytest.mark.parametrize('mode', ['off', 'on'])
def test_restatement_equals_the_flight_golden(flight, mode):
    g = flight
    st = {k: g['init_' + k] for k in adsb_np.ARRAYS}
    assert len(st['lat']) == 64 and int(g['ncalls']) == 40 and len(np.unique(st['lastupdate'])) == 64
    simt = 0.0
    for c in range(int(g['ncalls'])):
        assert simt == g['t'][c]
        traf = {k: g['traf_' + k][c] for k in adsb_np.FIELDS}
        assert len(adsb_np.due(st['lastupdate'], float(g['trunctime']), simt)) == g['ndue'][c]
        st = adsb_np.update(st, traf, simt, float(g['trunctime']), mode == 'on', g['transerror'],
                            g['on_z'][c] if mode == 'on' else None)
        for k in adsb_np.ARRAYS:
            assert same(st[k], g['%s_hist_%s' % (mode, k)][c]), (c, k)
        simt += float(g['simdt'])
    assert g['ndue'][1:].min() > 0 and g['ndue'].max() < 64
    # lastupdate advances by whole periods only: never set to the time
    periods = (st['lastupdate'] - g['init_lastupdate']) / 5.0
    assert np.all(np.abs(periods - np.round(periods)) < 1e-12) and set(np.round(periods)) == {7.0, 8.0}


def test_census_of_the_update_rule(upd, flight):
    """From the fixtures alone: every side of ``lastupdate + trunctime < time`` is taken, and a row that was on a
    side did what that side says."""
    t = float(upd['time'])
    sides = dict(on=0, below=0, above=0, nan=0, before=0, after=0)
    for name in [str(x) for x in upd['names']]:
        traf, st, exp, z, trunctime, noise = case_of(upd, name)
        with np.errstate(invalid='ignore'):
            s = st['lastupdate'] + trunctime
            updated = ~(exp['lastupdate'] == st['lastupdate']) & ~np.isnan(st['lastupdate']) if trunctime else \
                ~np.array([same(a, b) for a, b in zip(exp['trk'], st['trk'])])
        which = dict(on=s == t, below=s == np.nextafter(t, -np.inf), above=s == np.nextafter(t, np.inf), nan=np.isnan(s),
                     before=s < t - 1.0, after=s > t + 1.0)
        for k, m in which.items():
            sides[k] += int(m.sum())
            assert np.all(updated[m] == (k in ('below', 'before'))), (name, k)
        if trunctime:                                          # an updated row advances by exactly one period
            assert same(exp['lastupdate'][updated], st['lastupdate'][updated] + trunctime)
            behind = s < t - trunctime
            assert (behind.any() or len(s) < 63) and np.all(exp['lastupdate'][behind] + trunctime < t)
    assert all(v > 0 for v in sides.values()), sides
    assert flight['ndue'][0] == 0 and not flight['t'][0]       # time 0 with negative lastupdate + 5 > 0: nobody


def test_streams_differ():
    for seed, call, index in [(0, 0, 0), (7, 3, 100), (2 ** 64 - 1, 2 ** 40, 2 ** 33)]:
        s0 = turb_np.raw_words(1, seed, call, index)[0]
        s1 = adsb_np.raw_words(1, seed, call, index, adsb_np.STREAM_UPDATE)[0]
        s2 = adsb_np.raw_words(1, seed, call, index, adsb_np.STREAM_CREATE)[0]
        assert list(s0) == list(turb_np.philox4x64_10((index, call, 0, 0), (seed, 0)))
        assert list(s1) == list(turb_np.philox4x64_10((index, call, 1, 0), (seed, 0)))
        assert not set(s0) & set(s1) and not set(s0) & set(s2) and not set(s1) & set(s2)
    u = adsb_np.create_uniforms(70, seed=3, call=5)
    assert np.all((u > 0) & (u <= 1)) and len(np.unique(u)) == 70
    assert np.array_equal(u[10:20], adsb_np.create_uniforms(10, seed=3, call=5, first_index=10))


def test_stream_statistics():
    print('mean, variance ratio per component:', stat_check(adsb_np.draws(STAT_N, STAT_SEED, STAT_CALL)))
