"""CPU: a census of the committed kinematics / MVP fixtures.

kin::step (bsa_kin_math.h) and the MVP pair / row code (bsa_mvp_math.h,
bsa_mvp_row.h) are chains of strict comparisons, numpy-style sign / maximum /
remainder and where(isfinite).  Random traffic never lands on a threshold, so
the hand-made rows of kin_edge_*.npz and mvp_synth.npz (tools/make_golden.py)
put a row on each one and one nextafter beyond it.  Here every side of every
such comparison is recounted with numpy from the fixtures alone and must be
taken by at least one row (pair) across kin_*.npz (mvp_*.npz): regenerating
the fixtures cannot lose an edge unnoticed.  A count, not a tolerance."""
import numpy as np
import pytest

from oracle import kinematics as okin
from tests import util

KIN = util.golden('kin_*.npz')
MVP = util.golden('mvp_*.npz')

KIN_INPUTS = util.KIN_INPUTS


def up(x):
    return np.nextafter(x, np.inf)


def dn(x):
    return np.nextafter(x, -np.inf)


def threshold_sides(c, name, delta, thr, where=True):
    """|delta| > thr: on the threshold and one nextafter beyond, for both signs of
    delta, and clearly on either side."""
    a = np.abs(delta)
    for sgn, m in (('+', delta > 0), ('-', delta < 0)):
        c['%s: %s on the threshold' % (name, sgn)] = np.sum(where & m & (a == thr))
        c['%s: %s one ulp beyond' % (name, sgn)] = np.sum(where & m & (a == up(thr)))
        c['%s: %s beyond' % (name, sgn)] = np.sum(where & m & (a > up(thr)))
        c['%s: %s inside' % (name, sgn)] = np.sum(where & m & (a < thr))


def kin_census(z):
    """name -> number of rows of one kin_*.npz that take that side (UpdateAirSpeed /
    UpdateGroundSpeed / UpdatePosition, traffic.py:425-483, recomputed from the inputs)."""
    c = {}
    dt, wd = float(z['dt']), int(z['winddim'])
    s = {k: z[k] for k in KIN_INPUTS}
    with np.errstate(all='ignore'):
        dspd = s['ptas'] - s['tas']
        threshold_sides(c, '|delta_spd| > kts', dspd, okin.kts)
        need_ax = np.abs(dspd) > okin.kts
        ax = need_ax * np.sign(dspd) * s['accel']
        tas = s['tas'] + ax * dt
        c['tas < 0'] = np.sum(tas < 0)
        c['0 < tas < eps'] = np.sum((tas > 0) & (tas < s['eps']))
        c['tas == eps'] = np.sum(tas == s['eps'])
        c['tas == 0 and eps == 0'] = np.sum((tas == 0) & (s['eps'] == 0))
        c['tas subnormal'] = np.sum((tas != 0) & (np.abs(tas) < np.finfo(np.float64).tiny))
        c['bank == 0'] = np.sum(s['bank'] == 0)
        c['ax == -0.0'] = np.sum((ax == 0) & np.signbit(ax))
        # heading
        h = s['hdg']
        c['|hdg| >= 360 2^30 (fmod)'] = np.sum(np.isfinite(h) & (np.abs(h) >= 360.0 * 2 ** 30))
        c['360 <= |hdg| < 360 2^30 (fmod360)'] = np.sum((np.abs(h) >= 360.0) & (np.abs(h) < 360.0 * 2 ** 30))
        c['hdg < 0'] = np.sum(h < 0)
        c['hdg == -0.0'] = np.sum((h == 0) & np.signbit(h))
        c['hdg == 360'] = np.sum(h == 360.0)
        c['phdg == 360'] = np.sum(s['phdg'] == 360.0)
        delhdg = (s['phdg'] - h + 180) % 360 - 180
        c['delhdg == -180'] = np.sum(delhdg == -180.0)
        c['delhdg == 0'] = np.sum(delhdg == 0)
        c['delhdg > 0'] = np.sum(delhdg > 0)
        c['delhdg < 0'] = np.sum(delhdg < 0)
        turnrate = np.degrees(okin.g0 * np.tan(s['bank']) / np.maximum(tas, s['eps']))
        c['turn rate infinite'] = np.sum(np.isinf(turnrate))
        swhdg = np.abs(delhdg) > np.abs(2 * dt * turnrate)
        c['swhdgsel'], c['not swhdgsel'] = np.sum(swhdg), np.sum(~swhdg & np.isfinite(delhdg))
        c['the turn wraps past north'] = np.sum(swhdg & (np.abs(z['out_hdg'] - h % 360.0) > 180.0))
        # vertical
        dalt = s['palt'] - s['alt']
        t10, tvs = 10 * okin.ft, np.abs(2 * dt * np.abs(s['vs']))
        threshold_sides(c, '|delta_alt| > 10 ft', dalt, t10, tvs <= t10)
        threshold_sides(c, '|delta_alt| > |2 dt |vs||', dalt, tvs, tvs > t10)
        swalt = np.abs(dalt) > np.maximum(t10, tvs)
        target_vs = swalt * np.sign(dalt) * np.abs(s['pvs'])
        dvs = target_vs - s['vs']
        threshold_sides(c, '|delta_vs| > 300 fpm', dvs, 300 * okin.fpm)
        need_az = np.abs(dvs) > 300 * okin.fpm
        az = need_az * np.sign(dvs) * (300 * okin.fpm)
        vs = np.where(need_az, s['vs'] + az * dt, target_vs)
        c['vs not finite -> 0'] = np.sum(~np.isfinite(vs))
        c['vs not finite -> 0, from an infinite pvs'] = np.sum(~np.isfinite(vs) & np.isinf(s['pvs']))
        c['az == -0.0'] = np.sum((az == 0) & np.signbit(az))
        c['vs == -0.0'] = np.sum((vs == 0) & np.signbit(vs))
        # altitude: the wind gate (per winddim) and vatmos' tropopause
        alt = s['alt']
        if wd in (1, 2):
            g = 50. * okin.ft
            for name, m in (('alt == 50 ft', alt == g), ('alt == next(50 ft)', alt == up(g)), ('alt == 0', alt == 0),
                            ('alt < 0', alt < 0), ('alt > 50 ft', alt > up(g)), ('alt NaN', np.isnan(alt))):
                c['wind gate, winddim %d: %s' % (wd, name)] = np.sum(m)
        for name, m in (('== 11000', alt == 11000.), ('== prev(11000)', alt == dn(11000.)),
                        ('== next(11000)', alt == up(11000.)), ('> 11000', alt > up(11000.)),
                        ('< 11000', alt < dn(11000.))):
            c['vatmos: alt %s' % name] = np.sum(m)
        # position
        lat, lon = s['lat'], s['lon']
        c['lat == 90'], c['lat == -90'] = np.sum(lat == 90.0), np.sum(lat == -90.0)
        c['lat == next(90)'] = np.sum(lat == up(90.0))
        c['80 < |lat| < 90'] = np.sum((np.abs(lat) > 80.0) & (np.abs(lat) < 90.0))
        c['the step crosses the pole'] = np.sum((np.abs(lat) <= 90.0) & (np.abs(z['out_lat']) > 90.0))
        c['out_lon > 180'] = np.sum(np.isfinite(z['out_lon']) & (lon < 180.0) & (z['out_lon'] > 180.0))
        c['out_lon < -180'] = np.sum(np.isfinite(z['out_lon']) & (lon >= -180.0) & (z['out_lon'] < -180.0))
        if wd == 2:
            on = (lat[:, None] == z['wlat'][None, :]) & (lon[:, None] == z['wlon'][None, :])
            c['wind field: on a definition point'] = np.sum(on.any(axis=1))
            c['wind field: off the definition points'] = np.sum(~on.any(axis=1) & np.isfinite(lat + lon))
            c['wind field: lat NaN'] = np.sum(np.isnan(lat))
        # non-finite inputs, one kind per input
        for k in KIN_INPUTS:
            c['%s NaN' % k] = np.sum(np.isnan(s[k]))
            c['%s +inf' % k] = np.sum(s[k] == np.inf)
            c['%s -inf' % k] = np.sum(s[k] == -np.inf)
    return c


def total(censuses):
    out = {}
    for c in censuses:
        for k, v in c.items():
            out[k] = out.get(k, 0) + int(v)
    return out


def test_kin_fixtures_reach_every_side():
    files = [dict(np.load(p, allow_pickle=False)) for p in KIN]
    c = total(kin_census(z) for z in files)
    assert {int(z['winddim']) for z in files} >= {0, 1, 2}
    assert {float(z['dt']) for z in files} >= {0.0, 0.05, 1.0}
    missing = sorted(k for k, v in c.items() if v == 0)
    assert not missing, 'no row of kin_*.npz takes: %s' % missing
    assert len(c) > 120


def test_kin_census_counts_what_it_names():
    """The census on three hand-made rows, so that a side it names cannot be
    counted from the wrong rows."""
    base = dict(tas=200.0, hdg=45.0, alt=8000.0, vs=0.0, lat=52.0, lon=4.0, ptas=200.0, phdg=45.0, palt=8000.0,
                pvs=0.0, bank=0.4, eps=0.01, accel=0.5)
    rows = [dict(base), dict(base, tas=0.0, ptas=okin.kts), dict(base, tas=up(okin.kts), ptas=0.0),
            dict(base, alt=up(10 * okin.ft), palt=0.0, pvs=5.0)]
    s = {k: np.array([r[k] for r in rows]) for k in KIN_INPUTS}
    o = okin.step(s, 0.05)
    z = dict(s, dt=0.05, winddim=0, out_hdg=o['hdg'], out_lat=o['lat'], out_lon=o['lon'])
    c = kin_census(z)
    assert c['|delta_spd| > kts: + on the threshold'] == 1 and c['|delta_spd| > kts: - one ulp beyond'] == 1
    assert c['|delta_spd| > kts: - on the threshold'] == 0 and c['|delta_spd| > kts: + one ulp beyond'] == 0
    assert c['|delta_alt| > 10 ft: - one ulp beyond'] == 1 and c['|delta_alt| > 10 ft: + one ulp beyond'] == 0
    assert c['|delta_vs| > 300 fpm: - beyond'] == 1 and c['tas NaN'] == 0 and c['vatmos: alt < 11000'] == 4


def mvp_census(z):
    """name -> number of pairs / aircraft of one mvp_*.npz that take that side
    (MVP.MVP, MVP.py:149-231; prioRules, MVP.py:235-300; the finalize, MVP.py:67-143)."""
    c = {}
    ci, cj = z['ci'].astype(np.int64), z['cj'].astype(np.int64)
    mar = float(z['mar'])
    Rm, dhm, tla = float(z['rpz']) * mar, float(z['hpz']) * mar, float(z['tla'])
    vmin, vmax = 200.0 * 1852.0 / 3600., 500.0 * 1852.0 / 3600.
    n = len(z['alt'])
    with np.errstate(all='ignore'):
        qdr = np.radians(z['qdr'])
        dist, tcpa, tlos = z['dist'], z['tcpa'], z['tLOS']
        drel = np.array([np.sin(qdr) * dist, np.cos(qdr) * dist, z['alt'][cj] - z['alt'][ci]])
        vrel = np.array([z['gseast'][cj] - z['gseast'][ci], z['gsnorth'][cj] - z['gsnorth'][ci],
                         z['vs'][cj] - z['vs'][ci]])
        dcpa = drel + vrel * tcpa
        dabsH = np.sqrt(dcpa[0] * dcpa[0] + dcpa[1] * dcpa[1])
        c['dabsH < 10'], c['dabsH == 10'] = np.sum(dabsH < 10.), np.sum(dabsH == 10.)
        c['10 < dabsH <= 10 + 1e-9'] = np.sum((dabsH > 10.) & (dabsH <= 10. + 1e-9))
        c['dabsH > 10'] = np.sum(dabsH > 10. + 1e-9)
        dabsH = np.where(dabsH <= 10., 10., dabsH)
        c['erratum: Rm < dist and dabsH < dist'] = np.sum((Rm < dist) & (dabsH < dist))
        c['no erratum: Rm < dist and dabsH >= dist'] = np.sum((Rm < dist) & (dabsH >= dist))
        c['no erratum: Rm > dist'] = np.sum(Rm > dist)
        c['dist == Rm'], c['dist == next(Rm)'] = np.sum(dist == Rm), np.sum(dist == up(Rm))
        vz = np.abs(vrel[2]) > 0.0
        tsol = np.where(vz, np.abs(drel[2] / vrel[2]), tlos)
        c['tsolV == dtlookahead'], c['tsolV == next(dtlookahead)'] = np.sum(vz & (tsol == tla)), np.sum(vz & (tsol == up(tla)))
        c['tsolV > dtlookahead'], c['tsolV < dtlookahead'] = np.sum(vz & (tsol > up(tla))), np.sum(vz & (tsol < tla))
        c['vrel_z == 0 and |drel_z| > dhm'] = np.sum(~vz & (np.abs(drel[2]) > dhm))
        c['vrel_z == 0 and |drel_z| < dhm'] = np.sum(~vz & (np.abs(drel[2]) < dhm))
        takes_tlos = ~vz | (tsol > tla)
        c['tLOS NaN where tsolV takes it'] = np.sum(takes_tlos & np.isnan(tlos))
        c['tLOS inf where tsolV takes it'] = np.sum(takes_tlos & np.isinf(tlos))
        c['tLOS == 0 where tsolV takes it'] = np.sum(takes_tlos & (tlos == 0))
        c['tLOS inf with vrel_z == 0'], c['tLOS NaN with vrel_z == 0'] = np.sum(~vz & np.isinf(tlos)), np.sum(~vz & np.isnan(tlos))
        c['tcpa == +0.0'] = np.sum((tcpa == 0) & ~np.signbit(tcpa))
        c['tcpa == -0.0'] = np.sum((tcpa == 0) & np.signbit(tcpa))
        c['tcpa NaN'], c['tcpa +inf'], c['tcpa -inf'] = np.sum(np.isnan(tcpa)), np.sum(tcpa == np.inf), np.sum(tcpa == -np.inf)
        c['tcpa < 0'] = np.sum(tcpa < 0)
        # the priority rules' |vs| < 0.1 / > 0.1, ownship (vs1) and intruder (vs2)
        a1, a2 = np.abs(z['vs'][ci]), np.abs(z['vs'][cj])
        for name, a, b in (('vs1', a1, a2), ('vs2', a2, a1)):
            for v, lab in ((0.1, '== 0.1'), (dn(0.1), '== prev(0.1)'), (up(0.1), '== next(0.1)')):
                c['|%s| %s, the other climbing' % (name, lab)] = np.sum((a == v) & (b > 0.1))
                c['|%s| %s, the other level' % (name, lab)] = np.sum((a == v) & (b < 0.1))
        c1, c2 = (a1 < 0.1) & (a2 > 0.1), (a2 < 0.1) & (a1 > 0.1)
        c['c1: ownship level, intruder climbing'], c['c2: intruder level, ownship climbing'] = np.sum(c1), np.sum(c2)
        c['neither c1 nor c2'] = np.sum(~c1 & ~c2)
        c['a negative vs on 0.1'] = np.sum((z['vs'][ci] == -0.1) | (z['vs'][cj] == -0.1))
        # rows: mvp_fold takes 4 pairs a trip
        npairs = np.bincount(ci, minlength=n)
        c['a row of 9 pairs'], c['a row of 13 pairs'] = np.sum(npairs == 9), np.sum(npairs == 13)
        for r in range(4):
            c['a row of more than 4 pairs, %d mod 4' % r] = np.sum((npairs > 4) & (npairs % 4 == r))
        c['a row of more than 8 pairs'], c['a row of more than 12 pairs'] = np.sum(npairs > 8), np.sum(npairs > 12)
        c['a row without pairs'] = np.sum(npairs == 0)
        assert np.all(np.diff(ci) >= 0), 'pairs are not row-major'
        c['resooff ownship with pairs'] = np.sum(np.isin(ci, z['resooff_idx']))
        c['noreso intruder'] = np.sum(np.isin(cj, z['noreso_idx']))
        c['resooff ownship meets a noreso intruder'] = np.sum(np.isin(ci, z['resooff_idx']) & np.isin(cj, z['noreso_idx']))
        c['noreso aircraft as ownship'] = np.sum(np.isin(ci, z['noreso_idx']))
        # the finalize: a ground speed on the caps (no pairs: newgs = sqrt(v . v)), signdvs == 0
        newgs = np.sqrt(z['gseast'] ** 2 + z['gsnorth'] ** 2)
        free = npairs == 0
        for name, v in (('vmin', vmin), ('vmax', vmax)):
            c['new gs == %s' % name] = np.sum(free & (newgs == v) & (z['gs'] == v))
        c['new gs one ulp below vmin'] = np.sum(free & (newgs == dn(vmin)))
        c['new gs one ulp above vmax'] = np.sum(free & (newgs == up(vmax)))
        c['new gs capped at vmin'] = np.sum(z['default__tas'] == vmin)
        c['new gs capped at vmax'] = np.sum(z['default__tas'] == vmax)
        sdv = np.sign(z['default__vs'] - z['apvs'] * np.sign(z['selalt'] - z['alt']))
        c['signdvs == 0 on a row with pairs'] = np.sum((sdv == 0) & ~free)
        c['signdvs == 0 while climbing at ap.vs'] = np.sum((sdv == 0) & ~free & (z['vs'] != 0))
        c['signdvs != 0 on a row with pairs'] = np.sum((sdv != 0) & ~free)
        c['a non-finite resolution'] = np.sum(~np.isfinite(z['hv__vs']) | ~np.isfinite(z['hv__trk']))
    return c


def test_mvp_fixtures_reach_every_side():
    c = total(mvp_census(dict(np.load(p, allow_pickle=False))) for p in MVP)
    missing = sorted(k for k, v in c.items() if v == 0)
    assert not missing, 'no pair / aircraft of mvp_*.npz takes: %s' % missing
    assert len(c) > 55


@pytest.mark.parametrize('path', util.golden('kin_edge_*.npz') + util.golden('kinx_edge_*.npz'),
                         ids=util.case_name)
def test_edge_rows_are_named(path):
    """Every hand-made row carries the name of the edge it stands for."""
    z = np.load(path, allow_pickle=False)
    assert len(z['row_name']) == len(z['tas']) and len(set(z['row_name'].tolist())) == len(z['tas'])
