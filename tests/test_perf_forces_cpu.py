"""CPU: OpenAP drag / thrust / fuel flow (perfoap.py:133-173, thrust.py) -- the
numpy restatement (tests/openap_forces_np.py) and the host-side force table
(bluesky_amd.perf.force_table) against tests/golden/perf_forces3000.npz,
captured from the reference's own code on its own coefficient tables
(tools/make_golden.py run_forces)."""
import types

import numpy as np
import pytest

from bluesky_amd import perf
from tests import openap_forces_np as fnp
from tests import util

ENGINE_FIELDS = ('thr', 'bpr', 'ff_idl', 'ff_app', 'ff_co', 'ff_to')
POLAR_FIELDS = ('cd0_clean', 'cd0_gd', 'cd0_to', 'cd0_ic', 'cd0_ap', 'cd0_ld', 'k')


def load():
    """(golden dict, a stand-in for the reference's Coefficient object rebuilt
    from the raw table entries in the file)."""
    g = dict(np.load(util.golden('perf_forces3000.npz')[0]))
    acs, polar = {}, {}
    for k, m in enumerate(g['fw_types']):
        m = str(m)
        eng = {f: float(g['eng_' + f][k]) for f in ENGINE_FIELDS}
        acs[m] = dict(wa=float(g['ac_wa'][k]), oew=float(g['ac_oew'][k]), mtow=float(g['ac_mtow'][k]),
                      n_engines=g['ac_n_engines'][k].item(), engines={'first': eng, 'second': dict(eng, thr=1.0)})
        # a type without a drag polar of its own takes the 'NA' entry
        polar['NA' if not g['dp_known'][k] else m] = {f: float(g['dp_' + f][k]) for f in POLAR_FIELDS}
    polar.setdefault('NA', {f: 0.0 for f in POLAR_FIELDS})
    rot = {str(m): dict(oew=float(g['rot_mass'][k]), mtow=float(g['rot_mass'][k]),
                        n_engines=int(g['rot_engnum'][k])) for k, m in enumerate(g['rot_types'])}
    coeff = types.SimpleNamespace(acs_fixwing=acs, acs_rotor=rot, dragpolar_fixwing=polar)
    return g, coeff


def params(g):
    """Per-aircraft parameter arrays from the golden's per-type ones."""
    where = {str(m): k for k, m in enumerate(g['fw_types'])}
    fw = g['lifttype'] == perf.LIFT_FIXWING
    row = np.array([where.get(str(m), 0) for m in g['actypes']])
    par = {c: np.where(fw, g['par_' + c][row], 0.0) for c in fnp.COLS[:-1]}
    rmap = {str(m): int(g['rot_engnum'][k]) for k, m in enumerate(g['rot_types'])}
    par['engnum'] = np.where(fw, par['engnum'], [rmap.get(str(m), 0) for m in g['actypes']])
    return par


def test_helper_reproduces_reference_bitwise():
    g, _ = load()
    got = fnp.forces(params(g), g['lifttype'], g['phase'], g['mass'], g['tas'], g['vs'], g['alt'], g['bank0'])
    for o in fnp.OUTPUTS:
        assert np.array_equal(got[o], g['out_' + o], equal_nan=True), o


def test_golden_covers_the_edges():
    g, _ = load()
    fw = g['lifttype'] == perf.LIFT_FIXWING
    assert set(np.unique(g['phase'][fw]).astype(int)) == set(range(9))
    assert (~fw).sum() > 0 and not g['out_fuelflow'][~fw].any() and not g['out_drag'][~fw].any()
    for v in (0.0, 5.0, 10.0):
        assert (g['tas'][fw] == v).any()
    for a in (10000 * fnp.FT, 35000 * fnp.FT):
        assert (g['alt'][fw] == a).any() and (g['alt'][fw] == np.nextafter(a, np.inf)).any()
    for r in (1500., 2500.):
        assert (np.abs(g['vs'][fw]) == r * fnp.FPM).any()
    assert np.isnan(g['out_drag'][fw & (g['tas'] == 0.0)]).all()      # the tas == 0 quirk
    # breakpoint rows a test may skip: at most 0.1 % (none at capture)
    assert g['near_break'].sum() <= 0.001 * len(g['tas'])
    assert np.array_equal(g['near_break'], fnp.near_breakpoint(g['tas'], g['alt']) & fw)


def test_force_table_reproduces_reference_parameters():
    g, coeff = load()
    ftable, mass = perf.force_table(coeff, g['actypes'], g['lifttype'])
    table24, tidx = perf.type_table({str(m): dict.fromkeys(
        ('vminto', 'vmaxto', 'vminic', 'vmaxic', 'vminer', 'vmaxer', 'vminap', 'vmaxap', 'vminld', 'vmaxld',
         'vsmin', 'vsmax', 'hmax', 'axmax'), 0.0) for m in g['fw_types']},
        {str(m): dict.fromkeys(('vmin', 'vmax', 'vsmin', 'vsmax', 'hmax'), 0.0) for m in g['rot_types']},
        g['actypes'], g['lifttype'])
    assert ftable.shape == (len(table24), perf.FORCE_COLS) and mass.dtype == np.float64
    par = params(g)
    row = ftable[tidx]          # one type index serves both tables
    assert np.array_equal(table24[tidx, 22], g['lifttype'].astype(float))
    for k, c in enumerate(fnp.COLS[:-1]):
        if c in ('ff_a', 'ff_b', 'ff_c'):     # np.polyfit: LAPACK may differ by ulps across machines
            ok, msg = util.close(row[:, k], par[c], np.abs(par[c]).max())
            assert ok, '%s: %s' % (c, msg)
        else:
            assert np.array_equal(row[:, k], par[c]), c
    assert not row[:, 15].any()
    # default mass (oew + mtow) / 2; the golden's mass is that times a per-aircraft factor
    ratio = g['mass'] / mass
    assert np.isin(np.round(ratio, 12), [1.0, 0.8, 1.15]).all()
    assert np.array_equal(row[:, 14], mass)
    # ... and through the table the helper still gives the reference's outputs
    got = fnp.forces_table(ftable, table24, tidx, g['phase'], g['mass'], g['tas'], g['vs'], g['alt'], g['bank0'])
    for o in fnp.OUTPUTS:
        ok, msg = util.close(got[o], g['out_' + o], np.nanmax(np.abs(g['out_' + o])))
        assert ok, '%s: %s' % (o, msg)


def test_force_table_first_engine_and_na_polar():
    g, coeff = load()
    m = str(g['fw_types'][0])
    ft, _ = perf.force_table(coeff, [m], [perf.LIFT_FIXWING])
    assert ft[0, 2] == coeff.acs_fixwing[m]['engines']['first']['thr']       # not the second engine's 1.0
    unknown = [str(t) for k, t in enumerate(g['fw_types']) if not g['dp_known'][k]]
    for t in unknown:
        ft, _ = perf.force_table(coeff, [t], [perf.LIFT_FIXWING])
        assert ft[0, 7] == coeff.dragpolar_fixwing['NA']['cd0_clean']
    ft, mass = perf.force_table(coeff, ['XXXX', 'XXXX'], [0, 0])              # another lift type: zeros
    assert ft.shape == (1, perf.FORCE_COLS) and not ft.any() and mass.tolist() == [0.0, 0.0]


def test_bad_tables_raise():
    g, coeff = load()
    with pytest.raises(KeyError):
        perf.force_table(coeff, ['NOPE'], [perf.LIFT_FIXWING])               # unknown type
    m = str(g['fw_types'][0])
    coeff.acs_fixwing[m]['engines'] = {}
    with pytest.raises(ValueError):
        perf.force_table(coeff, [m], [perf.LIFT_FIXWING])                    # a type without an engine
    from bluesky_amd import _lib
    with pytest.raises(ValueError):
        _lib.Context._force_table(np.zeros((3, 15)))                         # not ntypes x 16
    with pytest.raises(ValueError):
        _lib.Context._force_table(np.zeros(16))
