"""OpenAP flight-phase envelope for the resident step.

``OpenAP.update`` (bluesky/traffic/performance/openap/perfoap.py:115-131)
re-derives every aircraft's flight phase from tas / vs / alt each step
(phase.py:14-62) and looks its speed / vertical-speed / altitude /
acceleration envelope up per aircraft type and phase
(``__construct_limit_matrix``, perfoap.py:211-262); ``acceleration()``
(perfoap.py:271-280) is 2 m/s^2 on the ground, 0.5 otherwise.  On the device
(``bsa_sim_set_perf``) this runs inside K4' of every step: the host hands
over one row per aircraft type and a type index per aircraft, built here from
the reference's own coefficient object (``bs.traf.perf.coeff``,
coeff.py:23-131) and per-aircraft ``perf.actypes`` / ``perf.lifttype``.

Table row (``PERF_COLS`` doubles): vmin by phase NA..GD (9), vmax by phase
(9), vsmin, vsmax, hmax, axmax, lifttype, 0.

The second half of ``OpenAP.update`` (perfoap.py:133-173: drag, thrust ratio,
thrust, fuel flow, the model's bank limit) is a kernel of its own
(``bsa_openap_forces`` standalone, ``bsa_sim_set_forces`` in the resident
step, which also sums the fuel burnt per aircraft).  Its per-type parameters
are a second table, ``force_table``, over the same sorted types.
"""
import numpy as np

NA, TO, IC, CL, CR, DE, AP, LD, GD = range(9)   # phase.py:4-12
LIFT_FIXWING, LIFT_ROTOR = 1, 2                  # coeff.py:9-10
PERF_COLS = 24


def _fixwing_row(c):
    """perfoap.py:232-250: the speed limits of a fixed-wing type per phase."""
    vmin = [0.0, c['vminto'], c['vminic'], c['vminer'], c['vminer'], c['vminer'], c['vminap'], c['vminld'], 0.0]
    vmax = [c['vmaxer'], c['vmaxto'], c['vmaxic'], c['vmaxer'], c['vmaxer'], c['vmaxer'], c['vmaxap'],
            c['vmaxld'], c['vmaxer']]
    return vmin + vmax + [c['vsmin'], c['vsmax'], c['hmax'], c['axmax'], float(LIFT_FIXWING), 0.0]


def _rotor_row(c):
    """perfoap.py:254-261: rotor limits do not depend on the phase; axmax is
    never set for rotors (0)."""
    return [c['vmin']] * 9 + [c['vmax']] * 9 + [c['vsmin'], c['vsmax'], c['hmax'], 0.0, float(LIFT_ROTOR), 0.0]


def type_table(limits_fixwing, limits_rotor, actypes, lifttype):
    """(table float64 [ntypes, PERF_COLS], type index int32 [n]) for the
    aircraft types ``actypes`` (str per aircraft, as ``perf.actypes``) with
    lift types ``lifttype`` (``perf.lifttype``).  ``limits_*``: the
    reference's ``Coefficient.limits_fixwing`` / ``limits_rotor`` dicts.
    Aircraft with another lift type get a row of zeros with lifttype 0 (the
    reference's limit matrix leaves them 0, phase.get gives them NA)."""
    actypes = np.asarray(actypes).astype(str)
    lifttype = np.asarray(lifttype).astype(np.int64)
    keys = sorted(set(zip(actypes.tolist(), lifttype.tolist())))
    rows = []
    for mdl, lt in keys:
        if lt == LIFT_FIXWING:
            rows.append(_fixwing_row(limits_fixwing[mdl]))
        elif lt == LIFT_ROTOR:
            rows.append(_rotor_row(limits_rotor[mdl]))
        else:
            rows.append([0.0] * PERF_COLS)
    where = {k: i for i, k in enumerate(keys)}
    tidx = np.array([where[k] for k in zip(actypes.tolist(), lifttype.tolist())], dtype=np.int32)
    return np.array(rows, dtype=np.float64).reshape(len(keys), PERF_COLS), tidx


def from_openap(perf):
    """Table + type index straight from a reference ``OpenAP`` instance
    (``bs.traf.perf``)."""
    return type_table(perf.coeff.limits_fixwing, perf.coeff.limits_rotor, perf.actypes, perf.lifttype)


# ---- drag / thrust / fuel flow (perfoap.py:133-173; bsa_sim_set_forces, bsa_openap_forces)
FORCE_COLS = 16     # Sref engnum engthrust engbpr ff_a ff_b ff_c cd0_clean cd0_gd cd0_to cd0_ic cd0_ap cd0_ld k mass 0
_CD0 = ('cd0_clean', 'cd0_gd', 'cd0_to', 'cd0_ic', 'cd0_ap', 'cd0_ld')


def _fixwing_forces(coeff, mdl):
    """OpenAP.create's lookups for a fixed-wing type (perfoap.py:69-109): the
    first engine of the type, its ICAO fuel-flow fit (thrust.py:132-153), the
    drag polar with the 'NA' default, mass = (oew + mtow) / 2."""
    ac = coeff.acs_fixwing[mdl]
    es = ac['engines']
    if not es:
        raise ValueError('aircraft type %s has no engine (the reference falls back to A320)' % mdl)
    e = es[list(es.keys())[0]]
    a, b, c = np.polyfit([0, 0.07, 0.3, 0.85, 1.0], [0, e['ff_idl'], e['ff_app'], e['ff_co'], e['ff_to']], 2)
    dp = coeff.dragpolar_fixwing[mdl] if mdl in coeff.dragpolar_fixwing.keys() else coeff.dragpolar_fixwing['NA']
    return ([ac['wa'], float(int(ac['n_engines'])), e['thr'], e['bpr'], a, b, c] + [dp[k] for k in _CD0] +
            [dp['k'], 0.5 * (ac['oew'] + ac['mtow']), 0.0])


def _rotor_forces(coeff, mdl):
    """perfoap.py:57-61: a rotor gets its mass and engine count, nothing else."""
    ac = coeff.acs_rotor[mdl]
    row = [0.0] * FORCE_COLS
    row[1] = float(int(ac['n_engines']))
    row[14] = 0.5 * (ac['oew'] + ac['mtow'])
    return row


def force_table(coeff, actypes, lifttype):
    """(ftable float64 [ntypes, FORCE_COLS], mass float64 [n]): the per-type
    parameters of OpenAP's drag / thrust / fuel-flow model from the reference's
    ``Coefficient`` object (``acs_fixwing`` / ``acs_rotor`` / ``dragpolar_fixwing``),
    as ``OpenAP.create`` looks them up, and every aircraft's default mass.
    Types are sorted exactly as ``type_table`` sorts them: its type index
    serves both tables."""
    actypes = np.asarray(actypes).astype(str)
    lifttype = np.asarray(lifttype).astype(np.int64)
    keys = sorted(set(zip(actypes.tolist(), lifttype.tolist())))
    rows = []
    for mdl, lt in keys:
        if lt == LIFT_FIXWING:
            rows.append(_fixwing_forces(coeff, mdl))
        elif lt == LIFT_ROTOR:
            rows.append(_rotor_forces(coeff, mdl))
        else:
            rows.append([0.0] * FORCE_COLS)
    where = {k: i for i, k in enumerate(keys)}
    tidx = np.array([where[k] for k in zip(actypes.tolist(), lifttype.tolist())], dtype=np.int64)
    ftable = np.array(rows, dtype=np.float64).reshape(len(keys), FORCE_COLS)
    return ftable, ftable[tidx, 14].copy()


def forces_from_openap(perf):
    """Force table + the live per-aircraft mass of a reference ``OpenAP``
    instance (``bs.traf.perf``)."""
    ftable, _ = force_table(perf.coeff, perf.actypes, perf.lifttype)
    return ftable, np.array(perf.mass, dtype=np.float64)


def forces(table, ftable, type_idx, mass, tas, vs, alt, phase=None, bank=None, ctx=None):
    """Drag / thrust / fuel flow of ``OpenAP.update`` (perfoap.py:133-173) on the
    device (bsa_openap_forces): dict of cd0, drag, thrustratio, thrust,
    fuelflow, bank.  ``phase`` (0..8) None: derived from vs / alt as the step
    does; ``bank``: the previous perf.bank (None: 0)."""
    from . import _lib
    ctx = ctx or _lib.default_context()
    return ctx.openap_forces(table, ftable, type_idx, mass, tas, vs, alt, phase, bank)
