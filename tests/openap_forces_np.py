"""numpy restatement of the drag / thrust / fuel-flow half of ``OpenAP.update``
(bluesky/traffic/performance/openap/perfoap.py:133-173, thrust.py:5-129,
aero.py:62-154), expression by expression in the reference's operation order.

TEST INFRASTRUCTURE ONLY: the expected values of the device kernels
(bsa_openap_forces, the resident step's k_sim_forces).  tools/make_golden.py
asserts it bitwise equal to the reference's own code when it captures
tests/golden/perf_forces3000.npz.
"""
import numpy as np

NA, TO, IC, CL, CR, DE, AP, LD, GD = range(9)   # phase.py:4-12
LIFT_FIXWING = 1                                # coeff.py:9
FT = 0.3048
FPM = FT / 60.
P0 = 101325.
RHO0 = 1.225
RGAS = 287.05287
GAMMA = 1.40
TSTRAT = 216.65
G0 = 9.80665
OUTPUTS = ('cd0', 'drag', 'thrustratio', 'thrust', 'fuelflow', 'bank')
# force-table columns (bluesky_amd.perf.force_table / bsa_sim_set_forces)
COLS = ('Sref', 'engnum', 'engthrust', 'engbpr', 'ff_a', 'ff_b', 'ff_c', 'cd0_clean', 'cd0_gd', 'cd0_to',
        'cd0_ic', 'cd0_ap', 'cd0_ld', 'k', 'mass')


def vatmos(h):
    T = np.maximum(288.15 - 0.0065 * h, TSTRAT)
    rhotrop = 1.225 * (T / 288.15)**4.256848030018761
    dhstrat = np.maximum(0., h - 11000.)
    rho = rhotrop * np.exp(-dhstrat / 6341.552161)
    p = rho * RGAS * T
    return p, rho, T


def vtas2mach(tas, h):
    T = np.maximum(288.15 - 0.0065 * h, TSTRAT)
    return tas / np.sqrt(GAMMA * RGAS * T)


def vtas2cas(tas, h):
    p, rho, _ = vatmos(h)
    qdyn = p * ((1. + rho * tas * tas / (7. * p))**3.5 - 1.)
    cas = np.sqrt(7. * P0 / RHO0 * ((qdyn / P0 + 1.)**(2. / 7.) - 1.))
    return np.where(tas < 0, -1 * cas, cas)


def vmach2cas(M, h):
    T = np.maximum(288.15 - 0.0065 * h, TSTRAT)
    return vtas2cas(M * np.sqrt(GAMMA * RGAS * T), h)


def tr_takeoff(bpr, v, h):
    """thrust.tr_takepff (thrust.py:41-56)."""
    G = 0.0606 * bpr + 0.6337
    mach = vtas2mach(v, h)
    PP = vatmos(h)[0] / P0
    A = -0.4327 * PP**2 + 1.3855 * PP + 0.0472
    Z = 0.9106 * PP**3 - 1.7736 * PP**2 + 1.8697 * PP
    X = 0.1377 * PP**3 - 0.4374 * PP**2 + 1.3003 * PP
    return A - 0.377 * (1 + bpr) / np.sqrt((1 + 0.82 * bpr) * G) * Z * mach \
        + (0.23 + 0.19 * np.sqrt(bpr)) * X * mach**2


def dfunc(mratio):
    return np.where(
        mratio < 0.85, 0.73, np.where(
            mratio < 0.92, 0.73 + (0.69 - 0.73) / (0.92 - 0.85) * (mratio - 0.85), np.where(
                mratio < 1.08, 0.66 + (0.63 - 0.66) / (1.08 - 1.00) * (mratio - 1.00), np.where(
                    mratio < 1.15, 0.63 + (0.60 - 0.63) / (1.15 - 1.08) * (mratio - 1.08), 0.60))))


def nfunc(roc):
    return np.where(roc < 1500, 0.89, np.where(roc < 2500, 0.93, 0.97))


def mfunc(vratio, roc):
    m = np.where(vratio < 0.67, 0.4, np.where(vratio < 0.75, 0.39, np.where(vratio < 0.83, 0.38, np.where(
        vratio < 0.92, 0.37, 0.36))))
    return np.where(roc < 1500, m - 0.06, np.where(roc < 2500, m - 0.01, m))


MACH_REF = 0.8
D_BREAKS = (0.85, 0.92, 1.08, 1.15)     # of mach / MACH_REF
M_BREAKS = (0.67, 0.75, 0.83, 0.92)     # of vcas / vcas_ref


def inflight_ratios(v, h):
    """(mach / mach_ref, vcas / vcas_ref) as thrust.inflight forms them: the
    arguments of dfunc / mfunc, whose breakpoints are step discontinuities."""
    v = np.where(v < 10, 10, v)
    vcas_ref = vmach2cas(MACH_REF, 35000 * FT)
    return vtas2mach(v, h) / MACH_REF, vtas2cas(v, h) / vcas_ref


def inflight(v, h, vs, thr0):
    """thrust.inflight (thrust.py:59-129)."""
    roc = np.abs(np.asarray(vs / FPM))
    v = np.where(v < 10, 10, v)
    mach = vtas2mach(v, h)
    vcas = vtas2cas(v, h)
    p = vatmos(h)[0]
    p10 = vatmos(10000 * FT)[0]
    p35 = vatmos(35000 * FT)[0]
    F35 = (200 + 0.2 * thr0 / 4.448) * 4.448
    vcas_ref = vmach2cas(MACH_REF, 35000 * FT)
    d = dfunc(mach / MACH_REF)
    b = (mach / MACH_REF) ** (-0.11)
    ratio_seg3 = d * np.log(p / p35) + b
    a = (vcas / vcas_ref) ** (-0.1)
    n = nfunc(roc)
    ratio_seg2 = a * (p / p35) ** (-0.355 * (vcas / vcas_ref) + n)
    F10 = F35 * a * (p10 / p35) ** (-0.355 * (vcas / vcas_ref) + n)
    m = mfunc(vcas / vcas_ref, roc)
    ratio_seg1 = m * (p / p35) + (F10 / F35 - m * (p10 / p35))
    ratio = np.where(h > 35000 * FT, ratio_seg3, np.where(h > 10000 * FT, ratio_seg2, ratio_seg1))
    return ratio * F35 / thr0


def thrust_ratio(phase, bpr, v, h, vs, thr0):
    """thrust.compute_thrust_ratio (thrust.py:5-39)."""
    ratio_takeoff = tr_takeoff(bpr, v, h)
    ratio_inflight = inflight(v, h, vs, thr0)
    ratio_idle = 0.15 * ratio_inflight
    tr = np.zeros(len(phase))
    tr = np.where(phase == TO, ratio_takeoff, tr)
    tr = np.where((phase == IC) | (phase == CL) | (phase == CR), ratio_inflight, tr)
    tr = np.where(phase == DE, ratio_idle, tr)
    return tr


def forces(par, lifttype, phase, mass, tas, vs, alt, bank):
    """The six outputs of perfoap.py:133-173 for per-aircraft parameter arrays
    ``par`` (dict of COLS without mass), the given phase and the previous
    perf.bank.  Rotors / other lift types keep the zeros the reference leaves."""
    n = len(tas)
    fw = np.where(np.asarray(lifttype) == LIFT_FIXWING)[0]
    phase = np.asarray(phase)
    cd0 = np.zeros(n)
    for phs, col in ((TO, 'cd0_to'), (IC, 'cd0_ic'), (AP, 'cd0_ap'), (LD, 'cd0_ld'), (GD, 'cd0_gd'),
                     (CL, 'cd0_clean'), (CR, 'cd0_clean'), (DE, 'cd0_clean'), (NA, 'cd0_clean')):
        cd0[phase == phs] = par[col][phase == phs]
    drag = np.zeros(n)
    thrustratio = np.zeros(n)
    thrust = np.zeros(n)
    with np.errstate(all='ignore'):
        rho = vatmos(alt[fw])[1]
        vtas = tas[fw]
        rhovs = 0.5 * rho * vtas**2 * par['Sref'][fw]
        cl = mass[fw] * G0 / rhovs
        drag[fw] = rhovs * (cd0[fw] + par['k'][fw] * cl**2)
        engnum = np.asarray(par['engnum']).astype(int)
        thr0 = engnum[fw] * par['engthrust'][fw]
        thrustratio[fw] = thrust_ratio(phase[fw], par['engbpr'][fw], tas[fw], alt[fw], vs[fw], thr0)
        thrust[fw] = engnum[fw] * par['engthrust'][fw] * thrustratio[fw]
        fuelflow = engnum * (par['ff_a'] * thrustratio**2 + par['ff_b'] * thrustratio + par['ff_c'])
    bank = np.where((phase == TO) | (phase == LD), 15, bank)
    bank = np.where((phase == IC) | (phase == CR) | (phase == AP), 35, bank)
    return dict(cd0=cd0, drag=drag, thrustratio=thrustratio, thrust=thrust, fuelflow=fuelflow,
                bank=np.asarray(bank, dtype=np.float64))


def forces_table(ftable, table24, tidx, phase, mass, tas, vs, alt, bank):
    """``forces`` for a force table (ntypes x 16) + the 24-column type table
    (lift type in column 22) + a type index per aircraft, as the device takes
    them; ``phase`` None derives it as the step does (oracle/perf.py)."""
    from oracle import perf as operf
    row = np.asarray(ftable)[tidx]
    lift = np.asarray(table24)[tidx, 22].astype(int)
    if phase is None:
        phase = operf.phase(lift, tas, vs, alt)
    par = {c: row[:, k].copy() for k, c in enumerate(COLS[:-1])}
    # rotors / lift type 0: every force is 0 whatever their row holds
    for c in ('ff_a', 'ff_b', 'ff_c'):
        par[c] = np.where(lift == LIFT_FIXWING, par[c], 0.0)
    return forces(par, lift, phase, mass, tas, vs, alt, bank)


def near_breakpoint(tas, alt, rel=1e-9):
    """Rows whose mach / mach_ref or vcas / vcas_ref lies within ``rel``
    (relative) of a dfunc / mfunc breakpoint."""
    mr, vr = inflight_ratios(np.asarray(tas, dtype=np.float64), np.asarray(alt, dtype=np.float64))
    near = np.zeros(len(mr), bool)
    for b in D_BREAKS:
        near |= np.abs(mr - b) <= rel * b
    for b in M_BREAKS:
        near |= np.abs(vr - b) <= rel * b
    return near
