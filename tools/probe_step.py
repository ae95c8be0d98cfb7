"""Per-rank share of the WHOLE sharded step on one GPU:
the resident step of one rank of R -- its detect (own tiles, halo plan, halo
tiles: bsa_sim_detect_rows' one-GPU halo mode), K2, K3 and K4' on its home
rows -- with no collective (bsa_sim_probe_rank), timed as one batch of STEPS
steps (one host synchronisation at its end, no stage events) after SETTLE
untimed ones (the device at steady clocks, as bench.py's --settle).  Collectives
(box all-gather, halo send / recv, gate all-reduce) are excluded: they need
the 8-GPU node.  Prints every rank's ms per step and the slowest.
Usage: python tools/probe_step.py [WORKLOAD [R [STEPS [RANK [SETTLE]]]]] [--perf | --forces] [--fms]
[--resume-nav] [--recover] [--turb] [--cond] [--exparea] [--adsb | --adsb-shared | --adsb-nonoise]  (RANK:
that rank of R only, -1 all; SETTLE default 200; --perf: OpenAP phase / envelope in the step,
--forces: also its drag / thrust / fuel-flow launch; --fms: Autopilot.update in the
step, every aircraft on a generated 4-waypoint route; --resume-nav: ASAS.update's
bookkeeping and ResumeNav in the CD step; --recover: waypoint recovery after ResumeNav, DESIGN.md 3.23
-- implies --fms and --resume-nav, its cost is --recover against --fms --resume-nav; --turb: Turbulence.Woosh
as the step's last stage, DESIGN.md 3.25: k_sim_turb and the next detect's own K0b in place of K4''s records;
--cond: 10 000 conditional commands of both types that never fire, DESIGN.md 3.29: k_sim_cond every step;
--exparea: the experiment area on a box around all the traffic that nobody leaves, TAXI OFF far below, a pass
every step, DESIGN.md 3.30: k_sim_exparea every step; --adsb: the ADS-B model with trunctime 0, so that every aircraft
updates in every step, noise on with per-aircraft draws, DESIGN.md 3.32: k_adsb every step at its most expensive;
--adsb-shared: the same with the default shared draw, one one-lane launch in front of k_adsb; --adsb-nonoise: the same
without noise, the kernel as a pure copy)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bluesky_amd import _lib, resident, synth  # noqa: E402


def openap_tables(n, seed=5):
    """Type table, type index, force table and mass for n aircraft of random
    OpenAP types, from the reference's coefficients as the goldens hold them."""
    import numpy as np
    from bluesky_amd import perf
    from tests.test_perf_forces_cpu import load as load_forces
    from tests.test_perf_oracle import load as load_perf
    g, coeff = load_forces()
    _, fw, rot = load_perf()
    types = np.array([str(m) for m in g['fw_types']] + sorted(rot))
    actypes = types[np.random.default_rng(seed).integers(0, len(types), n)]
    lifttype = np.where(np.isin(actypes, sorted(rot)), perf.LIFT_ROTOR, perf.LIFT_FIXWING)
    return perf.type_table(fw, rot, actypes, lifttype) + perf.force_table(coeff, actypes, lifttype)


def main():
    # --perf: OpenAP phase / envelope in the step (bsa_sim_set_perf); --forces: also its drag /
    # thrust / fuel flow launch (bsa_sim_set_forces) -- its cost is --forces against --perf
    forces = '--forces' in sys.argv
    with_perf = forces or '--perf' in sys.argv
    with_fms = '--fms' in sys.argv           # Autopilot.update in the step (bsa_sim_set_fms): its cost is --fms against none
    recover = '--recover' in sys.argv        # waypoint recovery after ResumeNav (bsa_sim_set_recovery)
    with_fms = with_fms or recover
    resume_nav = recover or '--resume-nav' in sys.argv
    turb = '--turb' in sys.argv              # Turbulence.Woosh in the step (bsa_sim_set_turbulence)
    with_cond = '--cond' in sys.argv         # conditional commands in the step (bsa_sim_set_conditions), none firing
    with_area = '--exparea' in sys.argv      # the experiment area in the step (bsa_sim_set_exparea), nobody leaving
    adsb_mode = ('noise' if '--adsb' in sys.argv else 'shared' if '--adsb-shared' in sys.argv else
                 'nonoise' if '--adsb-nonoise' in sys.argv else None)          # (bsa_sim_set_adsb)
    sys.argv = [a for a in sys.argv if a not in ('--forces', '--perf', '--fms', '--recover', '--resume-nav', '--turb',
                                                 '--cond', '--exparea', '--adsb', '--adsb-shared', '--adsb-nonoise')]
    name = sys.argv[1] if len(sys.argv) > 1 else 'global1m'
    R = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 40
    only = int(sys.argv[4]) if len(sys.argv) > 4 and int(sys.argv[4]) >= 0 else None
    settle = int(sys.argv[5]) if len(sys.argv) > 5 else 200
    t = synth.workload(name)
    ctx = _lib.Context(0)
    ctx.set_timing_sample(0)
    init = resident.initial_state(t)
    sim = resident.ResidentSim(init, resident.params(cd_every=1, resume_nav=resume_nav), ctx=ctx)
    if with_fms:
        from bluesky_amd import fms
        sim.set_fms(*fms.synthetic_routes(init, seed=5, nwp=4))
        if recover:
            sim.set_recovery()
    if turb:
        sim.set_turbulence(True, (0, 0.1, 0.1), seed=5)
    if with_cond:
        import numpy as np
        k = np.random.default_rng(5).integers(0, t.ntraf, 10000)
        typ = np.arange(10000) % 2
        target = np.where(typ == 0, init['alt'][k] + 20000.0, 1.0)      # far above / far below: no crossing
        sim.set_conditions(idx=k, condtype=typ, target=target, lastdif=np.where(typ == 0, 20000.0, -100.0))
    if with_perf:
        table, tidx, ftable, mass = openap_tables(t.ntraf)
        sim.set_perf(table, tidx)
        if forces:
            sim.set_forces(ftable, mass)
    if with_area:
        sim.set_areas({'ALL': ('BOX', [-89.9, -179.9, 89.9, 179.9], 1e9, -1e9)})
        sim.set_exparea('ALL', dt=0.5, every=1, taxi=False, taxialt=-1e9)
    if adsb_mode:
        sim.set_adsb(True, noise=adsb_mode != 'nonoise', trunctime=0.0, seed=5,
                     draws='shared' if adsb_mode == 'shared' else 'per_aircraft', simt=1.0)
    out = dict(adsb=adsb_mode, perf=with_perf, forces=forces, fms=with_fms, resume_nav=resume_nav, recover=recover, turb=turb, cond=with_cond,
               exparea=with_area)
    for ranks in sorted({1, R}) if only is None else [R]:
        per = []
        for r in range(ranks) if only is None else [only]:
            ctx.sim_probe_rank(r, ranks)
            sim.step(5)                      # warm-up: this rank's plan / lists / buffers
            ctx.sync()
            if settle > 0:
                sim.step(settle)
                ctx.sync()
            t0 = time.perf_counter()
            sim.step(steps)
            ctx.sync()
            per.append((time.perf_counter() - t0) / steps * 1e3)
            st = sim.stats()
            print('%s R=%d rank %d rows [%d, %d): %.4f ms per step' % (name, ranks, r, st['row_begin'],
                                                                      st['row_end'], per[-1]), flush=True)
        out['R=%d' % ranks] = dict(slowest_ms=max(per), per_rank_ms=[round(x, 4) for x in per])
    if with_fms:
        f = sim.read_fms()
        out['fms_ticks'] = f['ticks']
        out['fms_switched'] = int((f['iactwp'] > 0).sum())
    if resume_nav:
        out['dropped_pairs_last_cd'] = int(sim.read_dropcount().sum())
    ctx.sim_probe_rank(0, 1)
    print(json.dumps(dict(workload=name, steps=steps, settle=settle, **out)), flush=True)


if __name__ == '__main__':
    main()
