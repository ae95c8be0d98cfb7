"""Bitwise comparison of two library builds (A/B of a change that must not
move any result): the drop-in detect at box100k (pairs and payload), 40
resident steps at a 20k box with MVP, 120 resident steps of 400 aircraft with
conditions and the experiment area attached (the polled lists, the exit records,
the area's arrays, the state), and a 2048 x 2048 qdrdist matrix.
Each build runs in its own process (BSACCEL_LIB); exit 1 on any difference.
Usage: python tools/ab_bitwise.py bluesky_amd/libA.so bluesky_amd/libB.so"""
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(out):
    from bluesky_amd import _lib, areafilter, conditional, exparea, geo, resident, statebased, synth
    res = {}
    t = synth.workload('box100k')
    d = statebased.detect_indices(t, t, synth.RPZ, synth.HPZ, synth.TLOOKAHEAD, with_dcpa=True)
    res.update({'detect_' + k: np.asarray(v) for k, v in d.items()})
    ctx = _lib.Context(0)
    tb = synth.box(20000, 200.0, seed=11)
    sim = resident.ResidentSim(resident.initial_state(tb), resident.params(cd_every=1), ctx=ctx)
    sim.step(40)
    res.update({'sim_' + k: np.asarray(v) for k, v in sim.read().items()})
    # the stopping stages: aircraft 0 .. 39 climb (those out of conflict) through a condition each; the area is the
    # southern half, left northwards, a pass every 10th step
    init = resident.initial_state(synth.box(400, 60.0, seed=13))
    for k in ('ap_alt', 'selalt', 'asas_alt'):
        init[k][:40] += 600.0
    sim = resident.ResidentSim(init, resident.params(cd_every=1), ctx=ctx)
    traf = type('T', (), dict(id=['AC%d' % k for k in range(400)], alt=init['alt'], tas=init['tas'], cas=init['tas']))()
    cond = conditional.Condition(traf, stack=lambda cmd: None)
    for k in range(40):
        cond.ataltcmd(k, float(init['alt'][k] + 0.5), 'C%d' % k)
    cond.ataltcmd(40, float(init['alt'][40] + 5000.0), 'NEVER')
    areafilter.reset()
    areafilter.defineArea('SOUTH', 'BOX', [-89., -179., float(np.median(init['lat'])), 179.], 1e9, -1e9)
    area = exparea.Area()
    area.attach(sim, simt=0.0)
    area.set_area('SOUTH')
    log = []
    events, stops = exparea.run(sim, area, 120, cond=cond, execute=log.append)
    areafilter.reset()
    assert len(stops) > 1 and any(len(e['delidx']) for e in events), (log, len(events))
    res['xa_log'] = np.array(log)
    res['xa_stops'] = np.concatenate([[st, len(f)] + [int(x) for x in f] for st, f, _ in stops])
    for q, e in enumerate(events):
        res['xa_ev%d' % q] = np.concatenate([[e['step']], e['delidx'], [-1], e['delidxalt']]).astype(np.int64)
        res.update({'xa_ev%d_%s' % (q, k): np.asarray(v) for k, v in e['columns'].items()})
    res.update({'xa_' + k: np.asarray(v) for k, v in sim.read_exparea().items()})
    res.update({'xa_cond_' + k: np.asarray(v) for k, v in sim.read_conditions().items()})
    res.update({'xa_sim_' + k: np.asarray(v) for k, v in sim.read().items()})
    ctx.close()
    rng = np.random.default_rng(5)
    la, lo = rng.uniform(-60, 60, 2048), rng.uniform(-180, 180, 2048)
    q, dd = geo.qdrdist_matrix(la, lo, la[::-1].copy(), lo[::-1].copy())
    res['geo_qdr'], res['geo_dist'] = np.asarray(q), np.asarray(dd)
    np.savez(out, **res)


def main():
    if sys.argv[1] == '--run':
        run(sys.argv[2])
        return 0
    tmp = tempfile.mkdtemp()
    files = []
    for k, lib in enumerate(sys.argv[1:3]):
        f = os.path.join(tmp, '%d.npz' % k)
        env = dict(os.environ, BSACCEL_LIB=os.path.abspath(lib), BSACCEL_AB='1')
        subprocess.run([sys.executable, __file__, '--run', f], env=env, check=True, timeout=600)
        files.append(np.load(f))
    a, b = files
    bad = [k for k in sorted(set(a.files) | set(b.files))
           if k not in a.files or k not in b.files or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
    print('arrays compared: %d, differing: %s' % (len(a.files), bad or 'none'))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
