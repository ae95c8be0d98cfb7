"""CPU: tests/cond_np.py against the goldens tools/make_golden_cond.py recorded from the
reference's Condition class, bitwise; bluesky_amd.conditional's bookkeeping against
cond_delac.npz with ``update`` served by cond_np (no device here); the C entries' refusals
that need no device."""
import ctypes
import json
import os
import types

import numpy as np
import pytest

from bluesky_amd import _lib, conditional
from tests import cond_np, util


@pytest.fixture(scope='module')
def upd():
    return dict(np.load(os.path.join(util.GOLDEN, 'cond_update.npz')))


@pytest.fixture(scope='module')
def dac():
    return dict(np.load(os.path.join(util.GOLDEN, 'cond_delac.npz')))


def test_golden_holds_every_recorded_size(upd):
    names = [str(x) for x in upd['names']]
    assert [len(upd[k + '_idx']) for k in names] == [1, 63, 64, 65, 257, 65, 65]
    assert len(upd['nothing_fired']) == 0 and len(upd['everything_fired']) == 65
    assert np.isnan(upd['alt']).sum() == 1


def test_update_restated_bitwise(upd):
    for name in (str(x) for x in upd['names']):
        g = {k: upd[name + '_' + k] for k in ('idx', 'condtype', 'target', 'lastdif', 'fired', 'newdif')}
        fired, newdif = cond_np.update(g['idx'], g['condtype'], g['target'], g['lastdif'], upd['alt'], upd['cas'])
        assert np.array_equal(fired, g['fired']), name
        assert newdif.tobytes() == g['newdif'].tobytes(), name
        assert np.all(np.diff(fired) > 0)


def test_update_of_an_empty_table():
    fired, d = cond_np.update([], [], [], [], np.zeros(3), np.zeros(3))
    assert len(fired) == 0 and len(d) == 0


def replay(dac, on_op):
    """Every recorded call in order; on_op(op, arg) applies it; yields the golden table after it."""
    off = dac['off']
    for k, rec in enumerate(str(x) for x in dac['ops']):
        op, arg = json.loads(rec)
        on_op(op, arg)
        lo, hi = off[k], off[k + 1]
        yield k, op, {f: dac[f][lo:hi] for f in ('idx', 'condtype', 'target', 'lastdif', 'id', 'cmd')}


def test_delac_restated_bitwise(dac):
    t = {'t': cond_np.table()}

    def on_op(op, arg):
        if op in ('atalt', 'atspd'):
            actual = (dac['alt'] if op == 'atalt' else dac['tas'])[arg[0]]
            new = (arg[0], 0 if op == 'atalt' else 1, arg[1], arg[1] - actual)
            t['t'] = {f: np.append(t['t'][f], v) for f, v in zip(('idx', 'condtype', 'target', 'lastdif'), new)}
        elif op == 'delac_int':
            t['t'] = cond_np.delac(t['t'], int(arg))
        elif op == 'delac_list':
            t['t'] = cond_np.delac(t['t'], list(arg))
        elif op == 'delac_array':
            t['t'] = cond_np.delac(t['t'], np.sort(np.array(arg)))
        else:
            t['t'] = cond_np.delcondition(t['t'], list(arg))

    seen = set()
    for k, op, exp in replay(dac, on_op):
        for f in ('idx', 'condtype', 'target', 'lastdif'):
            assert np.asarray(t['t'][f], dtype=exp[f].dtype).tobytes() == exp[f].tobytes(), (k, op, f)
        seen.add(op)
    assert seen == {'atalt', 'atspd', 'delac_int', 'delac_list', 'delac_array', 'delcondition'}


def test_dropin_bookkeeping_matches_the_reference(dac):
    traf = types.SimpleNamespace(id=[str(x) for x in dac['ids']], alt=dac['alt'], tas=dac['tas'], cas=dac['tas'] / 1.1)
    stacked = []
    c = conditional.Condition(traf, stack=stacked.append, evaluate=cond_np.update)
    assert c.ncond == 0 and c.cmd == []
    c.update()                                                     # an empty table: nothing happens
    c.delac(3)

    def on_op(op, arg):
        if op == 'atalt':
            assert c.ataltcmd(*arg) is True
        elif op == 'atspd':
            assert c.atspdcmd(*arg) is True
        elif op == 'delac_int':
            c.delac(int(arg))
        elif op == 'delac_list':
            c.delac(list(arg))
        elif op == 'delac_array':
            c.delac(np.sort(np.array(arg)))
        else:
            c.delcondition(list(arg))

    for k, op, exp in replay(dac, on_op):
        assert c.ncond == len(exp['idx']) == len(c.cmd), (k, op)
        for f in ('idx', 'condtype', 'target', 'lastdif'):
            assert np.array_equal(np.asarray(getattr(c, f), dtype=exp[f].dtype), exp[f]), (k, op, f)
        assert [str(x) for x in c.id] == [str(x) for x in exp['id']] and c.cmd == [str(x) for x in exp['cmd']], (k, op)
    # update through the restatement: fired commands go to the stack in ascending order and leave the table
    before = dict(idx=np.array(c.idx), cmd=list(c.cmd), lastdif=np.array(c.lastdif), target=np.array(c.target),
                  condtype=np.array(c.condtype))
    assert c.ncond > 2
    c.lastdif[1] = 0.0                                             # fires whatever the state
    fired, newdif = cond_np.update(before['idx'], before['condtype'], before['target'], c.lastdif, traf.alt, traf.cas)
    assert 1 in fired
    c.update()
    assert stacked == [before['cmd'][i] for i in fired]
    assert c.ncond == len(before['idx']) - len(fired)
    assert np.array_equal(c.lastdif, np.delete(newdif, fired)) and c.cmd == [x for i, x in enumerate(before['cmd']) if i not in set(fired)]


class ScriptedSim:
    """A stand-in for ResidentSim: recorded answers of ``step`` and ``conditions``; ``read_conditions`` answers a
    lastdif that tells the calls apart; every ``set_conditions`` is noted with the table's version and commands."""

    def __init__(self, steps, polls):
        self.steps, self.polls, self.uploads, self.reads = list(steps), list(polls), [], 0
        self.ctx = types.SimpleNamespace(sim_exparea_simt=lambda simt: None, n=8)

    def set_conditions(self, cond):
        self.cond = cond
        self.uploads.append((cond.version, list(cond.cmd)))

    def step(self, nsteps):
        return self.steps.pop(0)

    def conditions(self):
        return self.polls.pop(0)

    def read_conditions(self):
        self.reads += 1
        return dict(lastdif=np.full(self.cond.ncond, float(self.reads)))

    def exparea_events(self):
        return dict(delidx=np.zeros(0, np.int32), delidxalt=np.zeros(0, np.int32), step=0, records=None)


def test_both_run_loops_handle_a_conditions_stop_alike():
    """conditional.run and the conditions' half of exparea.run over the same recorded sim answers -- 10 steps in
    batches that end after 3, 7, 9 and 10, conditions fired at the first two: ``execute`` sees the same commands in
    the same order, the returned stops are equal, and the table goes up again exactly when ``cond.version`` moved
    while a stop's commands ran (the first stop's 'ADD' appends a condition; the second changes nothing)."""
    from bluesky_amd import exparea
    none = np.zeros(0, np.int32)
    script = dict(steps=[3, 4, 2, 1], polls=[(np.array([0, 2], np.int32), 3), (np.array([1], np.int32), 7), (none, 7), (none, 7)])

    def drive(loop):
        traf = types.SimpleNamespace(id=['AC%d' % k for k in range(8)], alt=np.arange(8.) * 100., tas=np.full(8, 150.),
                                     cas=np.full(8, 140.))
        cond = conditional.Condition(traf, stack=lambda cmd: None)
        for k, cmd in enumerate(['A', 'B', 'ADD', 'D', 'E']):
            cond.ataltcmd(k, 5000. + k, cmd)
        sim, log = ScriptedSim(**script), []

        def execute(cmd):
            log.append((cmd, cond.version, list(cond.cmd)))
            if cmd == 'ADD':
                cond.atspdcmd(7, 99., 'F')

        if loop == 'conditional':
            stops = conditional.run(sim, 10, cond, execute)
        else:
            area = exparea.Area()
            area.sim, area.simt, area.simdt, area.ids = sim, 0.0, 0.05, list(traf.id)
            events, stops = exparea.run(sim, area, 10, cond=cond, execute=execute)
            assert events == []
        assert sim.steps == [] and sim.polls == []
        return dict(log=log, stops=[(s, list(f), c) for s, f, c in stops], uploads=sim.uploads, cmd=list(cond.cmd),
                    lastdif=list(cond.lastdif), reads=sim.reads)

    a, b = drive('conditional'), drive('exparea')
    assert a == b
    assert [x[0] for x in a['log']] == ['A', 'ADD', 'D']           # ascending condition index within a stop
    assert a['stops'] == [(3, [0, 2], ['A', 'ADD']), (7, [1], ['D'])]
    assert a['log'][0][2] == ['B', 'D', 'E']                       # the fired rows left the table before execute ran
    v0, v1 = a['uploads'][0][0], a['log'][1][1]
    assert a['uploads'] == [(v0, ['A', 'B', 'ADD', 'D', 'E']), (v1 + 1, ['B', 'D', 'E', 'F'])]   # not after the second stop
    assert a['cmd'] == ['B', 'E', 'F'] and a['lastdif'] == [3.0] * 3 and a['reads'] == 3


def test_c_entries_refuse_without_a_context():
    lib = _lib.load()
    count = ctypes.c_int64(7)
    assert lib.bsa_cond_update(None, 0, None, None, None, None, 0, None, None, None, ctypes.byref(count)) == -1
    assert lib.bsa_sim_set_conditions(None, 0, None, None, None, None) == -1
    assert lib.bsa_sim_steps_run(None, None, None) == -1
    assert lib.bsa_sim_cond_poll(None, 0, None, ctypes.byref(count), None) == -1
    assert lib.bsa_sim_read_conditions(None, 0, None, None, None, None, ctypes.byref(count)) == -1
    assert _lib.ABI_VERSION == 2 and lib.bsa_abi_version() == 2


def test_flight_golden_replays_bitwise_on_the_cpu():
    """cond_flight64 replayed with fms_np + oracle/step.py + cond_np (update, execute, delac): every
    stop's step, indices and commands, the table after it and the state at every sample equal the
    reference's record bitwise -- the CPU drift of the restatement is 0, as at capture."""
    from oracle import step as ostep
    from oracle.kinematics import vtas2cas
    from tests import fms_np
    from tests.fms_cases import FMS_KEYS, STEP_KEYS
    g = dict(np.load(os.path.join(util.GOLDEN, 'cond_flight64.npz')))
    me = {k[5:]: np.array(v) for k, v in g.items() if k.startswith('init_')}
    tab = [g['route_rows'], g['rt_off'], g['rt_n']]
    t = cond_np.table(g['cond_idx'], g['cond_condtype'], g['cond_target'], g['cond_lastdif'])
    cmds = [str(x) for x in g['cond_cmd']]
    op = dict(simdt=float(g['simdt']), rpz=1.0, hpz=1.0, tla=1.0, reso=False, wind=None, mvp=None)
    simt, t0, stops, every = 0.0, -999., 0, int(g['every'])
    off = g['ev_off']
    with np.errstate(all='ignore'):
        for step in range(int(g['nsteps']) + 1):
            if step % every == 0:
                q = step // every
                for k in fms_np.OUTPUTS + ('lat', 'lon', 'alt', 'tas', 'hdg', 'vs', 'ax', 'selvs'):
                    e = g['s%02d_%s' % (q, k)]
                    assert np.array_equal(np.asarray(me[k], dtype=e.dtype), e, equal_nan=True), (q, k)
                assert simt == g['s%02d_simt' % q] and t0 == g['s%02d_t0' % q]
            if step == int(g['nsteps']):
                break
            before = me['alt'].copy()
            tick = fms_np.ticks(simt, t0)
            new = fms_np.update(me, *tab, tick=tick)
            me.update({k: new[k] for k in fms_np.OUTPUTS})
            nxt = ostep.sim_step({k: v for k, v in me.items() if k not in FMS_KEYS}, op, do_cd=False)
            me.update({k: nxt[k] for k in STEP_KEYS})
            simt, t0 = simt + op['simdt'], (simt if tick else t0)
            fired, t['lastdif'] = cond_np.update(t['idx'], t['condtype'], t['target'], t['lastdif'], me['alt'],
                                                 vtas2cas(me['tas'], before))
            if len(fired) == 0:
                continue
            assert step + 1 == g['ev_step'][stops] and np.array_equal(fired, g['ev_idx'][off[stops]:off[stops + 1]])
            todo = [cmds[i] for i in fired]
            assert todo == [str(x) for x in g['ev_cmd'][off[stops]:off[stops + 1]]]
            t = cond_np.delcondition(t, fired)
            cmds = [x for i, x in enumerate(cmds) if i not in set(int(i) for i in fired)]
            for k in ('idx', 'condtype', 'target', 'lastdif'):
                e = g['t%02d_%s' % (stops, k)]
                assert np.asarray(t[k], dtype=e.dtype).tobytes() == e.tobytes(), (stops, k)
            stops += 1
            for cmd in todo:
                gone = cond_np.execute(me, me['alt'], cmd)
                if gone is not None:
                    keep = np.ones(len(t['idx']), bool) & (t['idx'] != gone)
                    cmds = [x for x, kp in zip(cmds, keep) if kp]
                    t = cond_np.delac(t, int(gone))
                    me = {k: np.delete(v, gone) for k, v in me.items()}
                    tab = list(cond_np.drop_route(tab[0], tab[1], tab[2], gone))
    assert stops == len(g['ev_step']) > 20 and len(me['lat']) == 63
