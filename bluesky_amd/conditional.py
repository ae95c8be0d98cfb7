"""Conditional commands (ATALT / ATSPD) on the device: a drop-in for
``bluesky/traffic/conditional.py`` with the reference's surface -- ``ataltcmd``,
``atspdcmd``, ``addcondition``, ``delcondition``, ``delac``, ``deloneac``, ``update``,
``ncond`` and ``id / idx / condtype / target / lastdif / cmd`` -- without its ``bs``
globals: the traffic object (``id alt tas cas``) is handed to the constructor, the
callable that receives a fired command too (default ``bluesky.stack.stack`` when that
is importable).  ``update`` evaluates through ``bsa_cond_update``.

Inside a resident run the same object goes to ``ResidentSim.set_conditions`` and
``run`` is the loop: step, and on a stop hand the fired commands to ``execute``.

The reference's properties, kept: a condition whose ``lastdif`` is 0
fires at the next update whatever the state; a non-finite product never fires and the
condition stays; ``atspdcmd`` seeds ``lastdif`` from ``traf.tas`` while ``update``
compares ``traf.cas``.
"""
import numpy as np

from . import _lib

alttype, spdtype = 0, 1


def _default_stack():
    try:
        from bluesky import stack
        return stack.stack
    except Exception:
        return None


class Condition:
    def __init__(self, traf=None, stack=None, ctx=None, evaluate=None):
        """``traf``: what the reference reads from ``bs.traf`` (``id``, ``alt``, ``tas``,
        ``cas``).  ``stack``: called with each fired command.  ``evaluate(idx, condtype,
        target, lastdif, alt, cas) -> (fired indices, new lastdif)`` replaces the device
        call (tests without a device)."""
        self.traf, self.ctx, self.evaluate = traf, ctx, evaluate
        self.stack = stack if stack is not None else _default_stack()
        self.version = 0                          # bumped by every change of the table's rows
        self.ncond = 0
        self.id = np.array([], dtype='<U1')       # Id of aircraft of condition
        self.idx = np.array([], dtype=int)        # Index of aircraft of condition
        self.condtype = []                        # Condition type (0=alt,1=spd)
        self.target = np.array([])                # Target value
        self.lastdif = np.array([])               # Difference during last update
        self.cmd = []                             # Commands to be issued

    def arrays(self):
        """(idx int32, type int32, target, lastdif) as the C entries take them."""
        return (np.ascontiguousarray(self.idx, dtype=np.int32), np.ascontiguousarray(self.condtype, dtype=np.int32),
                _lib.f64(self.target), _lib.f64(self.lastdif))

    def update(self):
        if self.ncond == 0:
            return
        idx, typ, target, lastdif = self.arrays()
        if self.evaluate is not None:
            idxtrue, newdif = self.evaluate(idx, typ, target, lastdif, self.traf.alt, self.traf.cas)
        else:
            ctx = self.ctx or _lib.default_context()
            idxtrue, newdif = ctx.cond_update(idx, typ, target, lastdif, self.traf.alt, self.traf.cas)
        self.lastdif = np.array(newdif, dtype=np.float64)
        if len(idxtrue) == 0:
            return
        for i in idxtrue:
            self.stack(self.cmd[i])
        self.delcondition(idxtrue)

    def ataltcmd(self, acidx, targalt, cmdtxt):
        self.addcondition(acidx, alttype, targalt, self.traf.alt[acidx], cmdtxt)
        return True

    def atspdcmd(self, acidx, targspd, cmdtxt):
        self.addcondition(acidx, spdtype, targspd, self.traf.tas[acidx], cmdtxt)   # (tas, not cas: conditional.py:57)
        return True

    def addcondition(self, acidx, icondtype, target, actual, cmdtxt):
        self.id = np.append(self.id, self.traf.id[acidx])
        self.idx = np.append(self.idx, acidx)
        self.condtype = np.append(self.condtype, icondtype)
        self.target = np.append(self.target, target)
        self.lastdif = np.append(self.lastdif, target - actual)
        self.cmd.append(cmdtxt)
        self.ncond = self.ncond + 1
        self.version += 1

    def delcondition(self, idelarray):
        if self.ncond == 0:
            return
        self.id = np.delete(self.id, idelarray)
        self.idx = np.delete(self.idx, idelarray)
        self.condtype = np.delete(self.condtype, idelarray)
        self.target = np.delete(self.target, idelarray)
        self.lastdif = np.delete(self.lastdif, idelarray)
        gone = set(int(i) for i in np.atleast_1d(idelarray))
        self.cmd = [c for i, c in enumerate(self.cmd) if i not in gone]
        self.ncond = len(self.id)
        self.version += 1

    def delac(self, acidx):
        if self.ncond == 0:
            return
        if type(acidx) == int:
            self.deloneac(acidx)
        else:
            for idx in acidx:
                self.deloneac(idx)

    def deloneac(self, acidx):
        idel = np.where(self.idx == acidx)[0]
        if len(idel) > 0:
            self.delcondition(idel)
        self.idx = np.where(self.idx <= acidx, self.idx, self.idx - 1)
        self.version += 1


def take_stop(sim, cond):
    """The conditions' half of a stop, before anything is deleted (a delete compacts the device
    table): poll; if conditions fired, take their commands off ``cond`` in the reference's order
    (ascending condition index) and refresh ``cond.lastdif`` from the device.  Returns
    ``(step, fired indices, commands)``, or None when nothing fired."""
    fired, step = sim.conditions()
    if len(fired) == 0:
        return None
    cmds = [cond.cmd[i] for i in fired]
    cond.delcondition(fired)
    cond.lastdif = sim.read_conditions()['lastdif']
    return step, fired, cmds


def execute_stop(sim, cond, cmds, execute):
    """``execute(cmd)`` for each command of a stop; the table is uploaded again if that changed it."""
    v = cond.version
    for c in cmds:
        execute(c)
    if cond.version != v:
        sim.set_conditions(cond)


def run(sim, nsteps, cond, execute):
    """Advance ``sim`` (a ``ResidentSim``) by ``nsteps`` with the conditions of ``cond``:
    the table is uploaded, the sim stepped in one batch; when a condition fires the batch
    ends after that step, the fired commands are taken off ``cond`` in the reference's
    order (ascending condition index) and ``execute(cmd)`` is called for each -- it may
    call ``sim.update``, ``sim.set_fms``, ``sim.delete`` (which also applies ``delac`` to
    ``cond``) or add conditions to ``cond`` -- and the loop steps on.  ``cond.lastdif`` is
    the device's whenever ``execute`` runs and when ``run`` returns.  Returns the list of
    ``(step, fired indices, commands)`` of every stop."""
    sim.set_conditions(cond)
    events, done = [], 0
    while done < nsteps:
        done += sim.step(nsteps - done)
        stop = take_stop(sim, cond)
        if stop is not None:
            events.append(stop)
            execute_stop(sim, cond, stop[2], execute)
    if cond.ncond:
        cond.lastdif = sim.read_conditions()['lastdif']
    return events
