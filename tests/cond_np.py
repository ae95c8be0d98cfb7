"""numpy restatement of Condition.update and Condition.delac
(bluesky/traffic/conditional.py:25-49, 108-128), asserted bitwise equal to the reference by
tools/make_golden_cond.py at capture and to the goldens in tests/test_cond_np.py.

A table is a dict of ``idx`` (int64), ``condtype`` (float64: the reference grows it with
``np.append`` from ``[]``), ``target``, ``lastdif`` (float64)."""
import numpy as np

ALT, SPD = 0, 1
MARGIN = 1e-9   # the project's relative margin (the FMS golden's rule)


def table(idx=(), condtype=(), target=(), lastdif=()):
    return dict(idx=np.array(idx, dtype=np.int64), condtype=np.array(condtype, dtype=np.float64),
                target=np.array(target, dtype=np.float64), lastdif=np.array(lastdif, dtype=np.float64))


def update(idx, condtype, target, lastdif, alt, cas):
    """(fired indices ascending, new lastdif) of one Condition.update."""
    idx = np.asarray(idx, dtype=np.int64)
    if len(idx) == 0:
        return np.zeros(0, np.int64), np.array(lastdif, dtype=np.float64)
    condtype = np.asarray(condtype)
    with np.errstate(all='ignore'):
        actual = (condtype == ALT) * np.asarray(alt)[idx] + (condtype == SPD) * np.asarray(cas)[idx]
        actdif = np.asarray(target) - actual
        idxtrue = np.where(actdif * np.asarray(lastdif) <= 0.0)[0]
    return idxtrue, actdif


def delcondition(t, idel):
    return {k: np.delete(v, idel) for k, v in t.items()}


def deloneac(t, acidx):
    idel = np.where(t['idx'] == acidx)[0]
    if len(idel) > 0:
        t = delcondition(t, idel)
    t = dict(t)
    t['idx'] = np.where(t['idx'] <= acidx, t['idx'], t['idx'] - 1)
    return t


def delac(t, acidx):
    """Condition.delac: an int, or a sequence processed one after another in its order."""
    if len(t['idx']) == 0:
        return t
    if type(acidx) == int:
        return deloneac(t, acidx)
    for a in acidx:
        t = deloneac(t, a)
    return t


def product_margin(target, lastdif, actual):
    """|actdif * lastdif| relative to the operands' scale: how far a flag is from flipping."""
    with np.errstate(all='ignore'):
        actdif = target - actual
        scale = (np.abs(target) + np.abs(actual)) * np.abs(lastdif)
        return np.abs(actdif * lastdif) / np.where(scale > 0, scale, 1.0)


# ---------------------------------------------------------------- the flight golden's interpreter
def execute(st, alt, cmd):
    """The stacked commands of tests/golden/cond_flight64.npz on a state dict (``selalt selvs
    selspd swvnav abco``; ``alt``: traf.alt), as the reference's Autopilot.selaltcmd /
    selspdcmd / selvspdcmd do them (autopilot.py:306-358; CAS values >= 2 m/s, below the
    crossover altitude).  ``DEL k`` is the caller's; returns the aircraft to delete or None."""
    w = cmd.split()
    k = int(w[1])
    if w[0] == 'DEL':
        return k
    v = float(w[2])
    if w[0] == 'ALT':
        st['selalt'][k] = v
        if st['selvs'][k] * (v - alt[k]) < 0. and abs(st['selvs'][k]) > 0.01:
            st['selvs'][k] = 0.
    elif w[0] == 'VS':
        st['selvs'][k] = v
    elif w[0] == 'SPD':
        assert v >= 2.0 and not st['abco'][k]
        st['selspd'][k] = v
    st['swvnav'][k] = False
    return None


def drop_route(rows, off, cnt, k):
    """The route table without aircraft k."""
    rows = np.delete(rows, np.arange(off[k], off[k] + cnt[k]), axis=0)
    cnt = np.delete(cnt, k)
    off = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.asarray(off).dtype)
    return rows, off, cnt
