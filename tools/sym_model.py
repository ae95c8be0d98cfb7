"""Host model of the symmetric prefilter sweep: the stage-1
blocks (64 rows x 8 columns) and the (tile pair, 64-row slice) items of a
detect whose rows are its columns, split by tile pair -- diagonal (a = a),
upper (a < b), lower (a > b).  Today's sweep runs all three; the symmetric
sweep lists the diagonal and the upper pairs only and refines the upper
pairs' stage-1 survivors in both orientations.  The triangular sweep (3.2d,
blocks['tri']) also drops, inside a diagonal pair, the blocks whose column
sub-group lies below the slice's own columns.

Order, records and box test are tools/octet_model.py's (the device's Hilbert
key, make_pf_mid in fp64, boxes_may_interact).
Usage: PYTHONPATH=. python tools/sym_model.py [WORKLOAD]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import octet_model as om  # noqa: E402

from bluesky_amd import synth  # noqa: E402

CLASSES = ('diagonal', 'upper', 'lower')


def sym_model(t, R=synth.RPZ, H=synth.HPZ, T=synth.TLOOKAHEAD, seed=7):
    """t: a workload name or a Traffic.  Returns dict(n, blocks, items), blocks
    and items being dicts over CLASSES plus 'today' (all three) and 'sym'
    (diagonal + upper); blocks also has 'tri' (sym without the diagonal pairs'
    lower blocks)."""
    if isinstance(t, str):
        t = synth.workload(t, seed=seed)
    P, s, lo, hi = om.records(t, R, H, T)
    o = np.argsort(om.curve_key(P), kind='stable')
    P, s, lo, hi = P[o], s[o], lo[o], hi[o]
    tb, gb, sb = (om.boxes(P, s, lo, hi, g) for g in (om.KT, om.KG, om.KS))
    nt, ng, nsb = len(tb['s']), len(gb['s']), len(sb['s'])
    ti, tj = np.nonzero(om.interact(tb, np.arange(nt)[:, None], tb, np.arange(nt)[None, :]))
    # items: (tile pair, slice) whose slice (group) box may reach the column tile box
    it_r = (ti[:, None] * 8 + np.arange(8)[None, :]).ravel()
    it_c = np.repeat(tj, 8)
    ok = (it_r < ng) & om.interact(gb, np.minimum(it_r, ng - 1), tb, it_c)
    it_r, it_c = it_r[ok], it_c[ok]
    cls = np.where(it_r // 8 == it_c, 0, np.where(it_r // 8 < it_c, 1, 2))
    blocks, items = np.zeros(3, np.int64), np.bincount(cls, minlength=3)
    low = 0   # blocks of diagonal items whose column sub-group lies below the slice's own eight
    CH = 4096
    for k in range(0, len(it_r), CH):
        r, c = it_r[k:k + CH], it_c[k:k + CH]
        col_sg = c[:, None] * 64 + np.arange(64)[None, :]       # the column tile's sub-groups
        gm = (col_sg < nsb) & om.interact(gb, r[:, None], sb, np.minimum(col_sg, nsb - 1))   # the sweep's mask
        blocks += np.bincount(cls[k:k + CH], weights=gm.sum(1), minlength=3).astype(np.int64)
        below = np.arange(64)[None, :] < 8 * (r % 8)[:, None]
        low += int((gm & below & (cls[k:k + CH] == 0)[:, None]).sum())

    def table(v):
        d = {name: int(v[q]) for q, name in enumerate(CLASSES)}
        d.update(today=int(v.sum()), sym=int(v[0] + v[1]))
        return d
    b = table(blocks)
    b['tri'] = b['sym'] - low   # the triangular sweep (3.2d): no lower blocks inside a diagonal tile pair
    return dict(n=len(P), blocks=b, items=table(items))


def main(wl):
    m = sym_model(wl)
    b, it = m['blocks'], m['items']
    print('%s: N=%d' % (wl, m['n']))
    print('%-22s %22s %26s' % ('tile pairs', 'stage-1 blocks (64 x 8)', 'items (tile pair, slice)'))
    for name in CLASSES:
        print('%-22s %22d %26d' % (name, b[name], it[name]))
    print('%-22s %22d %26d' % ('today', b['today'], it['today']))
    print('%-22s %14d (%+.1f %%) %18d (%+.1f %%)' % ('diagonal + upper only', b['sym'],
                                                     100.0 * (b['sym'] / max(b['today'], 1) - 1.0), it['sym'],
                                                     100.0 * (it['sym'] / max(it['today'], 1) - 1.0)))
    print('%-22s %14d (%+.1f %%)' % ('... triangular inside', b['tri'], 100.0 * (b['tri'] / max(b['today'], 1) - 1.0)))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else 'box100k')
