"""numpy restatement of Windfield.getdata for a 3-D field (winddim 3,
bluesky/traffic/windfield.py:158-202), vectorised over positions.

TEST INFRASTRUCTURE ONLY.  The reference's own getdata raises for array
arguments longer than one (windfield.py:177 takes the truth value of
``useralt==None``) but runs for one position at a time; this is the array form
of that per-position result, with the reference's own expressions (including
its ``ones((1, nvec)).dot(..)`` / ``.dot(ones((nvec, 1)))`` products, taken
position by position as one reference call has them), asserted bitwise equal
to per-aircraft calls of the reference at capture (tools/make_golden.py
--wind3d-only).

Build-defined where the reference raises or is undefined: the
lower level ``ialt`` is clamped into [0, nalt - 2] before any table read, so
``alt >= (nalt - 1) * altstep`` (the reference: IndexError) gives ``falt`` = 1,
the top level's wind, and a non-finite altitude reads level 0 (NaN) or the
clamped level (+-inf, which the reference's minimum / maximum already bound)
with ``falt`` carried through the blend.
"""
import numpy as np


def level(alt, nalt, altstep):
    """windfield.py:185-189: (ialt, falt) with ialt clamped into [0, nalt - 2]."""
    eps = 1e-20
    top = (nalt - 1) * altstep                       # self.altaxis[-1]
    with np.errstate(invalid='ignore'):
        idxalt = np.maximum(0., np.minimum(top - eps, alt) / altstep)
        fl = np.floor(idxalt)
        ialt = np.clip(np.where(np.isnan(fl), 0., fl), 0, nalt - 2).astype(int)
    falt = idxalt - ialt
    return ialt, falt


def getdata(lat, lon, alt, wlat, wlon, wvnorth, wveast, altstep):
    """(vnorth, veast) at positions lat / lon [deg], alt [m] of the field with
    points wlat / wlon and tables wvnorth / wveast of shape (nalt, nvec)."""
    eps = 1e-20
    lat, lon, alt = (np.asarray(x, dtype=np.float64) for x in (lat, lon, alt))
    wvnorth, wveast = np.asarray(wvnorth, dtype=np.float64), np.asarray(wveast, dtype=np.float64)
    npos = len(lat)
    nvec = len(wlat)
    lat = np.array(lat).reshape((1, npos))
    lon = np.array(lon).reshape((1, npos))
    wl = np.array([np.asarray(wlat, dtype=np.float64)]).transpose()
    wo = np.array([np.asarray(wlon, dtype=np.float64)]).transpose()
    cavelat = np.cos(np.radians(0.5 * (lat + wl)))
    dy = lat - wl
    dx = cavelat * (lon - wo)
    invd2 = 1. / (eps + dx * dx + dy * dy)
    # the reference's products, position by position: BLAS sums a product of
    # several columns / rows in another order than the one-position product the
    # reference can run (seen at capture: up to 1.4e-14 m/s apart), so each
    # position's (1, nvec) x (nvec, 1) products are taken on its own contiguous
    # slices, as one reference call has them; everything else is element-wise
    row1 = np.ones((1, nvec))
    col = np.ascontiguousarray(invd2.T)                   # (npos, nvec): position i's invd2 contiguous
    sumsid2 = np.array([row1.dot(col[i].reshape((nvec, 1)))[0, 0] for i in range(npos)]).reshape((1, npos))
    totals = np.repeat(sumsid2, nvec, axis=0)
    horfact = invd2 / totals
    ialt, falt = level(alt, wvnorth.shape[0], altstep)
    one = np.ones((nvec, 1))
    hT = horfact.T

    def hsum(tab, lev):
        prod = np.ascontiguousarray(tab[lev, :] * hT)     # (npos, nvec)
        return np.array([prod[i:i + 1].dot(one)[0, 0] for i in range(npos)])

    vnorth = (1. - falt) * hsum(wvnorth, ialt) + falt * hsum(wvnorth, ialt + 1)
    veast = (1. - falt) * hsum(wveast, ialt) + falt * hsum(wveast, ialt + 1)
    return vnorth, veast


def field_of(z, prefix='w'):
    """The field arrays of a wind3d fixture as getdata's keyword arguments."""
    return dict(wlat=z[prefix + 'lat'], wlon=z[prefix + 'lon'], wvnorth=z[prefix + 'vnorth'],
                wveast=z[prefix + 'veast'], altstep=float(z['altstep']))
