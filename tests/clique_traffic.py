"""Traffic whose per-row pair counts are known before any detect runs.

``cliques(sizes, seed)``: one clique per entry of ``sizes``, each on its own
site of a 2 deg latitude x 4 deg longitude grid with |lat| <= 50 deg.  The
grid's closest sites are 120 NM (two latitudes) or 4 x 60 x cos(50 deg) =
154 NM (two longitudes at 50 deg) apart, so two aircraft of different cliques
are more than 100 NM apart: at 500 kts each they close at most 83 NM in the
300 s look-ahead and stay outside a 5 NM zone.  A clique's members lie within
+-``jitter_nm`` (0.5 NM) of the site in both axes and within +-100 m of a
common altitude (FL100-400), so every two of them are in LoS (and so in
conflict) at RPZ 5 NM / HPZ 1000 ft: a member of a clique of k has exactly
k - 1 conflict pairs and k - 1 LoS pairs.  Track, ground speed and vertical
speed are ``synth``'s (200-500 kts, 70 % level); the aircraft are permuted at
random, so a clique's members are spread over the index range.

``hotspot(n_bg, L_bg, clique_sizes, seed)``: a uniform ``synth.box`` background
with a few cliques inside the box, centred at most a quarter of the box side
from its centre.  Background aircraft near a clique add to its rows' counts,
so there only lower bounds are known in advance; the tests take the exact
figures from the oracle.

``CASES`` are the cases of tests/test_gpu_k2_paths.py (and of the CPU test of
their preconditions, tests/test_clique_traffic.py).
"""
import numpy as np

from bluesky_amd import synth

GRID_LAT = np.arange(-50.0, 50.0 + 1e-9, 2.0)
GRID_LON = np.arange(-180.0, 180.0 - 1e-9, 4.0)


def _members(rng, k, lat0, lon0, jitter_nm):
    """k aircraft around (lat0, lon0): positions, a common altitude +- 100 m."""
    lat = lat0 + rng.uniform(-jitter_nm, jitter_nm, k) / 60.0
    lon = lon0 + rng.uniform(-jitter_nm, jitter_nm, k) / 60.0 / np.cos(np.radians(lat0))
    alt = rng.uniform(100.0, 400.0) * 100.0 * synth.FT + rng.uniform(-100.0, 100.0, k)
    return lat, lon, alt


def _assemble(rng, lat, lon, alt, trk, gs, vs, member):
    """Random permutation of the aircraft; ``member[i]`` = clique number or -1."""
    n = len(lat)
    assert len(set(zip(lat.tolist(), lon.tolist()))) == n, 'two aircraft share a position'
    o = rng.permutation(n)
    t = synth.Traffic(lat[o], lon[o], alt[o], trk[o], gs[o], vs[o])
    t.clique = member[o]
    return t


def cliques(sizes, seed, jitter_nm=0.5):
    """One clique per entry of ``sizes`` on distinct grid sites; ``.clique`` holds
    each aircraft's clique number."""
    sizes = np.asarray(sizes, dtype=np.int64)
    rng = np.random.default_rng(seed)
    nsite = len(GRID_LAT) * len(GRID_LON)
    if len(sizes) > nsite:
        raise ValueError('%d cliques on %d sites' % (len(sizes), nsite))
    site = rng.choice(nsite, len(sizes), replace=False)
    lat, lon, alt = [], [], []
    for k, s in zip(sizes, site):
        a, b, c = _members(rng, int(k), GRID_LAT[s // len(GRID_LON)], GRID_LON[s % len(GRID_LON)], jitter_nm)
        lat.append(a)
        lon.append(b)
        alt.append(c)
    n = int(sizes.sum())
    _, trk, gs, vs = synth._kinematics(rng, n)
    member = np.repeat(np.arange(len(sizes)), sizes)
    return _assemble(rng, np.concatenate(lat), np.concatenate(lon), np.concatenate(alt), trk, gs, vs, member)


def hotspot(n_bg, L_bg, clique_sizes, seed, jitter_nm=0.5, lat0=52.0, lon0=4.0):
    """``synth.box(n_bg, L_bg, seed)`` plus one clique per entry of ``clique_sizes``
    inside the box: clique q sits L_bg / 4 from the centre along both axes, in
    quadrant q (four at the most)."""
    if len(clique_sizes) > 4:
        raise ValueError('at most four cliques in a hot spot')
    bg = synth.box(n_bg, L_bg, seed, lat0, lon0)
    rng = np.random.default_rng([seed, 1])
    quad = [(1, 1), (-1, -1), (1, -1), (-1, 1)]
    lat, lon, alt = [bg.lat], [bg.lon], [bg.alt]
    for q, k in enumerate(clique_sizes):
        clat = lat0 + quad[q][0] * L_bg / 4.0 / 60.0
        clon = lon0 + quad[q][1] * L_bg / 4.0 / 60.0 / np.cos(np.radians(lat0))
        a, b, c = _members(rng, int(k), clat, clon, jitter_nm)
        lat.append(a)
        lon.append(b)
        alt.append(c)
    m = int(np.sum(clique_sizes))
    _, trk, gs, vs = synth._kinematics(rng, m)
    member = np.concatenate([np.full(n_bg, -1), np.repeat(np.arange(len(clique_sizes)), clique_sizes)])
    return _assemble(rng, np.concatenate(lat), np.concatenate(lon), np.concatenate(alt),
                     np.concatenate([bg.trk, trk]), np.concatenate([bg.gs, gs]), np.concatenate([bg.vs, vs]), member)


# The cases of tests/test_gpu_k2_paths.py: kind, sizes (cliques: every clique's
# size; hot spot: n_bg, L_bg, clique sizes), seed, the bucket widths set
# (the first one is the width of the runs compared with the oracle), the jitter
# where it is not 0.5 NM (g, h: 65 MVP terms per row cancel less well-conditioned
# at 0.5 NM; at 1 NM two members are still at most 2.9 NM apart, inside the zone).
CASES = {
    'a': dict(kind='cliques', sizes=[3] * 430, seed=101, widths=(8,)),
    'b': dict(kind='cliques', sizes=[4] * 320, seed=102, widths=(8,)),
    'c': dict(kind='cliques', sizes=[4] * 320 + [5], seed=103, widths=(8,)),
    'd': dict(kind='cliques', sizes=[5] * 258, seed=104, widths=(8,)),
    'e': dict(kind='cliques', sizes=[9] * 144, seed=105, widths=(8,)),
    'f': dict(kind='cliques', sizes=[10] * 129, seed=106, widths=(8, 16)),
    'g': dict(kind='cliques', sizes=[65] * 20, seed=107, widths=(64,), jitter_nm=1.0),
    'h': dict(kind='cliques', sizes=[66] * 20, seed=408, widths=(64, 0), jitter_nm=1.0),
    'i': dict(kind='hotspot', sizes=(1100, 166.0, [30, 70]), seed=109, widths=(8,)),
    'j': dict(kind='hotspot', sizes=(1100, 166.0, [12]), seed=110, widths=(8,)),
}


def case(name):
    c = CASES[name]
    if c['kind'] == 'cliques':
        return cliques(c['sizes'], c['seed'], c.get('jitter_nm', 0.5))
    n_bg, L_bg, ks = c['sizes']
    return hotspot(n_bg, L_bg, ks, c['seed'], c.get('jitter_nm', 0.5))


def row_counts(r, n):
    """Conflict and LoS pairs per row of a detect result (oracle or device)."""
    return (np.bincount(np.asarray(r['ci'], dtype=np.int64), minlength=n),
            np.bincount(np.asarray(r['li'], dtype=np.int64), minlength=n))


def check_clique_counts(t, r):
    """The preconditions every test of a case relies on, from a detect result of
    the case's traffic: a member of a clique of k has exactly k - 1 conflict and
    k - 1 LoS pairs, all inside its clique (pure clique traffic), at least that
    many in a hot spot; the totals follow."""
    n = t.ntraf
    nc, nl = row_counts(r, n)
    size = np.bincount(t.clique[t.clique >= 0])
    want = np.where(t.clique >= 0, size[np.maximum(t.clique, 0)] - 1, 0)
    if (t.clique >= 0).all():
        assert np.array_equal(nc, want), 'conflict pairs per row'
        assert np.array_equal(nl, want), 'LoS pairs per row'
        assert len(r['ci']) == len(r['li']) == int((size * (size - 1)).sum())
        assert np.array_equal(t.clique[r['ci']], t.clique[r['cj']])
        assert np.array_equal(np.asarray(r['inconf']).astype(bool), want > 0)
    else:
        m = t.clique >= 0
        assert (nc[m] >= want[m]).all() and (nl[m] >= want[m]).all()
    return nc, nl
