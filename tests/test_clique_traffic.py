"""The preconditions of tests/test_gpu_k2_paths.py, checked on the CPU with the
oracle detect: every case's traffic (tests/clique_traffic.py) has the per-row
conflict / LoS pair counts its K2 path needs -- k - 1 for every member of a
clique of k, nothing across cliques -- and so the block totals that decide
between the LDS fold and the global one (aircraft-index order: the standalone
detect's rows; the resident step's home order is read on the device)."""
import numpy as np
import pytest

from bluesky_amd import synth
from oracle import statebased as ocd
from tests import clique_traffic as ct

RPZ, HPZ, TLA = synth.RPZ, synth.HPZ, synth.TLOOKAHEAD
RANK_ROWS, RANK_LDS = 512, 1536     # kRankRows, kRankLds (bsa_cd_args.h)

# per case: (aircraft, conflict pairs, LoS pairs, largest conflict row, largest LoS row,
# conflict pairs per 512-row block in aircraft-index order)
EXPECT = {
    'a': (1290, 2580, 2580, 2, 2, [1024, 1024, 532]),
    'b': (1280, 3840, 3840, 3, 3, [1536, 1536, 768]),
    'c': (1285, 3860, 3860, 4, 4, [1539, 1537, 784]),
    'd': (1290, 5160, 5160, 4, 4, [2048, 2048, 1064]),
    'e': (1296, 10368, 10368, 8, 8, [4096, 4096, 2176]),
    'f': (1290, 11610, 11610, 9, 9, [4608, 4608, 2394]),
    'g': (1300, 83200, 83200, 64, 64, [32768, 32768, 17664]),
    'h': (1320, 85800, 85800, 65, 65, [33280, 33280, 19240]),
    'i': (1200, 7382, 5928, 73, 69, [2945, 3054, 1383]),
    'j': (1112, 1400, 332, 14, 11, [667, 627, 106]),
}


def block_sums(counts, order=None):
    c = counts if order is None else counts[order]
    return [int(c[k:k + RANK_ROWS].sum()) for k in range(0, len(c), RANK_ROWS)]


def grown_width(width, demand):
    """grow_k2_bucket (bsa_rank.hip): the next power of two that holds the
    largest row, or the scatter path (0) beyond 64."""
    b = max(width, 1)
    while b < demand and b <= 64:
        b *= 2
    return 0 if b > 64 else b


@pytest.fixture(scope='module', params=sorted(ct.CASES))
def detected(request):
    t = ct.case(request.param)
    return request.param, t, ocd.detect_arrays(t, t, RPZ, HPZ, TLA)


def test_counts_per_row_and_totals(detected):
    name, t, r = detected
    nc, nl = ct.check_clique_counts(t, r)
    n, P, L, cmax, lmax, blocks = EXPECT[name]
    assert (t.ntraf, len(r['ci']), len(r['li'])) == (n, P, L)
    assert (int(nc.max()), int(nl.max())) == (cmax, lmax)
    assert block_sums(nc) == blocks
    assert len(blocks) == 3 and n % RANK_ROWS != 0        # two full 512-row blocks and a partial one
    if ct.CASES[name]['kind'] == 'cliques':
        sizes = np.asarray(ct.CASES[name]['sizes'])
        assert P == L == int((sizes * (sizes - 1)).sum()) and cmax == sizes.max() - 1
        assert nc.min() == sizes.min() - 1


def test_each_case_meets_the_path_it_pins(detected):
    """What the table of tests/test_gpu_k2_paths.py promises, from the counts."""
    name, t, r = detected
    nc, nl = ct.row_counts(r, t.ntraf)
    blocks = block_sums(nc)
    demand = int(max(nc.max(), nl.max()))
    w0 = ct.CASES[name]['widths'][0]
    final = w0 if demand <= w0 else grown_width(w0, demand)
    if name == 'a':
        assert final == 8 and max(blocks) <= RANK_LDS and blocks[:2] == [1024, 1024]
    if name == 'b':
        assert final == 8 and blocks[:2] == [RANK_LDS, RANK_LDS]            # the LDS arrays exactly full
    if name == 'c':
        assert final == 8 and max(blocks) > RANK_LDS and min(blocks) <= RANK_LDS
        assert max(blocks) <= RANK_LDS + 5                                  # ... and just over them
    if name == 'd':
        assert final == 8 and min(blocks[:2]) > RANK_LDS and blocks[2] <= RANK_LDS
    if name == 'e':
        assert final == 8 and (nc == 8).all() and (nl == 8).all()          # every bucket exactly full, no retry
    if name == 'f':
        assert (nc == 9).all() and final == 16 and ct.CASES[name]['widths'] == (8, 16)
    if name == 'g':
        assert final == 64 and (nc == 64).all() and (nl == 64).all()
    if name == 'h':
        assert (nc == 65).all() and final == 0 and ct.CASES[name]['widths'] == (64, 0)
    if name == 'i':
        assert demand > 64 and final == 0
        bg = t.clique < 0
        assert np.median(nc[bg]) <= 2 and nc[t.clique == 1].min() >= 69     # sparse background, dense rows
    if name == 'j':
        assert 8 < demand <= 16 and final == 16 and max(blocks) <= RANK_LDS  # generic bucket loop + LDS fold


def test_cliques_are_far_apart_and_tight():
    t = ct.cliques([3, 4, 5] * 40, seed=5)
    lat0 = np.array([t.lat[t.clique == q].mean() for q in range(120)])
    lon0 = np.array([t.lon[t.clique == q].mean() for q in range(120)])
    for q in range(120):
        m = t.clique == q
        assert np.ptp(t.lat[m]) * 60.0 <= 1.0 and np.ptp(t.lon[m]) * 60.0 * np.cos(np.radians(lat0[q])) <= 1.0
        assert np.ptp(t.alt[m]) <= 200.0
    # closest two sites, flat-earth bound in NM (the grid: 2 deg x 4 deg, |lat| <= 50)
    dlat = (lat0[:, None] - lat0[None, :]) * 60.0
    dlon = (lon0[:, None] - lon0[None, :] + 180.0) % 360.0 - 180.0
    dlon = dlon * 60.0 * np.cos(np.radians(np.maximum(np.abs(lat0[:, None]), np.abs(lat0[None, :]))))
    d = np.hypot(dlat, dlon) + 1e9 * np.eye(120)
    assert d.min() > 100.0 and np.abs(lat0).max() <= 50.01
    assert np.array_equal(np.sort(t.clique), np.repeat(np.arange(120), [3, 4, 5] * 40))
    assert not np.array_equal(t.clique, np.sort(t.clique))                  # permuted
    u = ct.cliques([3, 4, 5] * 40, seed=5)
    assert np.array_equal(u.lat, t.lat) and np.array_equal(u.gs, t.gs)      # a function of the seed


def test_hotspot_keeps_the_background():
    t = ct.hotspot(300, 90.0, [6, 7], seed=11)
    bg = synth.box(300, 90.0, seed=11)
    m = t.clique < 0
    assert m.sum() == 300 and np.array_equal(np.sort(t.lat[m]), np.sort(bg.lat))
    for q, k in enumerate((6, 7)):
        c = t.clique == q
        assert c.sum() == k
        assert np.abs(t.lat[c] - 52.0).max() * 60.0 < 45.0                  # inside the box
