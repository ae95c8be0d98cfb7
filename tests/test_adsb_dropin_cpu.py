"""CPU: the ADS-B drop-in as a member of a TrafficArrays-style tree -- ``install`` takes the old object's place among
the parent's children, so that the parent's create / delete / reset reach it (no device: ``trunctime`` 0)."""
import numpy as np
import pytest

from bluesky_amd import adsb
from tests import adsb_np


def tree_with_reference_adsb(n=3):
    """A parent with three children; the middle one plays the reference's ADSB (it is what ``traf.adsb`` names)."""
    traf = adsb_np.ArrayTree()
    before, old, after = (adsb_np.ArrayTree(adsb_np.ARRAYS) for _ in range(3))
    for child in (before, old, after):
        child.parent = traf
        traf.children.append(child)
    old.transnoise, old.truncated, old.transerror, old.trunctime = True, True, [2e-4, 50.0], 0
    traf.adsb = old
    state = {k: np.arange(n) + 10.0 * q + 1.0 for q, k in enumerate(adsb_np.FIELDS)}
    traf.create(n, **state)
    for k in adsb_np.FIELDS:                       # the old object holds an earlier picture
        setattr(old, k, state[k] - 0.5)
    old.lastupdate = -np.arange(n, dtype=np.float64)
    return traf, before, old, after


def picture(ad):
    return {k: getattr(ad, k) for k in adsb_np.ARRAYS}


def test_install_takes_the_old_objects_place():
    traf, before, old, after = tree_with_reference_adsb()
    ad = adsb.install(traf, seed=3)
    assert traf.adsb is ad and traf.children == [before, ad, after] and ad.parent is traf and old.parent is None
    assert ad.children == [] and (ad.transnoise, ad.truncated, ad.transerror, ad.trunctime) == (True, True, [2e-4, 50.0], 0)
    for k in adsb_np.ARRAYS:
        assert np.array_equal(getattr(ad, k), getattr(old, k)) and getattr(ad, k) is not getattr(old, k)
    again = adsb.install(traf, seed=4, draws='per_aircraft')
    assert traf.children == [before, again, after] and ad.parent is None and again.draws == 'per_aircraft'


def test_install_without_an_old_object_or_without_a_tree():
    traf = adsb_np.ArrayTree()
    ad = adsb.install(traf)
    assert traf.children == [ad] and ad.parent is traf
    traf.create(2, lat=[1.0, 2.0], gs=[100.0, 200.0], vs=[3.0, 4.0])
    assert len(ad.lastupdate) == 2 and list(ad.lat) == [1.0, 2.0] and list(ad.gs) == [100.0, 200.0] and not ad.vs.any()
    import types
    flat = types.SimpleNamespace(lat=np.zeros(0))
    assert adsb.install(flat) is flat.adsb and not hasattr(flat, 'children')


def test_parent_create_delete_reset_reach_the_installed_object():
    traf, before, old, after = tree_with_reference_adsb(3)
    ad = adsb.install(traf, seed=3)
    exp = picture(ad)
    new = {k: np.array([7.0, 8.0]) + q for q, k in enumerate(adsb_np.FIELDS)}
    traf.create(2, **new)
    assert traf.ntraf == 5 and all(len(getattr(c, 'lastupdate')) == 5 for c in traf.children)
    assert len(old.lastupdate) == 3                                        # the replaced object is out of the tree
    exp = adsb_np.create(exp, {k: getattr(traf, k) for k in adsb_np.FIELDS}, 2, 0, np.ones(2))
    for k in adsb_np.ARRAYS:
        assert np.array_equal(getattr(ad, k), exp[k]), k
    assert not ad.vs[-2:].any() and np.array_equal(ad.trk[-2:], new['trk']) and not ad.lastupdate[-2:].any()
    traf.delete(np.array([0, 3]))
    exp = adsb_np.delete(exp, [0, 3])
    assert traf.ntraf == 3
    for k in adsb_np.ARRAYS:
        assert np.array_equal(getattr(ad, k), exp[k]), k
    traf.delete(1)                                                         # Traffic.delete also takes one index
    assert traf.ntraf == 2 and np.array_equal(ad.lat, np.delete(exp['lat'], 1))
    traf.reset()
    assert traf.ntraf == 0 and all(len(getattr(ad, k)) == 0 for k in adsb_np.ARRAYS)
    traf.create(1, lat=[5.0])
    assert len(ad.lastupdate) == 1 and ad.lat[0] == 5.0


def test_reparent_moves_it_between_parents():
    a, b = adsb_np.ArrayTree(), adsb_np.ArrayTree()
    ad = adsb.install(a)
    ad.reparent(b)
    assert a.children == [] and b.children == [ad] and ad.parent is b
    with pytest.raises(ValueError):
        adsb.ADSB(a, draws='each')
