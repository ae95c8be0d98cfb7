"""tools/sym_model.py's triangular count: the symmetric
sweep's stage-1 blocks without the lower blocks of the diagonal tile pairs."""
import os
import sys

from bluesky_amd import synth

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')


def model(t):
    sys.path.insert(0, TOOLS)
    try:
        from sym_model import sym_model
    finally:
        sys.path.remove(TOOLS)
    return sym_model(t)


def test_tri_blocks_box10k_and_the_existing_keys():
    m = model('box10k')
    b = m['blocks']
    assert b['tri'] == 12394, b
    assert (b['diagonal'], b['upper'], b['lower']) == (7215, 8144, 8097), b
    assert b['today'] == 23456 and b['sym'] == 15359, b
    assert m['n'] == 10000 and set(m['items']) == {'diagonal', 'upper', 'lower', 'today', 'sym'}


def test_tri_blocks_three_tiles():
    b = model(synth.box(1300, 60.0, seed=31))['blocks']
    assert (b['tri'], b['sym'], b['today']) == (1740, 2262, 3408), b
