"""tools/sym_model.py (host model of the symmetric prefilter sweep, DESIGN.md
3.2c): the stage-1 blocks of box10k by tile-pair class."""
import os
import sys

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')


def test_sym_model_box10k_blocks():
    sys.path.insert(0, TOOLS)
    try:
        from sym_model import sym_model
    finally:
        sys.path.remove(TOOLS)
    m = sym_model('box10k')
    b = m['blocks']
    assert (b['diagonal'], b['upper'], b['lower']) == (7215, 8144, 8097), b
    assert b['today'] == 23456 and b['sym'] == 15359, b
    assert m['n'] == 10000 and m['items']['sym'] < m['items']['today']
