"""-m gpu: a fixed, seeded slice of the randomised sweeps of tests/devtools (fuzz_parity.py, fuzz_more.py) inside the suite.

The only defect of round 3 -- rim queries of a brick's later batches, wrong in ~15 % of the runs of ONE planar cloud -- was
found by the sweep, not by the fixtures.  So 60 clouds of it now run with every `pytest -m gpu`: random sizes
1 ... 300k, nine shapes (planes, lines, duplicates, scenes with far floaters, anisotropic boxes 12 345 units from the origin,
tight blobs), k in {1 ... 64}, through the host entry point (adaptive mode), the device API with both phase-1 filters, the tree
path asked for explicitly, shares of the bricks / leaves, sub-range queries, the density filter and density -> SOR on the device
chain -- bit-exact against the cKDTree / numpy restatement (oracle/sor.py, oracle/density.py), which is pinned to the reference."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "devtools"))


def test_fuzz_parity_slice(gsx):
    import fuzz_parity
    assert fuzz_parity.main(cases=40, seed=20260926) == 0


def test_fuzz_more_slice(gsx):
    import fuzz_more
    assert fuzz_more.main(cases=20, seed=20260927) == 0


def test_fuzz_sog_slice(gsx):
    """round 6: the SOG writer's device-resident core (formats/sog_device.py) on 16 random tables -- sizes 1100 ... 400k, SH degree
    0-3 with zeroed coefficient tails, tied / duplicate / signed-zero / wide-range coordinates, rows widened by u1 fields, every
    compression level -- against the restated reference statements (oracle/sog.py), five images byte for byte"""
    import fuzz_sog
    assert fuzz_sog.main(cases=16, seed=20260930) == 0


def test_fuzz_chain_slice(gsx):
    """round 6: 25 random sequences of the drop-in DataProcessor's methods (bbox / alpha / density / SOR / SH cap / colours / auto-bbox in
    any order), lazy class -- device chain, deferred column fills and colours, ONE fused compaction (gsx_host_take_rows_shape) --
    against the eager class: the final tables are the same bytes and the printed status lines the same"""
    import fuzz_chain
    assert fuzz_chain.main(cases=25, seed=20261001) == 0
