"""-m "not gpu": tests/golden/chain_ref.json (oracle/make_golden_chain.py, recorded from the REFERENCE's own DataProcessor) is in step
with the cases the generator builds, and its sequences of host-only methods (crop_by_bbox, apply_alpha_filter, cap_sh_degree,
apply_auto_bbox) replay through the eager drop-in class on the CPU: same table bytes, same printed lines step by step -- the
1/8-grid coordinates put zeros of both signs at the axes' extremes, where the printed box must carry the reference's zero.
The whole fixture, all seven methods and the lazy class, is replayed on the GPU (tests/test_chain_reference_gpu.py)."""
import importlib
import json
import os

import pytest

from oracle import make_golden_chain as mgc

dp = importlib.import_module("3dgsconverter_amd.processing.data_processor")


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(os.path.dirname(__file__), "golden", "chain_ref.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def all_cases():
    return mgc.cases()


def test_fixture_in_step_with_the_generator(gold, all_cases):
    assert gold["_meta"]["cases"] == mgc.N_CASES == len(all_cases)
    assert len(gold) == len(all_cases) + 1
    for case, t, steps in all_cases:
        want = gold[str(case)]
        assert want["steps_repr"] == repr(steps), case
        assert len(want["steps"]) == len(steps) or want["steps"][-1]["exc"] is not None, case
        assert want["steps"][0]["sha256_in"] == mgc.sha256(t), case


def test_host_method_sequences_through_the_eager_class(gold, all_cases):
    host = [(c, t, s) for c, t, s in all_cases if all(name in mgc.HOST_METHODS for name, _ in s)]
    assert len(host) >= 10
    # the grid cases print a zero extreme of each sign somewhere: the companion checks what it claims to
    printed = " ".join(line for c, _, _ in host for st in gold[str(c)]["steps"] for line in st["log"] if line.startswith("Auto-BBox Applied"))
    assert "-0.0000" in printed and " 0.0000" in printed.replace("[0.0000", "[ 0.0000")
    for case, t, steps in host:
        got, want = mgc.run(lambda d: dp.DataProcessor(d, lazy=False), t, steps), gold[str(case)]
        for i, (g, w) in enumerate(zip(got["steps"], want["steps"])):
            assert g["exc"] == w["exc"], (case, i, steps[i], g["exc"], w["exc"])
            assert g["sha256_in"] == w["sha256_in"] and g["nonfinite"] == w["nonfinite"], (case, i, steps[i])
            assert g["log"] == w["log"], (case, i, steps[i], g["log"], w["log"])
        assert len(got["steps"]) == len(want["steps"]), case
        assert got["dtype"] == want["dtype"] and got["sha256"] == want["sha256"], (case, steps)
