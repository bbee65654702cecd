"""The weight gradients' bits are pinned: every call of tests/wgrad_bits_cases.py -- each flavour of the fixed-order reduce of the per-block
partial sums (csrc/wgrad_reduce.hpp), both regimes of its sum, accumulate on and off, db wanted and not, the two-branch encoder launch, a
deferred sequence -- gives the SHA-256 per output that golden F23 recorded.  The tolerance tests catch a wrong map; only this catches a
changed summation order.  G, and with it the bits, follow the compute-unit count: on a device with another count than the recorded one the
module skips as a whole."""
import json
import os

import pytest
import torch

import wgrad_bits_cases as B

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f23_wgrad_bits.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    if ncu != g["num_cus"]:
        pytest.skip(f"F23 was recorded on {g['num_cus']} compute units, this device has {ncu}: G and the summation order differ by design")
    return g["cases"]


@pytest.mark.parametrize("c", B.CASES, ids=lambda c: c.id)
def test_weight_gradient_bits(c, golden):
    want = golden[c.id]
    outs, inputs = B.run(c)
    assert inputs == want["inputs"], f"{c.id}: the INPUT operands differ from the recorded ones (generator / numpy change), not the kernels"
    assert sorted(outs) == sorted(want["outputs"])
    bad = []
    for name, t in sorted(outs.items()):
        h, s = B.digest(t)
        w = want["outputs"][name]
        print(f"{c.id} {name}: sum {s!r} recorded {w['sum']!r}")
        if h != w["sha256"]:
            bad.append(f"{name}: fp64 sum {s!r}, recorded {w['sum']!r}")
    assert not bad, f"{c.id}: bits differ from golden F23 -- " + "; ".join(bad)
