"""The SSIM family's bits are pinned: every call of tests/ssim_bits_cases.py -- the 'ssim' loss and the fused train-step loss, every
SSIMLoss mode with and without reflect padding, the per-window terms, the metric-side maps, sums and both MS-SSIM routes -- gives the
SHA-256 per output, value and gradient, that golden F24 recorded.  The tolerance sweeps catch a wrong formula; only this catches a changed
summation order or a differently contracted FMA."""
import json
import os

import pytest

import ssim_bits_cases as B

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f24_ssim_bits.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_the_golden_holds_every_case(golden):
    assert sorted(golden) == sorted(B.CASES)


@pytest.mark.parametrize("name", list(B.CASES))
def test_ssim_family_bits(name, golden):
    want = golden[name]
    outs, inputs = B.run(name)
    assert inputs == want["inputs"], f"{name}: the INPUT images differ from the recorded ones (generator / numpy change), not the kernels"
    assert sorted(outs) == sorted(want["outputs"])
    bad = []
    for k, t in sorted(outs.items()):
        h, s = B.digest(t)
        w = want["outputs"][k]
        print(f"{name} {k}: sum {s!r} recorded {w['sum']!r}")
        if h != w["sha256"]:
            bad.append(f"{k}: fp64 sum {s!r}, recorded {w['sum']!r}")
    assert not bad, f"{name}: bits differ from golden F24 -- " + "; ".join(bad)
