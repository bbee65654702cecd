"""Every workspace query of the SSIM family (loss side and metric side) returns the byte count golden F24 recorded: the layouts behind
them -- contiguous, + 64 floats, 256-byte aligned -- differ on purpose and are part of what a caller allocates.  Host functions: no GPU."""
import json
import os

import ssim_bits_cases as B

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f24_ssim_bits.json")


def test_workspace_queries_return_the_recorded_bytes():
    from mmif._lib import lib
    with open(GOLDEN) as f:
        want = json.load(f)["workspace"]
    got = B.workspace_queries(lib)
    assert sorted(got) == sorted(want)
    assert len(got) == len(B.WS_SHAPES) * 17
    bad = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not bad, f"workspace bytes (got, recorded) differ from golden F24: {bad}"
