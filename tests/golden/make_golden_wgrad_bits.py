"""Golden F23: the bits of every weight gradient that goes through the fixed-order reduce (tests/wgrad_bits_cases.py), per case and output
the SHA-256 of the float32 bytes of t + 0.0, the fp64 sum (for diagnosis) and the SHA-256 of the case's input operands; + the device's name
and compute-unit count (G, hence the bits, follow it) and the commit the library was built from.  Needs a GPU.

    MMIF_LIB=/path/to/libmmif_hip.so MMIF_GOLDEN_COMMIT=<commit of that build> python tests/golden/make_golden_wgrad_bits.py [out.json]

The fixture pins the summation order of the commit it was generated at: a change that is meant to keep every bit is tested AGAINST it and
must not regenerate it.  Two runs must give byte-identical files (the producers and the reduce are deterministic)."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "multi-modal-image-fusion_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import torch
    import wgrad_bits_cases as B
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "f23_wgrad_bits.json")
    commit = os.environ.get("MMIF_GOLDEN_COMMIT")
    if not commit:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
    prop = torch.cuda.get_device_properties(0)
    cases = {}
    for c in B.CASES:
        outs, inputs = B.run(c)
        rec = {"inputs": inputs, "outputs": {}}
        for name, t in sorted(outs.items()):
            h, s = B.digest(t)
            rec["outputs"][name] = {"sha256": h, "sum": s}
        cases[c.id] = rec
        print(c.id, len(outs), flush=True)
    with open(out, "w") as f:
        json.dump({"commit": commit, "device": prop.name, "num_cus": prop.multi_processor_count, "cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
