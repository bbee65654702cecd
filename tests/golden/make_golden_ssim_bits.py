"""Golden F24: the bits of the SSIM family (tests/ssim_bits_cases.py) -- the byte count of every workspace query, and per case and output
the SHA-256 of the bytes of t + 0.0, the fp64 sum (for diagnosis) and the SHA-256 of the case's input images; + the device's name and the
commit the library was built from.

    MMIF_LIB=/path/to/libmmif_hip.so MMIF_GOLDEN_COMMIT=<commit of that build> python tests/golden/make_golden_ssim_bits.py [out.json]

The workspace part needs no GPU; without one the script records it alone and keeps the "cases" the file already holds.  The fixture pins
the arithmetic of the commit it was generated at: a change that is meant to keep every bit is tested AGAINST it and must not regenerate
it.  Two runs must give byte-identical files (every kernel of the family is deterministic)."""
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
    import ssim_bits_cases as B
    from mmif._lib import lib
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "f24_ssim_bits.json")
    commit = os.environ.get("MMIF_GOLDEN_COMMIT")
    if not commit:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
    rec = {}
    if os.path.exists(out):
        with open(out) as f:
            rec = json.load(f)
    rec["commit"] = commit
    rec["workspace"] = B.workspace_queries(lib)
    if torch.cuda.is_available():
        rec["device"] = torch.cuda.get_device_properties(0).name
        cases = {}
        for name in B.CASES:
            outs, inputs = B.run(name)
            cases[name] = {"inputs": inputs, "outputs": {}}
            for k, t in sorted(outs.items()):
                h, s = B.digest(t)
                cases[name]["outputs"][k] = {"sha256": h, "sum": s}
            print(name, len(outs), flush=True)
        rec["cases"] = cases
    else:
        print("no GPU: workspace part only")
    with open(out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
