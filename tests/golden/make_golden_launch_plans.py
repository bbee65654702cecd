"""Golden F22: the launch plans of the model engines (tests/launch_plan_cases.py), per case and step the ordered entry-point names, a
SHA-256 over the canonical full record and 6 hex digits per call.  Needs a GPU (the plan is recorded from real steps).

    python tests/golden/make_golden_launch_plans.py [out.json]

The fixture pins the routes of the commit it was generated at (its "commit" field): a change that is meant to keep every route is
tested AGAINST it and must not regenerate it."""
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
    import launch_plan_cases as LP
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "f22_launch_plans.json")
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = os.environ.get("MMIF_GOLDEN_COMMIT", "unknown")
    plans = {}
    for case in LP.CASES:
        steps = LP.run_case(case)
        plans[case["id"]] = {str(k): LP.summarise(v) for k, v in steps.items()}
        print(case["id"], {k: len(v) for k, v in steps.items()}, flush=True)
    with open(out, "w") as f:
        json.dump({"commit": commit, "plans": plans}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
