#!/usr/bin/env python
"""Write tests/golden/launch_plan.json: the launch plan of every scenario of
tests/test_gpu_launch_plan.py, recorded by that test's own code on this tree.

  python scripts/record_launch_plan.py [--out PATH]

Run it on the tree whose routing is the intended one (the parent commit of a
refactor; the new tree of a change that reroutes on purpose) and commit the
file.  Prints the conv-unit labels no scenario reached."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "3d-mask-r-cnn_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import torch
    from tests import test_gpu_launch_plan as T
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=T.GOLDEN)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    results = {}
    for name in T.SCENARIOS:
        results[name] = T.record(name, dev)
        print(name, [len(s) for s in results[name]["steps"]], "launches,", len(results[name]["log"]), "log records",
              flush=True)
    T.dump(results, args.out)
    seen = {s for r in results.values() for step in r["steps"] for s in step}
    print("not reached:", sorted(T.CONV_UNIT_LABELS - T.SLAB_LABELS - seen))
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
