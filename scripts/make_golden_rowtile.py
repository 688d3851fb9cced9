#!/usr/bin/env python3
"""Records tests/golden/rowtile_bits.json: per row of tests/test_gpu_rowtile_bits.py the plan of the net's convolutions and
the SHA-256 of every block output, on the device and the build it is run with.  Run it on the build whose bits are to be
kept (before a change to conv_small_kernel that must not alter them).

usage: python scripts/make_golden_rowtile.py [OUT.json]"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    import torch

    import tests.gpu_utils as gu
    import tests.test_gpu_rowtile_bits as tr
    out = sys.argv[1] if len(sys.argv) > 1 else tr.GOLDEN
    os.environ.update(tr.DIRECT_ENV)
    rec = {}
    for row in tr.ROWS:
        outs, trace, convs = tr.run_row(gu, row)
        rec[row] = {"device": torch.cuda.get_device_name(0), "plan": tr.plan_of(convs), "digests": tr.digests_of(outs)}
        on = sum(1 for o in convs if o["kernel"] == tr.ROWTILE)
        worst = max(gu.rel_err(o, trace[tag]) for tag, o in outs.items())
        print(row, len(convs), "convolutions,", on, "on", tr.ROWTILE + ",", len(outs), "blocks, worst rel_err %.2e" % worst)
        for p in rec[row]["plan"]:
            print("   ", p)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
