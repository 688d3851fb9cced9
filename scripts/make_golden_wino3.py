#!/usr/bin/env python3
"""Records tests/golden/wino3_item_boundary.json: per row of tests/test_gpu_wino3_item_boundary.py the plan of the net's
convolutions and the SHA-256 of every block output, on the device and the build it is run with.  Run it on the build whose
bits are to be kept (before a change to conv_wino3_kernel that must not alter them).

usage: python scripts/make_golden_wino3.py [OUT.json]"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    import torch

    import tests.gpu_utils as gu
    import tests.test_gpu_wino3_item_boundary as tw
    out = sys.argv[1] if len(sys.argv) > 1 else tw.GOLDEN
    os.environ["HOLO_KEEP_INTERMEDIATES"] = "1"
    os.environ.update(tw.W3_ENV)
    rec = {}
    for row in tw.ROWS:
        outs, _, _, convs = tw.run_row(gu, row)
        rec[row] = {"device": torch.cuda.get_device_name(0), "plan": tw.plan_of(convs), "digests": tw.digests_of(outs)}
        print(row, len(convs), "convolutions,", len(outs), "blocks")
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
