"""tests/golden/norm_kernels_parent.json: SHA-256 of every output tensor of the BatchNorm and per-ROI GroupNorm kernels, per case and
library kind, as the built libraries of the checked-out commit produce them on the GPU.  Results only: the cases and the integer
formula of the inputs live in tests/test_norm_kernels_parent_bits_gpu.py, which this script imports and which asserts the digests.

RUN IT ON THE COMMIT WHOSE BITS ARE MEANT (build that commit's libraries first) and name it with --commit: the fixture pins the
arithmetic of that commit, not of the tree the test later runs in.  A later change that alters this arithmetic on purpose regenerates
the file from its own build and says so in its description.

    python tests/golden/gen_golden_norm_parent.py --commit <hash> [--out tests/golden/norm_kernels_parent.json]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "unbiased-teacher-v2_amd"))

from tests import test_norm_kernels_parent_bits_gpu as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit whose kernels are built in lib/")
    ap.add_argument("--out", default=T.FIXTURE)
    args = ap.parse_args()
    digests = {}
    for case in T.BN_CASES:
        digests[T.bn_id(case)] = {kind: T.bn_digests(case, kind) for kind in T.KINDS}
    for case in T.ROI_CASES:
        for relu in (True, False):
            digests[T.roi_id(case, relu)] = {kind: T.roi_digests(case, relu, kind) for kind in T.KINDS}
    with open(args.out, "w") as f:
        json.dump({"commit": args.commit, "digests": digests}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases, %d digests" % (args.out, len(digests), sum(len(k) for c in digests.values() for k in c.values())))


if __name__ == "__main__":
    main()
