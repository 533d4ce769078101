"""Data fixtures that let the tests run without the reference tree (CPU, wherever a checkout of the reference exists).

    tests/golden/reference_configs.json      the eight shipped coco-standard YAMLs and the two base files they name, each parsed
                                             (yaml.safe_load) into a plain mapping, keyed by its path under configs/
    tests/golden/coco_supervision_subset.json the index lists of dataseed/COCO_supervision.txt that tests/test_data_pipeline.py splits by
                                             (1 % seed 0, 5 % seed 3, 10 % seed 1), in the table's own {percent: {seed: [indices]}} layout

Nothing else of the reference is stored.

    python tests/golden/gen_golden_fixtures.py <reference checkout>
"""
import json
import os
import sys

import yaml

HERE = os.path.dirname(os.path.abspath(__file__))

CONFIGS = ["FCOS/Base-FCOS.yaml", "Faster-RCNN/Base-RCNN-FPN.yaml"]
CONFIGS += ["FCOS/coco-standard/fcos_R_50_ut2_sup%d_run0.yaml" % s for s in (1, 2, 5, 10)]
CONFIGS += ["Faster-RCNN/coco-standard/faster_rcnn_R_50_FPN_ut2_sup%d_run0.yaml" % s for s in (1, 2, 5, 10)]
SPLITS = (("1.0", "0"), ("5.0", "3"), ("10.0", "1"))


def gen_reference_configs(ref):
    out = {}
    for rel in CONFIGS:
        with open(os.path.join(ref, "configs", rel)) as f:
            out[rel] = yaml.safe_load(f) or {}
    with open(os.path.join(HERE, "reference_configs.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("reference_configs.json:", len(out), "files")


def gen_coco_supervision_subset(ref):
    with open(os.path.join(ref, "dataseed", "COCO_supervision.txt")) as f:
        table = json.load(f)
    out = {}
    for pct, seed in SPLITS:
        out.setdefault(pct, {})[seed] = [int(v) for v in table[pct][seed]]
    with open(os.path.join(HERE, "coco_supervision_subset.json"), "w") as f:
        json.dump(out, f)
    print("coco_supervision_subset.json:", sum(len(v) for d in out.values() for v in d.values()), "indices")


if __name__ == "__main__":
    gen_reference_configs(sys.argv[1])
    gen_coco_supervision_subset(sys.argv[1])
