"""Test-time augmentation (TEST.AUG) timed on synthetic 800 x 1333 loader images with the default view list (9 sizes x
flip = 18 views), both detectors, fp16 activations, random weights with the test thresholds as shipped.  Per detector one JSON line:
seconds per image under TTA, seconds per image of plain inference on the same build, the sum of 18 plain single-view inferences at the
views' sizes (the no-overhead bound), and the share of a TTA call spent in collect + merge (device time between events).

    python tools/bench_tta.py [--images 4] [--repeat 3] [--kinds fcos rcnn] [--precision fp16]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unbiased-teacher-v2_amd"))


def timed(fn, repeat):
    fn()                                   # warm-up: workspaces, shape-keyed caches
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--kinds", nargs="+", default=["fcos", "rcnn"])
    ap.add_argument("--precision", default="fp16", choices=["fp16", "bf16", "fp32"])
    args = ap.parse_args()
    from ubteacher import ops
    from ubteacher.data.synthetic import SyntheticTestLoader
    from ubteacher.modeling import DetectorWithTTA, build_model, tta_views
    from ubteacher.presets import get_config
    for kind in args.kinds:
        cfg = get_config(kind, 1, ["MODEL.DEVICE", "cuda", "SOLVER.AMP.ENABLED", args.precision != "fp32"])
        ops.set_precision(args.precision)
        torch.manual_seed(0)
        model = build_model(cfg).eval()
        tta = DetectorWithTTA(cfg, model)
        nms_method = cfg.MODEL.FCOS.NMS_CRITERIA_TEST if kind == "fcos" else None
        # the same records for every column: image + size only (the loader's ground-truth `instances` would be uploaded by the plain FCOS call)
        batches = [[{k: v for k, v in d.items() if k != "instances"} for d in b]
                   for b in SyntheticTestLoader(cfg, num_images=args.images, height=800, width=1333, orig_scale=1.0)]
        views = tta_views(cfg, (800, 1333), (800, 1333))

        def plain(recs):
            with torch.no_grad():
                return model(recs, nms_method=nms_method) if nms_method else model(recs)

        t_tta = timed(lambda: [tta(b) for b in batches], args.repeat) / len(batches)
        t_plain = timed(lambda: [plain(b) for b in batches], args.repeat) / len(batches)
        # the 18 views of the first image, each as a plain single-image inference at its own size
        vimgs = tta.view_images(batches[0][0]["image"], views)
        t_views = timed(lambda: [plain([{"image": im, "height": 800, "width": 1333}]) for im in vimgs], args.repeat)
        # collect + merge: device time between two events around the stage, the views' detections already there
        with torch.no_grad():
            dets = [tta.detect_view(im) for im in vimgs]
            table = tta.transform_table(views, (800, 1333), vimgs[0].device)
            tta.merge(dets, table, (800, 1333))
            torch.cuda.synchronize()
            ms = []
            for _ in range(max(args.repeat, 5)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                tta.merge(dets, table, (800, 1333))
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
        t_merge = statistics.median(ms) / 1e3
        print(json.dumps({"bench": "tta", "model": kind, "precision": args.precision, "views": len(views), "images": len(batches),
                          "device": torch.cuda.get_device_name(0), "tta_s_per_image": round(t_tta, 4), "plain_s_per_image": round(t_plain, 4),
                          "sum_of_single_view_inferences_s": round(t_views, 4), "collect_merge_s": round(t_merge, 6),
                          "collect_merge_share": round(t_merge / t_tta, 5)}), flush=True)
        ops.set_precision("fp32")


if __name__ == "__main__":
    main()
