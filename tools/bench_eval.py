"""Host vs device COCO box evaluation on a COCO-val-shaped synthetic split (5000 images, 80 classes, ~7 ground-truth boxes and 100
detections per image, a few crowd boxes, json `area` fields): times coco_box_ap on a subsample (extrapolated linearly to the split),
then DeviceCOCOBoxEvaluator.evaluate() on the whole split (one warm-up, the median of 5), checks the device precision / recall arrays
against coco_box_eval's with np.array_equal and prints one JSON line.

    python tools/bench_eval.py [--images 5000] [--host-images 1000] [--check-images 5000]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unbiased-teacher-v2_amd"))


def make_split(n_images, num_classes=80, seed=0):
    """dataset dicts (XYXY_ABS annotations) + the model outputs as host arrays, image ids in dataset order"""
    rng = np.random.default_rng(seed)
    dicts, preds = [], {}
    for i in range(n_images):
        W, H = float(rng.integers(320, 640)), float(rng.integers(320, 640))
        ng = int(rng.integers(1, 15))
        xy = rng.uniform(0, 1, (ng, 2)) * [W * 0.9, H * 0.9]
        wh = rng.uniform(1, 4, (ng, 2)) * rng.choice([8, 40, 160], (ng, 1)) + 2
        gb = np.concatenate([xy, np.minimum(xy + wh, [W, H])], 1)
        gc = rng.integers(0, num_classes, ng)
        crowd = rng.random(ng) < 0.01
        annos = [{"bbox": gb[j].tolist(), "bbox_mode": "XYXY_ABS", "category_id": int(gc[j]), "iscrowd": int(crowd[j]),
                  "area": float((gb[j, 2] - gb[j, 0]) * (gb[j, 3] - gb[j, 1]) * rng.uniform(0.5, 1.0))} for j in range(ng)]
        dicts.append({"image_id": i, "height": int(H), "width": int(W), "annotations": annos})
        nd = 100
        ncopy = min(3 * ng, 40)
        src = rng.integers(0, ng, ncopy)
        b1 = gb[src] + rng.normal(0, 1, (ncopy, 4)) * wh[src][:, [0, 1, 0, 1]] * 0.1
        c1 = np.where(rng.random(ncopy) < 0.8, gc[src], rng.integers(0, num_classes, ncopy))
        xy = rng.uniform(0, 1, (nd - ncopy, 2)) * [W, H]
        b2 = np.concatenate([xy, xy + rng.uniform(4, 200, (nd - ncopy, 2))], 1)
        boxes = np.concatenate([b1, b2]).astype(np.float32)
        boxes[:, 2:] = np.maximum(boxes[:, 2:], boxes[:, :2])
        scores = np.sort(rng.uniform(0.05, 1.0, nd))[::-1].astype(np.float32)
        preds[i] = dict(boxes=boxes, scores=scores, classes=np.concatenate([c1, rng.integers(0, num_classes, nd - ncopy)]).astype(np.int64))
    return dicts, preds


def host_gt(dicts):
    """COCOBoxEvaluator's ground-truth dicts of the split"""
    return {d["image_id"]: dict(boxes=np.asarray([a["bbox"] for a in d["annotations"]], float).reshape(-1, 4),
                                classes=np.asarray([a["category_id"] for a in d["annotations"]], np.int64),
                                iscrowd=np.asarray([a["iscrowd"] for a in d["annotations"]], bool),
                                area=np.asarray([a["area"] for a in d["annotations"]], float)) for d in dicts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--host-images", type=int, default=1000, help="images of the timed coco_box_ap run (extrapolated to --images)")
    ap.add_argument("--check-images", type=int, default=5000, help="images of the array comparison against coco_box_eval (0: none)")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    from ubteacher.d2.structures import Boxes, Instances
    from ubteacher.data import DatasetCatalog, MetadataCatalog
    from ubteacher.evaluation import DeviceCOCOBoxEvaluator, coco_box_ap, coco_box_eval

    K = 80
    dicts, preds = make_split(args.images, K)
    gt = host_gt(dicts)
    name = "bench_eval_synthetic_%d" % os.getpid()
    DatasetCatalog.register(name, lambda: dicts)
    MetadataCatalog.get(name).set(thing_classes=["c%d" % k for k in range(K)])

    nh = min(args.host_images, args.images)
    sub = dict(list(gt.items())[:nh])
    t0 = time.perf_counter()
    coco_box_ap(preds, sub, K)
    host_s = (time.perf_counter() - t0) * args.images / nh

    dev = torch.device("cuda", 0)
    ev = DeviceCOCOBoxEvaluator(K, dataset_name=name, device=dev)
    for lo in range(0, args.images, 8):
        ins, outs = [], []
        for d in dicts[lo:lo + 8]:
            p = preds[d["image_id"]]
            inst = Instances((d["height"], d["width"]))
            inst.pred_boxes = Boxes(torch.from_numpy(p["boxes"]).to(dev))
            inst.scores = torch.from_numpy(p["scores"].copy()).to(dev)
            inst.pred_classes = torch.from_numpy(p["classes"]).to(dev)
            ins.append({"image_id": d["image_id"], "height": d["height"], "width": d["width"]})
            outs.append({"instances": inst})
        ev.process(ins, outs)
    torch.cuda.synchronize()
    res = ev.evaluate()["bbox"]                       # warm-up (library load, first launches)
    times = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ev.evaluate()["bbox"]
        times.append(time.perf_counter() - t0)
    dev_s = statistics.median(times)

    out = {"metric": "coco_box_eval", "images": args.images, "classes": K,
           "detections": int(sum(len(p["scores"]) for p in preds.values())), "gt": int(sum(len(g["classes"]) for g in gt.values())),
           "host_coco_box_ap_s": round(host_s, 3), "host_timed_images": nh, "device_evaluate_s": round(dev_s, 4),
           "device_evaluate_all_s": [round(t, 4) for t in times], "speedup": round(host_s / dev_s, 1), "AP": res["AP"], "AR100": res["AR100"]}
    if args.check_images:
        nc = min(args.check_images, args.images)
        if nc < args.images:
            ev2 = DeviceCOCOBoxEvaluator(K, dataset_name=name, device=dev)
            ev2._ids, ev2._det = ev._ids[:nc], ev._det[:nc]
            ev2.evaluate()
            p_dev, r_dev = ev2.precision, ev2.recall
        else:
            p_dev, r_dev = ev.precision, ev.recall
        t0 = time.perf_counter()
        p_host, r_host, s_host = coco_box_eval(preds, dict(list(gt.items())[:nc]), K)
        out["host_coco_box_eval_s"] = round(time.perf_counter() - t0, 3)
        out["checked_images"] = nc
        out["precision_equal"] = bool(np.array_equal(p_dev, p_host))
        out["recall_equal"] = bool(np.array_equal(r_dev, r_host))
        if nc == args.images:
            out["six_equal"] = all(res[k] == s_host[k] for k in ("AP", "AP50", "AP75", "APs", "APm", "APl"))
    print(json.dumps(out))
    DatasetCatalog.remove(name)
    ok = out.get("precision_equal", True) and out.get("recall_equal", True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
