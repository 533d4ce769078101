"""Host reference of the full COCO box evaluation (evaluation/coco_eval.py:coco_box_eval): its six AP numbers are coco_box_ap's bit for
bit, and known answers pin the recall summary (pycocotools' AR) and the per-class AP (Detectron2's `AP-<name>`).  make_split() is the
random split generator the device test (test_coco_eval_device_gpu.py) shares."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unbiased-teacher-v2_amd"))


def make_split(seed, n_images=30, num_classes=6, gt_max=8, det_max=40, tie_scores=False, crowd_p=0.0, json_area=False, big_pair=0,
               many_gt=0, empty_p=0.0, foreign_classes=False, zero_area=False):
    """(predictions, ground_truth) in coco_box_ap's input format, fp32 detections as a model emits them.
    tie_scores: scores quantised to 0.1; big_pair: one (image, class) pair with that many detections; many_gt: one image with that many
    ground-truth boxes of class 0; empty_p: share of images without ground truth / without detections; foreign_classes: detections of
    classes >= num_classes and of a class without ground truth; zero_area: degenerate boxes in both."""
    rng = np.random.default_rng(seed)
    gt_classes = num_classes - 1 if foreign_classes else num_classes      # the last class never has ground truth then
    preds, gts = {}, {}
    for i in range(n_images):
        iid = int(rng.integers(0, 10 ** 6)) * 1000 + i                    # ids in no particular order
        W, H = float(rng.uniform(100, 800)), float(rng.uniform(100, 800))
        ng = int(rng.integers(0, gt_max + 1))
        if empty_p and rng.random() < empty_p:
            ng = 0
        if many_gt and i == 0:
            ng = many_gt
        xy = rng.uniform(0, 1, (ng, 2)) * [W, H]
        wh = rng.uniform(2, 300, (ng, 2)) * rng.choice([0.05, 0.3, 1.0], (ng, 1))
        gb = np.concatenate([xy, xy + wh], 1)
        gc = rng.integers(0, gt_classes, ng) if not (many_gt and i == 0) else np.zeros(ng, np.int64)
        if zero_area and ng:
            gb[0, 2] = gb[0, 0]
        g = dict(boxes=gb, classes=gc.astype(np.int64))
        if crowd_p:
            g["iscrowd"] = rng.random(ng) < crowd_p
        if json_area and rng.random() < 0.7:
            g["area"] = ((gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1])) * rng.uniform(0.3, 1.2, ng)
        gts[iid] = g
        nd = int(rng.integers(0, det_max + 1))
        if empty_p and rng.random() < empty_p:
            nd = 0
        # jittered copies of the ground truth (matches at many IoUs) + random boxes
        ncopy = min(ng, nd // 2) if ng else 0
        src = rng.integers(0, max(ng, 1), ncopy)
        jit = rng.normal(0, 1, (ncopy, 4)) * np.maximum(wh[src][:, [0, 1, 0, 1]], 1) * rng.choice([0.02, 0.1, 0.3], (ncopy, 1)) if ng else np.zeros((0, 4))
        b1 = gb[src] + jit if ng else np.zeros((0, 4))
        c1 = gc[src] if ng else np.zeros(0, np.int64)
        nr = nd - ncopy
        xy = rng.uniform(0, 1, (nr, 2)) * [W, H]
        b2 = np.concatenate([xy, xy + rng.uniform(1, 250, (nr, 2))], 1)
        c2 = rng.integers(0, num_classes + (2 if foreign_classes else 0), nr)
        boxes = np.concatenate([b1, b2]).reshape(-1, 4)
        boxes[:, 2:] = np.maximum(boxes[:, 2:], boxes[:, :2])
        cls = np.concatenate([c1, c2]).astype(np.int64)
        if big_pair and i == n_images // 2:
            xy = rng.uniform(0, 1, (big_pair, 2)) * [W, H]
            boxes = np.concatenate([boxes, np.concatenate([xy, xy + rng.uniform(5, 200, (big_pair, 2))], 1)])
            cls = np.concatenate([cls, np.full(big_pair, 1)])
            if ng:
                boxes[-1] = gb[0]
        if zero_area and len(boxes):
            boxes[-1, 3] = boxes[-1, 1]
        scores = rng.uniform(0.01, 1.0, len(cls))
        if tie_scores:
            scores = np.round(scores * 10) / 10
        preds[iid] = dict(boxes=boxes.astype(np.float32), scores=scores.astype(np.float32), classes=cls)
    return preds, gts


SPLITS = [
    dict(seed=1),
    dict(seed=2, tie_scores=True),
    dict(seed=3, crowd_p=0.2, json_area=True),
    dict(seed=4, big_pair=140, det_max=20),
    dict(seed=5, many_gt=90, gt_max=4),
    dict(seed=6, empty_p=0.3, foreign_classes=True),
    dict(seed=7, zero_area=True, tie_scores=True, crowd_p=0.1),
]


@pytest.mark.parametrize("kw", SPLITS, ids=[str(k["seed"]) for k in SPLITS])
def test_six_numbers_equal_coco_box_ap(kw):
    from ubteacher.evaluation import coco_box_ap, coco_box_eval
    pred, gt = make_split(n_images=12, **kw)
    prec, rec, stats = coco_box_eval(pred, gt, 6)
    assert prec.shape == (10, 101, 6, 4) and rec.shape == (10, 6, 4, 3)
    ref = coco_box_ap(pred, gt, 6)
    for k, v in ref.items():
        assert stats[k] == v, (k, stats[k], v)        # bit for bit
    assert ((rec == -1) | ((rec >= 0) & (rec <= 1))).all()
    assert (rec[..., 0] <= rec[..., 1]).all() and (rec[..., 1] <= rec[..., 2]).all()


def _box_pred(boxes, classes, scores=None):
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    return dict(boxes=boxes, classes=np.asarray(classes, np.int64),
                scores=np.asarray(scores if scores is not None else np.linspace(0.9, 0.5, len(boxes)), np.float32))


def test_perfect_detections_give_ar_100():
    from ubteacher.evaluation import coco_box_eval
    gt = {1: dict(boxes=np.array([[0, 0, 10, 10], [20, 20, 60, 50.0]]), classes=np.array([0, 1])),
          2: dict(boxes=np.array([[5, 5, 200, 150.0]]), classes=np.array([1]))}
    pred = {k: _box_pred(v["boxes"], v["classes"]) for k, v in gt.items()}
    _, _, s = coco_box_eval(pred, gt, 2)
    assert s["AP"] == 100.0 and s["AR1"] == 100.0 and s["AR10"] == 100.0 and s["AR100"] == 100.0
    assert s["ARs"] == 100.0 and s["ARm"] == 100.0 and s["ARl"] == 100.0


def test_two_boxes_one_detection_give_ar1_50():
    from ubteacher.evaluation import coco_box_eval
    gt = {1: dict(boxes=np.array([[0, 0, 10, 10], [50, 50, 70, 70.0]]), classes=np.array([0, 0]))}
    pred = {1: _box_pred([[0, 0, 10, 10], [50, 50, 70, 70]], [0, 0], [0.9, 0.8])}
    _, rec, s = coco_box_eval(pred, gt, 1)
    assert s["AR1"] == 50.0 and s["AR10"] == 100.0 and s["AR100"] == 100.0
    assert (rec[:, 0, 0, 0] == 0.5).all()
    pred = {1: _box_pred([[0, 0, 10, 10]], [0])}
    _, _, s = coco_box_eval(pred, gt, 1)
    assert s["AR1"] == 50.0 and s["AR100"] == 50.0


def test_per_class_ap_and_nan_for_a_class_without_ground_truth():
    from ubteacher.evaluation import coco_box_eval
    from ubteacher.evaluation.coco_eval import summarize
    gt = {1: dict(boxes=np.array([[0, 0, 10, 10], [30, 30, 40, 40.0]]), classes=np.array([0, 1]))}
    pred = {1: _box_pred([[0, 0, 10, 10], [100, 100, 120, 120], [1, 1, 5, 5]], [0, 1, 2])}
    prec, rec, s = coco_box_eval(pred, gt, 3)
    named = summarize(prec, rec, ["a", "b", "c"])
    assert named["AP-a"] == 100.0 and named["AP-b"] == 0.0 and math.isnan(named["AP-c"])
    assert s["AP-0"] == 100.0 and s["AP-1"] == 0.0 and math.isnan(s["AP-2"])
    assert s["AP"] == 50.0 and s["AR100"] == 50.0
    assert (prec[:, :, 2, :] == -1).all() and (rec[:, 2] == -1).all()
