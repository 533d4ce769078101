"""An independent oracle of the COCO box protocol for the tests (numpy and the standard library only), written from the published
pycocotools COCOeval in that program's own shape: evaluate_img() per (image, category, area range) returns dtm / gtm / dtIg / gtIg,
accumulate() runs over them, the recall summary is rc[-1] at maxDets 1 / 10 / 100.  It shares no code with evaluation/coco_eval.py and
exists to disagree with that file (and with csrc/coco_eval.hip) where they are wrong.

Boxes are xyxy.  The tests feed it small-integer coordinates and areas only: every quantity before the one IoU division and before
tp / npig and tp / (tp + fp) is then exact in fp64 and each division is correctly rounded, so any correct implementation gives the same
bits in any operation order and every comparison against this file is `==`.

structured_split() is the random generator of the tests: integer boxes on a coarse grid, scores from a small set, so equal IoUs, equal
scores, IoUs on a threshold and areas on a range edge are frequent."""
import numpy as np

IOU_THRS = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)
REC_THRS = np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True)
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]   # all, small, medium, large
MAX_DETS = [1, 10, 100]


def match_start(t):
    """the IoU a detection has to reach at threshold t: a threshold of 1 is met by an IoU of 1 - 1e-10"""
    return min([t, 1 - 1e-10])


def score_order(scores):
    """indices by descending score, equal scores (+0 and -0 are equal) in input order"""
    return np.argsort([-float(s) for s in scores], kind="mergesort")


def bb_iou(d, g, crowd):
    """IoU of two xyxy boxes; against a crowd box the union is the detection's own area.  No overlap (also: a degenerate box) is 0."""
    w = min(d[2], g[2]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[3], g[3]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    da = (d[2] - d[0]) * (d[3] - d[1])
    ga = (g[2] - g[0]) * (g[3] - g[1])
    u = da if crowd else da + ga - i
    return i / u


def evaluate_img(dt, gt, a_rng, max_det, iou_thrs):
    """dt: [dict(id, bbox, score, area)], gt: [dict(id > 0, bbox, area, iscrowd)] of one image and category.  None without both."""
    if len(gt) == 0 and len(dt) == 0:
        return None
    ignore = [1 if (g["iscrowd"] or g["area"] < a_rng[0] or g["area"] > a_rng[1]) else 0 for g in gt]
    gtind = np.argsort(ignore, kind="mergesort")
    gt = [gt[i] for i in gtind]
    dtind = score_order([d["score"] for d in dt])
    dt = [dt[i] for i in dtind[0:max_det]]
    iscrowd = [int(g["iscrowd"]) for g in gt]
    ious = [[bb_iou(d["bbox"], g["bbox"], g["iscrowd"]) for g in gt] for d in dt]
    T, G, D = len(iou_thrs), len(gt), len(dt)
    gtm = np.zeros((T, G), np.int64)
    dtm = np.zeros((T, D), np.int64)
    gt_ig = np.array([ignore[i] for i in gtind], np.int64)
    dt_ig = np.zeros((T, D), bool)
    for tind, t in enumerate(iou_thrs):
        for dind, d in enumerate(dt):
            iou = match_start(t)
            m = -1
            for gind in range(G):
                if gtm[tind, gind] > 0 and not iscrowd[gind]:
                    continue
                if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                    break
                if ious[dind][gind] < iou:
                    continue
                iou = ious[dind][gind]
                m = gind
            if m == -1:
                continue
            dt_ig[tind, dind] = gt_ig[m]
            dtm[tind, dind] = gt[m]["id"]
            gtm[tind, m] = d["id"]
    a = np.array([d["area"] < a_rng[0] or d["area"] > a_rng[1] for d in dt], bool).reshape(1, D)
    dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
    return dict(dtIds=[d["id"] for d in dt], gtIds=[g["id"] for g in gt], dtMatches=dtm, gtMatches=gtm,
                dtScores=np.array([float(d["score"]) for d in dt]), gtIgnore=gt_ig, dtIgnore=dt_ig)


def accumulate(eval_imgs, num_classes, n_images, iou_thrs, rec_thrs, max_dets, n_areas):
    """eval_imgs[(k, a, i)] -> precision [T, R, K, A, M], recall [T, K, A, M]; -1 where there is no non-ignored ground truth"""
    T, R, K, A, M = len(iou_thrs), len(rec_thrs), num_classes, n_areas, len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    for k in range(K):
        for a in range(A):
            for m, max_det in enumerate(max_dets):
                E = [eval_imgs[(k, a, i)] for i in range(n_images)]
                E = [e for e in E if e is not None]
                if len(E) == 0:
                    continue
                dt_scores = np.concatenate([e["dtScores"][0:max_det] for e in E])
                inds = np.argsort(-dt_scores, kind="mergesort")
                dtm = np.concatenate([e["dtMatches"][:, 0:max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dtIgnore"][:, 0:max_det] for e in E], axis=1)[:, inds]
                gt_ig = np.concatenate([e["gtIgnore"] for e in E])
                npig = np.count_nonzero(gt_ig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / np.maximum(tp + fp, np.spacing(1))
                    q = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds_r = np.searchsorted(rc, rec_thrs, side="left")
                    for ri, pi in enumerate(inds_r):
                        if pi < nd:
                            q[ri] = pr[pi]
                    precision[t, :, k, a, m] = q
    return precision, recall


def _mean(x):
    x = x[x > -1]
    return float(np.mean(x) * 100.0) if x.size else -1.0


def evaluate(predictions, ground_truth, num_classes, iou_thrs=None, rec_thrs=None, area_rng=None, max_dets=None):
    """predictions {image: dict(boxes [D, 4], scores [D], classes [D])}, ground_truth {image: dict(boxes [G, 4], classes [G], iscrowd [G]
    optional, area [G] optional)}; images are scored in ground_truth's order and only those.  Returns a dict:
      precision [T, R, K, A] (maxDets 100), recall [T, K, A, 3] (maxDets 1 / 10 / 100),
      matched / ignored {image: bool [D, A, T]} and scored {image: bool [D]} in the image's own detection order (a detection of a class
      outside [0, K) or beyond its pair's 100 best is not scored and has no bits),
      stats: AP, AP50, AP75, APs, APm, APl, AR1, AR10, AR100, ARs, ARm, ARl in percent."""
    iou_thrs = IOU_THRS if iou_thrs is None else np.asarray(iou_thrs, float)
    rec_thrs = REC_THRS if rec_thrs is None else np.asarray(rec_thrs, float)
    area_rng = AREA_RNG if area_rng is None else area_rng
    max_dets = MAX_DETS if max_dets is None else list(max_dets)
    K, T, A = int(num_classes), len(iou_thrs), len(area_rng)
    images = list(ground_truth.keys())
    gts, dts = {}, {}
    matched, ignored, scored = {}, {}, {}
    for i, img in enumerate(images):
        g = ground_truth[img]
        gb = np.asarray(g["boxes"], float).reshape(-1, 4)
        gc = np.asarray(g["classes"]).reshape(-1)
        crowd = np.asarray(g["iscrowd"]).reshape(-1) if g.get("iscrowd") is not None else np.zeros(len(gc))
        area = np.asarray(g["area"], float).reshape(-1) if g.get("area") is not None else None
        for j in range(len(gc)):
            b = [float(v) for v in gb[j]]
            ann = dict(id=j + 1, bbox=b, iscrowd=bool(crowd[j]), area=float(area[j]) if area is not None else (b[2] - b[0]) * (b[3] - b[1]))
            gts.setdefault((i, int(gc[j])), []).append(ann)
        p = predictions.get(img)
        n = len(np.asarray(p["classes"]).reshape(-1)) if p is not None else 0
        if n:
            pb = np.asarray(p["boxes"], float).reshape(-1, 4)
            ps = np.asarray(p["scores"]).reshape(-1)
            pc = np.asarray(p["classes"]).reshape(-1)
            for j in range(n):
                b = [float(v) for v in pb[j]]
                dts.setdefault((i, int(pc[j])), []).append(dict(id=j + 1, bbox=b, score=float(ps[j]), area=(b[2] - b[0]) * (b[3] - b[1])))
        matched[img] = np.zeros((n, A, T), bool)
        ignored[img] = np.zeros((n, A, T), bool)
        scored[img] = np.zeros(n, bool)
    eval_imgs = {}
    for k in range(K):
        for a, rng in enumerate(area_rng):
            for i, img in enumerate(images):
                e = evaluate_img(dts.get((i, k), []), gts.get((i, k), []), rng, max_dets[-1], iou_thrs)
                eval_imgs[(k, a, i)] = e
                if e is None:
                    continue
                for pos, did in enumerate(e["dtIds"]):
                    scored[img][did - 1] = True
                    matched[img][did - 1, a, :] = e["dtMatches"][:, pos] > 0
                    ignored[img][did - 1, a, :] = e["dtIgnore"][:, pos]
    precision, recall = accumulate(eval_imgs, K, len(images), iou_thrs, rec_thrs, max_dets, A)
    precision = precision[..., -1]
    stats = {}
    if T == 10 and A == 4 and len(max_dets) == 3:
        stats = {"AP": _mean(precision[..., 0]), "AP50": _mean(precision[0:1, ..., 0]), "AP75": _mean(precision[5:6, ..., 0]),
                 "APs": _mean(precision[..., 1]), "APm": _mean(precision[..., 2]), "APl": _mean(precision[..., 3]),
                 "AR1": _mean(recall[:, :, 0, 0]), "AR10": _mean(recall[:, :, 0, 1]), "AR100": _mean(recall[:, :, 0, 2]),
                 "ARs": _mean(recall[:, :, 1, 2]), "ARm": _mean(recall[:, :, 2, 2]), "ARl": _mean(recall[:, :, 3, 2])}
    return dict(precision=precision, recall=recall, matched=matched, ignored=ignored, scored=scored, stats=stats)


SIX = ("AP", "AP50", "AP75", "APs", "APm", "APl")


def structured_split(seed, n_images=16, num_classes=4):
    """(predictions, ground_truth): integer boxes on a grid of 4, sides from a set that holds 32 and 96 (areas on both range edges),
    detections that are a ground-truth box cut to k / 20 of its width (IoUs on the thresholds), exact copies and free boxes; scores from
    eight values; crowd flags; an `area` field on about half of the images, on or next to a range edge at times; images without ground
    truth and without detections; classes outside [0, num_classes) in both."""
    rng = np.random.default_rng(seed)
    sides = np.array([8, 16, 20, 32, 40, 60, 96, 100])
    score_set = np.array([0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0], np.float32)
    preds, gts = {}, {}
    for i in range(n_images):
        iid = 1000 - 7 * i if i % 2 else 10 * i           # ids in no particular order
        ng = 0 if rng.random() < 0.15 else int(rng.integers(1, 7))
        xy = 4 * rng.integers(0, 48, (ng, 2))
        wh = np.stack([rng.choice(sides, ng), rng.choice(sides, ng)], 1) if ng else np.zeros((0, 2), np.int64)
        gb = np.concatenate([xy, xy + wh], 1).astype(np.float64).reshape(-1, 4)
        gc = rng.integers(0, num_classes + 1, ng) if rng.random() < 0.2 else rng.integers(0, num_classes, ng)
        g = dict(boxes=gb, classes=gc.astype(np.int64), iscrowd=rng.random(ng) < 0.15)
        if rng.random() < 0.5:
            box_area = (gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1])
            edge = rng.choice([32 ** 2 - 1, 32 ** 2, 32 ** 2 + 1, 96 ** 2 - 1, 96 ** 2, 96 ** 2 + 1], ng).astype(np.float64)
            g["area"] = np.where(rng.random(ng) < 0.3, edge, box_area + rng.integers(-1, 2, ng))
        gts[iid] = g
        if rng.random() < 0.15:
            continue                                       # no entry in predictions at all
        boxes, cls = [], []
        for j in range(ng):
            for _ in range(int(rng.integers(0, 4))):
                b = gb[j].copy()
                kind = rng.random()
                if kind < 0.5 and wh[j, 0] % 20 == 0:      # k / 20 of the width
                    b[2] = b[0] + (wh[j, 0] // 20) * int(rng.integers(9, 21))
                elif kind < 0.7:
                    b[[0, 2]] += 4 * int(rng.integers(-2, 3))
                boxes.append(b)
                cls.append(int(gc[j]) if rng.random() < 0.9 else int(rng.integers(-1, num_classes + 2)))
        for _ in range(int(rng.integers(0, 5))):
            x, y = 4 * rng.integers(0, 48, 2)
            boxes.append(np.array([x, y, x + rng.choice(sides), y + rng.choice(sides)], np.float64))
            cls.append(int(rng.integers(-1, num_classes + 2)))
        if rng.random() < 0.1:
            boxes, cls = [], []                            # an entry without detections
        n = len(boxes)
        preds[iid] = dict(boxes=np.asarray(boxes, np.float32).reshape(-1, 4), scores=rng.choice(score_set, n).astype(np.float32),
                          classes=np.asarray(cls, np.int64).reshape(-1))
    return preds, gts
