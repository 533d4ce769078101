"""The COCO box protocol at its decision points, on the host: hand-written known answers asserted on the independent oracle
(tests/coco_ref.py), then evaluation/coco_eval.py:coco_box_eval asserted equal to the oracle, bit for bit, on every case and on
structured random splits.  All inputs are small integers, so every comparison is exact (see coco_ref's docstring).
CASES is shared with the device test (test_coco_eval_edges_gpu.py)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unbiased-teacher-v2_amd"))
sys.path.insert(0, ROOT)

from tests import coco_ref as ref  # noqa: E402

F32 = np.float32
ALL, SMALL, MEDIUM, LARGE = 0, 1, 2, 3


def image(dets, gts, area=False):
    """dets: [(box, score, class)], gts: [(box, class, crowd, area or None)] -> (prediction entry, ground-truth entry)"""
    p = dict(boxes=np.asarray([d[0] for d in dets], F32).reshape(-1, 4), scores=np.asarray([d[1] for d in dets], F32),
             classes=np.asarray([d[2] for d in dets], np.int64))
    g = dict(boxes=np.asarray([x[0] for x in gts], np.float64).reshape(-1, 4), classes=np.asarray([x[1] for x in gts], np.int64),
             iscrowd=np.asarray([x[2] for x in gts], bool))
    if area:
        g["area"] = np.asarray([x[3] for x in gts], np.float64)
    return p, g


def split(images):
    pred, gt = {}, {}
    for iid, (p, g) in images.items():
        gt[iid] = g
        if p is not None:
            pred[iid] = p
    return pred, gt


def bits(arr, img, d, a):
    """the ten threshold bits of detection d of an image at area range a, as a string"""
    return "".join("1" if v else "0" for v in arr[img][d, a])


def far(i):
    """a 10 x 10 box that overlaps nothing the cases place below x = 2000"""
    return [3000 + 20 * i, 3000, 3010 + 20 * i, 3010]


# ------------------------------------------------------------------------------------------------------------------------------------
# IoU exactly on each threshold, and one step under / over
def case_iou_thresholds():
    ims = {}
    for k in range(10, 20):
        ims["on%d" % k] = image([([0, 0, k, 20], 0.9, 0)], [([0, 0, 20, 20], 0, 0, None)])                       # k / 20
        ims["under%d" % k] = image([([0, 0, 10 * k - 1, 1], 0.8, 0)], [([0, 0, 200, 1], 0, 0, None)])             # (10 k - 1) / 200
        ims["over%d" % k] = image([([0, 0, 10 * k + 1, 1], 0.7, 0)], [([0, 0, 200, 1], 0, 0, None)])              # (10 k + 1) / 200
    ims["one"] = image([([4, 4, 24, 24], 0.6, 0)], [([4, 4, 24, 24], 0, 0, None)])                                # 1
    return split(ims) + (1,)


HITS_ON = {10: "1000000000", 11: "1100000000", 12: "1110000000", 13: "1111000000", 14: "1111100000", 15: "1111110000",
           16: "1111111000", 17: "1111111100", 18: "1111111110", 19: "1111111111"}     # 18: 9 / 10 is a hit at "0.90"
HITS_UNDER = {10: "0000000000", 11: "1000000000", 12: "1100000000", 13: "1110000000", 14: "1111000000", 15: "1111100000",
              16: "1111110000", 17: "1111111000", 18: "1111111100", 19: "1111111110"}


def check_iou_thresholds(r):
    assert ref.IOU_THRS[8] == 0.8999999999999999 and ref.IOU_THRS[8] < 0.9 and 18 / 20 == 0.9
    assert all(ref.IOU_THRS[j] == (10 + j) / 20 for j in range(10) if j != 8)
    for k in range(10, 20):
        for a in (ALL, SMALL):
            assert bits(r["matched"], "on%d" % k, 0, a) == HITS_ON[k], k
            assert bits(r["matched"], "under%d" % k, 0, a) == HITS_UNDER[k], k
            assert bits(r["matched"], "over%d" % k, 0, a) == HITS_ON[k], k
            assert bits(r["ignored"], "on%d" % k, 0, a) == "0000000000"
        for a in (MEDIUM, LARGE):           # the ground truth is small: ignored there, and so is what it matches or what misses it
            assert bits(r["matched"], "on%d" % k, 0, a) == HITS_ON[k]
            assert bits(r["ignored"], "on%d" % k, 0, a) == "1111111111"
    assert bits(r["matched"], "one", 0, ALL) == "1111111111"
    # 31 ground-truth boxes; the hits at threshold j: 10 - j on, 9 - j under, 10 - j over, and the IoU of 1
    hits = [30, 27, 24, 21, 18, 15, 12, 9, 6, 3]
    for j in range(10):
        assert r["recall"][j, 0, ALL, 2] == hits[j] / 31 and r["recall"][j, 0, SMALL, 2] == hits[j] / 31
        assert r["recall"][j, 0, MEDIUM, 2] == -1 and r["recall"][j, 0, LARGE, 2] == -1
        assert r["recall"][j, 0, ALL, 0] == hits[j] / 31          # one detection per pair: every one has rank 0


def test_threshold_of_one_is_met_by_an_iou_of_one():
    assert ref.match_start(1.0) == 1 - 1e-10 and ref.match_start(0.95) == 0.95
    pred, gt, K = case_iou_thresholds()
    thrs = list(ref.IOU_THRS[:9]) + [1.0]
    r = ref.evaluate(pred, gt, K, iou_thrs=thrs)
    assert bits(r["matched"], "one", 0, ALL) == "1111111111"
    assert bits(r["matched"], "on19", 0, ALL) == "1111111110"


# ------------------------------------------------------------------------------------------------------------------------------------
# equal IoU to two free ground-truth boxes: the later one is taken; the next detection takes the earlier
def case_equal_iou():
    dets = [([0, 0, 20, 10], 0.9, 0),      # A: IoU 120 / 200 = 0.6 with both
            ([8, 0, 20, 10], 0.8, 0),      # B: the second box exactly (IoU 0.2 with the first)
            ([0, 0, 20, 10], 0.7, 0)]      # C: as A
    gts = [([0, 0, 12, 10], 0, 0, None), ([8, 0, 20, 10], 0, 0, None)]
    return split({"i": image(dets, gts)}) + (1,)


def check_equal_iou(r):
    for a in (ALL, SMALL):
        assert bits(r["matched"], "i", 0, a) == "1110000000"     # A takes the second box up to 0.60 ...
        assert bits(r["matched"], "i", 1, a) == "0001111111"     # ... so B finds it taken there, and free above
        assert bits(r["matched"], "i", 2, a) == "1110000000"     # C takes the first
        for d in range(3):
            assert bits(r["ignored"], "i", d, a) == "0000000000"
    for a in (MEDIUM, LARGE):               # both boxes ignored (area 120): same matches, everything ignored (the detections are small too)
        assert bits(r["matched"], "i", 0, a) == "1110000000" and bits(r["matched"], "i", 1, a) == "0001111111"
        for d in range(3):
            assert bits(r["ignored"], "i", d, a) == "1111111111"
    P, R = r["precision"], r["recall"]
    for t in range(3):                      # TP FP TP over 2 boxes: pr 1, 1/2, 2/3 -> envelope 1, 2/3, 2/3; rc 1/2, 1/2, 1
        assert np.array_equal(P[t, :51, 0, ALL], np.full(51, 1.0)) and np.array_equal(P[t, 51:, 0, ALL], np.full(50, 2 / 3))
        assert list(R[t, 0, ALL]) == [0.5, 1.0, 1.0]
    for t in range(3, 10):                  # FP TP FP: pr 0, 1/2, 1/3 -> envelope 1/2, 1/2, 1/3; rc 0, 1/2, 1/2
        assert np.array_equal(P[t, :51, 0, ALL], np.full(51, 0.5)) and np.array_equal(P[t, 51:, 0, ALL], np.zeros(50))
        assert list(R[t, 0, ALL]) == [0.0, 0.5, 0.5]
    assert np.all(P[:, :, 0, MEDIUM] == -1) and np.all(R[:, 0, LARGE] == -1)


# ------------------------------------------------------------------------------------------------------------------------------------
# the break rule: a regular match is not traded for an ignored box of higher IoU
def case_break_rule():
    det = [([0, 0, 20, 10], 0.9, 0)]
    ims = {"area": image(det, [([0, 0, 18, 10], 0, 0, 2000), ([0, 0, 12, 10], 0, 0, 120)], area=True),   # IoU 0.9 (medium by its field), 0.6
           "crowd": image(det, [([0, 0, 18, 10], 0, 1, 180), ([0, 0, 12, 10], 0, 0, 120)], area=True),   # crowd: 180 / 200 = 0.9
           "only": image(det, [([0, 0, 18, 10], 0, 1, 180)], area=True)}
    return split(ims) + (1,)


def check_break_rule(r):
    M, I = r["matched"], r["ignored"]
    # small: the 0.6 box is regular, the 0.9 box ignored: the regular match is kept to 0.60, the ignored box is taken to 0.90
    assert bits(M, "area", 0, SMALL) == "1111111110" and bits(I, "area", 0, SMALL) == "0001111110"
    assert bits(M, "area", 0, ALL) == "1111111110" and bits(I, "area", 0, ALL) == "0000000000"          # both regular: the 0.9 box
    assert bits(M, "area", 0, MEDIUM) == "1111111110" and bits(I, "area", 0, MEDIUM) == "0000000001"    # 0.9 box regular; unmatched + small
    assert bits(M, "area", 0, LARGE) == "1111111110" and bits(I, "area", 0, LARGE) == "1111111111"
    for a in (ALL, SMALL):
        assert bits(M, "crowd", 0, a) == "1111111110" and bits(I, "crowd", 0, a) == "0001111110"
        assert bits(M, "only", 0, a) == "1111111110" and bits(I, "only", 0, a) == "1111111110"
    # small: 2 regular boxes (one per image), the detections of "area" and "crowd" are true positives to 0.60 and ignored or missing above
    for t in range(10):
        assert list(r["recall"][t, 0, SMALL]) == ([1.0, 1.0, 1.0] if t < 3 else [0.0, 0.0, 0.0])


# ------------------------------------------------------------------------------------------------------------------------------------
# crowd: IoU is inter / area(det), a crowd box takes any number of detections, all ignored, and never counts as ground truth
def case_crowd():
    dets = [([10, 10, 20, 20], 0.9, 0), ([30, 30, 40, 40], 0.8, 0), ([0, 0, 10, 10], 0.7, 0)]
    gts = [([0, 0, 100, 100], 0, 1, None), ([200, 200, 210, 210], 0, 0, None)]
    return split({"i": image(dets, gts)}) + (1,)


def check_crowd(r):
    for d in range(3):
        for a in range(4):
            assert bits(r["matched"], "i", d, a) == "1111111111" and bits(r["ignored"], "i", d, a) == "1111111111"
    for a in (ALL, SMALL):                   # one regular box, no detection that counts: the np.spacing(1) denominator
        assert np.all(r["precision"][:, :, 0, a] == 0.0) and np.all(r["recall"][:, 0, a] == 0.0)
    for a in (MEDIUM, LARGE):                # the crowd box is 100 x 100 = large, and still no ground truth
        assert np.all(r["precision"][:, :, 0, a] == -1.0) and np.all(r["recall"][:, 0, a] == -1.0)


# ------------------------------------------------------------------------------------------------------------------------------------
# area edges: the ranges are closed on both sides
EDGE_BOXES = [(33, 31), (32, 32), (25, 41), (95, 97), (96, 96), (13, 709)]       # areas 1023, 1024, 1025, 9215, 9216, 9217
EDGE_IGNORED = ["0011", "0001", "0101", "0101", "0100", "0110"]                  # ignored in all / small / medium / large


def case_area_edges():
    boxes = [[100 * i, 0, 100 * i + w, h] for i, (w, h) in enumerate(EDGE_BOXES)]
    ims = {"gt": image([(b, 0.9 - 0.1 * i, 0) for i, b in enumerate(boxes)], [(b, 0, 0, None) for b in boxes]),
           "det": image([(b, 0.95 - 0.1 * i, 0) for i, b in enumerate(boxes)], [(far(0), 0, 0, None)]),
           # the field says large, the box is 32 x 32: the field decides on ignoring, the box on the IoU
           "field": image([([0, 0, 32, 32], 0.99, 0)], [([0, 0, 32, 32], 0, 0, 9217)], area=True)}
    return split(ims) + (1,)


def check_area_edges(r):
    assert [w * h for w, h in EDGE_BOXES] == [1023, 1024, 1025, 9215, 9216, 9217]
    for i in range(6):
        for a in range(4):
            ig = "1111111111" if EDGE_IGNORED[i][a] == "1" else "0000000000"
            assert bits(r["matched"], "gt", i, a) == "1111111111" and bits(r["ignored"], "gt", i, a) == ig, (i, a)
            assert bits(r["matched"], "det", i, a) == "0000000000" and bits(r["ignored"], "det", i, a) == ig, (i, a)
    for a, ig in enumerate("0110"):
        assert bits(r["matched"], "field", 0, a) == "1111111111"
        assert bits(r["ignored"], "field", 0, a) == ("1111111111" if ig == "1" else "0000000000")
    # non-ignored ground truth: all 6 + 1 + 1, small 2 + 1 + 0, medium 4 + 0 + 0, large 2 + 0 + 1; all but the far box are found
    for t in range(10):
        assert [r["recall"][t, 0, a, 2] for a in range(4)] == [7 / 8, 2 / 3, 1.0, 1.0]


# ------------------------------------------------------------------------------------------------------------------------------------
# the cut at 100 detections per pair, and the ranks < 1 / < 10 of the recall columns
def case_cut_100():
    g = [0, 0, 10, 10]
    fp = [(far(i % 50), F32(1.0) - F32(i) / 256, 0) for i in range(99)]
    tie = F32(0.25)
    dets, gts = [], [(g, c, 0, None) for c in range(6)]
    # class 0: the true positive is the 101st by input order among equal scores -> rank 100, dropped; class 1: the 100th, kept
    dets += [(b, s, 0) for b, s, _ in fp] + [(far(1), tie, 0), (g, tie, 0)]
    dets += [(b, s, 1) for b, s, _ in fp] + [(g, tie, 1), (far(1), tie, 1)]
    for c, rank in ((2, 0), (3, 1), (4, 9), (5, 10)):       # twelve detections, the true positive at that rank
        dets += [(g if i == rank else far(i), F32(0.75) - F32(i) / 64, c) for i in range(12)]
    return split({"i": image(dets, gts)}) + (6,)


def check_cut_100(r):
    sc, M, R, P = r["scored"]["i"], r["matched"], r["recall"], r["precision"]
    assert list(np.nonzero(~sc)[0]) == [100, 201]               # the 101st of classes 0 and 1
    assert bits(M, "i", 200, ALL) == "1111111111" and bits(M, "i", 99, ALL) == "0000000000"
    for t in range(10):
        assert list(R[t, 0, ALL]) == [0.0, 0.0, 0.0] and np.all(P[t, :, 0, ALL] == 0.0)
        assert list(R[t, 1, ALL]) == [0.0, 0.0, 1.0] and np.all(P[t, :, 1, ALL] == 1 / 100)
        assert list(R[t, 2, ALL]) == [1.0, 1.0, 1.0] and np.all(P[t, :, 2, ALL] == 1.0)
        assert list(R[t, 3, ALL]) == [0.0, 1.0, 1.0] and np.all(P[t, :, 3, ALL] == 1 / 2)
        assert list(R[t, 4, ALL]) == [0.0, 1.0, 1.0] and np.all(P[t, :, 4, ALL] == 1 / 10)
        assert list(R[t, 5, ALL]) == [0.0, 0.0, 1.0] and np.all(P[t, :, 5, ALL] == 1 / 11)


# ------------------------------------------------------------------------------------------------------------------------------------
# equal scores keep the image order in the class merge
def _tie_images(order):
    g = [0, 0, 10, 10]
    ims = {}
    for n, kind in enumerate(order):
        ims["i%d" % n] = image([(g, 0.5, 0)], [(g, 0, 0, None)]) if kind == "T" else image([(g, 0.5, 0)], [])
    return ims


def case_ties_tp_first():
    return split(_tie_images("TFT")) + (1,)


def case_ties_fp_first():
    return split(_tie_images("FTT")) + (1,)


def check_ties_tp_first(r):                   # tp 1 1 2, fp 0 1 1 over 2 boxes: envelope 1, 2/3, 2/3
    for t in range(10):
        assert np.array_equal(r["precision"][t, :, 0, ALL], np.concatenate([np.full(51, 1.0), np.full(50, 2 / 3)]))
        assert list(r["recall"][t, 0, ALL]) == [1.0, 1.0, 1.0]


def check_ties_fp_first(r):                   # tp 0 1 2, fp 1 1 1: pr 0, 1/2, 2/3 -> envelope 2/3 throughout
    for t in range(10):
        assert np.array_equal(r["precision"][t, :, 0, ALL], np.full(101, 2 / 3))


# ------------------------------------------------------------------------------------------------------------------------------------
# score order: descending, +0 and -0 tied in input order, one float32 ulp apart is apart
SCORE_LIST = [F32(-1.0), F32(-0.0), F32(2.0 ** -149), F32(np.inf), F32(0.0), F32(1.0), F32(-2.0 ** -149), F32(0.5),
              np.nextafter(F32(0.5), F32(1.0))]
SCORE_ORDER = [3, 5, 8, 7, 2, 1, 4, 6, 0]


def case_score_order():
    # the detection of even rank has its own ground-truth box, the one of odd rank has none: T F T F T F T F T in score order
    dets, gts = [], []
    rank = {d: p for p, d in enumerate(SCORE_ORDER)}
    for d, s in enumerate(SCORE_LIST):
        b = [40 * d, 0, 40 * d + 10, 10]
        dets.append((b, s, 0))
        if rank[d] % 2 == 0:
            gts.append((b, 0, 0, None))
    return split({"i": image(dets, gts)}) + (1,)


def check_score_order(r):
    assert list(ref.score_order(SCORE_LIST)) == SCORE_ORDER
    assert SCORE_LIST[8] > SCORE_LIST[7] and SCORE_LIST[8].view(np.uint32) - SCORE_LIST[7].view(np.uint32) == 1
    # tp 1 1 2 2 3 3 4 4 5, fp 0 1 1 2 2 3 3 4 4 over 5 boxes: pr 1 1/2 2/3 1/2 3/5 1/2 4/7 1/2 5/9 -> envelope 1 2/3 2/3 3/5 3/5 4/7 4/7 5/9 5/9
    want = np.concatenate([np.full(21, 1.0), np.full(20, 2 / 3), np.full(20, 3 / 5), np.full(20, 4 / 7), np.full(20, 5 / 9)])
    for t in range(10):
        assert np.array_equal(r["precision"][t, :, 0, ALL], want)


# ------------------------------------------------------------------------------------------------------------------------------------
# recall points: the fp64 doubles of linspace against tp / npig, not rational arithmetic
RECALL_CASES = [(10, 7), (20, 7), (20, 14), (20, 19), (3, 1), (3, 2)]
LAST_POINT = [69, 34, 69, 94, 33, 66]         # exact rationals would give 70, 35, 70, 95, 33, 66


def case_recall_points():
    dets, gts = [], []
    for c, (npig, tp) in enumerate(RECALL_CASES):
        for i in range(npig):
            b = [20 * i, 40 * c, 20 * i + 10, 40 * c + 10]
            gts.append((b, c, 0, None))
            if i < tp:
                dets.append((b, F32(1.0) - F32(i) / 64, c))
    return split({"i": image(dets, gts)}) + (len(RECALL_CASES),)


def check_recall_points(r):
    differ = [i for i in range(101) if ref.REC_THRS[i] != i / 100]
    assert differ == [35, 41, 47, 57, 69, 70, 82, 83, 94, 95]
    assert ref.REC_THRS[70] > 7 / 10 and ref.REC_THRS[35] > 7 / 20 and ref.REC_THRS[95] > 19 / 20
    for c, last in enumerate(LAST_POINT):
        for t in range(10):
            q = r["precision"][t, :, c, ALL]
            assert np.all(q[:last + 1] == 1.0) and np.all(q[last + 1:] == 0.0), (c, int(np.nonzero(q)[0][-1]))
            assert r["recall"][t, c, ALL, 2] == RECALL_CASES[c][1] / RECALL_CASES[c][0]


# ------------------------------------------------------------------------------------------------------------------------------------
# every detection ignored: tp + fp = 0 takes the np.spacing(1) denominator
def case_all_ignored():
    return split({"i": image([([1000, 1000, 1100, 1100], 0.9, 0)], [([0, 0, 10, 10], 0, 0, None)])}) + (1,)


def check_all_ignored(r):
    assert bits(r["matched"], "i", 0, SMALL) == "0000000000" and bits(r["ignored"], "i", 0, SMALL) == "1111111111"
    assert bits(r["ignored"], "i", 0, ALL) == "0000000000"
    for a in (ALL, SMALL):                   # small: nothing counts, 0 / spacing(1) = 0; all: one false positive
        assert np.all(r["precision"][:, :, 0, a] == 0.0) and np.all(r["recall"][:, 0, a] == 0.0)
    for a in (MEDIUM, LARGE):
        assert np.all(r["precision"][:, :, 0, a] == -1.0) and np.all(r["recall"][:, 0, a] == -1.0)


# ------------------------------------------------------------------------------------------------------------------------------------
# empty pairs, classes without ground truth, foreign classes, images without ground truth
def case_empty_and_foreign():
    g = [0, 0, 10, 10]
    ims = {"a": image([(g, 0.9, 2), (g, 0.8, 1), (g, 0.95, -1), (g, 0.95, 3), (g, 0.95, 7)],
                      [(g, 0, 0, None), (g, 2, 0, None), (g, 5, 0, None)]),
           "b": image([], [(g, 0, 0, None)])}
    pred, gt = split(ims)
    pred["not in the ground truth"] = dict(boxes=np.asarray([far(0)], F32), scores=np.asarray([1.0], F32), classes=np.asarray([2]))
    return pred, gt, 3


def check_empty_and_foreign(r):
    assert list(r["scored"]["a"]) == [True, True, False, False, False]
    assert np.all(r["precision"][:, :, 0, ALL] == 0.0) and np.all(r["recall"][:, 0, ALL] == 0.0)       # ground truth, no detections
    assert np.all(r["precision"][:, :, 1] == -1.0) and np.all(r["recall"][:, 1] == -1.0)               # detections, no ground truth
    assert np.all(r["precision"][:, :, 2, ALL] == 1.0) and np.all(r["recall"][:, 2, ALL] == 1.0)       # the unscored image's FP is absent
    assert r["stats"]["AP"] == 50.0 and r["stats"]["APs"] == 50.0 and r["stats"]["APm"] == -1.0


# ------------------------------------------------------------------------------------------------------------------------------------
# zero-area boxes: the union is 0, pycocotools' box IoU leaves 0 where there is no overlap; the host's and the device's 1e-12 floor of
# the union gives 0 / 1e-12 = 0 as well.  An area of 0 lies in "all" and "small" (closed at 0).
def case_zero_area():
    z = [5, 5, 5, 9]
    ims = {"i": image([(z, 0.9, 0), ([50, 50, 50, 50], 0.8, 0), ([120, 120, 120, 130], 0.7, 0)],
                      [(z, 0, 0, None), ([100, 100, 200, 200], 0, 1, None)])}
    return split(ims) + (1,)


def check_zero_area(r):
    for d in range(3):
        for a in range(4):
            assert bits(r["matched"], "i", d, a) == "0000000000"
            assert bits(r["ignored"], "i", d, a) == ("0000000000" if a in (ALL, SMALL) else "1111111111")
    for a in (ALL, SMALL):
        assert np.all(r["precision"][:, :, 0, a] == 0.0) and np.all(r["recall"][:, 0, a] == 0.0)
    for a in (MEDIUM, LARGE):
        assert np.all(r["precision"][:, :, 0, a] == -1.0)


CASES = {
    "iou_thresholds": (case_iou_thresholds, check_iou_thresholds),
    "equal_iou": (case_equal_iou, check_equal_iou),
    "break_rule": (case_break_rule, check_break_rule),
    "crowd": (case_crowd, check_crowd),
    "area_edges": (case_area_edges, check_area_edges),
    "cut_100": (case_cut_100, check_cut_100),
    "ties_tp_first": (case_ties_tp_first, check_ties_tp_first),
    "ties_fp_first": (case_ties_fp_first, check_ties_fp_first),
    "score_order": (case_score_order, check_score_order),
    "recall_points": (case_recall_points, check_recall_points),
    "all_ignored": (case_all_ignored, check_all_ignored),
    "empty_and_foreign": (case_empty_and_foreign, check_empty_and_foreign),
    "zero_area": (case_zero_area, check_zero_area),
}
SEEDS = [101, 102, 103, 104, 105, 106, 107]
_ORACLE = {}


def oracle(name):
    """(pred, gt, K, oracle result) of a known-answer case or of the structured split of a seed, computed once and left unchanged"""
    if name not in _ORACLE:
        pred, gt, K = CASES[name][0]() if name in CASES else ref.structured_split(name) + (4,)
        _ORACLE[name] = (pred, gt, K, ref.evaluate(pred, gt, K))
    return _ORACLE[name]


@pytest.mark.parametrize("name", list(CASES))
def test_known_answer_on_the_oracle(name):
    CASES[name][1](oracle(name)[3])


@pytest.mark.parametrize("name", list(CASES) + SEEDS)
def test_host_equals_oracle(name):
    from ubteacher.evaluation import coco_box_ap, coco_box_eval
    pred, gt, K, r = oracle(name)
    prec, rec, stats = coco_box_eval(pred, gt, K)
    assert np.array_equal(prec, r["precision"]), np.argwhere(prec != r["precision"])[:8]
    assert np.array_equal(rec, r["recall"]), np.argwhere(rec != r["recall"])[:8]
    six = coco_box_ap(pred, gt, K)
    for k in ref.SIX:
        assert six[k] == r["stats"][k] and stats[k] == r["stats"][k], (k, six[k], stats[k], r["stats"][k])
    for k in ("AR1", "AR10", "AR100", "ARs", "ARm", "ARl"):
        assert stats[k] == r["stats"][k], k


def test_structured_splits_reach_the_decision_points():
    """the generator is only worth its name if ties and edges are frequent: counted on the oracle's inputs over the seeds"""
    on_thr = ties = edge = crowd = 0
    for s in SEEDS:
        pred, gt, K, _ = oracle(s)
        for iid, g in gt.items():
            crowd += int(np.sum(g["iscrowd"]))
            ar = g["area"] if "area" in g else (g["boxes"][:, 2] - g["boxes"][:, 0]) * (g["boxes"][:, 3] - g["boxes"][:, 1])
            edge += int(np.sum((ar == 1024) | (ar == 9216)))
            p = pred.get(iid)
            if p is None:
                continue
            ties += len(p["scores"]) - len(set(zip(p["classes"].tolist(), p["scores"].tolist())))
            for d, c in zip(p["boxes"], p["classes"]):
                for b, gc in zip(g["boxes"], g["classes"]):
                    if c == gc and any(ref.bb_iou(list(map(float, d)), list(b), False) == t for t in (0.5, 0.55, 0.6, 0.75, 0.9, 0.95)):
                        on_thr += 1
    assert on_thr >= 20 and ties >= 20 and edge >= 10 and crowd >= 10, (on_thr, ties, edge, crowd)


def test_coco_box_ap_leaves_a_class_without_ground_truth_out():
    from ubteacher.evaluation import coco_box_ap
    pred, gt, K, r = oracle("empty_and_foreign")
    six = coco_box_ap(pred, gt, K)
    assert six["AP"] == 50.0 and six["AP50"] == 50.0 and six["APs"] == 50.0 and six["APl"] == -1.0      # classes 0 (AP 0) and 2 (AP 1)


def twice_inputs(device="cpu"):
    """process() calls of the twice-seen-image case: image 1 (a false positive only), image 2 (a false positive), then image 1 again
    with a true positive - all three detections with one score.  dict semantics keep image 1 at the first position with its last
    value: TP then FP gives AP 100; the last position would give FP, TP = 50, the first value FP, FP = 0."""
    import torch
    from ubteacher.d2.structures import Boxes, Instances
    g = [0.0, 0.0, 10.0, 10.0]

    def pair(iid, gt_boxes, det_box):
        gi = Instances((800, 800))
        gi.gt_boxes = Boxes(torch.tensor(gt_boxes, dtype=torch.float32, device=device).reshape(-1, 4))
        gi.gt_classes = torch.zeros(len(gt_boxes), dtype=torch.int64, device=device)
        pi = Instances((800, 800))
        pi.pred_boxes = Boxes(torch.tensor([det_box], dtype=torch.float32, device=device))
        pi.scores = torch.tensor([0.5], dtype=torch.float32, device=device)
        pi.pred_classes = torch.zeros(1, dtype=torch.int64, device=device)
        return {"image_id": iid, "instances": gi}, {"instances": pi}

    return [pair(1, [g], [float(v) for v in far(0)]), pair(2, [], g), pair(1, [g], g)]


def test_image_processed_twice_keeps_first_position_and_last_value():
    from ubteacher.evaluation import COCOBoxEvaluator
    ev = COCOBoxEvaluator(1)
    for inp, out in twice_inputs():
        ev.process([inp], [out])
    res = ev.evaluate()["bbox"]
    assert res["AP"] == 100.0 and res["AP50"] == 100.0 and res["APs"] == 100.0 and res["APm"] == -1.0
    pred = {1: image([([0, 0, 10, 10], 0.5, 0)], [])[0], 2: image([([0, 0, 10, 10], 0.5, 0)], [])[0]}
    gt = {1: image([], [([0, 0, 10, 10], 0, 0, None)])[1], 2: image([], [])[1]}
    r = ref.evaluate(pred, gt, 1)
    assert all(res[k] == r["stats"][k] for k in ref.SIX)
