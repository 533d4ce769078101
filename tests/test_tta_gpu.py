"""Test-time augmentation (TEST.AUG) on the device: utv2_tta_collect bit for bit against the numpy fp32 return trip, the identity view
against the plain eval-mode detectors, both detectors against the CPU reference of tests/tta_ref.py, no host synchronisation in the
collect + merge stage, and train_net.py --eval-only with TEST.AUG.ENABLED under both evaluators."""
import argparse
import warnings

import numpy as np
import pytest
import torch

from tests import tta_ref as R
from tests.test_coco_dataset import tiny  # noqa: F401  (the registered tiny COCO-format set)

pytestmark = pytest.mark.gpu
LOADER, ORIG = (96, 128), (144, 192)
# chosen on the CPU with the reference alone (tests/tta_ref.py: tuned_case + margins): every view returns detections and no decision
# is near a flip.  Merge stage: (min |IoU - thr| over same-class pairs, min |score - 1e-8|, gap at the top-k cut); per view: the score /
# probability threshold, the view's own NMS, its top-k:
#   rcnn  seed 31, SCORE_THRESH_TEST 0.4, DETECTIONS_PER_IMAGE 20: merge (2.2e-3, 0.40, 4.6e-3); views return 6 / 1 / 34 / 35, their
#         scores 7.8e-4 from 0.4 (the oracle's own 0.05 and its NMS lie below the 0.4 cut, see tta_ref.rcnn_views)
#   fcos  seed 7, cls bias -7.5, DETECTIONS_PER_IMAGE 8: merge (2.6e-2, 0.14, 6.9e-3); views return 4 / 5 / 8 / 9, every class
#         probability 2.0e-4 from INFERENCE_TH_TEST, the views' pre-NMS same-class IoUs 4.5e-3 from NMS_TH, at most 16 candidates per
#         level (PRE_NMS_TOPK_TEST 1000) and 9 NMS survivors (POST_NMS_TOPK_TEST 100): neither top-k acts
CASES = {"rcnn": dict(seed=31, topk=20, score_thresh=0.4), "fcos": dict(seed=7, topk=8, fcos_bias=-7.5)}
_CASE = {}


def case(kind):
    """the tuned model on the GPU + the CPU reference of its TTA run, computed once per kind"""
    if kind in _CASE:
        return _CASE[kind]
    c = CASES[kind]
    cfg, model, sd, image, mean, pstd = R.tuned_case(kind, c["seed"], "cuda", fcos_bias=c.get("fcos_bias", -4.5))
    cfg.TEST.AUG.MIN_SIZES, cfg.TEST.AUG.FLIP = (64, 96), True
    cfg.TEST.DETECTIONS_PER_IMAGE = c["topk"]
    vl = R.views(LOADER, (64, 96), cfg.TEST.AUG.MAX_SIZE, True)
    if kind == "rcnn":
        cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST = c["score_thresh"]
        model.roi_heads.box_predictor.test_score_thresh = c["score_thresh"]
        per = R.rcnn_views(sd, image, vl, mean, pstd, c["score_thresh"])
        thr, sthr = cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST, [1e-8]
        all_scores = torch.cat([p["all_scores"] for p in per]).numpy()
        d_view_thr = float(np.abs(all_scores - c["score_thresh"]).min())
    else:
        per = R.fcos_views(sd, image, vl, mean, pstd, cfg.MODEL.FCOS.NMS_CRITERIA_TEST)
        thr, sthr = cfg.MODEL.FCOS.NMS_TH, [1e-8]
        d_view_thr = min(p["d_prob"] for p in per)
        assert min(p["d_iou"] for p in per) > 1e-3, "a view's own NMS is near a flip"
        assert max(p["n_pre"] for p in per) < cfg.MODEL.FCOS.PRE_NMS_TOPK_TEST and max(p["n_nms"] for p in per) < cfg.MODEL.FCOS.POST_NMS_TOPK_TEST
    b, s, c_ = R.candidates(per, vl, LOADER, ORIG)
    _CASE[kind] = dict(cfg=cfg, model=model, image=image, views=vl, per=per, cand=(b, s, c_), thr=thr, ref=R.merge(b, s, c_, thr, c["topk"]),
                       margins=R.margins(b, s, c_, thr, c["topk"], sthr) + (d_view_thr,))
    return _CASE[kind]


def _records(image, orig=ORIG):
    return [{"image": image.cuda(), "height": orig[0], "width": orig[1], "image_id": 0}]


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------------
def test_tta_collect_bit_exact_against_numpy_fp32():
    from ubteacher import hip
    from ubteacher.modeling.test_time_augmentation import tta_table, tta_views
    from tests.test_tta import _cfg
    V, D = 4, 5
    orig = (150, 199)                                   # a non-identity leading resize with ratios that are not exact in fp32
    cfg = _cfg(MIN_SIZES=(64, 96), FLIP=True)
    views = tta_views(cfg, LOADER, orig)
    vl = R.views(LOADER, (64, 96), 4000, True)
    assert [(h, w, f) for h, w, f in vl] == [v["size"] + (v["flip"],) for v in views]
    rng = np.random.default_rng(5)
    thr = np.float32(1e-8)
    counts = [3, 0, 5, 2]                                # ragged: an empty view and a full one
    dets = []
    for v, (h, w, f) in enumerate(vl):
        x1 = rng.uniform(0, w - 8, D); y1 = rng.uniform(0, h - 8, D)
        b = np.stack([x1, y1, x1 + rng.uniform(2, 40, D), y1 + rng.uniform(2, 30, D)], 1).astype(np.float32)
        s = rng.uniform(0.05, 1.0, D).astype(np.float32)
        c = rng.integers(0, 80, D).astype(np.int32)
        m = (np.arange(D) < counts[v]).astype(np.uint8)
        dets.append([b, s, c, m])
    dets[0][0][0] = [60.5, 40.25, 120.0, 90.0]           # leaves the 64 x 85 view: the clip acts after the return trip
    dets[0][1][1] = thr                                  # a score equal to fp32(1e-8): dropped
    dets[0][1][2] = np.nextafter(thr, np.float32(1))     # the next fp32 above: kept
    dets[3][0][0] = [0.0, 10.0, 31.5, 50.0]              # flipped view, x1 = 0: lands on the original's width
    dets[3][0][1] = [17.3, 5.5, 128.0, 96.0]             # flipped view, x2 = W_view: lands on 0
    dets[2][1][4] = 0.0                                  # a valid slot with score 0
    dets[1][0][:] = np.nan                               # slots beyond a view's count may hold anything
    want = R.collect([tuple(d) for d in dets], vl, LOADER, orig)
    table = torch.from_numpy(tta_table(views, orig)).cuda()
    got = hip.tta_collect([tuple(torch.from_numpy(a).cuda() for a in d) for d in dets], table)
    torch.cuda.synchronize()
    gb, gs, gc, gv = (g[0].cpu().numpy() for g in got)
    assert gb.shape == (V * D, 4) and gs.shape == gc.shape == gv.shape == (V * D,)
    assert np.array_equal(gv, want[3]) and gv.sum() == 3 - 1 + 5 - 1 + 2
    assert np.array_equal(gb.view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(gs.view(np.uint32), want[1].view(np.uint32)) and np.array_equal(gc, want[2])
    slots = np.arange(V * D) % D
    assert not gv[slots >= np.repeat(counts, D)].any()   # invalid slots never carry a valid flag
    assert gv[0] == 1 and gb[0, 2] == 199 and gb[0, 3] == 150 and gv[1] == 0 and gv[2] == 1
    assert gb[3 * D, 2] == 199 and gb[3 * D + 1, 0] == 0 and np.all(gb[D:2 * D] == 0)


# ---- 2. the identity view ---------------------------------------------------------------------------------------------------------
# FCOS runs its own NMS on boxes that may leave the image and the merge clips before its NMS: the identity holds where the
# clip moves no same-class IoU across NMS_TH.  The random box tower of the shared cases emits image-sized boxes that the clip makes
# coincide, so this case gives the distance logits a bias of -1 per bin (boxes of a few pixels, tta_ref.tuned_case).  Chosen on the CPU
# with the reference alone: seed 7, cls bias -7.5 - 15 detections with 25 same-class pairs, the largest clipped IoU 0.17.
ID_FCOS = dict(seed=7, fcos_bias=-7.5, fcos_box_slope=1.0)


@pytest.mark.parametrize("kind", ["rcnn", "fcos"])
def test_identity_view_equals_plain_inference(kind):
    from ubteacher.modeling.test_time_augmentation import DetectorWithTTA
    if kind == "rcnn":
        cs = case(kind)
        cfg, model, image = cs["cfg"].clone(), cs["model"], cs["image"]
    else:
        cfg, model, _, image, _, _ = R.tuned_case("fcos", ID_FCOS["seed"], "cuda", fcos_bias=ID_FCOS["fcos_bias"], fcos_box_slope=ID_FCOS["fcos_box_slope"])
    cfg.TEST.AUG.MIN_SIZES, cfg.TEST.AUG.FLIP = (96,), False
    cfg.TEST.DETECTIONS_PER_IMAGE = 100
    recs = _records(image, orig=LOADER)
    with torch.no_grad():
        plain = model(recs, nms_method=cfg.MODEL.FCOS.NMS_CRITERIA_TEST)[0]["instances"] if kind == "fcos" else model(recs)[0]["instances"]
    # the stated precondition, on the plain (clipped) output: no same-class pair above the NMS threshold
    b, c = plain.pred_boxes.tensor.cpu(), plain.pred_classes.cpu()
    from oracle import utv2_oracle as O
    iou = O.pairwise_iou(b, b)
    same = (c[:, None] == c[None, :]) & ~torch.eye(len(c), dtype=torch.bool)
    thr = cfg.MODEL.FCOS.NMS_TH if kind == "fcos" else cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST
    assert len(plain) >= 2 and bool(same.any()) and not bool((iou[same] > thr).any())     # same-class pairs exist: the second NMS has work
    got = DetectorWithTTA(cfg, model)(recs)[0]["instances"]
    assert len(got) == len(plain) and tuple(got.image_size) == tuple(plain.image_size)
    assert torch.equal(got.pred_classes, plain.pred_classes.long())
    assert torch.equal(got.pred_boxes.tensor, plain.pred_boxes.tensor) and torch.equal(got.scores, plain.scores)


# ---- 3. both detectors against the CPU reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rcnn", "fcos"])
def test_tta_against_cpu_reference(kind):
    """kept set identical in count and classes; scores rtol 1e-3 and boxes 1e-3 of the image size, the tolerances of
    test_rcnn_eval_detections_vs_reference_golden / test_fcos_eval_detections_vs_reference_golden"""
    from ubteacher.modeling.test_time_augmentation import DetectorWithTTA
    cs = case(kind)
    d_iou, d_thr, d_cut, d_view_thr = cs["margins"]
    print(kind, "margins: IoU %.3g, score threshold %.3g (views' %.3g), top-k cut %.3g" % (d_iou, d_thr, d_view_thr, d_cut))
    assert all(len(p["scores"]) > 0 for p in cs["per"]), "every view returns detections"
    assert d_iou > 1e-3 and d_thr > 1e-4 and d_view_thr > 1e-4 and d_cut > 1e-4
    got = DetectorWithTTA(cs["cfg"], cs["model"])(_records(cs["image"]))[0]["instances"]
    rb, rs, rc = cs["ref"]
    assert tuple(got.image_size) == ORIG and len(rs) == CASES[kind]["topk"] < len(cs["cand"][1])      # the cut acts
    assert len(got) == len(rs), (len(got), len(rs))
    assert np.array_equal(got.pred_classes.cpu().numpy(), rc)
    np.testing.assert_allclose(got.scores.cpu().numpy(), rs, rtol=1e-3)
    np.testing.assert_allclose(got.pred_boxes.tensor.cpu().numpy(), rb, rtol=0, atol=1e-3 * max(ORIG))


# ---- 4. no host synchronisation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rcnn", "fcos"])
def test_collect_and_merge_do_not_synchronise(kind):
    """torch's sync debug mode in "error" around the collect + merge stage (transform table, utv2_tta_collect, NMS, gathers) after a
    warm-up: the stage between the last view's forward and the merged device result never waits for the host.  The per-view forwards are
    the plain inference chain, which re-uploads small shape-keyed tables when the input shape changes: they are run in
    "warn" mode and what they report is printed, not asserted."""
    from ubteacher.modeling.test_time_augmentation import DetectorWithTTA, tta_views
    cs = case(kind)
    tta = DetectorWithTTA(cs["cfg"], cs["model"])
    recs = _records(cs["image"])
    want = tta.detect(recs)[0]                                      # warm-up: workspaces, caches, the pinned staging block
    torch.cuda.synchronize()
    image = recs[0]["image"]
    views = tta_views(cs["cfg"], LOADER, ORIG)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with torch.no_grad():
                dets = [tta.detect_view(im) for im in tta.view_images(image, views)]
        finally:
            torch.cuda.set_sync_debug_mode("default")
    print(kind, "synchronising calls reported in the %d view forwards: %d" % (len(views), len(seen)))
    tta._tables.clear()                                              # a new image size: the table is built and uploaded inside the stage
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            table = tta.transform_table(views, ORIG, image.device)
            got = tta.merge(dets, table, ORIG)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for k in ("boxes", "scores", "classes", "valid", "count"):
        assert got[k].is_cuda and torch.equal(got[k], want[k]), k


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fcos", "rcnn"])
def test_eval_only_with_tta_under_both_evaluators(tiny, kind, tmp_path, monkeypatch):  # noqa: F811
    import os
    import train_net
    monkeypatch.setattr(train_net, "setup_logger", lambda *a, **k: None)
    conf = os.path.join(os.path.dirname(os.path.abspath(train_net.__file__)), "configs", "utv2_%s_r50.yaml" % ("fcos" if kind == "fcos" else "frcnn"))
    low = ["MODEL.FCOS.INFERENCE_TH_TEST", 0.005] if kind == "fcos" else ["MODEL.ROI_HEADS.SCORE_THRESH_TEST", 0.002]   # random weights: let detections through
    res = {}
    for ev in ("COCOeval", "COCOeval_device"):
        opts = ["MODEL.WEIGHTS", "", "MODEL.DEVICE", "cuda", "SEED", 0, "OUTPUT_DIR", str(tmp_path), "DATASETS.TEST", "('%s',)" % tiny[0],
                "INPUT.MIN_SIZE_TEST", 96, "INPUT.MAX_SIZE_TEST", 160, "TEST.AUG.ENABLED", True, "TEST.AUG.MIN_SIZES", "(64, 96)",
                "TEST.EVALUATOR", ev] + low
        res[ev] = train_net.main(argparse.Namespace(config_file=conf, eval_only=True, resume=False, opts=opts))
    for ev, r in res.items():
        assert "AP" in r["bbox"] and "AP" in r["bbox_TTA"], (ev, sorted(r))
        assert r["_speed_TTA"]["images"] >= 1
    for task in ("bbox", "bbox_TTA"):
        for k in ("AP", "AP50", "AP75", "APs", "APm", "APl"):
            a, b = res["COCOeval"][task][k], res["COCOeval_device"][task][k]
            assert a == b or (a != a and b != b), (task, k, a, b)
    assert res["COCOeval"]["bbox_TTA"]["AP"] >= 0.0
