"""CPU reference of test-time augmentation (TEST.AUG), assembled from what the suite already trusts: Pillow's bilinear resize for the
views, the oracle's eval-mode detectors without detector_postprocess for the per-view detections, numpy float32 for the return trip
(written from the rules of DESIGN 31, not from the kernel), the oracle's batched_nms plus a top-k for the merge.  Not a test."""
import numpy as np
import torch

from oracle import utv2_oracle as O

F32 = np.float32
SCORE_THRESH = F32(1e-8)


def shortest_edge(h, w, size, max_size):
    """Detectron2 ResizeShortestEdge.get_output_shape [D2-recall]"""
    scale = size * 1.0 / min(h, w)
    newh, neww = (size, scale * w) if h < w else (scale * h, size)
    if max(newh, neww) > max_size:
        scale = max_size * 1.0 / max(newh, neww)
        newh, neww = newh * scale, neww * scale
    return int(newh + 0.5), int(neww + 0.5)


def views(loader_hw, min_sizes, max_size, flip):
    """[(h, w, flipped)] in DatasetMapperTTA's order: per size the plain view, then the flipped one"""
    out = []
    for s in min_sizes:
        h, w = shortest_edge(loader_hw[0], loader_hw[1], s, max_size)
        out.append((h, w, False))
        if flip:
            out.append((h, w, True))
    return out


def view_image(img, h, w, flip):
    """uint8 [3][H][W] torch CPU image -> the view, through Pillow (PIL.Image.resize BILINEAR, then the horizontal flip)"""
    hwc = np.ascontiguousarray(img.permute(1, 2, 0).numpy())
    try:
        from PIL import Image
        out = np.asarray(Image.fromarray(hwc).resize((w, h), Image.BILINEAR))
    except ImportError:
        from oracle import aug_oracle
        out = aug_oracle.resize_bilinear(hwc, h, w)
    if flip:
        out = out[:, ::-1]
    return torch.from_numpy(np.array(out)).permute(2, 0, 1).contiguous()


def unflip(boxes, w_view):
    """HFlipTransform(w_view).apply_box on float32 [n, 4]: x <- W - x on the corners, then min / max"""
    b = np.asarray(boxes, F32).reshape(-1, 4)
    xa, xb = F32(w_view) - b[:, 0], F32(w_view) - b[:, 2]
    return np.stack([np.minimum(xa, xb), np.minimum(b[:, 1], b[:, 3]), np.maximum(xa, xb), np.maximum(b[:, 1], b[:, 3])], 1).astype(F32)


def unresize(boxes, from_hw, to_hw):
    """ResizeTransform(to -> from).inverse().apply_box: float32 coordinates times the ratio, formed in fp64 and rounded once to fp32"""
    b = np.asarray(boxes, F32).reshape(-1, 4).copy()
    rx, ry = F32(to_hw[1] / from_hw[1]), F32(to_hw[0] / from_hw[0])
    b[:, 0::2] = b[:, 0::2] * rx
    b[:, 1::2] = b[:, 1::2] * ry
    return b


def return_trip(boxes, view, loader_hw, orig_hw):
    """view-frame float32 boxes -> the original image's frame: the chain's inverses in reverse order, one multiplication per resize"""
    h, w, flip = view
    b = np.asarray(boxes, F32).reshape(-1, 4)
    if flip:
        b = unflip(b, w)
    b = unresize(b, (h, w), loader_hw)
    if tuple(loader_hw) != tuple(orig_hw):
        b = unresize(b, loader_hw, orig_hw)
    return b


def clip(boxes, hw):
    b = np.asarray(boxes, F32).reshape(-1, 4).copy()
    b[:, 0::2] = np.minimum(np.maximum(b[:, 0::2], F32(0)), F32(hw[1]))
    b[:, 1::2] = np.minimum(np.maximum(b[:, 1::2], F32(0)), F32(hw[0]))
    return b


def collect(view_dets, view_list, loader_hw, orig_hw):
    """what utv2_tta_collect writes: per view D padded slots (boxes [D, 4], scores [D], classes [D], valid [D]) -> the packed view-major
    [V * D] set; slots that are not valid are zeros"""
    ob, osc, oc, ov = [], [], [], []
    for (b, s, c, m), view in zip(view_dets, view_list):
        b, s, c, m = np.asarray(b, F32), np.asarray(s, F32), np.asarray(c, np.int32), np.asarray(m, np.uint8)
        ok = (m != 0) & (s > SCORE_THRESH)
        rb = clip(return_trip(b, view, loader_hw, orig_hw), orig_hw)
        ob.append(np.where(ok[:, None], rb, F32(0)).astype(F32))
        osc.append(np.where(ok, s, F32(0)).astype(F32))
        oc.append(np.where(ok, c, 0).astype(np.int32))
        ov.append(ok.astype(np.uint8))
    return np.concatenate(ob), np.concatenate(osc), np.concatenate(oc), np.concatenate(ov)


def merge(boxes, scores, classes, nms_thresh, topk):
    """class-aware NMS over the candidates (score desc, index asc), the topk best; -> (boxes, scores, classes) numpy, descending score"""
    if len(scores) == 0:
        return boxes, scores, classes
    keep = O.batched_nms(torch.from_numpy(boxes), torch.from_numpy(scores), torch.from_numpy(classes).long(), nms_thresh)[:topk].numpy()
    return boxes[keep], scores[keep], classes[keep]


def candidates(per_view, view_list, loader_hw, orig_hw):
    """the views' ragged detections ({boxes, scores, classes} torch) in the original frame, clipped, score > 1e-8, view-major"""
    bs, ss, cs = [], [], []
    for det, view in zip(per_view, view_list):
        b = clip(return_trip(det["boxes"].numpy().astype(F32), view, loader_hw, orig_hw), orig_hw)
        s = det["scores"].numpy().astype(F32)
        ok = s > SCORE_THRESH
        bs.append(b[ok]); ss.append(s[ok]); cs.append(det["classes"].numpy().astype(np.int64)[ok])
    return np.concatenate(bs).astype(F32), np.concatenate(ss).astype(F32), np.concatenate(cs)


def rcnn_views(sd, image, view_list, mean, pstd, score_thresh=0.05):
    """the oracle's eval-mode Faster-RCNN on every view, one view per forward, no detector_postprocess.  The oracle's inference has
    SCORE_THRESH_TEST 0.05 built in; a higher threshold is applied to its output: greedy NMS visits candidates in descending score, so
    a candidate never changes the fate of a higher-scoring one and `score > t` commutes with the NMS and with the top-100 cut."""
    out = []
    with torch.no_grad():
        for h, w, f in view_list:
            det = O.rcnn_inference(sd, [view_image(image, h, w, f)], mean, pstd, out_sizes=None)[0][0]
            m = det["scores"] > score_thresh
            out.append({k: v[m] for k, v in det.items()})
            out[-1]["all_scores"] = det["scores"]
    return out


def fcos_views(sd, image, view_list, mean, pstd, nms_method="cls_n_ctr", fcfg=None):
    """the oracle's eval-mode FCOS on every view, one view per forward, no detector_postprocess.  Each result also carries how far the
    view's own decisions are from flipping: `d_prob` = min | p - INFERENCE_TH_TEST | over every (location, class) probability,
    `d_iou` = min | IoU - NMS_TH | over the same-class pairs of the view's pre-NMS candidates (fcos_predict with the NMS and the top-k
    switched off returns them), `n_pre` / `n_nms` = candidates per level at most / survivors, to be held against the two top-k."""
    import copy
    fcfg = fcfg or O.FCOSCfg()
    loose = copy.copy(fcfg)
    loose.nms_thresh, loose.post_nms_topk = 2.0, 10 ** 9
    out = []
    with torch.no_grad():
        for h, w, f in view_list:
            logits, reg, std, ctr, locations, sizes = O.fcos_forward(sd, [view_image(image, h, w, f)], mean, pstd)
            det = O.fcos_predict(fcfg, logits, reg, std, ctr, locations, sizes, nms_method)[0]
            pre = O.fcos_predict(loose, logits, reg, std, ctr, locations, sizes, nms_method)[0]
            det["d_prob"] = min(float((l.sigmoid() - fcfg.pre_nms_thresh).abs().min()) for l in logits)
            c = pre["classes"].numpy()
            iou = O.pairwise_iou(pre["boxes"], pre["boxes"]).numpy()
            same = (c[:, None] == c[None, :]) & ~np.eye(len(c), dtype=bool)
            det["d_iou"] = float(np.abs(iou[same] - fcfg.nms_thresh).min()) if same.any() else float("inf")
            det["n_pre"] = max(int((l.sigmoid() > fcfg.pre_nms_thresh).sum()) for l in logits)
            det["n_nms"] = len(O.batched_nms(pre["boxes"], pre["scores"], pre["classes"], fcfg.nms_thresh))
            out.append(det)
    return out


def tuned_case(kind, seed, device, fcos_bias=-4.5, rcnn_bg_bias=3.0, fcos_box_slope=0.0):
    """(cfg, model in eval mode on `device`, its tuned CPU state, the 96 x 128 uint8 CPU image, pixel mean, pixel std): the small seeded
    problems of the eval-mode parity tests - random initialisation under `seed`, prediction layers rescaled by tests/utv2_testutil so
    that the views return detections."""
    from tests.utv2_testutil import cpu_state, make_batch, rcnn_tune, tune_state_for_pseudo_labels
    from ubteacher.modeling import build_model
    from ubteacher.presets import get_config
    cfg = get_config(kind, 1, ["SOLVER.IMG_PER_BATCH_LABEL", 2, "SOLVER.IMG_PER_BATCH_UNLABEL", 2, "SEMISUPNET.BURN_UP_STEP", 0,
                               "SOLVER.AMP.ENABLED", False, "MODEL.DEVICE", device])
    cfg.MODEL.DEVICE = "cpu"
    torch.manual_seed(seed)
    model = build_model(cfg)               # the state is always drawn by a host model: the seeds were chosen with exactly this state
    _, orac = make_batch(seed, 1, 1, 96, 128, "cpu")
    image = orac[3][0]["image"]
    mean = torch.tensor(cfg.MODEL.PIXEL_MEAN).view(3, 1, 1)
    pstd = torch.tensor(cfg.MODEL.PIXEL_STD).view(3, 1, 1)
    sd = cpu_state(model)
    sd = rcnn_tune(sd, [image], mean, pstd, seed=seed) if kind == "rcnn" else tune_state_for_pseudo_labels(sd, [image], bias=fcos_bias, seed=seed)
    if kind == "rcnn":     # rcnn_tune's background bias (3.0 unless the caller raises it)
        sd["roi_heads.box_predictor.cls_score.bias"][-1] = rcnn_bg_bias
    if kind == "fcos" and fcos_box_slope:
        # the random box tower leaves the 17-bin distance distributions near uniform: every side ~8 bins, boxes of the image's size.  A bias
        # of -slope * bin on each side's logits makes them a few pixels, so that boxes stay inside the image and the clip changes little
        k = "proposal_generator.fcos_head.bbox_pred.bias"
        sd[k] = (-fcos_box_slope * torch.arange(17, dtype=torch.float32)).repeat(4).to(sd[k].dtype).reshape(sd[k].shape)
    if kind == "fcos":     # persistent buffers of the one-stage detector: what the product normalises with
        mean, pstd = sd["pixel_mean"], sd["pixel_std"]
    cfg.MODEL.DEVICE = device
    if torch.device(device).type != "cpu":
        model = build_model(cfg)
    model.load_state_dict(sd)
    model.eval()
    return cfg, model, sd, image, mean, pstd


def margins(boxes, scores, classes, nms_thresh, topk, score_thresholds):
    """how far the merge is from a decision flipping: (min | IoU - nms_thresh | over same-class candidate pairs, min | score - t | over
    the thresholds, the gap at the top-k cut of the kept set - inf when fewer than topk + 1 are kept)"""
    b = torch.from_numpy(boxes)
    iou = O.pairwise_iou(b, b).numpy()
    same = (classes[:, None] == classes[None, :]) & ~np.eye(len(classes), dtype=bool)
    d_iou = float(np.abs(iou[same] - nms_thresh).min()) if same.any() else float("inf")
    d_thr = min(float(np.abs(scores.astype(np.float64) - t).min()) for t in score_thresholds) if len(scores) else float("inf")
    keep = O.batched_nms(b, torch.from_numpy(scores), torch.from_numpy(classes).long(), nms_thresh).numpy()
    d_cut = float(scores[keep[topk - 1]] - scores[keep[topk]]) if len(keep) > topk else float("inf")
    return d_iou, d_thr, d_cut
