"""Test-time augmentation (TEST.AUG) for both detectors: multi-scale + horizontal-flip views of every test image, each run through the
eval-mode detector on its own, the detections brought back into the original image's frame and merged by one class-aware NMS.  The
views' forwards, the return trip (csrc/tta.hip) and the merge (hip.nms_batched) are enqueued on one stream.  The return trip and the
merge never wait for the host; the per-view forwards are the plain inference chain, which rebuilds small shape-keyed device tables with a
synchronising copy whenever the input shape changes (FCOSOutputs._topk_rows holds one shape, rcnn._DEVICE_CONSTS 16 entries) - about
one wait per new view size, as on the plain path (wider caches there are a follow-up outside this module).

The Faster-RCNN rules restate Detectron2's DatasetMapperTTA + GeneralizedRCNNWithTTA for a box-only model [D2-recall] (Detectron2 is not
installed here).  For FCOS neither Detectron2, AdelaiDet nor the reference defines a merge: the same procedure with MODEL.FCOS.NMS_TH and
each detection's reported score is THIS PROJECT's definition.  One view per forward call, on its own canvas padded to the backbone's
size divisibility: Detectron2 batches three views padded to the largest, which changes border features slightly and is not reproduced.
"""
import numpy as np
import torch

from .. import hip
from ..d2.structures import Boxes, Instances
from ..data.transforms import ResizeShortestEdge
from .fcos import PaddedBoxes

SCORE_THRESH = 1e-8   # GeneralizedRCNNWithTTA._merge_detections: fast_rcnn_inference_single_image(..., 1e-8, NMS_THRESH_TEST, DETECTIONS_PER_IMAGE) [D2-recall]


def check_cfg(cfg):
    """the TEST.AUG values no view list can be built from: ValueError naming the key"""
    aug = cfg.TEST.AUG
    sizes = tuple(aug.MIN_SIZES)
    if len(sizes) == 0:
        raise ValueError("TEST.AUG.MIN_SIZES is empty: test-time augmentation needs at least one size")
    for s in sizes:
        if int(s) != s or s <= 0:
            raise ValueError("TEST.AUG.MIN_SIZES %r: every size is a positive integer" % (sizes,))
    if aug.MAX_SIZE < max(sizes):
        raise ValueError("TEST.AUG.MAX_SIZE %r is smaller than the largest of TEST.AUG.MIN_SIZES %r" % (aug.MAX_SIZE, sizes))
    return [int(s) for s in sizes], int(aug.MAX_SIZE), bool(aug.FLIP)


def tta_views(cfg, loader_hw, orig_hw):
    """The ordered views of one test image (Detectron2 DatasetMapperTTA [D2-recall]): for each s of TEST.AUG.MIN_SIZES, in order,
    ResizeShortestEdge(s, TEST.AUG.MAX_SIZE) of the image the test loader delivers and, with TEST.AUG.FLIP, the same resize followed by a
    horizontal flip.  Each view is a dict: `size` (h, w) of the view, `flip`, and `transforms` - the chain from the ORIGINAL image to
    the view, ("resize", h, w, new_h, new_w) and ("hflip", width) steps; a leading resize from the original to the loader size is part
    of every chain when the two differ.  Pure host code."""
    sizes, max_size, flip = check_cfg(cfg)
    lh, lw = int(loader_hw[0]), int(loader_hw[1])
    oh, ow = int(orig_hw[0]), int(orig_hw[1])
    lead = [("resize", oh, ow, lh, lw)] if (oh, ow) != (lh, lw) else []
    views = []
    for s in sizes:
        h, w = ResizeShortestEdge.output_size(lh, lw, s, max_size)
        resize = ("resize", lh, lw, h, w)
        views.append({"size": (h, w), "flip": False, "transforms": lead + [resize]})
        if flip:
            views.append({"size": (h, w), "flip": True, "transforms": lead + [resize, ("hflip", w)]})
    return views


def tta_table(views, orig_hw):
    """float32 [V, hip.TTA_STRIDE]: every view's inverse chain as utv2_tta_collect reads it.  Each resize step's inverse is ONE ratio,
    formed in fp64 and rounded once to fp32 (ResizeTransform.inverse().apply_coords multiplies float32 coordinates by new_w * 1.0 / w
    [D2-recall]); the steps are not combined."""
    t = np.zeros((len(views), hip.TTA_STRIDE), np.float32)
    for i, v in enumerate(views):
        steps = [s for s in v["transforms"] if s[0] == "resize"]
        view, lead = steps[-1], (steps[0] if len(steps) == 2 else None)
        t[i, hip.TTA_FLIP] = 1.0 if v["flip"] else 0.0
        t[i, hip.TTA_WVIEW] = v["size"][1]
        t[i, hip.TTA_RX_VIEW] = np.float32(view[2] / view[4])
        t[i, hip.TTA_RY_VIEW] = np.float32(view[1] / view[3])
        t[i, hip.TTA_RX_LEAD] = np.float32(lead[2] / lead[4]) if lead else 1.0
        t[i, hip.TTA_RY_LEAD] = np.float32(lead[1] / lead[3]) if lead else 1.0
        t[i, hip.TTA_ORIG_H], t[i, hip.TTA_ORIG_W] = orig_hw
    return t


class DetectorWithTTA:
    """Either detector (TwoStagePseudoLabGeneralizedRCNN or OneStageDetector; a student, a teacher or an EnsembleTSModel member) behind
    TEST.AUG: called with a batch of test-loader records it returns what the plain eval-mode model returns, [{"instances": Instances}]
    in original-image coordinates with pred_boxes / scores / pred_classes (the boundary-variance std columns are not merged)."""

    def __init__(self, cfg, model):
        check_cfg(cfg)
        self.cfg = cfg
        self.model = model
        self.two_stage = hasattr(model, "roi_heads")
        self.nms_thresh = cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST if self.two_stage else cfg.MODEL.FCOS.NMS_TH
        self.nms_method = None if self.two_stage else cfg.MODEL.FCOS.NMS_CRITERIA_TEST
        self.topk = int(cfg.TEST.DETECTIONS_PER_IMAGE)
        self._tables = {}

    # the nn.Module-like surface inference_on_dataset uses
    @property
    def training(self):
        return self.model.training

    @property
    def device(self):
        return self.model.device

    def train(self, mode=True):
        self.model.train(mode)
        return self

    def eval(self):
        return self.train(False)

    # -- the stages --------------------------------------------------------------------------------
    def view_images(self, image, views):
        """the views' uint8 [3][h][w] images from the loader's: hip.aug_resize (Pillow's bilinear resize + flip, bit-exact); a view of
        the loader's own size without a flip is the image itself"""
        if image.dtype != torch.uint8:
            raise TypeError("test-time augmentation resizes the loader's uint8 images (got %s)" % image.dtype)
        lhw = (int(image.shape[1]), int(image.shape[2]))
        hwc = None
        out = []
        for v in views:
            if v["size"] == lhw and not v["flip"]:
                out.append(image)
                continue
            if hwc is None:
                hwc = image.permute(1, 2, 0).contiguous()
            out.append(hip.aug_to_chw(hip.aug_resize(hwc, v["size"][0], v["size"][1], v["flip"])))
        return out

    def detect_view(self, image, nms_method=None):
        """the eval-mode detector's ordinary inference on one view, without detector_postprocess: (boxes [D, 4] in the view's pixel
        frame, scores [D], classes int32 [D], valid uint8 [D]), padded, on the device"""
        if self.two_stage:
            dets, _ = self.model.detect([{"image": image}])
        else:
            dets, _ = self.model([{"image": image}], output_raw=True, nms_method=nms_method or self.nms_method)
        return (dets["boxes"][0].contiguous(), dets["scores"][0].contiguous(), dets["classes"][0].to(torch.int32).contiguous(),
                dets["valid"][0].contiguous())

    def transform_table(self, views, orig_hw, device):
        """the views' inverse chains on the device: built once per (view list, original size) and uploaded from pinned memory without
        waiting for the copy"""
        key = (tuple((v["size"], v["flip"], tuple(v["transforms"])) for v in views), tuple(orig_hw), str(device))
        t = self._tables.get(key)
        if t is None:
            if len(self._tables) >= 64:
                self._tables.clear()
            host = torch.from_numpy(tta_table(views, orig_hw))
            t = self._tables[key] = host.pin_memory().to(device, non_blocking=True) if torch.device(device).type == "cuda" else host
        return t

    def merge(self, view_dets, table, orig_hw):
        """Return trip + merge of one image, all on the device: utv2_tta_collect packs the views' detections in the original frame
        (clipped, score > 1e-8), class-aware NMS at the detector's test threshold over the whole set, the DETECTIONS_PER_IMAGE best.
        -> PaddedBoxes of one image (boxes [1, K, 4], scores, classes, valid, count)."""
        V, D = len(view_dets), int(view_dets[0][1].numel())
        if V * D > hip.NMS_MAX_CANDIDATES:
            raise ValueError("TEST.AUG.MIN_SIZES (with FLIP: %d views) times the detector's %d detection slots per view (TEST.DETECTIONS_PER_IMAGE / "
                             "POST_NMS_TOPK_TEST) is %d merge candidates; the NMS kernel takes at most %d: shorten TEST.AUG.MIN_SIZES or lower "
                             "TEST.DETECTIONS_PER_IMAGE" % (V, D, V * D, hip.NMS_MAX_CANDIDATES))
        boxes, scores, classes, valid = hip.tta_collect(view_dets, table)
        K = self.topk
        keep, cnt = hip.nms_batched(boxes, scores, classes, valid, self.nms_thresh, class_aware=True, post_topk=K, max_out=K)
        idx = keep.clamp(min=0).long()
        ok = torch.arange(K, device=boxes.device)[None, :] < cnt[:, None]
        return PaddedBoxes([tuple(orig_hw)], boxes=torch.gather(boxes, 1, idx[:, :, None].expand(-1, -1, 4)), scores=torch.gather(scores, 1, idx),
                           classes=torch.gather(classes, 1, idx), valid=ok.to(torch.uint8), count=cnt)

    @torch.no_grad()
    def detect(self, batched_inputs, nms_method=None):
        """the merged, padded, device-resident detections of every record (a list of one-image PaddedBoxes, original-image frame)"""
        assert not self.model.training, "test-time augmentation runs the eval-mode detector"
        out = []
        for x in batched_inputs:
            image = x["image"].to(self.device)
            lhw = (int(image.shape[1]), int(image.shape[2]))
            orig = (int(x.get("height", lhw[0])), int(x.get("width", lhw[1])))
            views = tta_views(self.cfg, lhw, orig)
            table = self.transform_table(views, orig, image.device)
            dets = [self.detect_view(im, nms_method) for im in self.view_images(image, views)]
            out.append(self.merge(dets, table, orig))
        return out

    def forward(self, batched_inputs, nms_method=None):
        res = []
        for merged in self.detect(batched_inputs, nms_method):
            m = merged["valid"][0].bool()
            inst = Instances(merged.image_sizes[0])
            inst.pred_boxes = Boxes(merged["boxes"][0][m])
            inst.scores = merged["scores"][0][m]
            inst.pred_classes = merged["classes"][0][m].long()
            res.append({"instances": inst})
        return res

    __call__ = forward


GeneralizedRCNNWithTTA = DetectorWithTTA   # the name Detectron2 users know
