"""Golden vectors of the RPN under MODEL.RPN.SMOOTH_L1_BETA, BBOX_REG_LOSS_TYPE "giou", BOUNDARY_THRESH and of the anchor generator's
keys: the reference's own `PseudoLabRPN.label_and_sample_anchors_pseudo` and `PseudoLabRPN.losses` (proposal_generator/rpn.py:78-225)
executed here (CPU, build container only) through the Detectron2 / fvcore shims of gen_golden.py, which this script imports and does not
edit.  Detectron2 is absent: its `_dense_box_regression_loss` (with the giou branch), `Box2BoxTransform`, `Boxes.inside_box` and
`DefaultAnchorGenerator` are restated below, each marked [D2-recall].

Everything runs in FLOAT64 on inputs that are exact in fp32 (multiples of 1/64; the anchor tables are the float32 tables Detectron2
builds), so the arrays are the reference's arithmetic to ~1e-15; the one fp32 step left is the VALUE of loss_rpn_cls: rpn.py:207-212
casts the BCE target to float32 and ATen forms the terms in that buffer (its gradient comes from autograd in fp64).

  rpn_keys.npz   scene: canvas 96 x 128, levels (6, 8) at stride 16 with 16-pixel anchors and (3, 4) at stride 32 with 64-pixel anchors,
                 3 ratios (A = 3, R = 180); image 0 is 80 x 104 with 3 gt boxes, image 1 is 96 x 128 without gt
      anchors / gt0 / sc0 / sizes / keys      the scene, the pseudo scores of image 0, the image sizes (h, w), the sampling keys [2, R]
      labels_t<i> / sampled_t<i>              labels of every anchor at BOUNDARY_THRESH thresholds[i] before the subsampling, and after
                                              the "k smallest keys" subsampling (16 per image, a quarter positive)
      obj / deltas                            head outputs [2, R] / [2, R, 4]
      <type>_b<i>_loss_cls / _loss_loc / _gobj / _gdeltas    type = smooth_l1 (i = index into betas) | giou (i = 0): the two losses on
                                              sampled_t0 (threshold -1), d loss_rpn_cls / d obj and d loss_rpn_loc / d deltas
      anc_<case>_l<level>                     DefaultAnchorGenerator tables: a6 = SIZES [[32, 64]] x 3 ratios, a1 = [[32], [64]] x [[1.0]],
                                              off = [[32], [64]] x 3 ratios at OFFSET 0.5; levels (8, 6) / (4, 3) at strides 16 / 32

    python tests/golden/gen_golden_rpn_keys.py
"""
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import gen_golden as G  # noqa: E402
from oracle import utv2_oracle as O  # noqa: E402

BETAS = (0.0, 0.11, 1.0)
THRESHOLDS = (-1.0, 0.0, 8.0)
SCALE_CLAMP = math.log(1000.0 / 16)
F64 = torch.float64


def quant(t):
    return torch.round(t * 64.0) / 64.0


# ---- [D2-recall] ------------------------------------------------------------------------------------------------------------------------
class Box2BoxTransform:
    """[D2-recall] detectron2.modeling.box_regression.Box2BoxTransform"""

    def __init__(self, weights, scale_clamp=SCALE_CLAMP):
        self.weights, self.scale_clamp = weights, scale_clamp

    def get_deltas(self, src_boxes, target_boxes):
        src_widths = src_boxes[:, 2] - src_boxes[:, 0]
        src_heights = src_boxes[:, 3] - src_boxes[:, 1]
        src_ctr_x = src_boxes[:, 0] + 0.5 * src_widths
        src_ctr_y = src_boxes[:, 1] + 0.5 * src_heights
        target_widths = target_boxes[:, 2] - target_boxes[:, 0]
        target_heights = target_boxes[:, 3] - target_boxes[:, 1]
        target_ctr_x = target_boxes[:, 0] + 0.5 * target_widths
        target_ctr_y = target_boxes[:, 1] + 0.5 * target_heights
        wx, wy, ww, wh = self.weights
        dx = wx * (target_ctr_x - src_ctr_x) / src_widths
        dy = wy * (target_ctr_y - src_ctr_y) / src_heights
        dw = ww * torch.log(target_widths / src_widths)
        dh = wh * torch.log(target_heights / src_heights)
        return torch.stack((dx, dy, dw, dh), dim=1)

    def apply_deltas(self, deltas, boxes):
        boxes = boxes.to(deltas.dtype)
        widths = boxes[:, 2] - boxes[:, 0]
        heights = boxes[:, 3] - boxes[:, 1]
        ctr_x = boxes[:, 0] + 0.5 * widths
        ctr_y = boxes[:, 1] + 0.5 * heights
        wx, wy, ww, wh = self.weights
        dx = deltas[:, 0::4] / wx
        dy = deltas[:, 1::4] / wy
        dw = torch.clamp(deltas[:, 2::4] / ww, max=self.scale_clamp)
        dh = torch.clamp(deltas[:, 3::4] / wh, max=self.scale_clamp)
        pred_ctr_x = dx * widths[:, None] + ctr_x[:, None]
        pred_ctr_y = dy * heights[:, None] + ctr_y[:, None]
        pred_w = torch.exp(dw) * widths[:, None]
        pred_h = torch.exp(dh) * heights[:, None]
        x1, y1 = pred_ctr_x - 0.5 * pred_w, pred_ctr_y - 0.5 * pred_h
        x2, y2 = pred_ctr_x + 0.5 * pred_w, pred_ctr_y + 0.5 * pred_h
        return torch.stack((x1, y1, x2, y2), dim=-1).reshape(deltas.shape)


def dense_box_regression_loss(anchors, box2box_transform, pred_anchor_deltas, gt_boxes, fg_mask, box_reg_loss_type="smooth_l1",
                              smooth_l1_beta=0.0):
    """[D2-recall] detectron2.modeling.box_regression._dense_box_regression_loss, smooth_l1 and giou branches"""
    anchors = type(anchors[0]).cat(anchors).tensor
    if box_reg_loss_type == "smooth_l1":
        gt_anchor_deltas = torch.stack([box2box_transform.get_deltas(anchors, k) for k in gt_boxes])
        return G._fv_smooth_l1(torch.cat(pred_anchor_deltas, dim=1)[fg_mask], gt_anchor_deltas[fg_mask], beta=smooth_l1_beta, reduction="sum")
    if box_reg_loss_type == "giou":
        pred_boxes = [box2box_transform.apply_deltas(k, anchors) for k in torch.cat(pred_anchor_deltas, dim=1)]
        return G._fv_giou(torch.stack(pred_boxes)[fg_mask], torch.stack(gt_boxes)[fg_mask], reduction="sum")
    raise ValueError("Invalid dense box regression loss type '%s'" % box_reg_loss_type)


def inside_box(self, box_size, boundary_threshold=0):
    """[D2-recall] detectron2.structures.Boxes.inside_box"""
    height, width = box_size
    return ((self.tensor[..., 0] >= -boundary_threshold) & (self.tensor[..., 1] >= -boundary_threshold)
            & (self.tensor[..., 2] < width + boundary_threshold) & (self.tensor[..., 3] < height + boundary_threshold))


def default_anchor_generator(level_hw, strides, sizes, aspect_ratios, offset):
    """[D2-recall] detectron2.modeling.anchor_generator.DefaultAnchorGenerator: _broadcast_params, generate_cell_anchors, _create_grid_offsets"""
    def broadcast(params, n):
        if not isinstance(params[0], (list, tuple)):
            return [params] * n
        if len(params) == 1:
            return list(params) * n
        assert len(params) == n
        return params
    sizes, aspect_ratios = broadcast(sizes, len(strides)), broadcast(aspect_ratios, len(strides))
    out = []
    for (gh, gw), stride, s_, a_ in zip(level_hw, strides, sizes, aspect_ratios):
        cell = []
        for size in s_:
            area = size ** 2.0
            for aspect_ratio in a_:
                w = math.sqrt(area / aspect_ratio)
                h = aspect_ratio * w
                cell.append([-w / 2.0, -h / 2.0, w / 2.0, h / 2.0])
        base = torch.tensor(cell)
        shifts_x = torch.arange(offset * stride, gw * stride, step=stride, dtype=torch.float32)
        shifts_y = torch.arange(offset * stride, gh * stride, step=stride, dtype=torch.float32)
        shift_y, shift_x = torch.meshgrid(shifts_y, shifts_x, indexing="ij")
        shift_x, shift_y = shift_x.reshape(-1), shift_y.reshape(-1)
        shifts = torch.stack((shift_x, shift_y, shift_x, shift_y), dim=1)
        out.append((shifts.view(-1, 1, 4) + base.view(1, -1, 4)).reshape(-1, 4))
    return out


# ---- the scene ------------------------------------------------------------------------------------------------------------------------------
HW, STRIDES, SIZES, RATIOS = [(6, 8), (3, 4)], [16, 32], [[16], [64]], [[0.5, 1.0, 2.0]]
IMAGE_SIZES = [(80, 104), (96, 128)]
GT0 = [[0.0, 0.0, 12.0, 12.0],      # its best anchor, (-8, -8, 8, 8) at IoU 0.19, is a low-quality match that leaves the image by 8
       [24.0, 24.0, 40.0, 40.0],    # equal to an anchor
       [30.0, 10.0, 100.0, 70.0]]   # IoU 0.714 with the 64-pixel anchor (32, 0, 96, 64)
BATCH, FRAC = 16, 0.25


def main():
    structures, fo, pg, tr = G.install_shims()
    sys.modules["detectron2.modeling.box_regression"]._dense_box_regression_loss = dense_box_regression_loss
    rp = G._load("ubteacher.modeling.proposal_generator.rpn", G.REF + "/ubteacher/modeling/proposal_generator/rpn.py")
    Boxes, Instances = structures.Boxes, structures.Instances
    Boxes.inside_box = inside_box
    g = torch.Generator().manual_seed(9031)
    anchors = default_anchor_generator(HW, STRIDES, SIZES, RATIOS, 0.0)
    A = torch.cat(anchors)
    R = A.shape[0]
    keys = torch.rand(2, R, generator=g)
    gt0 = torch.tensor(GT0)
    sc0 = quant(torch.rand(3, generator=g) * 0.3 + 0.7)
    d = {"anchors": G.npy(A), "gt0": G.npy(gt0), "sc0": G.npy(sc0), "sizes": np.array(IMAGE_SIZES, dtype=np.int64), "keys": G.npy(keys),
         "betas": np.array(BETAS), "thresholds": np.array(THRESHOLDS), "batch": np.int64(BATCH), "frac": np.float64(FRAC)}
    iou = O.pairwise_iou(gt0.double(), A.double())
    assert float(torch.min((iou - 0.3).abs().min(), (iou - 0.7).abs().min())) > 1e-3       # nothing rides on a rounding at a threshold

    def instances():
        out = []
        for i, hw in enumerate(IMAGE_SIZES):
            x = Instances(hw)
            x.gt_boxes = Boxes(gt0.to(F64) if i == 0 else torch.zeros(0, 4, dtype=F64))
            x.scores = sc0.to(F64) if i == 0 else torch.zeros(0, dtype=F64)
            out.append(x)
        return out

    def duck(thresh, sub, typ="smooth_l1", beta=0.0):
        return types.SimpleNamespace(anchor_matcher=lambda m: O.matcher(m, [0.3, 0.7], [0, -1, 1], True), anchor_boundary_thresh=thresh,
                                     _subsample_labels=sub, box2box_transform=Box2BoxTransform((1.0, 1.0, 1.0, 1.0)), box_reg_loss_type=typ,
                                     smooth_l1_beta=beta, batch_size_per_image=BATCH, loss_weight={"loss_rpn_cls": 1.0, "loss_rpn_loc": 1.0})

    def by_keys():
        kit = iter([keys[0], keys[1]])

        def sub(labels):
            pos, neg = O.subsample_by_keys(labels, next(kit), BATCH, FRAC, 0)
            labels.fill_(-1); labels.scatter_(0, pos, 1); labels.scatter_(0, neg, 0)
            return labels
        return sub

    ab = [Boxes(a.to(F64)) for a in anchors]
    sampled0 = None
    for ti, t in enumerate(THRESHOLDS):
        labs, _, _ = rp.PseudoLabRPN.label_and_sample_anchors_pseudo(duck(t, lambda l: l), ab, instances())
        d["labels_t%d" % ti] = G.npy(torch.stack(labs))
        labs, mboxes, confs = rp.PseudoLabRPN.label_and_sample_anchors_pseudo(duck(t, by_keys()), ab, instances())
        d["sampled_t%d" % ti] = G.npy(torch.stack(labs))
        if ti == 0:
            sampled0 = (labs, mboxes, confs)
    labs, mboxes, confs = sampled0
    # head outputs: logits of a few units; deltas around the regression target of the positives so that |delta - target| falls on both
    # sides of 0.11 and of 1, the rest small
    obj = quant(torch.randn(2, R, generator=g) * 2)
    tf = Box2BoxTransform((1.0, 1.0, 1.0, 1.0))
    deltas = quant(torch.randn(2, R, 4, generator=g) * 0.3)
    pos0 = torch.nonzero(labs[0] == 1).squeeze(1)
    tgt = tf.get_deltas(A[pos0].double(), mboxes[0][pos0]).float()
    spread = torch.tensor([0.06, 0.2, 0.6, 2.0])[torch.randint(0, 4, (pos0.numel(), 4), generator=g)]
    deltas[0, pos0] = quant(tgt + (torch.rand(pos0.numel(), 4, generator=g) * 2 - 1) * spread)
    d["obj"], d["deltas"] = G.npy(obj), G.npy(deltas)
    split = [a.shape[0] for a in anchors]
    for typ, betas in (("smooth_l1", BETAS), ("giou", (0.0,))):
        for bi, beta in enumerate(betas):
            ol = [o.to(F64).clone().requires_grad_(True) for o in obj.split(split, dim=1)]
            dl = [x.to(F64).clone().requires_grad_(True) for x in deltas.split(split, dim=1)]
            ls = rp.PseudoLabRPN.losses(duck(-1.0, None, typ, beta), ab, ol, [l.clone() for l in labs], dl, mboxes, confs)
            q = "%s_b%d" % (typ, bi)
            d[q + "_loss_cls"], d[q + "_loss_loc"] = G.npy(ls["loss_rpn_cls"]), G.npy(ls["loss_rpn_loc"])
            gobj = torch.autograd.grad(ls["loss_rpn_cls"], ol, retain_graph=True)
            gdl = torch.autograd.grad(ls["loss_rpn_loc"], dl)
            d[q + "_gobj"], d[q + "_gdeltas"] = G.npy(torch.cat(gobj, dim=1)), G.npy(torch.cat(gdl, dim=1))
    lv = [(8, 6), (4, 3)]
    for name, sizes, ratios, off in (("a6", [[32, 64]], [[0.5, 1.0, 2.0]], 0.0), ("a1", [[32], [64]], [[1.0]], 0.0),
                                     ("off", [[32], [64]], [[0.5, 1.0, 2.0]], 0.5)):
        for l, t in enumerate(default_anchor_generator(lv, STRIDES, sizes, ratios, off)):
            d["anc_%s_l%d" % (name, l)] = G.npy(t)
    out = os.path.join(HERE, "rpn_keys.npz")
    np.savez_compressed(out, **d)
    print("rpn_keys.npz:", len(d), "arrays,", os.path.getsize(out), "bytes")
    for ti in range(3):
        print("threshold", THRESHOLDS[ti], "labels", [int((d["labels_t%d" % ti] == v).sum()) for v in (-1, 0, 1)],
              "sampled", [int((d["sampled_t%d" % ti] == v).sum()) for v in (-1, 0, 1)])


if __name__ == "__main__":
    main()
