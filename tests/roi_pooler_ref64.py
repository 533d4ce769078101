"""Pure-torch restatement of the ROI pooler's three types (MODEL.ROI_BOX_HEAD.POOLER_TYPE "ROIAlignV2" / "ROIAlign" / "ROIPool", the
RoIAlign ones with POOLER_SAMPLING_RATIO 0 or fixed) - torchvision's roi_align / roi_pool behind Detectron2's ROIPooler level assignment.
Differentiable through autograd (RoIPool: gather by argmax); values are computed in the features' dtype (fp64 or fp32).

RoIAlign geometry is computed in the features' dtype too.  RoIPool geometry is ALWAYS fp32: its rule is stated in C floats (roundf of
the scaled corners, `bin = roi / P` as a float, floor / ceil of float products), and which pixels a window holds depends on those
roundings - 7 * float(3 / 7) is not 3.

One level: roi_align / roi_pool take feat [C, H, W] of one image and rois [R, 4], like oracle.utv2_oracle.roi_align.
All levels: roi_pooler takes NCHW level lists, rois [R, 4], the image index per ROI and an optional valid mask."""
import math

import torch

POOLERS = ("ROIAlignV2", "ROIAlign", "ROIPool")


def _axis(v, L):
    """tap rule of one axis: a sample outside [-1, L] contributes 0; the position is clamped at 0; floor >= L - 1 puts both taps on
    L - 1 with fraction 0"""
    ok = (v >= -1.0) & (v <= L)
    v = v.clamp(min=0)
    lo = v.floor().long()
    edge = lo >= L - 1
    lo = torch.where(edge, torch.full_like(lo, L - 1), lo)
    hi = torch.where(edge, lo, lo + 1)
    v = torch.where(edge, lo.to(v.dtype), v)
    return ok, lo, hi, v - lo.to(v.dtype)


def roi_align(feat, rois, scale, out=7, aligned=True, sampling_ratio=0):
    """feat [C, H, W]; rois [R, 4] xyxy in image coordinates -> [R, C, out, out]"""
    C, H, W = feat.shape
    dt = feat.dtype
    res = []
    off = 0.5 if aligned else 0.0
    ar = torch.arange(out, dtype=dt)
    for r in range(rois.shape[0]):
        x1, y1, x2, y2 = [rois[r, i].to(dt) * scale - off for i in range(4)]
        rw, rh = x2 - x1, y2 - y1
        if not aligned:
            rw, rh = rw.clamp(min=1.0), rh.clamp(min=1.0)
        bw, bh = rw / out, rh / out
        gh = sampling_ratio if sampling_ratio > 0 else int(math.ceil(float(rh / out)))
        gw = sampling_ratio if sampling_ratio > 0 else int(math.ceil(float(rw / out)))
        if gh <= 0 or gw <= 0:
            res.append(feat.new_zeros((C, out, out)) + 0 * feat.sum())
            continue
        ys = (y1 + ar[:, None] * bh + (torch.arange(gh, dtype=dt)[None, :] + 0.5) * bh / gh).reshape(-1)
        xs = (x1 + ar[:, None] * bw + (torch.arange(gw, dtype=dt)[None, :] + 0.5) * bw / gw).reshape(-1)
        oky, yl, yh, ly = _axis(ys, H)
        okx, xl, xh, lx = _axis(xs, W)
        hy, hx = 1 - ly, 1 - lx
        v = (feat[:, yl][:, :, xl] * (hy[:, None] * hx[None, :]) + feat[:, yl][:, :, xh] * (hy[:, None] * lx[None, :]) +
             feat[:, yh][:, :, xl] * (ly[:, None] * hx[None, :]) + feat[:, yh][:, :, xh] * (ly[:, None] * lx[None, :]))
        v = v * (oky[:, None] & okx[None, :]).to(dt)
        res.append(v.view(C, out, gh, out, gw).sum(dim=(2, 4)) / max(gh * gw, 1))
    return torch.stack(res) if res else feat.new_zeros((0, C, out, out))


def _round_half_away(x):
    """C roundf on an fp32 tensor (torch.round goes to even)"""
    t = torch.trunc(x)
    return t + torch.where((x - t).abs() >= 0.5, torch.sign(x), torch.zeros_like(x))


def _pool_windows(first, last, P, size):
    """[P] window starts and ends of one axis for the rounded corners first / last: fp32 arithmetic, clipped to [0, size]"""
    n = torch.clamp(last - first + 1, min=1).to(torch.float32)
    b = n / torch.tensor(float(P), dtype=torch.float32)
    p = torch.arange(P, dtype=torch.float32)
    lo = (torch.floor(p * b).long() + first).clamp(0, size)
    hi = (torch.ceil((p + 1) * b).long() + first).clamp(0, size)
    return lo, hi


def roi_pool(feat, rois, scale, out=7, return_argmax=False):
    """feat [C, H, W]; rois [R, 4] -> [R, C, out, out] (and argmax [R, C, out, out] int64: pixel index y * W + x, -1 = empty window).
    The maximum is the FIRST one of the window in row-major order (torch.argmax returns the first maximal value)."""
    C, H, W = feat.shape
    flat = feat.reshape(C, H * W)
    res, args = [], []
    for r in range(rois.shape[0]):
        c = _round_half_away(rois[r].to(torch.float32) * torch.tensor(scale, dtype=torch.float32)).long()
        ws, we = _pool_windows(c[0], c[2], out, W)
        hs, he = _pool_windows(c[1], c[3], out, H)
        y0, y1, x0, x1 = int(hs.min()), int(he.max()), int(ws.min()), int(we.max())
        if y1 <= y0 or x1 <= x0:
            res.append(feat.new_zeros((C, out, out)) + 0 * feat.sum())
            args.append(torch.full((C, out, out), -1, dtype=torch.long))
            continue
        yy, xx = torch.arange(y0, y1), torch.arange(x0, x1)
        my = (yy[None, :] >= hs[:, None]) & (yy[None, :] < he[:, None])          # [out, h]
        mx = (xx[None, :] >= ws[:, None]) & (xx[None, :] < we[:, None])          # [out, w]
        m = (my[:, None, :, None] & mx[None, :, None, :]).reshape(out * out, -1)  # [bins, h * w], row-major inside the crop
        crop = feat.detach()[:, y0:y1, x0:x1].reshape(C, 1, -1)
        neg = torch.full((), -float("inf"), dtype=feat.dtype)
        k = torch.argmax(torch.where(m[None], crop, neg), dim=2)                  # [C, bins]: first maximum
        gidx = (y0 + k // (x1 - x0)) * W + x0 + k % (x1 - x0)
        nonempty = m.any(dim=1)[None, :].expand(C, -1)
        v = torch.where(nonempty, flat.gather(1, gidx), feat.new_zeros(()))
        res.append(v.view(C, out, out))
        args.append(torch.where(nonempty, gidx, torch.full_like(gidx, -1)).view(C, out, out))
    y = torch.stack(res) if res else feat.new_zeros((0, C, out, out))
    if return_argmax:
        return y, (torch.stack(args) if args else torch.zeros((0, C, out, out), dtype=torch.long))
    return y


def one_level(pooler, sampling_ratio=0):
    """the single-level function of a pooler type with the signature of oracle.utv2_oracle.roi_align(feat, rois, scale, out)"""
    assert pooler in POOLERS
    if pooler == "ROIPool":
        return lambda feat, rois, scale, out=7: roi_pool(feat, rois, scale, out)
    return lambda feat, rois, scale, out=7: roi_align(feat, rois, scale, out, pooler == "ROIAlignV2", sampling_ratio)


def assign_levels(rois, num_levels=4, min_level=2):
    """D2 assign_boxes_to_levels: canonical size 224 at level 4, clamped to the pooler's levels -> level index from 0"""
    area = (rois[:, 2] - rois[:, 0]) * (rois[:, 3] - rois[:, 1])
    lv = torch.floor(4 + torch.log2(torch.sqrt(area.float()) / 224 + 1e-8))
    return lv.clamp(min_level, min_level + num_levels - 1).long() - min_level


def roi_pooler(feats, rois, roi_batch, out=7, pooler="ROIAlignV2", sampling_ratio=0, scales=(1 / 4, 1 / 8, 1 / 16, 1 / 32), min_level=2,
               roi_valid=None, return_argmax=False):
    """feats: NCHW level list; rois [R, 4]; roi_batch [R] image index; roi_valid [R] (invalid slots: zero output, no gradient,
    argmax -1) -> [R, C, out, out] (and, for "ROIPool" with return_argmax, the argmax inside each ROI's own level)"""
    assert pooler in POOLERS
    R, C = rois.shape[0], feats[0].shape[1]
    lv = assign_levels(rois, len(feats), min_level)
    ys, args = [], []
    for r in range(R):
        if roi_valid is not None and not bool(roi_valid[r]):
            ys.append(feats[0].new_zeros((C, out, out)))
            args.append(torch.full((C, out, out), -1, dtype=torch.long))
            continue
        f = feats[int(lv[r])][int(roi_batch[r])]
        if pooler == "ROIPool":
            y, a = roi_pool(f, rois[r:r + 1], scales[int(lv[r])], out, return_argmax=True)
            args.append(a[0])
        else:
            y = roi_align(f, rois[r:r + 1], scales[int(lv[r])], out, pooler == "ROIAlignV2", sampling_ratio)
        ys.append(y[0])
    y = torch.stack(ys) if ys else feats[0].new_zeros((0, C, out, out))
    if return_argmax:
        assert pooler == "ROIPool"
        return y, torch.stack(args)
    return y
