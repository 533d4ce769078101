"""fp64 autograd reference of the ROI box loss with per-class regression (roi_heads/fast_rcnn.py:950-959, :1036-1045): a foreground row's
deltas / std logits are the four columns 4 * cls .. 4 * cls + 3 of its [4K] row.  The gather is the only new step: the loss on the gathered
columns is tests/loss_ref64.roi_box_loss as it is, and its per-element addends are scattered back; every other element has no addend."""
import torch

from tests import loss_ref64 as L64


def percls_case(R, K, seed):
    """loss_ref64.roi_case (rows ON the kernel's branch points) spread over [R, 4K] heads: the selected columns hold the case's values,
    every other column random.  Classes: -1 (empty), K (background), 0 and K - 1 (the last four columns) are all present."""
    c = L64.roi_case(R, seed)
    g = torch.Generator().manual_seed(seed + 1)
    cls = c["cls"].clone()
    fg = (cls >= 0) & (cls < 80)
    cls[fg] = cls[fg] % K
    cls[~fg & (cls >= 0)] = K
    f = torch.nonzero(fg).squeeze(1)
    cls[f[0]], cls[f[1]] = 0, K - 1
    deltas = torch.randn((R, 4 * K), generator=g) * 0.5
    std = torch.randn((R, 4 * K), generator=g)
    col = select_columns(cls, K)
    deltas.scatter_(1, col, c["mat"][:, :4])
    std.scatter_(1, col, c["mat"][:, 4:])
    return {"deltas": deltas, "std": std, "cls": cls, "prop": c["prop"], "gtb": c["gtb"], "col": col}


def select_columns(cls, K):
    """[R, 4] column indices of each row's class (background / empty rows: class 0's, masked by the loss)"""
    fg = (cls >= 0) & (cls < K)
    return (4 * torch.where(fg, cls, torch.zeros_like(cls)))[:, None] + torch.arange(4)[None, :]


def roi_box_loss_pc(deltas, stdl, cls, prop, gtb, K, mode, wx, wy, scale_clamp):
    """-> (per-row loss [R], [addends of gd [R, 4K]], [addends of gs [R, 4K]])"""
    col = select_columns(cls, K)
    loss, gd, gs = L64.roi_box_loss(torch.gather(deltas, 1, col), torch.gather(stdl, 1, col), cls, prop, gtb, None, K, mode, wx, wy,
                                    scale_clamp, 0.0, 0.0)
    fg = ((cls >= 0) & (cls < K))[:, None].to(deltas.dtype)

    def spread(parts):
        return [torch.zeros_like(deltas).scatter_(1, col, p * fg) for p in parts]
    return loss, spread(gd), spread(gs)
