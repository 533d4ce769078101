"""float64 reference of the per-ROI GroupNorm (+ ReLU) kernels (csrc/groupnorm_roi.hip) and the yardstick their tolerance comes from.

reference(...)   torch.nn.functional.group_norm (+ ReLU) in float64 on the CPU, autograd for the backward, on the inputs AS THE KERNEL
                 READS THEM (for 16-bit I/O: x and dy rounded to that type first).
The tolerance is not a chosen number: the SAME function in float32 (torch's own CPU kernels) is run on the same inputs and its maximum
error against float64 is measured per output (y, dx, dgamma, dbeta); the fp32 kernel may be 4 times as far off (its summation order
over the at most 196 * 8 elements of a group differs), and a 16-bit output one ulp of its type at the output's magnitude on top (a
value next to a rounding boundary).

ReLU: the sign of a pre-activation within rounding of zero is ill-conditioned in any arithmetic, and one flipped mask element changes the
gradient of its whole (ROI, group) cell and of its channel's dgamma / dbeta.  Cells and channels where an fp32 evaluation disagrees
with float64 on a sign are left out of the comparison; they may be at most 0.1 % of an output's elements (SHARE), and the seeds are
chosen so that torch's fp32 result stays inside that share (checked here, on the CPU)."""
import functools

import torch
import torch.nn.functional as F

EPS = 1e-5
SHARE = 1e-3

# (R, HW, C, G): R 1 / 5 / 2100 (one workgroup; several; past the 1024-workgroup grid: the grid-stride and the partial-sum stage),
# HW 1 / 4 / 49 / 196, 128 and 256 channels in 32 groups - and the two shapes at which the kernels take another path:
# 196 x 512 (more than 13 rows per thread: the ROI is read again instead of kept in registers) and 96 channels (24 channel quads do
# not divide the 256 threads: 16 of them idle)
SHAPES = [(R, HW, C, 32) for R in (1, 5) for HW in (1, 4, 49, 196) for C in (128, 256)] + [(2100, 4, 128, 32), (3, 196, 512, 32), (3, 5, 96, 8)]
OFFCENTRE = [(5, 49, 256, 32), (5, 49, 128, 32)]


def inputs(R, HW, C, G, offcentre=False):
    """fp32 x, dy [R, HW, C], gamma, beta [C].  From three ROIs on: ROI 1 is all zero (a padding slot of the fixed-size ROI batch) and
    group 0 of ROI 2 holds a single non-zero element.  offcentre: mean 100, std 1."""
    g = torch.Generator().manual_seed(1000 * R + 7 * HW + C + (1 if offcentre else 0))
    x = torch.randn(R, HW, C, generator=g)
    x = x + 100.0 if offcentre else x * 1.5 + 0.3
    dy = torch.randn(R, HW, C, generator=g)
    ga = torch.rand(C, generator=g) + 0.5
    be = torch.randn(C, generator=g) * 0.1
    if R >= 3 and not offcentre:
        x[1] = 0.0
        x[2, :, :C // G] = 0.0
        x[2, HW // 2, 1] = 3.0
    return x, dy, ga, be


def group_norm(x, dy, ga, be, G, relu, dtype):
    """-> dict(pre, y, dx, dga, dbe) in `dtype` arithmetic; x, dy [R, HW, C]"""
    xr = x.detach().to(dtype).clone().requires_grad_(True)
    gar, ber = ga.detach().to(dtype).clone().requires_grad_(True), be.detach().to(dtype).clone().requires_grad_(True)
    pre = F.group_norm(xr.permute(0, 2, 1), G, gar, ber, EPS).permute(0, 2, 1)
    y = F.relu(pre) if relu else pre
    y.backward(dy.to(dtype))
    return dict(pre=pre.detach(), y=y.detach(), dx=xr.grad, dga=gar.grad, dbe=ber.grad)


def ulp(ref, dt):
    """one ulp of the 16-bit type `dt` at the magnitude of each element of ref (float64)"""
    mant, emin = (7, -126) if dt == torch.bfloat16 else (10, -14)
    a = ref.abs()
    e = torch.frexp(a).exponent.to(torch.float64) - 1
    e = torch.where(a == 0, torch.full_like(e, emin), e).clamp_(min=emin)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - mant)


def flipped(pre, pre64, C, G):
    """where an evaluation `pre` of the pre-activation disagrees with float64 on the ReLU mask -> (cells [R, G] bool, channels [C] bool)"""
    d = (pre.double() > 0) != (pre64 > 0)
    R, HW, _ = d.shape
    return d.view(R, HW, G, C // G).any(dim=3).any(dim=1), d.any(dim=0).any(dim=0)


@functools.lru_cache(maxsize=None)
def case(R, HW, C, G, relu, offcentre=False, io=None):
    """inputs as the kernel reads them (io: None = fp32, or the 16-bit torch dtype), the float64 reference, torch's fp32 error err32 per
    output, and the cells / channels torch's fp32 mask leaves out"""
    x, dy, ga, be = inputs(R, HW, C, G, offcentre)
    if io is not None:
        x, dy = x.to(io).float(), dy.to(io).float()
    ref = group_norm(x, dy, ga, be, G, relu, torch.float64)
    f32 = group_norm(x, dy, ga, be, G, relu, torch.float32)
    cells, chans = flipped(f32["pre"], ref["pre"], C, G) if relu else (torch.zeros(R, G, dtype=torch.bool), torch.zeros(C, dtype=torch.bool))
    return dict(R=R, HW=HW, C=C, G=G, relu=relu, io=io, x=x, dy=dy, ga=ga, be=be, ref=ref, f32=f32, cells=cells, chans=chans)


def keep_masks(c, cells, chans):
    """what stays in the comparison once the (ROI, group) cells and channels in `cells` / `chans` are left out, per output; asserts
    that at most SHARE of each output is left out"""
    R, HW, C, G = c["R"], c["HW"], c["C"], c["G"]
    elem = ~cells[:, None, :, None].expand(R, HW, G, C // G).reshape(R, HW, C)
    keep = dict(y=torch.ones(R, HW, C, dtype=torch.bool), dx=elem, dga=~chans, dbe=~chans)
    for k, m in keep.items():
        assert float((~m).double().mean()) <= SHARE, "%s: %d of %d elements left out of the comparison: pick another seed" % (k, int((~m).sum()), m.numel())
    return keep


def bounds(c, keep):
    """-> {output: (err32, bound tensor)}: 4 x torch's own fp32 error over the kept elements, plus one 16-bit ulp for a 16-bit output"""
    out = {}
    for k in ("y", "dx", "dga", "dbe"):
        ref, m = c["ref"][k], keep[k]
        err32 = float(((c["f32"][k].double() - ref).abs() * m).max())
        b = torch.full_like(ref, 4.0 * err32)
        if c["io"] is not None and k in ("y", "dx"):
            b = b + ulp(ref, c["io"])
        out[k] = (err32, b)
    return out
