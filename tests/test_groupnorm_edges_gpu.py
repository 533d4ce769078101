"""Every segmented GroupNorm entry at the smallest shapes where its row walk and its segment-edge logic branch, with the epilogue
partials (part32 / part64) built in torch - no conv involved.

Channels: C = 32 / G = 4 (32 row lanes: one unrolled step of the chunk walk covers 128 rows) and C = 256 / G = 32 (4 row lanes: 16 rows).
Segments [1, 31, 33, 64, 65, 255, 256, 257, 130] start off the 32- and 64-row grids and cover: a segment inside one block, one that
straddles a block boundary without holding a whole block, 255 / 256 / 257 rows around the chunk size, an unrolled loop that runs zero
times and exactly once with an empty tail.

Reference: per-segment F.group_norm + ReLU under autograd in float64 (CPU, once per C).  x and dy lie on a grid (multiples of 1/16 and
1/32, 7 significant bits) that fp32, bf16 and fp16 all hold exactly, so one reference serves the three element types and "the stored x
and dy" are the same numbers everywhere.  Tolerances are the project's:
  fp32            test_groupnorm_relu_fwd_bwd: y rtol 1e-4 / atol 1e-5, dx 1e-3 / 1e-5, dgamma and dbeta 1e-4 / 1e-4
  16-bit          the GroupNorm block of test_elementwise_bf16: the same statistics and parameter gradients bit for bit, y and dx = the fp32
                  kernel's result on the same values rounded once
  _p32 statistics test_groupnorm_statistics_from_the_conv_epilogue: mean rtol 1e-5 / atol 1e-6, rstd rtol 1e-5
  _p64 dx         test_dgrad_epilogue_partials_and_groupnorm_backward: the neighbouring 16-bit value at most, beyond 1e-5 of the range
The ReLU mask of an element whose pre-activation is within rounding of zero is ill-conditioned in any arithmetic; the seeds are chosen
(on the CPU, from the float64 reference alone) so that no pre-activation lies within 2e-6 of zero, and the fixture asserts it."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SEG_ROWS = [1, 31, 33, 64, 65, 255, 256, 257, 130]
ROWS = sum(SEG_ROWS)
SHAPES = {32: (4, 1), 256: (32, 1)}       # C -> (G, seed)
EPS = 1e-5
MARGIN = 2e-6


def close(a, b, rtol, atol):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.allclose(a, b, rtol=rtol, atol=atol), (float((a - b).abs().max()), float(b.abs().max()))


@functools.lru_cache(maxsize=None)
def case(C):
    """inputs (fp32, on the grid) and the float64 reference"""
    G, seed = SHAPES[C]
    g = torch.Generator().manual_seed(seed)
    x = ((torch.randn(ROWS, C, generator=g) * 2 + 0.5) * 16).round().clamp(-127, 127) / 16
    dy = (torch.randn(ROWS, C, generator=g) * 32).round().clamp(-127, 127) / 32
    ga = torch.rand(C, generator=g) + 0.5
    be = torch.randn(C, generator=g) * 0.1
    xr = x.double().requires_grad_(True)
    gar, ber = ga.double().requires_grad_(True), be.double().requires_grad_(True)
    pre, r0 = [], 0
    for n in SEG_ROWS:       # one segment = one "image" [1, C, n]
        pre.append(F.group_norm(xr[r0:r0 + n].t().unsqueeze(0), G, gar, ber, EPS).squeeze(0).t())
        r0 += n
    pre = torch.cat(pre)
    y = F.relu(pre)
    y.backward(dy.double())
    assert float(pre.detach().abs().min()) > MARGIN, "pick another seed: a pre-activation within rounding of zero"
    return dict(C=C, G=G, x=x, dy=dy, ga=ga, be=be, y=y.detach(), pos=pre.detach() > 0, dx=xr.grad, dga=gar.grad, dbe=ber.grad)


def select(kind):
    """-> the torch dtype of `kind` after pointing the wrappers at its library"""
    from ubteacher import hip, ops
    ops.set_precision(kind)
    return torch.float32 if kind == "fp32" else hip.h16_dtype()


def bwd(c, dy, y, x, mean, rstd, beta=None, want_colsum=False):
    from ubteacher import hip
    dga, dbe = torch.zeros(c["C"], device="cuda"), torch.zeros(c["C"], device="cuda")
    out = hip.groupnorm_relu_seg_bwd(dy, y, x, SEG_ROWS, mean, rstd, c["ga"].cuda(), dga, dbe, c["G"], True, beta=beta, want_colsum=want_colsum)
    return (out[0] if want_colsum else out), dga, dbe


def pack_bits(t):
    b = (t > 0).reshape(-1, 8).to(torch.int32)
    return (b << torch.arange(8, device=t.device, dtype=torch.int32)).sum(-1).to(torch.uint8)


@pytest.mark.parametrize("kind", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("C", [32, 256])
def test_plain_forward_and_backward(C, kind):
    from ubteacher import hip
    c = case(C)
    dt = select(kind)
    ga, be = c["ga"].cuda(), c["be"].cuda()
    x32, dy32 = c["x"].cuda(), c["dy"].cuda()
    # the fp32 kernels against float64; mask read from y, and recomputed from x (beta given)
    y32, m, r = hip.groupnorm_relu_seg_fwd(x32, SEG_ROWS, ga, be, c["G"], EPS)
    close(y32, c["y"], 1e-4, 1e-5)
    ref32 = {}
    for beta in (None, be):
        dx, dga, dbe = bwd(c, dy32, y32, x32, m, r, beta)
        close(dx, c["dx"], 1e-3, 1e-5)
        close(dga, c["dga"], 1e-4, 1e-4)
        close(dbe, c["dbe"], 1e-4, 1e-4)
        dxc, dgac, dbec = bwd(c, dy32, y32, x32, m, r, beta, want_colsum=True)
        assert torch.equal(dx, dxc) and torch.equal(dga, dgac) and torch.equal(dbe, dbec)
        ref32[beta is None] = (dx, dga, dbe)
    assert torch.equal(ref32[True][0], ref32[False][0])       # the two mask rules agree (no pre-activation near zero)
    if kind == "fp32":
        return
    # 16-bit: the same statistics, one rounding of y / dx, the same parameter gradients
    x16, dy16 = x32.to(dt), dy32.to(dt)
    assert torch.equal(x16.float(), x32) and torch.equal(dy16.float(), dy32)
    y16, m16, r16 = hip.groupnorm_relu_seg_fwd(x16, SEG_ROWS, ga, be, c["G"], EPS)
    assert torch.equal(m16, m) and torch.equal(r16, r) and torch.equal(y16, y32.to(dt))
    for beta in (None, be):
        want = bwd(c, dy32, y16.float(), x32, m, r, beta)     # the mask (y > 0) and x identical in both runs
        dx, dga, dbe = bwd(c, dy16, y16, x16, m, r, beta)
        assert torch.equal(dx, want[0].to(dt)) and torch.equal(dga, want[1]) and torch.equal(dbe, want[2])
        dxc, dgac, dbec = bwd(c, dy16, y16, x16, m, r, beta, want_colsum=True)
        assert torch.equal(dx, dxc) and torch.equal(dga, dgac) and torch.equal(dbe, dbec)


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("C", [32, 256])
def test_forward_from_part32_and_backward_from_part64(C, kind):
    from ubteacher import hip
    c = case(C)
    dt = select(kind)
    G = c["G"]
    ga, be = c["ga"].cuda(), c["be"].cuda()
    x16, dy16 = c["x"].cuda().to(dt), c["dy"].cuda().to(dt)
    # part32[b][g] = {sum x, sum x^2} over rows [32 b, 32 b + 32) of the stored x, blocks past the last row from zero padding
    nb = (ROWS + 31) // 32
    blk = torch.cat((x16.float(), torch.zeros(nb * 32 - ROWS, C, device="cuda"))).view(nb, 32, G, 8)
    part32 = hip.gn_part_buffer(ROWS, C, "cuda")
    part32.copy_(torch.stack((blk.sum(dim=(1, 3)), (blk * blk).sum(dim=(1, 3))), dim=-1))
    y0, m0, r0 = hip.groupnorm_relu_seg_fwd(x16, SEG_ROWS, ga, be, G, EPS)
    y1, m1, r1 = hip.groupnorm_relu_seg_fwd_p32(x16, SEG_ROWS, ga, be, part32, G, EPS)
    bits = torch.zeros(ROWS * C // 8, dtype=torch.uint8, device="cuda")
    y2, m2, r2 = hip.groupnorm_relu_seg_fwd_p32(x16, SEG_ROWS, ga, be, part32, G, EPS, relu_bits=bits)
    assert torch.equal(y1, y2) and torch.equal(m1, m2) and torch.equal(r1, r2)
    assert torch.allclose(m1, m0, rtol=1e-5, atol=1e-6) and torch.allclose(r1, r0, rtol=1e-5)
    d = (y1.float() - y0.float()).abs()                            # the same normalised output to one 16-bit rounding
    assert float(d.max()) <= (2.0 ** -7 if dt == torch.bfloat16 else 2.0 ** -10) * float(y0.float().abs().max()) and float((d > 0).float().mean()) < 1e-3
    stored = pack_bits(y1.float())
    assert torch.equal(bits & stored, stored)                      # every stored positive has its bit
    assert torch.equal(bits, pack_bits(c["pos"].cuda().float()))   # and the plane is the sign of the fp32 value
    # part64[b][c] = {sum g, sum g x} over rows [64 b, 64 b + 64) of the stored masked gradient and x
    mask = ((bits.view(-1, 1).to(torch.int32) >> torch.arange(8, device="cuda", dtype=torch.int32)) & 1).bool().view(ROWS, C)
    gm = torch.where(mask, dy16, torch.zeros_like(dy16))
    nb = (ROWS + 63) // 64
    pad = torch.zeros(nb * 64 - ROWS, C, device="cuda")
    g64, x64 = torch.cat((gm.float(), pad)).view(nb, 64, C), torch.cat((x16.float(), pad)).view(nb, 64, C)
    part64 = hip.gnb_part_buffer(ROWS, C, "cuda")
    part64.copy_(torch.stack((g64.sum(1), (g64 * x64).sum(1)), dim=-1))
    dx_ref, dga_ref, dbe_ref = bwd(c, dy16, y1, x16, m1, r1, be)
    res = []
    for want_colsum in (False, True):
        dga, dbe = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        out = hip.groupnorm_seg_bwd_p64(gm, x16, SEG_ROWS, m1, r1, ga, dga, dbe, G, part64, want_colsum=want_colsum)
        res.append((out[0] if want_colsum else out, dga, dbe))
    assert all(torch.equal(a, b) for a, b in zip(*res))
    dx, dga, dbe = res[0]
    # dx: the neighbouring 16-bit value at most, on a small fraction of the elements; 1e-5 of the range where the terms cancel
    af, bf = dx.float(), dx_ref.float()
    d = (af - bf).abs()
    ulp = torch.maximum(af.abs(), bf.abs()) * (2.0 ** -7 if dt == torch.bfloat16 else 2.0 ** -10)
    atol = 1e-5 * float(bf.abs().max())
    worst = float(((d - atol).clamp(min=0) / (ulp + 1e-30)).max())
    assert worst <= 1.01 and float((d > 0).float().mean()) < 2e-2, (worst, float((d > 0).float().mean()))
    # parameter gradients: sums taken in another order, relative to the sum of magnitudes
    seg_of_row = torch.repeat_interleave(torch.arange(len(SEG_ROWS), device="cuda"), torch.tensor(SEG_ROWS, device="cuda"))
    xhat = (x16.double() - m1.double()[seg_of_row].repeat_interleave(8, dim=1)) * r1.double()[seg_of_row].repeat_interleave(8, dim=1)
    for got, ref, t64 in ((dga, dga_ref, gm.double() * xhat), (dbe, dbe_ref, gm.double())):
        assert float((got - ref).abs().max() / t64.abs().sum(0).max()) < 4e-6


def _iarr(vals):
    return ctypes.cast((ctypes.c_int * len(vals))(*vals), ctypes.c_void_p)


def test_argument_errors_are_refused_on_the_host():
    """a null seg_rows, a negative row count, nseg = 0 and nseg = 161 on every GroupNorm entry; a dtype code of 7 on relu_bwd_scale and
    the max-pool pair: a non-zero status (the wrapper raises), before any launch"""
    from ubteacher import hip
    select("bf16")
    C, G, rows = 32, 4, 256
    p = lambda t: t.data_ptr()
    x, y, dy, dx = (torch.zeros(rows, C, dtype=torch.bfloat16, device="cuda") for _ in range(4))
    # fp32 operands, each larger than any accepted call would touch
    ga, be, mean, rstd, dga, dbe, part, ws = (torch.ones(rows * C, device="cuda") for _ in range(8))
    bad_segs = ((1, None), (3, _iarr([4, -1, 4])), (0, _iarr([4])), (161, _iarr([1] * 161)))
    good = (1, _iarr([4]))

    def entries(nseg, sr):
        s = hip._stream()
        return (("utv2_groupnorm_relu_seg_fwd", p(x), p(ga), p(be), p(y), p(mean), p(rstd), p(ws), nseg, sr, C, G, EPS, 1, 1, s),
                ("utv2_groupnorm_relu_seg_fwd_p32", p(x), p(ga), p(be), p(y), p(mean), p(rstd), p(part), nseg, sr, C, G, EPS, 1, None, s),
                ("utv2_groupnorm_relu_seg_bwd", p(dy), p(y), p(x), p(mean), p(rstd), p(ga), p(be), p(dx), p(dga), p(dbe), p(ws), nseg, sr, C, G,
                 1, 1, None, s),
                ("utv2_groupnorm_seg_bwd_p64", p(dy), p(x), p(mean), p(rstd), p(ga), p(dx), p(dga), p(dbe), p(ws), nseg, sr, C, G, p(part),
                 None, s))

    for args in entries(*good):       # the argument lists themselves are accepted
        hip.call(*args)
    for nseg, sr in bad_segs:
        for args in entries(nseg, sr):
            with pytest.raises(RuntimeError):
                hip.call(*args)
    s = hip._stream()
    for args in (("utv2_relu_bwd_scale", p(dy), p(y), None, p(dx), rows, C, 7, s),
                 ("utv2_maxpool3x3s2_nhwc", p(x), 7, p(y), 1, 1, 8, 8, C, 4, 4, s),
                 ("utv2_maxpool3x3s2_nhwc", p(x), 1, p(y), 7, 1, 8, 8, C, 4, 4, s),
                 ("utv2_maxpool3x3s2_bwd_nhwc", p(x), 7, p(dy), p(dx), 1, 1, 8, 8, C, 4, 4, 1, s),
                 ("utv2_maxpool3x3s2_bwd_nhwc", p(x), 1, p(dy), p(dx), 7, 1, 8, 8, C, 4, 4, 1, s)):
        with pytest.raises(RuntimeError):
            hip.call(*args)
    torch.cuda.synchronize()
