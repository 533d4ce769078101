"""csrc/basicblock.hip: one frozen 64-channel identity BasicBlock (every res2 block of R-18 / R-34) as ONE kernel with c1 in LDS, in both
builds of the kernel library - against the two conv launches it replaces, against torch on the same rounded operands, and bit for bit
against the fp64 expression on operands for which fp32 accumulation is exact (tests/basicblock_ref.py)."""
import pytest
import torch
import torch.nn.functional as F

from tests import basicblock_ref as B
from tests import exact_conv_ref as R

pytestmark = pytest.mark.gpu

# ragged tiles (H % 8, W % 16 != 0), several images, one exact tile per image, an image smaller than one 8 x 16 tile, an image thinner
# than the two-pixel halo of x
SHAPES = [(2, 24, 48), (1, 21, 37), (3, 8, 16), (1, 5, 7), (1, 2, 19)]


@pytest.fixture(params=["bf16", "fp16"])
def h16(request):
    from ubteacher import hip
    hip.set_h16(request.param)
    try:
        yield hip.h16_dtype()
    finally:
        hip.set_h16("bf16")


def relerr(a, b):
    return (a.double() - b.double()).abs().max().item() / (b.double().abs().max().item() + 1e-12)


def _operands(shape, h16, C=64):
    """as in test_fused_frozen_bottleneck_equals_the_conv_chain: x a clamped normal, weights of about 0.05, scales in 0.5 .. 1.5"""
    N, H, W = shape
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(N, H, W, C, generator=g).clamp(min=0) * 0.7).to(h16).cuda()
    w1 = (torch.randn(C, 9 * C, generator=g) * 0.05).to(h16).cuda()
    w2 = (torch.randn(C, 9 * C, generator=g) * 0.05).to(h16).cuda()
    s1, b1, s2, b2 = [(torch.rand(C, generator=g) + 0.5).cuda() if i % 2 == 0 else (torch.randn(C, generator=g) * 0.2).cuda() for i in range(4)]
    return x, w1, w2, s1, b1, s2, b2


def _chain(x, w1, w2, s1, b1, s2, b2):
    from ubteacher import hip
    c1 = hip.conv2d_fwd_bf16(x, w1, scale=s1, bias=b1, relu=True, kh=3, kw=3, pad=1)
    return hip.conv2d_fwd_bf16(c1, w2, scale=s2, bias=b2, relu=True, kh=3, kw=3, pad=1, residual=x), c1


@pytest.mark.parametrize("shape", SHAPES)
def test_fused_basicblock_equals_the_conv_chain(shape, h16):
    """against conv2d_fwd_bf16 twice (same 16-bit rounding of c1, fp32 accumulation in another order): at most 4 output ulps of the largest
    value apart, fewer than 5 % of the elements differing (the bounds of the bottleneck's test: c1 may flip by one 16-bit ulp between two
    accumulation orders, which then propagates through conv2); against torch on the same rounded operands with c1 rounded to 16 bits;
    a second call returns the same bits"""
    from ubteacher import hip
    N, H, W = shape
    ops_ = _operands(shape, h16)
    x, w1, w2, s1, b1, s2, b2 = ops_
    y = hip.basicblock_fwd_bf16(*ops_)
    y2, _ = _chain(*ops_)
    assert y.shape == y2.shape == (N, H, W, 64) and y.dtype == h16
    d = (y.float() - y2.float()).abs()
    ulp = 2 ** -7 if h16 == torch.bfloat16 else 2 ** -10
    print("fused vs chain: max |d| %.4g (bound %.4g), share differing %.4g" % (float(d.max()), 4 * ulp * float(y2.float().abs().max()),
                                                                                float((d > 0).float().mean())))
    assert float(d.max()) <= 4 * ulp * float(y2.float().abs().max()), float(d.max())
    assert float((d > 0).float().mean()) < 0.05
    xf = x.float().permute(0, 3, 1, 2)
    v = lambda t: t.view(1, -1, 1, 1)
    k4 = lambda w: w.float().view(64, 3, 3, 64).permute(0, 3, 1, 2)
    t1 = F.relu(F.conv2d(xf, k4(w1), padding=1) * v(s1) + v(b1)).to(h16).float()
    t2 = F.relu(F.conv2d(t1, k4(w2), padding=1) * v(s2) + v(b2) + xf)
    assert relerr(y.float().permute(0, 3, 1, 2), t2) < (2e-2 if h16 == torch.bfloat16 else 3e-3)
    assert torch.equal(y, hip.basicblock_fwd_bf16(*ops_))     # deterministic


def test_basicblock_supported_and_bad_arguments(h16):
    from ubteacher import hip
    assert hip.basicblock_supported(64, 1, False)
    assert not hip.basicblock_supported(128, 1, False) and not hip.basicblock_supported(64, 2, True) and not hip.basicblock_supported(64, 1, True)
    x, w1, w2, s1, b1, s2, b2 = _operands((1, 4, 4), h16, C=128)
    with pytest.raises(RuntimeError, match="-1000"):          # UTV2_EARG
        hip.basicblock_fwd_bf16(x, w1, w2, s1, b1, s2, b2)
    x, w1, w2, s1, b1, s2, b2 = _operands((1, 4, 4), h16)
    with pytest.raises(RuntimeError, match="-1000"):          # y == x
        hip.basicblock_fwd_bf16(x, w1, w2, s1, b1, s2, b2, out=x)


@pytest.mark.parametrize("shape", B.SHAPES)
def test_fused_basicblock_is_exact(shape, h16):
    """fused kernel == the two conv launches == the fp64 expression with c1 rounded once, bit for bit (the preconditions - exact domain,
    live ReLUs, a decisive residual - are asserted on the CPU reference before any GPU call)"""
    from ubteacher import hip
    o = B.basicblock_operands(shape)
    y64, c1_64, _ = B.basicblock_domain(o, h16)
    d = {k: (v.cuda().to(h16) if k[0] in "xw" else v.cuda()) for k, v in o.items()}
    assert all(torch.equal(d[k].float().cpu(), o[k]) for k in d)
    args = [d[k] for k in ("x", "w1", "w2", "s1", "b1", "s2", "b2")]
    y = hip.basicblock_fwd_bf16(*args)
    y2, c1 = _chain(*args)
    assert torch.equal(c1.cpu(), R.to_out(c1_64, h16))
    want = R.to_out(y64, h16)
    assert torch.equal(y2.cpu(), want)
    assert torch.equal(y.cpu(), want) and torch.equal(y, y2)
