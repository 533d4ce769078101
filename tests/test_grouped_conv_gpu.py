"""Grouped 3x3 conv kernels (csrc/conv_grouped.hip; the ResNeXt conv2) against torch.nn.functional.conv2d(..., groups=G) on the CPU:
forward with the FrozenBN / ReLU epilogue, dgrad with the folded multiplier, the producer's ReLU mask and a residual, wgrad with the
row scale.  fp32 operands: 2e-4 relative; 16-bit operands: against the fp32 conv of the rounded operands, 2e-4 with fp32 output and
close16 with 16-bit output (the bounds of test_conv_bf16_gpu.py).  The weight gradient is bit-identical from run to run."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (g channels per group, G groups): C = g * G
SHAPES = [(4, 16), (8, 32), (16, 8), (32, 8), (64, 4)]


def relerr(a, b):
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-12)


def close16(y, ref):
    y = y.float()
    tol = 2.0 ** -8 * ref.abs() + 2e-4 * ref.abs().max()
    return bool(((y - ref).abs() <= tol).all())


@pytest.fixture(params=["fp32", "bf16", "fp16"])
def mode(request):
    from ubteacher import hip
    hip.set_h16("fp16" if request.param == "fp16" else "bf16")
    yield request.param
    hip.set_h16("bf16")


def _ops(mode):
    from ubteacher import hip
    return torch.float32 if mode == "fp32" else hip.h16_dtype()


def _nhwc(t, dt):
    return t.permute(0, 2, 3, 1).contiguous().cuda().to(dt)


def _nchw(t):
    return t.float().cpu().permute(0, 3, 1, 2)


def _rnd(t, dt):
    return t.to(dt).to(torch.float32)


def _check(mode, y, ref):
    if mode == "fp32" or y.dtype == torch.float32:
        assert relerr(y.float(), ref) < 2e-4, relerr(y.float(), ref)
    else:
        assert close16(y, ref)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("g,G", SHAPES)
def test_gconv_fwd(mode, g, G, stride):
    from ubteacher import hip
    C, N, H, W = g * G, 2, 13, 11
    dt = _ops(mode)
    gen = torch.Generator().manual_seed(g * 100 + stride)
    x = torch.randn(N, C, H, W, generator=gen)
    w = torch.randn(C, g, 3, 3, generator=gen) * (1.0 / (3 * g ** 0.5))
    sc, sh = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.1
    xr, wr = _rnd(x, dt), _rnd(w, dt)
    conv = F.conv2d(xr, wr, None, stride, 1, 1, G)
    ref = torch.relu(conv * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    wa = w.permute(0, 2, 3, 1).reshape(C, 9 * g).contiguous().cuda().to(dt)       # the arena matrix [C][3][3][g]
    for out_dt in ({torch.float32, dt}):
        y = hip.gconv3x3_fwd(_nhwc(x, dt), wa, G, stride, sc.cuda(), sh.cuda(), relu=True, out_dtype=out_dt)
        assert y.dtype == out_dt and tuple(y.shape) == (N, ref.shape[2], ref.shape[3], C)
        _check(mode, _nchw(y) if out_dt == torch.float32 else y.cpu().permute(0, 3, 1, 2), ref)
    y = hip.gconv3x3_fwd(_nhwc(x, dt), wa, G, stride)                                # no epilogue
    _check(mode, y.cpu().permute(0, 3, 1, 2), conv)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("g,G", SHAPES)
def test_gconv_dgrad(mode, g, G, stride):
    from ubteacher import hip
    C, N, H, W = g * G, 2, 13, 11
    dt = _ops(mode)
    gen = torch.Generator().manual_seed(g * 100 + stride + 7)
    w = torch.randn(C, g, 3, 3, generator=gen) * (1.0 / (3 * g ** 0.5))
    sc = torch.rand(C, generator=gen) + 0.5
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    dy = torch.randn(N, C, OH, OW, generator=gen)
    mask = torch.randn(N, C, H, W, generator=gen)
    res = torch.randn(N, C, H, W, generator=gen)
    xr = torch.zeros(N, C, H, W, requires_grad=True)
    F.conv2d(xr, _rnd(w, dt), None, stride, 1, 1, G).backward(_rnd(dy, dt) * sc.view(1, -1, 1, 1))
    ref = xr.grad
    wa = w.permute(0, 2, 3, 1).reshape(C, 9 * g).contiguous().cuda().to(dt)
    dx = hip.gconv3x3_dgrad(_nhwc(dy, dt), wa, G, stride, (N, H, W, C), scale=sc.cuda())
    assert dx.dtype == dt
    _check(mode, dx.cpu().permute(0, 3, 1, 2), ref)
    # the producer's ReLU mask and a residual in the epilogue (both of dx's type)
    mh, rh = _nhwc(mask, dt), _nhwc(res, dt)
    dx2 = hip.gconv3x3_dgrad(_nhwc(dy, dt), wa, G, stride, (N, H, W, C), scale=sc.cuda(), mask=mh, residual=rh)
    ref2 = torch.where(_nchw(mh) > 0, ref, torch.zeros_like(ref)) + _nchw(rh)
    _check(mode, dx2.cpu().permute(0, 3, 1, 2), ref2)
    if dt != torch.float32:        # 16-bit operands, fp32 gradient
        dx3 = hip.gconv3x3_dgrad(_nhwc(dy, dt), wa, G, stride, (N, H, W, C), scale=sc.cuda(), out_dtype=torch.float32)
        assert relerr(_nchw(dx3), ref) < 2e-4


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("g,G", SHAPES)
def test_gconv_wgrad(mode, g, G, stride):
    from ubteacher import hip
    C, N, H, W = g * G, 2, 13, 11
    dt = _ops(mode)
    gen = torch.Generator().manual_seed(g * 100 + stride + 13)
    x = torch.randn(N, C, H, W, generator=gen)
    sc = torch.rand(C, generator=gen) + 0.5
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    dy = torch.randn(N, C, OH, OW, generator=gen)
    wr = torch.zeros(C, g, 3, 3, requires_grad=True)
    F.conv2d(_rnd(x, dt), wr, None, stride, 1, 1, G).backward(_rnd(dy, dt))
    ref = wr.grad * sc.view(-1, 1, 1, 1)
    xh, dyh = _nhwc(x, dt), _nhwc(dy, dt)
    dw0 = torch.randn(C, 9 * g, generator=gen).cuda()
    dw = dw0.clone()
    hip.gconv3x3_wgrad(xh, dyh, dw, G, stride, scale=sc.cuda(), accumulate=True)          # accumulates into the gradient arena
    got = (dw - dw0).cpu().view(C, 3, 3, g).permute(0, 3, 1, 2)
    assert relerr(got, ref) < 2e-4 * 4, relerr(got, ref)     # the pre-existing values (O(1)) add one rounding per element
    runs = []
    for _ in range(2):
        d = torch.zeros(C, 9 * g, device="cuda")
        hip.gconv3x3_wgrad(xh, dyh, d, G, stride, scale=sc.cuda(), accumulate=False)
        runs.append(d.cpu())
    assert relerr(runs[0].view(C, 3, 3, g).permute(0, 3, 1, 2), ref) < 2e-4
    assert torch.equal(runs[0], runs[1])                     # deterministic: fixed split order, no atomics


def test_gconv_wgrad_many_splits_deterministic():
    """a res2-like pixel count (hundreds of splits): still bit-identical between runs and equal to the reference"""
    from ubteacher import hip
    N, H, W, G, g = 2, 67, 101, 32, 8
    C = G * g
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(N, C, H, W, generator=gen)
    dy = torch.randn(N, C, H, W, generator=gen)
    wr = torch.zeros(C, g, 3, 3, requires_grad=True)
    F.conv2d(x, wr, None, 1, 1, 1, G).backward(dy)
    assert hip.load().utv2_gconv3x3_wgrad_splits(N, H, W, C, G) > 8
    xh, dyh = _nhwc(x, torch.float32), _nhwc(dy, torch.float32)
    runs = []
    for _ in range(2):
        d = torch.zeros(C, 9 * g, device="cuda")
        hip.gconv3x3_wgrad(xh, dyh, d, G, 1, accumulate=False)
        runs.append(d.cpu())
    assert torch.equal(runs[0], runs[1])
    assert relerr(runs[0].view(C, 3, 3, g).permute(0, 3, 1, 2), wr.grad) < 2e-4


def test_conv_layer_autograd_fp32():
    """ops.Conv with a grouped FrozenBN layer (the ResNeXt conv2) through autograd in the exact-fp32 mode: one forward, dgrad and wgrad
    launch for all groups, against torch's grouped conv"""
    from ubteacher import ops
    from ubteacher.modeling.backbone import BNFolder, _conv_bn
    from ubteacher.params import ParamStore
    ops.set_precision("fp32")
    st = ParamStore()
    folder = BNFolder(st)
    G, g, N, H, W = 32, 8, 2, 15, 9
    C = G * g
    layer = _conv_bn(st, folder, "c", C, C, 3, 2, 1, True, True, groups=G)
    st.finalize(torch.device("cuda"))
    folder.materialize()
    gen = torch.Generator().manual_seed(3)
    st.flat.copy_(torch.randn(st.flat.numel(), generator=gen).cuda() * 0.1)
    for kind in ("bn_w", "bn_v"):
        st.region(kind).abs_().add_(0.5)
    folder.fold()
    x = torch.randn(N, H, W, C, generator=gen).cuda().requires_grad_(True)
    y = layer(x)
    dy = torch.randn(y.shape, generator=gen).cuda()
    y.backward(dy)
    ops.join_wgrad_stream()
    w = layer.w.t.detach().cpu().view(C, 3, 3, g).permute(0, 3, 1, 2).clone().requires_grad_(True)
    xc = x.detach().cpu().permute(0, 3, 1, 2).clone().requires_grad_(True)
    sc, sh = layer.bn.scale.cpu(), layer.bn.shift.cpu()
    yr = torch.relu(F.conv2d(xc, w, None, 2, 1, 1, G) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    yr.backward(dy.cpu().permute(0, 3, 1, 2))
    assert relerr(y.detach().cpu().permute(0, 3, 1, 2), yr.detach()) < 2e-4
    assert relerr(x.grad.cpu().permute(0, 3, 1, 2), xc.grad) < 2e-4
    assert relerr(layer.w.g.cpu().view(C, 3, 3, g).permute(0, 3, 1, 2), w.grad) < 2e-4
