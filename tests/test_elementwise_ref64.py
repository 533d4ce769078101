"""tests/elementwise_ref64.py on the CPU: the references agree with ATen where ATen has the operation (or with a second, independent
statement of it), and the operands test_elementwise_edges_gpu.py draws meet the precondition of its bit-for-bit comparisons - every
fp32 sum the kernels form is exactly representable."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import elementwise_ref64 as R

F64 = torch.float64
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def test_round16_is_one_rne_step():
    # ties to even, both types: 1 + 2^-8 is halfway between two bf16 values, 1 + 2^-11 between two fp16 values
    x = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65519.0, 65520.0, 2.0 ** -25, 3 * 2.0 ** -25], dtype=F64)
    b = R.round16(x, torch.bfloat16).double()
    assert b[0] == 1.0 and b[1] == 1 + 2.0 ** -6
    h = R.round16(x, torch.float16).double()
    assert h[2] == 1.0 and h[3] == 1 + 2.0 ** -9 and h[4] == 65504.0 and torch.isinf(h[5])
    assert h[6] == 0.0 and h[7] == 2.0 ** -23                      # fp16 subnormals: ties to even on the 2^-24 grid
    with pytest.raises(AssertionError):
        R.round16(torch.tensor([1 + 2.0 ** -40], dtype=F64), torch.bfloat16)
    assert R.round16(x, torch.float32).dtype == torch.float32
    u = R.ulp32(torch.tensor([1.0, 1.5, 2.0, -3.0, 0.0, 2.0 ** -127], dtype=F64))
    assert u.tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -22, 2.0 ** -149, 2.0 ** -149]
    assert all(float(u[i]) == float(np.spacing(np.float32(v))) for i, v in enumerate([1.0, 1.5, 2.0]))


def test_same_is_by_value_with_nan():
    a = torch.tensor([0.0, float("nan"), float("-inf"), 1.0])
    assert R.same(a, torch.tensor([-0.0, float("nan"), float("-inf"), 1.0]))
    assert not R.same(a, torch.tensor([0.0, 0.0, float("-inf"), 1.0]))
    assert not R.same(a, torch.tensor([0.0, float("nan"), float("inf"), 1.0]))
    assert not R.same(a, a.double())


def _pool_by_hand(x):
    """max_pool2d(3, 2, 1) from its definition, window by window: the maximum over the taps that exist; NaN if any tap is NaN"""
    N, H, W, C = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((N, OH, OW, C), dtype=x.dtype)
    for oh in range(OH):
        for ow in range(OW):
            win = x[:, max(2 * oh - 1, 0):2 * oh + 2, max(2 * ow - 1, 0):2 * ow + 2].reshape(N, -1, C)
            m = win.nan_to_num(nan=float("-inf"), neginf=float("-inf")).amax(1)
            y[:, oh, ow] = torch.where(win.isnan().any(1), torch.full_like(m, float("nan")), m)
    return y


@pytest.mark.parametrize("dtype", DTYPES)
def test_pool_reference_and_operands(dtype):
    for i, shape in enumerate(R.POOL_FWD_SHAPES):
        x = R.pool_input(shape, dtype, i)
        assert torch.equal(x.to(dtype).float(), x)                                    # the operand is exact in dtype
        ref = R.maxpool_fwd(x)
        assert tuple(ref.shape) == R.pool_out_shape(shape) and R.same(ref, _pool_by_hand(x.double()))
        R.assert_exact(ref, x)
        assert float(ref[-1, 0, 0, 0]) == float("-inf")                               # a whole window of -inf stays -inf
        if shape[1] * shape[2] > 1:
            assert bool((ref[..., 2::4] < 0).all())                                   # all-negative windows: no padded 0 won
    x = R.pool_nan_input(dtype, 9)
    ref = R.maxpool_fwd(x)
    assert R.same(ref, _pool_by_hand(x.double()))
    assert bool(ref[0, 1, 1, 0].isnan() and ref[0, 2, 3, 1].isnan() and ref[1, 0, 0, 2].isnan() and ref[1, 3, 4, 3].isnan())
    assert bool(ref[1, 1, 2, 4:].isnan().all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_pool_backward_reference_and_operands(dtype):
    for i, shape in enumerate(R.POOL_BWD_SHAPES):
        x, d = R.pool_input(shape, dtype, 20 + i), R.pool_grad(shape, dtype, i)
        for relu in (False, True):
            ref = R.maxpool_bwd(x, d, relu)
            R.assert_exact(ref, d, d, d, d)                                           # a pixel is the maximum of at most four windows
            if not relu:                                                              # every window's gradient lands exactly once
                assert torch.equal(ref.sum((1, 2)), d.double().sum((1, 2)))
            else:
                assert bool((ref[x <= 0] == 0).all())
    # ties go to the FIRST maximum: a constant image sends each window's gradient to its first existing tap
    x = torch.ones(1, 4, 4, 4)
    d = torch.arange(1.0, 5.0).view(1, 2, 2, 1).expand(1, 2, 2, 4).contiguous()
    ref = R.maxpool_bwd(x, d, False)[0, :, :, 0]
    want = torch.zeros(4, 4, dtype=F64)
    want[0, 0], want[0, 1], want[1, 0], want[1, 1] = 1, 2, 3, 4
    assert torch.equal(ref, want)
    # a NaN is a window's maximum
    x = R.pool_nan_input(dtype, 9)
    ref = R.maxpool_bwd(x, torch.ones(R.pool_out_shape(x.shape)), False)
    assert float(ref[0, 1, 1, 0]) == 4.0 and float(ref[1, 0, 0, 2]) == 1.0             # odd pixel: four windows; the corner: one
    assert torch.equal(ref.sum((1, 2)), torch.full((2, 8), 20.0, dtype=F64))          # each of the 4 x 5 windows lands exactly once
    one = R.maxpool_bwd(torch.full((1, 2, 2, 4), float("nan")), torch.ones(1, 1, 1, 4), False)[0, :, :, 0]
    assert one.tolist() == [[0.0, 0.0], [0.0, 1.0]]                                   # a whole window of NaN: its LAST tap takes it


@pytest.mark.parametrize("dtype", DTYPES)
def test_resampling_references_and_operands(dtype):
    for i, shape in enumerate(R.LATERAL_SHAPES):
        lat, top = R.lateral_operands(shape, dtype, 40 + i)
        up = R.upsample_add(lat, top)
        want = _nchw(lat.double()) + F.interpolate(_nchw(top.double()), scale_factor=2.0, mode="nearest")
        assert torch.equal(_nchw(up), want)
        R.assert_exact(up, lat, top)
        down = R.downsample_sum(lat)
        assert torch.equal(_nchw(down), F.avg_pool2d(_nchw(lat.double()), 2) * 4)
        acc = R.downsample_sum(lat, top)
        assert torch.equal(acc, down + top.double())
        R.assert_exact(acc, lat, lat, lat, lat, top)
        # the adjoint of the upsample, by autograd
        t = top.double().clone().requires_grad_(True)
        R.upsample_add(lat, t).backward(lat.double())
        assert torch.equal(t.grad, down)
    with pytest.raises(AssertionError):
        R.downsample_sum(torch.zeros(1, 3, 4, 4))


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_interleave_reference_and_operands(dtype):
    for i, (H, W) in enumerate(R.INTERLEAVE_HW):
        for C in (4, 8, 12, 16):
            src, mask, add = R.interleave_operands(2, H, W, C, dtype, 60 + i)
            assert torch.equal(mask.to(dtype).float().nan_to_num(nan=7.0), mask.nan_to_num(nan=7.0))
            # the adjoint of taking every second pixel, by autograd
            full = torch.zeros(2, H, W, C, dtype=F64, requires_grad=True)
            full[:, ::2, ::2].backward(src.double())
            assert torch.equal(R.zero_interleave(src, H, W), full.grad)
            ref = R.zero_interleave(src, H, W, mask, add)
            passes = mask > 0
            assert not bool(passes[mask.isnan() | (mask <= 0)].any())                 # -0.0, negatives, NaN stop the value
            want = torch.where(passes, full.grad, torch.zeros_like(full.grad)) + add.double()
            assert torch.equal(ref, want) and not bool(ref.isnan().any())
            R.assert_exact(ref, src, add)
            if C % 8 == 0:
                bits = R.pack_mask_bits(mask)
                assert bits.shape == (2, H, W, C // 8) and bits.dtype == torch.uint8
                un = ((bits.view(2, H, W, C // 8, 1).int() >> torch.arange(8)) & 1).bool().view(2, H, W, C)
                assert torch.equal(un, passes)


@pytest.mark.parametrize("dtype", DTYPES)
def test_relu_bwd_scale_reference_and_operands(dtype):
    dy, y, sc = R.relu_bwd_operands(37, 12, dtype, 80)
    ref = R.relu_bwd_scale(dy, y, sc)
    # autograd of relu(x) * scale at an x with the sign pattern of y (NaN and -0.0 of y: no gradient)
    x = torch.where(y > 0, y, -torch.ones_like(y)).double().requires_grad_(True)
    (torch.relu(x) * sc.double()).backward(dy.double())
    assert torch.equal(ref, x.grad)
    assert bool((ref[y.isnan() | (y == 0)] == 0).all()) and bool(y.isnan().any()) and bool(((y == 0) & torch.signbit(y)).any())
    R.assert_exact(ref, dy * 3)
    assert torch.equal(R.relu_bwd_scale(dy), dy.double()) and torch.equal(R.relu_bwd_scale(dy, None, sc), dy.double() * sc.double())
    assert len(set(sc.tolist())) > 2
    # the big case of the GPU test: the same generator, exact as well
    dy, y, sc = R.relu_bwd_operands(4096, 12, torch.float32, 81)
    R.assert_exact(R.relu_bwd_scale(dy, y, sc), dy * 3)


def test_preprocess_reference_and_the_one_ulp_bound():
    """the fp64 reference against the plain torch expression, and the GPU test's bound: on the images and pixel statistics it draws
    the subtraction is exact, so the kernels' expression in numpy float32 - correctly rounded - is within 0.5 ulp32 of the fp64 value
    and the bound of 1 ulp32 rejects no correct kernel"""
    sizes, kinds = [(37, 50), (40, 45), (1, 1), (64, 64)], ["u8", "f32", "u8", "f32"]
    ims = R.images_of(sizes, kinds, 5)
    ref = R.preprocess(ims, R.PRE_MEAN, R.PRE_STD, 32)
    assert tuple(ref.shape) == (4, 64, 64, 4) and R.canvas_of(ims, 1) == (64, 64) and R.canvas_of(ims[:2], 1) == (40, 50)
    m = torch.tensor(R.PRE_MEAN, dtype=torch.float32).double().view(3, 1, 1)
    s = torch.tensor(R.PRE_STD, dtype=torch.float32).double().view(3, 1, 1)
    for n, im in enumerate(ims):
        h, w = sizes[n]
        want = F.pad((im.double() - m) / s, (0, 64 - w, 0, 64 - h))
        assert torch.equal(ref[n, :, :, :3].permute(2, 0, 1), want)
    assert float(ref[..., 3].abs().max()) == 0.0
    pad = R.preprocess_pad(ims, R.PRE_MEAN, R.PRE_STD, 32)
    assert tuple(pad.shape) == (4, 70, 72, 4) and torch.equal(pad[:, 3:67, 3:67], ref)
    border = pad.clone()
    border[:, 3:67, 3:67] = 0
    assert float(border.abs().max()) == 0.0                                           # nothing but zeros around it
    emu = R.preprocess_f32(ims, R.PRE_MEAN, R.PRE_STD, 32).double()
    err = ((emu - ref).abs() / R.ulp32(ref)).max()
    print("preprocess: numpy float32 restatement vs fp64: %.3f ulp32" % float(err))
    assert float(err) <= 0.5
    assert all(float(i.max()) > 250 for i in (ims[0], ims[1], ims[3]))                # bytes above 127 and the top of the range


def test_frozenbn_fold_reference():
    g = torch.Generator().manual_seed(3)
    n = 257
    w, b, mean = (torch.randn(n, generator=g) for _ in range(3))
    var = torch.rand(n, generator=g) * 4
    sc, sh = R.frozenbn_fold(w, b, mean, var, 1e-5)
    e = float(np.float32(1e-5))
    for x0 in (0.0, 1.0, -2.5):
        x = torch.full((1, n, 1, 1), x0, dtype=F64)
        y = F.batch_norm(x, mean.double(), var.double(), w.double(), b.double(), False, 0.0, e).view(n)
        assert float((y - (x0 * sc + sh)).abs().max()) <= 1e-12 * (1 + float(y.abs().max()))


def test_arena_references():
    """the float32 restatements against fp64 torch (torch.optim.SGD; the EMA expression) to fp32 accuracy, and their own edge rules"""
    p, g, m = R.arena_operands(1021, 7)
    keep = 0.9996
    t = R.ema_axpby(p, g, keep)
    want = g.double() * (1 - keep) + p.double() * keep
    assert t.dtype == torch.float32 and float((t.double() - want).abs().max()) <= 2.0 ** -22 * float(want.abs().max())
    lr, mo, wd, gs = 0.01, 0.9, 1e-4, 0.5
    pn, mn = R.sgd_momentum(p, g, m, lr, mo, wd, gs)
    q = p.double().clone().requires_grad_(True)
    opt = torch.optim.SGD([q], lr=lr, momentum=mo, weight_decay=wd)
    opt.state[q]["momentum_buffer"] = m.double().clone()
    q.grad = g.double() * gs
    opt.step()
    assert float((pn.double() - q.detach()).abs().max()) <= 2.0 ** -21 * float(q.detach().abs().max())
    assert float((mn.double() - opt.state[q]["momentum_buffer"]).abs().max()) <= 2.0 ** -21 * float(mn.abs().max())
    # AMP: the gradient is divided by the loss scale; a set flag freezes everything
    st = torch.tensor([1024.0, 0.0, 3.0])
    pa, ma = R.sgd_momentum_amp(p, g * 1024, m, lr, mo, wd, gs, st)
    assert torch.equal(pa, pn) and torch.equal(ma, mn)
    st[1] = 1.0
    pa, ma = R.sgd_momentum_amp(p, g * 1024, m, lr, mo, wd, gs, st)
    assert torch.equal(pa, p) and torch.equal(ma, m)
    assert not R.found_inf(torch.tensor([3.4e38, -3.4e38, 1e-45, 0.0])) and R.found_inf(torch.tensor([0.0, float("nan")]))
    # the fp16 edge operands reach past fp16's range and into its subnormals after the update
    p, g, m = R.arena_operands(1021, 8, fp16_edges=True)
    pn, _ = R.sgd_momentum(p, g, m, lr, mo, wd, gs)
    h = R.round16(pn.double(), torch.float16)
    assert bool(torch.isinf(h).any()) and bool(((h != 0) & (h.float().abs() < 6.1e-5)).any())
