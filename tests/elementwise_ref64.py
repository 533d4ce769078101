"""Plain CPU references of the glue kernels in csrc/elementwise.hip, stated from each operation's definition (plain module; used by
test_elementwise_ref64.py on the CPU and test_elementwise_edges_gpu.py on the GPU).

Activations are NHWC, fp64.  Nothing here restates a kernel's index arithmetic: the pools are ATen's max_pool2d and its autograd on fp64
NCHW (they bring ATen's first-maximum and NaN rules), the resampling ops are repeat / reshape / strided assignment.

The method for the activation kernels is exact_conv_ref.py's: operands are integer multiples of 2^-2 (`grid`), few enough bits that every
fp32 sum a kernel forms (at most five terms) is exact in any order, so an fp32 output must equal the fp64 reference and a 16-bit output
ONE round-to-nearest-even of it (`round16`) - bit for bit.  assert_exact says so before anything is compared.

The arena updates (EMA, SGD, AMP SGD) are restated in numpy float32 with one rounding per written operation, which is how the kernels
are written (the library is built with -ffp-contract=off): bit-equal, too."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import exact_conv_ref as X

F64 = torch.float64
UNIT_EXP = -2                     # the grid: multiples of 1/4


# ----------------------------------------------------------------------------------------------------------------------------------
# roundings and operands
def round16(x64, dtype, exact=True):
    """one round-to-nearest-even step of an fp64 tensor to `dtype` (bf16, fp16; fp32 passes through).  exact (default): x64 must be an
    fp32 value (exact_conv_ref.to_out checks it), so the step to 16 bits is the only rounding.  exact=False, for the BOUNDS of a
    tolerance only: fp64 -> fp32 -> dtype; both steps are monotone, so the result brackets what any fp32 value on the far side of x64
    rounds to."""
    if exact:
        nan = torch.isnan(x64)                       # a NaN is a NaN in every type; to_out compares values
        out = X.to_out(torch.where(nan, torch.zeros_like(x64), x64), dtype)
        return torch.where(nan, torch.full_like(out, float("nan")), out)
    return x64.to(torch.float32).to(dtype)


def ulp32(x64):
    """spacing of fp32 at |x64| (fp64 tensor): 2^(floor(log2 |x|) - 23), the subnormal spacing 2^-149 below 2^-126"""
    e = torch.floor(torch.log2(x64.abs().clamp(min=2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=F64), e - 23.0)


def grid_bits(dtype):
    """significant bits of a grid operand that `dtype` holds exactly (bf16 keeps 8, fp16 11) and whose sums of five still fit fp32"""
    return 7 if dtype == torch.bfloat16 else 10


def grid(shape, dtype, generator, relu_like=False, zero_frac=0.125):
    """fp32 multiples of 1/4, |v| < 2^(grid_bits - 2), exactly representable in `dtype`; many ties, many zeros"""
    return X.dyadic(shape, grid_bits(dtype), UNIT_EXP, generator, relu_like=relu_like, zero_frac=zero_frac)


SCALE_UNIT_EXP = -1               # exact_conv_ref.small_scale multipliers are multiples of 1/2
PRODUCT_UNIT_EXP = UNIT_EXP + SCALE_UNIT_EXP


def assert_exact(ref64, *operands):
    """the precondition of a bit-for-bit comparison: ref64 (non-finite entries aside) is a multiple of the product grid 2^-3, the sum of
    the operands' largest magnitudes - which bounds every partial sum in any order - stays below 2^24 grid units, and ref64 survives
    fp32 unchanged: an fp32 evaluation of the operation is exact"""
    f = torch.where(torch.isfinite(ref64), ref64, torch.zeros_like(ref64))
    X.assert_on_grid(f, PRODUCT_UNIT_EXP, "the reference")
    bound = sum(float(torch.where(torch.isfinite(t), t, torch.zeros_like(t)).abs().max()) for t in operands if t is not None)
    assert bound * 2.0 ** -PRODUCT_UNIT_EXP < X.LIMIT, "partial sums may leave the fp32 grid"
    assert float(f.abs().max()) <= bound or not operands, "the bound does not bound the reference"
    assert torch.equal(f.to(torch.float32).to(F64), f), "the reference is not exact in fp32"


def scale_vec(C, generator):
    """per-channel multipliers {.5, 1, 1.5, 2, 3}: exact products with grid values, and a period that nothing divides by accident"""
    return X.small_scale((C,), generator)


def same(got, want):
    """equal by VALUE (signed zeros are not told apart) with NaN == NaN, same dtype and shape"""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    gn, wn = torch.isnan(got), torch.isnan(want)
    z = torch.zeros((), dtype=got.dtype, device=got.device)
    return bool(torch.equal(gn, wn)) and bool(torch.equal(torch.where(gn, z, got), torch.where(wn, z, want)))


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ----------------------------------------------------------------------------------------------------------------------------------
# the stem pool: max_pool2d(3, stride 2, padding 1)
def maxpool_fwd(x64):
    """[N,H,W,C] -> [N,OH,OW,C]: ATen's pool - the padding is absent (not 0), a NaN in a window is its maximum"""
    return _nhwc(F.max_pool2d(_nchw(x64.to(F64)), 3, 2, 1))


def maxpool_bwd(x64, dpool64, relu):
    """gradient of maxpool_fwd w.r.t. x by ATen's autograd (each window's gradient goes to its FIRST maximum in scan order; a NaN counts
    as a maximum); relu: only where x > 0 (the ReLU in front of the pool) - 0, not NaN * 0, elsewhere"""
    x = _nchw(x64.to(F64)).clone().requires_grad_(True)
    F.max_pool2d(x, 3, 2, 1).backward(_nchw(dpool64.to(F64)).contiguous())
    g = x.grad
    if relu:
        g = torch.where(x.detach() > 0, g, torch.zeros_like(g))
    return _nhwc(g)


# ----------------------------------------------------------------------------------------------------------------------------------
# FPN resampling
def upsample_add(lat64, top64):
    """lateral + nearest-neighbour x2 of top"""
    return lat64.to(F64) + top64.to(F64).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def downsample_sum(g64, base64=None):
    """the upsample's adjoint: each output pixel is the sum of its 2x2 block (plus base64 when the kernel accumulates)"""
    N, H, W, C = g64.shape
    assert H % 2 == 0 and W % 2 == 0
    s = g64.to(F64).reshape(N, H // 2, 2, W // 2, 2, C).sum(dim=(2, 4))
    return s if base64 is None else s + base64.to(F64)


def zero_interleave(src64, H, W, mask64=None, add64=None):
    """src on the even pixels of [N,H,W,C], zeros elsewhere; mask: the value passes only where mask > 0 (so -0.0, negatives and NaN
    all stop it); add: summed in afterwards, unmasked"""
    N, TH, TW, C = src64.shape
    assert TH == (H + 1) // 2 and TW == (W + 1) // 2
    v = src64.to(F64)
    if mask64 is not None:
        v = torch.where(mask64.to(F64)[:, ::2, ::2] > 0, v, torch.zeros_like(v))
    out = torch.zeros((N, H, W, C), dtype=F64)
    out[:, ::2, ::2] = v
    return out if add64 is None else out + add64.to(F64)


def pack_mask_bits(mask):
    """uint8 [N,H,W,C/8] bit plane of `mask > 0`: bit q of byte j is channel 8 j + q (hip.relu_bits_buffer's layout)"""
    N, H, W, C = mask.shape
    assert C % 8 == 0
    b = (mask > 0).reshape(N, H, W, C // 8, 8).to(torch.int64)
    return (b << torch.arange(8)).sum(-1).to(torch.uint8)


def relu_bwd_scale(dy64, y64=None, scale64=None):
    """(y > 0 ? dy : 0) * scale[c] on [..., C]; y = -0.0 or NaN: 0"""
    g = dy64.to(F64)
    if y64 is not None:
        g = torch.where(y64.to(F64) > 0, g, torch.zeros_like(g))
    return g if scale64 is None else g * scale64.to(F64)


# ----------------------------------------------------------------------------------------------------------------------------------
# image normalisation and FrozenBN fold (fp64 of the definition; the kernels' roundings are bounded by the tests, not restated)
def canvas_of(images, size_divisibility):
    H, W = max(int(i.shape[1]) for i in images), max(int(i.shape[2]) for i in images)
    d = size_divisibility
    return ((H + d - 1) // d * d, (W + d - 1) // d * d) if d > 1 else (H, W)


def preprocess(images, mean, std, size_divisibility):
    """list of [3,H,W] (u8 or fp32) -> fp64 [N,Hp,Wp,4]: (x - mean[c]) / std[c] in channels 0..2 at the top-left of a zero canvas,
    channel 3 zero.  mean / std enter as the fp32 values the C entry receives."""
    Hp, Wp = canvas_of(images, size_divisibility)
    m = torch.tensor([float(np.float32(v)) for v in mean], dtype=F64).view(3, 1, 1)
    s = torch.tensor([float(np.float32(v)) for v in std], dtype=F64).view(3, 1, 1)
    out = torch.zeros((len(images), Hp, Wp, 4), dtype=F64)
    for n, im in enumerate(images):
        out[n, :im.shape[1], :im.shape[2], :3] = ((im.to(F64) - m) / s).permute(1, 2, 0)
    return out


def preprocess_pad(images, mean, std, size_divisibility):
    """the same inside the stem's zero border: [N,Hp+6,Wp+8,4] with the image at pixel offset (3, 3)"""
    return F.pad(preprocess(images, mean, std, size_divisibility), (0, 0, 3, 5, 3, 3))


def frozenbn_fold(w, b, mean, var, eps=1e-5):
    """scale = w / sqrt(var + eps), shift = b - mean * scale in fp64 (eps as the fp32 value the C entry receives)"""
    e = float(np.float32(eps))
    scale = w.to(F64) / torch.sqrt(var.to(F64) + e)
    return scale, b.to(F64) - mean.to(F64) * scale


# ----------------------------------------------------------------------------------------------------------------------------------
# flat-arena updates: numpy float32, one rounding per written operation
def _f32(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    assert a.dtype == np.float32
    return a


def ema_axpby(teacher, student, keep_rate):
    """new teacher = student * (1 - keep) + teacher * keep, the two factors rounded to fp32 first"""
    a, b = np.float32(1.0 - keep_rate), np.float32(keep_rate)
    with np.errstate(all="ignore"):
        return torch.from_numpy(_f32(student) * a + _f32(teacher) * b)


def sgd_momentum(param, grad, mom, lr, momentum, weight_decay, grad_scale=1.0, inv_loss_scale=None):
    """torch.optim.SGD (momentum, weight decay, no nesterov) on a gradient multiplied by grad_scale (after 1 / loss scale under AMP):
    g = grad * gscale + wd * p;  buf = momentum * buf + g;  p = p - lr * buf.  Returns (param, mom)."""
    p, g, m = _f32(param), _f32(grad), _f32(mom)
    lr, mo, wd, gs = np.float32(lr), np.float32(momentum), np.float32(weight_decay), np.float32(grad_scale)
    with np.errstate(all="ignore"):
        if inv_loss_scale is not None:
            g = g * np.float32(inv_loss_scale)
        gv = g * gs + wd * p
        mv = mo * m + gv
        pn = p - lr * mv
    return torch.from_numpy(pn), torch.from_numpy(mv)


def sgd_momentum_amp(param, grad, mom, lr, momentum, weight_decay, grad_scale, state):
    """GradScaler.step: nothing changes when state = {scale, found_inf, tracker} has found_inf set, else the update on grad / scale"""
    st = _f32(state)
    if st[1] != 0:
        return torch.from_numpy(_f32(param).copy()), torch.from_numpy(_f32(mom).copy())
    return sgd_momentum(param, grad, mom, lr, momentum, weight_decay, grad_scale, inv_loss_scale=np.float32(1.0) / st[0])


def found_inf(grad):
    return not bool(np.isfinite(_f32(grad)).all())


# ----------------------------------------------------------------------------------------------------------------------------------
# the cases of test_elementwise_edges_gpu.py and their operands (built once per case on the CPU; test_elementwise_ref64.py checks that
# every one of them meets assert_exact)
POOL_FWD_SHAPES = [(1, 1, 1, 4), (1, 2, 3, 4), (2, 7, 9, 12), (1, 8, 8, 8), (2, 15, 17, 24), (1, 16, 14, 64)]
POOL_BWD_SHAPES = [(2, 14, 18, 64), (1, 15, 17, 8), (2, 9, 12, 4), (1, 1, 1, 4), (1, 2, 2, 4), (1, 1, 6, 8), (2, 3, 1, 12)]
LATERAL_SHAPES = [(1, 2, 2, 4), (1, 4, 2, 8), (2, 6, 10, 12)]
INTERLEAVE_HW = [(1, 1), (5, 7), (6, 4), (2, 1)]
# Pixel means with few bits and sources on the 1/8 grid (images_of): x - mean is then exact and the division is the only rounding left,
# so a correctly rounding kernel is within 0.5 ulp32 of the fp64 value and the tests' bound of 1 ulp32 holds for every correct kernel.
# (With D2's 103.53 / 116.28 / 123.675 the subtraction rounds as well; two correct roundings reach 1.5 ulp32 of the quotient in the
# worst case - 1.06 on random images - so that bound would reject correct code.)  The divisors keep all their bits.
PRE_MEAN, PRE_STD = [103.5, 116.25, 123.75], [57.375, 57.12, 58.395]


def pool_out_shape(shape):
    N, H, W, C = shape
    return (N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C)


def pool_input(shape, dtype, seed, neg_inf=True):
    """grid values whose channels take turns at what a pool gets wrong: c % 4 == 0 signed values, 1 a ReLU output (windows full of equal
    zeros), 2 strictly negative (a padded tap that counted as 0 would win), 3 multiples of 8 (ties everywhere); -inf sprinkled on top, and over one whole window"""
    g = torch.Generator().manual_seed(seed)
    x = grid(shape, dtype, g)
    c = torch.arange(shape[-1]) % 4
    x = torch.where(c == 1, x.clamp(min=0), x)
    x = torch.where(c == 2, -x.abs() - 0.25, x)
    x = torch.where(c == 3, (x / 8).round() * 8, x)
    if neg_inf:
        x = torch.where(torch.rand(shape, generator=g) < 0.04, torch.full_like(x, float("-inf")), x)
        x[-1, :2, :2, 0] = float("-inf")              # every tap of the last image's corner window: its maximum is -inf
    return x


def pool_nan_input(dtype, seed):
    """(2, 7, 9, 8) with NaNs on the first tap of a window, on the last tap of one, in a border window and over a whole window"""
    x = pool_input((2, 7, 9, 8), dtype, seed, neg_inf=False)
    nan = float("nan")
    x[0, 1, 1, 0] = nan          # first tap (dh = dw = 0) of window (1, 1)
    x[0, 5, 7, 1] = nan          # last tap (dh = dw = 2) of window (2, 3)
    x[1, 0, 0, 2] = nan          # border window (0, 0)
    x[1, 6, 8, 3] = nan          # the bottom-right border window
    x[1, 1:4, 3:6, 4:] = nan     # every tap of window (1, 2)
    return x


def pool_grad(shape, dtype, seed):
    return grid(pool_out_shape(shape), dtype, torch.Generator().manual_seed(seed + 1000), zero_frac=0.0)


def lateral_operands(shape, dtype, seed):
    """(lateral / gradient [N,H,W,C], top / accumulation target [N,H/2,W/2,C])"""
    g = torch.Generator().manual_seed(seed)
    N, H, W, C = shape
    return grid(shape, dtype, g), grid((N, H // 2, W // 2, C), dtype, g, zero_frac=0.0)


def interleave_operands(N, H, W, C, dtype, seed):
    """(src, mask, add): the mask holds -0.0, negative values and NaN besides positive ones and plain zeros"""
    g = torch.Generator().manual_seed(seed)
    src = grid((N, (H + 1) // 2, (W + 1) // 2, C), dtype, g, zero_frac=0.0)
    src = torch.where(src == 0, torch.full_like(src, 0.25), src)        # a stopped value is visible
    kind = torch.randint(0, 5, (N, H, W, C), generator=g)
    mask = grid((N, H, W, C), dtype, g, zero_frac=0.0).abs() + 0.25
    mask = torch.where(kind == 1, -mask, mask)
    mask = torch.where(kind == 2, torch.full_like(mask, -0.0), mask)
    mask = torch.where(kind == 3, torch.full_like(mask, float("nan")), mask)
    add = grid((N, H, W, C), dtype, g)
    return src, mask, add


def relu_bwd_operands(M, C, dtype, seed):
    """(dy, y, scale): y is a ReLU output sprinkled with -0.0 and NaN"""
    g = torch.Generator().manual_seed(seed)
    dy = grid((M, C), dtype, g, zero_frac=0.0)
    dy = torch.where(dy == 0, torch.full_like(dy, 0.25), dy)
    y = grid((M, C), dtype, g, relu_like=True)
    kind = torch.randint(0, 8, (M, C), generator=g)
    y = torch.where(kind == 1, torch.full_like(y, -0.0), y)
    y = torch.where(kind == 2, torch.full_like(y, float("nan")), y)
    return dy, y, scale_vec(C, g)


def preprocess_f32(images, mean, std, size_divisibility):
    """the kernels' own two roundings in numpy float32 - (float(x) - mean) / std - on the CPU: what a correct kernel returns"""
    Hp, Wp = canvas_of(images, size_divisibility)
    out = np.zeros((len(images), Hp, Wp, 4), dtype=np.float32)
    for n, im in enumerate(images):
        x = im.numpy().astype(np.float32)
        for c in range(3):
            out[n, :x.shape[1], :x.shape[2], c] = (x[c] - np.float32(mean[c])) / np.float32(std[c])
    return torch.from_numpy(out)


def images_of(sizes, kinds, seed):
    """[3,H,W] images: kind "u8" random bytes, "f32" a byte plus a multiple of 1/8, so up to 255.875"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for (h, w), k in zip(sizes, kinds):
        u = torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8)
        out.append(u if k == "u8" else (u.float() + torch.randint(0, 8, (3, h, w), generator=g).float() / 8))
    return out


def arena_operands(n, seed, fp16_edges=False):
    """(param, grad, mom) fp32 of ordinary training magnitudes; fp16_edges: params whose update lands beyond fp16's range (the mirror
    rounds to inf) and inside its subnormals"""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g) * 0.5
    gr = torch.randn(n, generator=g) * 0.01
    m = torch.randn(n, generator=g) * 0.02
    if fp16_edges:
        k = torch.arange(n) % 4
        p = torch.where(k == 1, p * 2.0e5, p)          # |p| up to ~1e5 .. 1e6: fp16 inf from 65520 on
        p = torch.where(k == 2, p * 1.0e-5, p)         # ~5e-6: below fp16's smallest normal 6.1e-5
        m = torch.where(k == 2, m * 1.0e-5, m)
        gr = torch.where(k == 2, gr * 1.0e-5, gr)
    return p.contiguous(), gr.contiguous(), m.contiguous()
