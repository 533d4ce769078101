"""Exact-arithmetic operands and fp64 references for the conv kernels: the 16-bit routes, the fp32 implicit-GEMM convs and the grouped 3x3
conv (plain module; used by test_exact_conv_ref.py on the CPU and test_conv_exact_gpu.py, test_conv_f32_exact_gpu.py and
test_gconv_exact_gpu.py on the GPU).

The method: every operand is an integer multiple of a power of two (its *unit*), small enough that every product and every partial sum
of a conv is an integer multiple of the product of the units (the *product grid*) below 2^24 of it.  An fp32 accumulation of such terms is
exact in ANY order - tile shape, split-K slab order, ping-pong / row-span / persistent schedules, the MFMA's internal order - so a kernel's
fp32 output must equal the fp64 reference bit for bit, and a 16-bit output must equal ONE round-to-nearest-even of it.  assert_exact_domain
is that precondition; every test calls it before it compares anything.

Layouts are the kernels': activations NHWC, weights [K, kh*kw*C] with the reduction index (kh, kw, ci)."""
import torch
import torch.nn.functional as F

F64 = torch.float64
LIMIT = float(2 ** 24)


# ----------------------------------------------------------------------------------------------------------------------------------
# operands
def dyadic(shape, bits, scale_exp, generator, relu_like=False, zero_frac=0.125):
    """fp32 integers in [-(2^bits - 1), 2^bits - 1] times 2^scale_exp, with exact zeros (about zero_frac of the elements on top of the
    integer 0 itself); relu_like: the negative values are zeros too (a ReLU output).  bits <= 7: exact in bf16 and in fp16."""
    top = 2 ** bits - 1
    v = torch.randint(-top, top + 1, shape, generator=generator, dtype=torch.int64)
    if relu_like:
        v = v.clamp(min=0)
    keep = torch.rand(shape, generator=generator) >= zero_frac
    return (v * keep).to(torch.float32) * (2.0 ** scale_exp)


def dyadic_wide(shape, scale_exp, generator, zero_frac=0.125):
    """fp32 values with 12 .. 16 significant bits, all in one binade: +-(2^15 + r) * 2^scale_exp with r of 11 .. 15 random leading bits.
    Neither 16-bit type holds them (bf16 keeps 8 bits, fp16 11): for the kernels that round an fp32 operand on load.  After that rounding
    every value is a multiple of 2^(scale_exp + 8) (bf16) / 2^(scale_exp + 5) (fp16) of at most 2^(scale_exp + 16): see wide_unit_exp."""
    sig = torch.randint(12, 17, shape, generator=generator, dtype=torch.int64)
    r = torch.randint(0, 2 ** 15, shape, generator=generator, dtype=torch.int64)
    drop = 16 - sig
    r = (r >> drop) << drop
    r = r | (1 << drop)                      # the lowest kept bit is set: exactly `sig` significant bits
    sign = torch.randint(0, 2, shape, generator=generator, dtype=torch.int64) * 2 - 1
    keep = torch.rand(shape, generator=generator) >= zero_frac
    return (sign * (2 ** 15 + r) * keep).to(torch.float32) * (2.0 ** scale_exp)


def wide_unit_exp(scale_exp, h16):
    """unit exponent of dyadic_wide(..., scale_exp) values after one rounding to h16"""
    return scale_exp + (8 if h16 == torch.bfloat16 else 5)


def pow2(shape, lo_exp, hi_exp, generator):
    """fp32 powers of two 2^e, e in [lo_exp, hi_exp]"""
    return torch.pow(2.0, torch.randint(lo_exp, hi_exp + 1, shape, generator=generator).to(torch.float32))


def small_scale(shape, generator, exp=0):
    """per-channel multipliers {1, 2, 3, 4, 6} * 2^(exp - 1) = {.5, 1, 1.5, 2, 3} * 2^exp: two significant bits, none of them 1 only - a scale
    that is applied after the bias instead of before it changes the result"""
    tab = torch.tensor([1.0, 2.0, 3.0, 4.0, 6.0])
    return tab[torch.randint(0, 5, shape, generator=generator)] * (2.0 ** (exp - 1))


# ----------------------------------------------------------------------------------------------------------------------------------
# layout helpers (CPU, fp64)
def _x64(x):
    return x.detach().to("cpu").to(F64).permute(0, 3, 1, 2).contiguous()


def _w64(w2, k, C):
    K = w2.shape[0]
    return w2.detach().to("cpu").to(F64).view(K, k, k, C).permute(0, 3, 1, 2).contiguous()


def _v64(t):
    return None if t is None else t.detach().to("cpu").to(F64)


def _epilogue(y, scale, bias, residual, relu):
    """y NHWC fp64: relu?((y * scale + bias) + residual), the order of operations of the kernels' epilogue"""
    if scale is not None:
        y = y * _v64(scale)
    if bias is not None:
        y = y + _v64(bias)
    if residual is not None:
        y = y + _v64(residual)
    return torch.relu(y) if relu else y


# ----------------------------------------------------------------------------------------------------------------------------------
# fp64 references
def conv_fwd_ref(x, w2, k, stride, pad, scale=None, bias=None, residual=None, relu=False, groups=1, acc0=None):
    """NHWC fp64 relu?((conv(x, w) * scale + bias) + residual) (+ acc0: the output's earlier content under accumulate, added AFTER the ReLU as
    the kernels do); groups > 1: w2 is the arena matrix [K, k*k*C/groups] of a grouped conv (row = output channel, reading its group's inputs)"""
    C = x.shape[-1] // groups
    y = F.conv2d(_x64(x), _w64(w2, k, C), None, stride, pad, 1, groups).permute(0, 2, 3, 1)
    y = _epilogue(y, scale, bias, residual, relu)
    if acc0 is not None:
        y = y + _v64(acc0)
    return y.contiguous()


def conv_dgrad_ref(dy, w2, in_shape, k, stride, pad, mask=None, residual=None, post_mask=None, groups=1, scale=None, acc0=None):
    """NHWC fp64 gradient of conv(x, w) w.r.t. x for the output gradient dy (w2: the FORWARD weights [K, k*k*C/groups]);
    scale [K]: every weight of output channel k is multiplied by scale[k] BEFORE the accumulation (the grouped dgrad's folded FrozenBN);
    dx = mask > 0 ? dx : 0; dx += residual; dx = post_mask > 0 ? dx : 0 (the expression of test_post_mask_epilogue_and_masked_zero_interleave);
    dx += acc0 (accumulate)"""
    N, H, W, C = in_shape
    OH, OW = dy.shape[1:3]
    oph, opw = H - ((OH - 1) * stride - 2 * pad + k), W - ((OW - 1) * stride - 2 * pad + k)
    w = _w64(w2, k, C // groups)
    if scale is not None:
        w = w * _v64(scale).view(-1, 1, 1, 1)
    dx = F.conv_transpose2d(_x64(dy), w, None, stride, pad, output_padding=(oph, opw), groups=groups).permute(0, 2, 3, 1)
    if mask is not None:
        dx = torch.where(_v64(mask) > 0, dx, torch.zeros_like(dx))
    if residual is not None:
        dx = dx + _v64(residual)
    if post_mask is not None:
        dx = torch.where(_v64(post_mask) > 0, dx, torch.zeros_like(dx))
    if acc0 is not None:
        dx = dx + _v64(acc0)
    return dx.contiguous()


def conv_wgrad_ref(x, dy, k, stride, pad, rowscale=None, dw0=None, db0=None, groups=1):
    """(dw [K, k*k*C/groups], db [K]) fp64: dw0 + rowscale * weight gradient, db0 + rowscale * column sums of dy (autograd in float64)"""
    C, K = x.shape[-1] // groups, dy.shape[-1]
    w = torch.zeros(K, C, k, k, dtype=F64, requires_grad=True)
    F.conv2d(_x64(x), w, None, stride, pad, 1, groups).backward(_x64(dy))
    dw = w.grad.permute(0, 2, 3, 1).reshape(K, -1)
    db = _v64(dy).reshape(-1, K).sum(0)
    if rowscale is not None:
        dw, db = dw * _v64(rowscale)[:, None], db * _v64(rowscale)
    if dw0 is not None:
        dw = dw + _v64(dw0)
    if db0 is not None:
        db = db + _v64(db0)
    return dw.contiguous(), db.contiguous()


def flip_transpose_ref(w2, K, k, C):
    """the dgrad weight image [C, k*k*K] of forward weights [K, k*k*C]: wt[ci][k-1-kh][k-1-kw][co] = w[co][kh][kw][ci]"""
    return w2.view(K, k, k, C).flip(1, 2).permute(3, 1, 2, 0).reshape(C, k * k * K).contiguous()


def conv_rows_ref(x, w2, k, stride, pad, rows, out_hw=None):
    """fp64 [len(rows), K]: the rows (flattened (n, oh, ow) indices) of conv(x, w) - the im2col rows gathered tap by tap, one fp64 GEMM"""
    N, H, W, C = x.shape
    OH, OW = out_hw if out_hw is not None else ((H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1)
    xp = F.pad(x.detach().cpu().to(F64), (0, 0, pad, pad, pad, pad))
    n = rows // (OH * OW)
    oh = (rows // OW) % OH
    ow = rows % OW
    cols = [xp[n, oh * stride + a, ow * stride + b] for a in range(k) for b in range(k)]
    return torch.cat(cols, dim=1) @ w2.detach().cpu().to(F64).t()


def rows_domain(x, w2, k, stride, pad, rows, unit_exp, scale=None, bias=None, residual2d=None, relu=False):
    """fp64 reference of the selected output rows with the forward epilogue, after assert_exact_domain on them"""
    def run(x_, w_, s_, b_, r_, relu_):
        y = conv_rows_ref(x_, w_, k, stride, pad, rows)
        return _epilogue(y, s_, b_, None if r_ is None else r_[rows], relu_)
    ab = lambda t: None if t is None else t.detach().cpu().to(F64).abs()
    ref = run(x, w2, scale, bias, residual2d, relu)
    assert_exact_domain(run(ab(x), ab(w2), ab(scale), ab(bias), ab(residual2d), False), ref, unit_exp)
    return ref


def level_rows(level_hw, N):
    rows, r = [], 0
    for h, w in level_hw:
        rows.append((r, r + N * h * w))
        r += N * h * w
    return rows


def ml_views(t2d, level_hw, N):
    """the levels of a level-first [P, C] matrix as NHWC views"""
    return [t2d[r0:r1].view(N, h, w, t2d.shape[1]) for (r0, r1), (h, w) in zip(level_rows(level_hw, N), level_hw)]


def ml_fwd_ref(x2d, w2, level_hw, N, k, pad, scale=None, bias=None, residual=None, relu=False, acc0=None):
    """level-first [P, K] fp64: conv_fwd_ref per level (stride 1); acc0 [P, K]: added after the epilogue (accumulate)"""
    res = ml_views(residual, level_hw, N) if residual is not None else [None] * len(level_hw)
    outs = [conv_fwd_ref(xl, w2, k, 1, pad, scale, bias, rl, relu).reshape(-1, w2.shape[0])
            for xl, rl in zip(ml_views(x2d, level_hw, N), res)]
    y = torch.cat(outs)
    return y if acc0 is None else y + _v64(acc0)


def ml_dgrad_ref(dy2d, w2, level_hw, N, k, pad, C):
    """level-first [P, C] fp64: conv_dgrad_ref per level (w2: the FORWARD weights [K, k*k*C])"""
    return torch.cat([conv_dgrad_ref(dl, w2, (N, h, w, C), k, 1, pad).reshape(-1, C)
                      for dl, (h, w) in zip(ml_views(dy2d, level_hw, N), level_hw)])


def ml_wgrad_ref(x2d, dy2d, level_hw, N, k, pad, rowscale=None, dw0=None, db0=None):
    dw = db = None
    for xl, dl in zip(ml_views(x2d, level_hw, N), ml_views(dy2d, level_hw, N)):
        a, b = conv_wgrad_ref(xl, dl, k, 1, pad)
        dw, db = (a, b) if dw is None else (dw + a, db + b)
    if rowscale is not None:
        dw, db = dw * _v64(rowscale)[:, None], db * _v64(rowscale)
    if dw0 is not None:
        dw = dw + _v64(dw0)
    if db0 is not None:
        db = db + _v64(db0)
    return dw, db


def r16(t64, h16):
    """one rounding of an (fp32-exact) fp64 tensor to h16, back in fp64: the roundings the fused kernels apply to their intermediates"""
    return to_out(t64, h16).to(F64)


def bottleneck_ref(x, w1, w2, w3, s1, b1, s2, b2, s3, b3, h16, wsc=None, ssc=None, bsc=None, abs_bound=False):
    """fp64 chain of one frozen bottleneck with the 16-bit roundings of c1, c2 and the shortcut: returns (y, c1, c2, shortcut) fp64 NHWC.
    abs_bound: no roundings (the operands are absolute values: the bound of assert_exact_domain)"""
    rnd = (lambda t: t) if abs_bound else (lambda t: r16(t, h16))
    MID = w1.shape[0]
    c1 = rnd(conv_fwd_ref(x, w1, 1, 1, 0, s1, b1, relu=True))
    c2 = rnd(conv_fwd_ref(c1, w2, 3, 1, 1, s2, b2, relu=True))
    sc = rnd(conv_fwd_ref(x, wsc, 1, 1, 0, ssc, bsc)) if wsc is not None else _v64(x)
    y = conv_fwd_ref(c2, w3, 1, 1, 0, s3, b3, residual=sc, relu=True)
    assert c1.shape[-1] == MID
    return y, c1, c2, sc


def stem_operands(x16pad, w16s):
    """(x NHWC [N, Hc, Wc, 3], w2 [K, 7*7*3]) of the 7x7 stride-2 pad-3 stem conv from the stored zero-bordered 16-bit image and the
    [K, 7*32] stem weight image"""
    Hc, Wc = x16pad.canvas
    xi = x16pad[:, 3:3 + Hc, 3:3 + Wc, :3]
    K = w16s.shape[0]
    w2 = w16s.view(K, 7, 8, 4)[:, :, :7, :3].reshape(K, 147)
    return xi, w2


def stem_ref(xi, w2, scale, shift, h16=None):
    """fp64 relu(conv7x7s2p3 * scale + shift) NHWC; h16: rounded once to it (the stem output as stored)"""
    y = conv_fwd_ref(xi, w2, 7, 2, 3, scale, shift, relu=True)
    return y if h16 is None else r16(y, h16)


def maxpool_ref(y64):
    return F.max_pool2d(y64.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()


# ----------------------------------------------------------------------------------------------------------------------------------
# the precondition and the expectation
def to_out(ref64, dtype):
    """fp64 -> fp32 (checked lossless) -> dtype: a 16-bit expectation is ONE rounding (to nearest even) of the exact value"""
    f = ref64.to(torch.float32)
    assert torch.equal(f.to(F64), ref64), "the reference is not exact in fp32"
    return f.to(dtype)


def _units(t64, unit_exp):
    return t64 * (2.0 ** -unit_exp)


def assert_on_grid(t, unit_exp, what="operand"):
    u = _units(_v64(t), unit_exp)
    assert torch.equal(u, u.round()), "%s is not an integer multiple of 2^%d" % (what, unit_exp)


def assert_exact_domain(bound64, ref64, unit_exp):
    """bound64: the same expression as ref64 computed in fp64 from the ABSOLUTE operands (conv of |x| and |w|, times |scale|, plus |bias|,
    plus |residual|) - it bounds every product and every partial sum in any order; unit_exp: exponent of the product grid.
    Asserts: the reference sits on the grid, everything is below 2^24 grid units, and the fp64 reference survives fp32 unchanged."""
    b = _units(bound64, unit_exp)
    assert float(b.max()) < LIMIT, "partial sums may reach %.3g grid units (limit 2^24)" % float(b.max())
    assert_on_grid(ref64, unit_exp, "the reference")
    assert bool((ref64.abs() <= bound64).all()), "the bound does not bound the reference"
    assert torch.equal(ref64.to(torch.float32).to(F64), ref64)


def fwd_domain(x, w2, k, stride, pad, unit_exp, scale=None, bias=None, residual=None, relu=False, groups=1, acc0=None):
    """fp64 forward reference, after assert_exact_domain on it; unit_exp = exponent of unit(x) * unit(w) * unit(scale)"""
    ab = lambda t: None if t is None else t.detach().cpu().to(F64).abs()
    ref = conv_fwd_ref(x, w2, k, stride, pad, scale, bias, residual, relu, groups, acc0)
    bound = conv_fwd_ref(ab(x), ab(w2), k, stride, pad, ab(scale), ab(bias), ab(residual), False, groups, ab(acc0))
    for t, n in ((bias, "bias"), (residual, "residual"), (acc0, "accumulate addend")):
        if t is not None:
            assert_on_grid(t, unit_exp, n)
    assert_exact_domain(bound, ref, unit_exp)
    return ref


def dgrad_domain(dy, w2, in_shape, k, stride, pad, unit_exp, mask=None, residual=None, post_mask=None, groups=1, scale=None, acc0=None):
    ab = lambda t: None if t is None else t.detach().cpu().to(F64).abs()
    ref = conv_dgrad_ref(dy, w2, in_shape, k, stride, pad, mask, residual, post_mask, groups, scale, acc0)
    bound = conv_dgrad_ref(ab(dy), ab(w2), in_shape, k, stride, pad, None, ab(residual), None, groups, ab(scale), ab(acc0))
    for t, n in ((residual, "residual"), (acc0, "accumulate addend")):
        if t is not None:
            assert_on_grid(t, unit_exp, n)
    assert_exact_domain(bound, ref, unit_exp)
    return ref


def wgrad_domain(x, dy, k, stride, pad, unit_exp, rowscale=None, dw0=None, db0=None, db_unit_exp=None, groups=1):
    """(dw, db) fp64 after assert_exact_domain on both; unit_exp = unit(x) * unit(dy) * unit(rowscale), db_unit_exp = unit(dy) * unit(rowscale)"""
    ab = lambda t: None if t is None else t.detach().cpu().to(F64).abs()
    dw, db = conv_wgrad_ref(x, dy, k, stride, pad, rowscale, dw0, db0, groups)
    bw, bb = conv_wgrad_ref(ab(x), ab(dy), k, stride, pad, ab(rowscale), ab(dw0), ab(db0), groups)
    assert_exact_domain(bw, dw, unit_exp)
    assert_exact_domain(bb, db, unit_exp if db_unit_exp is None else db_unit_exp)
    return dw, db


def ml_fwd_domain(x2d, w2, level_hw, N, k, pad, unit_exp, scale=None, bias=None, residual=None, relu=False, acc0=None):
    ab = lambda t: None if t is None else t.detach().cpu().to(F64).abs()
    ref = ml_fwd_ref(x2d, w2, level_hw, N, k, pad, scale, bias, residual, relu, acc0)
    bound = ml_fwd_ref(ab(x2d), ab(w2), level_hw, N, k, pad, ab(scale), ab(bias), ab(residual), False, ab(acc0))
    assert_exact_domain(bound, ref, unit_exp)
    return ref


def ml_dgrad_domain(dy2d, w2, level_hw, N, k, pad, C, unit_exp):
    ab = lambda t: t.detach().cpu().to(F64).abs()
    ref = ml_dgrad_ref(dy2d, w2, level_hw, N, k, pad, C)
    assert_exact_domain(ml_dgrad_ref(ab(dy2d), ab(w2), level_hw, N, k, pad, C), ref, unit_exp)
    return ref


def ml_wgrad_domain(x2d, dy2d, level_hw, N, k, pad, unit_exp, rowscale=None, dw0=None, db0=None, db_unit_exp=None):
    ab = lambda t: None if t is None else t.detach().cpu().to(F64).abs()
    dw, db = ml_wgrad_ref(x2d, dy2d, level_hw, N, k, pad, rowscale, dw0, db0)
    bw, bb = ml_wgrad_ref(ab(x2d), ab(dy2d), level_hw, N, k, pad, ab(rowscale), ab(dw0), ab(db0))
    assert_exact_domain(bw, dw, unit_exp)
    assert_exact_domain(bb, db, unit_exp if db_unit_exp is None else db_unit_exp)
    return dw, db


def tie_and_inexact_share(ref64, h16):
    """(share of exact ties, share of values that need rounding at all) of a 16-bit expectation: a tie is a value exactly half way between
    two neighbouring h16 values"""
    f = ref64.to(torch.float32)
    r = f.to(h16).to(torch.float32)
    inexact = r != f
    # the neighbours of f in h16 on either side: r and the next h16 value in the direction of f
    bits = r.to(h16).view(torch.int16).to(torch.int32)
    step = torch.where((f.abs() > r.abs()), 1, -1)
    other = (bits + step).to(torch.int16).view(h16).to(torch.float32)
    tie = inexact & ((r.to(F64) + other.to(F64)) * 0.5 == f.to(F64))
    n = max(f.numel(), 1)
    return float(tie.sum()) / n, float(inexact.sum()) / n


# ----------------------------------------------------------------------------------------------------------------------------------
# the project's Gaussian criteria (test_conv_bf16_gpu.py), for the fp16 build
def relerr(a, b):
    return (a.double() - b.double()).abs().max().item() / (b.double().abs().max().item() + 1e-12)


def close16(y, ref, eps):
    """test_conv_bf16_gpu.close16 with the half-ulp term 2^-8 (bf16) replaced by eps (fp16: 2^-11)"""
    y, ref = y.double(), ref.double()
    tol = eps * ref.abs() + 2e-4 * ref.abs().max()
    return bool(((y - ref).abs() <= tol).all())


# ----------------------------------------------------------------------------------------------------------------------------------
# the route table: the smallest shape that reaches each kernel of launch_igemm16 (csrc/conv_bf16.hip), with the rule that selects it
# NHWC cases: name -> (N, H, W, C, K, k, stride, pad, x_is_fp32, bits_x, bits_w); the bits are chosen so that a result has 12 .. 15
# significant bits: enough that both 16-bit types round it, few enough that a good share of the roundings are exact ties
NHWC_CASES = {
    # x fp32 or C % 32 != 0 -> not v2-eligible -> conv_igemm_bf16<BN>; K <= 64 -> BN = 64 (launch_nhwc16)
    "generic64": (1, 7, 9, 24, 64, 1, 1, 0, False, 5, 4),
    # fp32 x -> conv_igemm_bf16<128> (K = 136 > 64: two column tiles, the second one 8 wide)
    "generic128": (1, 9, 9, 32, 136, 3, 1, 1, True, 4, 3),
    # 16-bit x, C % 32 == 0, K <= 64, Kred = 288 < 1024 -> v2<64, ., 32>
    "v2_64_bk32": (1, 9, 9, 32, 40, 3, 1, 1, False, 4, 3),
    # K > 64, Kred = 864 < 1024 and C % 64 != 0 -> not deep -> v2<128, ., 32>
    "v2_128_bk32": (2, 12, 10, 96, 136, 3, 1, 1, False, 3, 3),
    # C % 64 == 0, Kred = 1152 >= 1024 -> deep; K = 80 < 256 -> below the 256 tile -> v2<128, ., 64>
    "v2_128_bk64": (1, 20, 20, 128, 80, 3, 1, 1, False, 3, 3),
    # K > 32, 3x3, M = 257 * 256 = 65792 >= 65536, BN = 64 -> v2<64, ., 32, ., TALL>; every 256-row tile is full ...
    "tall64": (1, 257, 256, 32, 40, 3, 1, 1, False, 4, 3),
    # ... M = 258 * 255 = 65790 = 256 * 256 + 254: the last row tile is ragged
    "tall64_ragged": (1, 258, 255, 32, 40, 3, 1, 1, False, 4, 3),
    # 1x1 (no rowinfo -> no row-span), C % 64 == 0, Kred = 1024, K = 512 >= 256: tiles_all = cdiv(16510, 256) * 2 = 130 > 128 ->
    # every row on the 256 tile; grid 130 <= 256 -> one tile per workgroup; M % 256 = 126
    "pp_one_tile": (1, 130, 127, 1024, 512, 1, 1, 0, False, 3, 3),
    # 1x1, K = 1024: tilesN = 4, M / 256 = 129 -> 516 tiles -> main_tiles = 512 (two persistent rounds: grid 512 > 256 -> ntiles),
    # tiles_all - 512 = 8 <= 128 -> rows [32768, 33068) on the 128 kernel with m_begin = 32768
    "pp_persistent_rem": (1, 28, 1181, 1024, 1024, 1, 1, 0, False, 3, 3),
    # strided 3x3: stride 2 -> rs_ok false -> plain ping-pong; the issue's (2,181,181,128,256): M = 16562, tiles_all = 65 <= 128 ->
    # main_tiles = 0 -> it stays on v2<128, ., 64> (kept as the strided case of that kernel) ...
    "strided_bk64": (2, 181, 181, 128, 256, 3, 2, 1, False, 3, 3),
    # ... K = 512 doubles the column tiles: tiles_all = 130 > 128 -> conv_igemm_bf16_pp with a strided 3x3 gather
    "pp_strided": (2, 181, 181, 128, 512, 3, 2, 1, False, 3, 3),
    # 3x3 stride 1 pad 1 with rowinfo (16-bit x, C % 32 == 0) -> row-span; M = 36000: tiles_all = 141 > 128 -> all rows; W = 3
    "rs_narrow": (40, 300, 3, 128, 256, 3, 1, 1, False, 3, 3),
    # K = 512: tiles_m = 139 -> 278 tiles -> main_tiles = 256 (one round, 128 row tiles), 280 - 256 = 24 <= 128 -> rows [32768, 35631) on
    # the 128 kernel
    "rs_rem": (3, 111, 107, 256, 512, 3, 1, 1, False, 3, 2),
}
BIG_M = ("tall64", "tall64_ragged", "pp_persistent_rem", "rs_narrow", "rs_rem")     # M > 30000: the fp64 reference is compared on a stratified row subset

# dgrad-only: stride 2 -> in_dil = 2 -> not v2-eligible -> the generic kernel's dilated gather
DGRAD_DILATED = (2, 13, 21, 64, 128, 3, 2, 1)

# multi-level cases: name -> (level_hw, N, C, K, bits_x, bits_w)
ML_CASES = {
    # ml_fwd_g sends K <= 64 to launch_igemm16<64, true> only when the call is `plain`: dense, ungrouped and WITHOUT a geometry table.  The
    # Python wrapper passes a table whenever k > 1, x is 16-bit, C % 32 == 0, K % 4 == 0 and both row pitches are multiples of 8: K = 36
    # (pitch 36, not a multiple of 8; K % 4 == 0 as the epilogue needs) gets none -> v2<64, true, 32>; levels down to (1, 1)
    "ml64": ([(12, 16), (6, 8), (3, 4), (2, 2), (1, 1)], 2, 32, 36, 4, 3),
    # K = 40 gets the table -> not plain -> launch_igemm16<128, true> although K <= 64: v2<128, true, 32> with one 40-wide column tile
    "ml128_k40": ([(12, 16), (6, 8), (3, 4), (2, 2), (1, 1)], 2, 32, 40, 4, 3),
    # K = 136 > 96 -> launch_igemm16<128, true>; Kred = 576 < 1024 -> v2<128, true, 32>
    "ml128": ([(12, 16), (6, 8), (3, 4), (2, 2), (1, 1)], 3, 64, 136, 3, 3),
    # C % 64 == 0, Kred = 1152 >= 1024, K = 512 with rowinfo, M = 22401: tiles_all = 88 * 2 = 176 > 128 -> row-span, every row (the last
    # row tile ragged); levels down to (1, 1)
    "ml_rs": ([(100, 168), (50, 84), (25, 42), (13, 21), (7, 11), (1, 1)], 1, 128, 512, 3, 3),
    # n96_eligible: 64 < K <= 96, K % 4 == 0, C % 32 == 0, M = 12800 >= 8192 -> v2<96, true, 32>
    "n96_72": ([(64, 80), (32, 40)], 2, 64, 72, 3, 3),
    "n96_96": ([(64, 80), (32, 40)], 2, 64, 96, 3, 3),
    # M = 12800 = 50 * 256 fills every row tile of the two cases above; M = 2 * (64 * 81 + 32 * 40) = 12928 = 50 * 256 + 128: ragged
    "n96_72_ragged": ([(64, 81), (32, 40)], 2, 64, 72, 3, 3),
}

# weight gradients: name -> (N, H, W, C, K, k, stride, pad)
WGRAD_128 = {
    "one_split": (3, 9, 9, 32, 40, 3, 1, 1),          # chunks = cdiv(243, 32) = 8 -> max_by_chunks = 1 -> one split
    "many_splits": (2, 25, 42, 64, 128, 3, 1, 1),     # chunks = 66 -> max_by_chunks = 8 -> 8 splits
    "ragged_1x1": (2, 8, 8, 200, 136, 1, 1, 0),       # C % 128 != 0, K % 128 != 0
}
WGRAD_PP = {
    # wgrad16_w8_shape_ok: 16-bit x and dy, C % 256 == K % 256 == 0, chunks = cdiv(M, 64) >= 16
    "pp_3x3": (1, 33, 37, 256, 256, 3, 1, 1),         # M = 1221: 20 chunks, ragged
    "pp_strided": (2, 41, 41, 256, 256, 3, 2, 1),     # M = 882: 14 chunks < 16 -> the 128-tile kernel (kept: the issue's shape) ...
    "pp_strided_big": (3, 41, 41, 256, 256, 3, 2, 1),  # ... M = 1323: 21 chunks -> conv_wgrad_bf16_pp
}
WGRAD_PP_TOWER = ([(25, 42), (13, 21), (7, 11), (4, 6), (2, 3)], 2, 256, 256)

BOTTLENECK_SHAPES = [(2, 24, 48), (1, 21, 37), (3, 8, 16), (1, 5, 7)]
STEM_CANVASES = [(50, 70), (64, 61)]
STEM_POOL_HW = [(64, 96), (70, 66), (33, 18)]


def nhwc_operands(name, seed=0):
    """(x NHWC fp32 dyadic, w2 [K, k*k*C] fp32 dyadic, unit_exp) of one NHWC_CASES entry: x integers * 2^-3, w integers * 2^-5"""
    N, H, W, C, K, k, s, p, x32, bx, bw = NHWC_CASES[name]
    g = torch.Generator().manual_seed(seed)
    x = dyadic((N, H, W, C), bx, -3, g)
    w2 = dyadic((K, k * k * C), bw, -5, g)
    return x, w2, -8


def epilogue_operands(K, out_shape, unit_exp, seed, res_bits=4):
    """(scale [K] two-bit multipliers, bias [K], residual out_shape) on the grid 2^(unit_exp - 1) (scale has unit 2^-1)"""
    g = torch.Generator().manual_seed(1000 + seed)
    scale = small_scale((K,), g)
    bias = dyadic((K,), 9, unit_exp - 1, g)
    # the residual is a 16-bit tensor when the output is: 7 bits (exact in either type), placed high so that it meets the conv sum's top bits
    res = dyadic(out_shape, 7, unit_exp - 1 + res_bits, g)
    return scale, bias, res


def bottleneck_operands(shape, shortcut, seed=7):
    """operands of one frozen bottleneck inside the exact domain: x in {0 .. 3}, weights in {-1, 0, 1} (sparse for the 3x3), scales powers of
    two times a 2-bit multiplier where the next layer's bound allows it.  Returns a dict of CPU fp32 tensors."""
    N, H, W = shape
    C, MID, K = (64 if shortcut else 256), 64, 256
    g = torch.Generator().manual_seed(seed)
    o = dict(x=dyadic((N, H, W, C), 2, 0, g, relu_like=True, zero_frac=0.0),
             w1=dyadic((MID, C), 1, 0, g, zero_frac=0.25), w2=dyadic((MID, 9 * MID), 1, 0, g, zero_frac=0.5),
             w3=dyadic((K, MID), 1, 0, g, zero_frac=0.25),
             s1=small_scale((MID,), g, 1), b1=dyadic((MID,), 4, 0, g),
             s2=pow2((MID,), -4, -3, g), b2=dyadic((MID,), 4, -4, g),
             s3=pow2((K,), -3, -2, g), b3=dyadic((K,), 4, -7, g))
    if shortcut:
        o.update(wsc=dyadic((K, C), 1, 0, g, zero_frac=0.25), ssc=small_scale((K,), g, 0), bsc=dyadic((K,), 4, -1, g))
    return o


BOTTLENECK_UNIT_EXP = -7     # x 2^0 * w 2^0 * s1 2^0 -> c1 on 2^0; * s2 2^-4 -> c2 on 2^-4; * s3 2^-3 -> y on 2^-7 (shortcut: 2^-1)


def bottleneck_domain(o, h16):
    """fp64 chain (y, c1, c2, shortcut) of bottleneck_operands after assert_exact_domain on every stage"""
    keys = ("x", "w1", "w2", "w3", "s1", "b1", "s2", "b2", "s3", "b3")
    kw = {k: o[k] for k in ("wsc", "ssc", "bsc") if k in o}
    y, c1, c2, sc = bottleneck_ref(*[o[k] for k in keys], h16, **kw)
    ab = {k: v.abs() for k, v in o.items()}
    # rounding an intermediate to h16 can raise it by half an ulp: 2^-8 relative covers bf16 and fp16, three stages deep
    by, b1_, b2_, bs = bottleneck_ref(*[ab[k] for k in keys], h16, abs_bound=True, **{k: ab[k] for k in kw})
    grow = (1 + 2.0 ** -8)
    assert_exact_domain(b1_, conv_fwd_ref(o["x"], o["w1"], 1, 1, 0, o["s1"], o["b1"], relu=True), 0)
    assert_exact_domain(b2_ * grow, conv_fwd_ref(c1, o["w2"], 3, 1, 1, o["s2"], o["b2"], relu=True), -4)
    if "wsc" in o:
        assert_exact_domain(bs, conv_fwd_ref(o["x"], o["wsc"], 1, 1, 0, o["ssc"], o["bsc"]), -1)
    assert_exact_domain(by * grow * grow, y, BOTTLENECK_UNIT_EXP)
    return y, c1, c2, sc


def stem_images(hw, N, seed=3):
    """N integer-valued [3, H, W] fp32 images in [0, 255]"""
    g = torch.Generator().manual_seed(seed)
    H, W = hw
    return [torch.randint(0, 256, (3, H, W), generator=g).to(torch.float32) for _ in range(N)]


STEM_MEAN, STEM_STD = [128.0, 128.0, 128.0], [64.0, 64.0, 64.0]     # (v - 128) / 64: multiples of 2^-6 in [-2, 2): exact in bf16 and fp16


def stem_weights(seed=3, K=64):
    """(w208 fp32 [K, 208] - 7x7x4 taps, 16-padded rows -, scale [K], shift [K]): weights 5-bit integers * 2^-5, shift on the output grid"""
    g = torch.Generator().manual_seed(100 + seed)
    w208 = torch.zeros(K, 208)
    w = dyadic((K, 7, 7, 3), 5, -5, g)
    w208[:, :196].view(K, 7, 7, 4)[..., :3] = w
    return w208, small_scale((K,), g), dyadic((K,), 6, -12, g)


STEM_UNIT_EXP = -12      # x 2^-6 * w 2^-5 * scale 2^-1


def subset_rows(M, tile, seed=0, share=0.1):
    """the stratified row subset of the M > 30000 cases: the first and last 512 rows, every tile boundary +- 1, and a seeded sample of
    `share` of the rest (sorted, unique)"""
    idx = set(range(min(512, M))) | set(range(max(M - 512, 0), M))
    for b in range(tile, M, tile):
        idx.update(i for i in (b - 1, b, b + 1) if 0 <= i < M)
    g = torch.Generator().manual_seed(seed)
    extra = torch.randperm(M, generator=g)[:int(share * M) + 1].tolist()
    idx.update(extra)
    return torch.tensor(sorted(idx), dtype=torch.int64)


WGRAD_UNIT_EXP = -8        # x integers * 2^-3, dy integers * 2^-4, rowscale 2^-1 .. 2^1
WGRAD_DB_UNIT_EXP = -5     # dy 2^-4 * rowscale 2^-1


def _wgrad_tail_operands(K, Kred, g):
    """(rowscale [K] powers of two, dw0 [K, Kred] and db0 [K] non-zero dyadic starting values on the result grids)"""
    return pow2((K,), -1, 1, g), dyadic((K, Kred), 6, WGRAD_UNIT_EXP + 3, g, zero_frac=0.0), dyadic((K,), 6, WGRAD_DB_UNIT_EXP + 2, g, zero_frac=0.0)


def wgrad_operands(N, H, W, C, K, k, s, p, seed=2):
    g = torch.Generator().manual_seed(seed)
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    x = dyadic((N, H, W, C), 3, -3, g, relu_like=True)
    dy = dyadic((N, OH, OW, K), 3, -4, g)
    return (x, dy) + _wgrad_tail_operands(K, k * k * C, g)


def wgrad_ml_operands(level_hw, N, C, K, seed=5):
    g = torch.Generator().manual_seed(seed)
    P = N * sum(h * w for h, w in level_hw)
    return (dyadic((P, C), 3, -3, g, relu_like=True), dyadic((P, K), 3, -4, g)) + _wgrad_tail_operands(K, 9 * C, g)


def gaussian_operands(name, seed=0):
    """the randn operands of test_conv_bf16_gpu.py rounded to fp16 (as fp32 tensors): x NHWC, w2 [K, k*k*C], bias [K], residual NHWC"""
    N, H, W, C, K, k, s, p = NHWC_CASES[name][:8]
    g = torch.Generator().manual_seed(seed)
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    h = lambda t: t.to(torch.float16).to(torch.float32)
    return (h(torch.randn(N, H, W, C, generator=g)), h(torch.randn(K, k * k * C, generator=g) * 0.05), torch.randn(K, generator=g),
            h(torch.randn(N, OH, OW, K, generator=g)))


def stem_taps(w208):
    """the 7x7x3 taps [K, 147] (reduction index (kh, kw, ci)) of an fp32 [K, 208] stem weight (7x7x4 taps, 16-padded rows)"""
    K = w208.shape[0]
    return w208[:, :196].view(K, 7, 7, 4)[..., :3].reshape(K, 147).contiguous()


def gaussian_ml_operands(name, seed=0):
    """randn operands of one ML_CASES entry rounded to fp16 (as fp32 tensors): x [P, C], w2 [K, 9*C], bias [K], residual [P, K]"""
    level_hw, N, C, K = ML_CASES[name][:4]
    g = torch.Generator().manual_seed(seed)
    P = N * sum(h * w for h, w in level_hw)
    h = lambda t: t.to(torch.float16).to(torch.float32)
    return (h(torch.randn(P, C, generator=g)), h(torch.randn(K, 9 * C, generator=g) * 0.05), torch.randn(K, generator=g),
            h(torch.randn(P, K, generator=g)))


# ----------------------------------------------------------------------------------------------------------------------------------
# the fp32 implicit-GEMM convs (csrc/conv.hip) and the grouped 3x3 conv (csrc/conv_grouped.hip): test_conv_f32_exact_gpu.py,
# test_gconv_exact_gpu.py.  fp32 operands carry as many bits as the reduction length leaves room for.
def dyadic_nonzero(shape, bits, scale_exp, generator):
    """dyadic without a single zero (an integer 0 becomes 1): what an accumulate launch adds onto, so that an ignored flag shows everywhere"""
    t = dyadic(shape, bits, scale_exp, generator, zero_frac=0.0)
    t[t == 0] = 2.0 ** scale_exp
    return t


def f32_operand_bits(Kred):
    """(bits_x, bits_w) of an fp32 case: the widest pair (x at most one bit ahead) with (2^bx - 1) * (2^bw - 1) * Kred * 6 < 2^23 - the
    largest scale multiplier is 6 units, and half of the 2^24 units stay free for the bias, the residual and the accumulate addend"""
    bx, bw = 12, 11
    while (2 ** bx - 1) * (2 ** bw - 1) * Kred * 6 >= 2 ** 23:
        if bx > bw:
            bx -= 1
        else:
            bw -= 1
    return bx, bw


# channel cases of utv2_conv2d_nhwc_fwd: name -> (C, K).  The rules (conv.hip): K <= 64 -> conv_igemm_f32<64, .>, else <128, .>;
# C % 16 == 0 -> MODE 0 (vector gather), else MODE 2 (scalar gather); K % 4 == 0 -> epilogue_rows, else the scalar epilogue
F32_CASES = {
    "m0_bn64_k8": (16, 8),          # MODE 0, 64-wide tile, 8 of its 64 columns
    "m0_bn64_k64": (32, 64),        # MODE 0, the 64-wide tile full, two channel slabs
    "m0_bn128_k72": (16, 72),       # MODE 0, one partial 128-wide tile
    "m0_bn128_k136": (32, 136),     # MODE 0, two column tiles, the second 8 wide
    "m2_bn64_k8": (20, 8),          # MODE 2: C = 20, a 16-wide k chunk straddles taps
    "m2_bn64_k64": (12, 64),
    "m2_bn128_k72": (20, 72),
    "m2_bn128_k136": (12, 136),
    "m0_bn64_k7_scalar": (16, 7),   # K % 4 != 0 -> the scalar epilogue, MODE 0 / 64
    "m0_bn128_k73_scalar": (32, 73),
    "m2_bn64_k7_scalar": (20, 7),
    "m2_bn128_k73_scalar": (12, 73),
}
# geometries of every channel case: (N, H, W, k, stride, pad).  (2, 9, 7) stride 1: M = 126 < 128, one partial row tile; (2, 9, 8): M = 144,
# two row tiles, the second 16 rows; stride 2: the odd sides 9 and 7 and the even side 8
F32_GEOMS = [(2, 9, 7, 3, 1, 1), (2, 9, 8, 3, 1, 1), (2, 9, 7, 3, 2, 1), (2, 9, 8, 3, 2, 1),
             (2, 9, 7, 1, 1, 0), (2, 9, 8, 1, 1, 0), (2, 9, 7, 1, 2, 0), (2, 9, 8, 1, 2, 0)]

# dgrads (utv2_conv2d_nhwc_fwd over dY with in_dil = stride): name -> (N, H, W, C, K, k, stride, pad) of the FORWARD conv.  The gather
# mode follows the reduction channels K (K % 16 == 0 -> MODE 0), the tile and the epilogue follow the output channels C
F32_DGRAD = {
    "m0_s1": (2, 9, 7, 16, 32, 3, 1, 1),            # MODE 0, in_dil 1, odd sides
    "m0_s2": (2, 9, 8, 20, 16, 3, 2, 1),            # MODE 0, in_dil 2, an odd and an even side (output_padding 1 on the even one)
    "m2_s2": (2, 9, 8, 16, 20, 3, 2, 1),            # MODE 2 with in_dil 2
    "m2_s2_scalar": (2, 8, 7, 7, 12, 3, 2, 1),      # MODE 2, in_dil 2, C = 7: the scalar epilogue
    "m2_s1_bn128": (2, 9, 7, 72, 24, 3, 1, 1),      # MODE 2, in_dil 1, the 128-wide tile
    "m0_1x1_s2": (2, 9, 8, 16, 16, 1, 2, 0),        # 1x1 stride 2: only the even pixels receive a gradient (the last column of W = 8 none)
    "m2_1x1_s2": (2, 9, 8, 12, 20, 1, 2, 0),
}
F32_FLIP = [(7, 3, 20), (64, 1, 16), (72, 3, 16)]   # (K, k, C) of weight_flip_transpose_f32

# the image stem (utv2_conv2d_stem_fwd -> conv_igemm_f32<., 1>): 7x7 stride 2 pad 3 on an NHWC4 image, weight rows padded from 196 to 208;
# K = 64 -> the 64-wide tile, K = 72 -> the 128-wide one.  (N, H, W): M = 60 (one partial row tile) and M = 144 (two)
F32_STEM_K = [64, 72]
F32_STEM_IMAGES = [(2, 9, 11), (2, 16, 18)]
F32_STEM_UNIT_EXP = -9      # x 2^-3 * w 2^-5 * scale 2^-1

# multi-level convs (utv2_conv2d_ml_fwd -> conv_igemm_f32<., 0, true>, utv2_conv2d_ml_wgrad -> conv_wgrad_f32<1, true>): C % 16 == 0 and
# K % 4 == 0 are required; K <= 64 -> the 64-wide tile.  P = 2 * (35 + 12 + 1) = 96 rows: one partial 128-row tile across all levels and images
F32_ML_LEVELS, F32_ML_N = [(5, 7), (3, 4), (1, 1)], 2
F32_ML = {"ml64": (16, 8), "ml128": (32, 72)}       # name -> (C, K), each with k = 1 and k = 3

# weight gradients (utv2_conv2d_nhwc_wgrad): name -> (N, H, W, C, K, k, stride, pad); C % 4 == 0 and K % 4 == 0 -> conv_wgrad_f32<1>, else <0>.
# Every output is 2 x 12 x 11: M = 264 = 16 chunks of 16 + 8 -> 17 chunks -> max_by_chunks = 2 -> two splits of 9 and 8 chunks, the last partial
F32_WGRAD = {
    "vec_s1": (2, 12, 11, 16, 136, 3, 1, 1),        # Kred = 144: a second column tile of 16; K = 136: a second row tile of 8
    "vec_s2": (2, 24, 21, 16, 136, 3, 2, 1),
    "scalar_k7": (2, 12, 11, 20, 7, 3, 1, 1),       # K % 4 != 0
    "scalar_k7_s2": (2, 23, 22, 16, 7, 3, 2, 1),
    "scalar_c6": (2, 12, 11, 6, 8, 3, 1, 1),        # C % 4 != 0
    "scalar_c6_1x1_s2": (2, 23, 21, 6, 8, 1, 2, 0),
}
F32_WGRAD_UNIT_EXP = -7     # x integers * 2^-3, dy integers * 2^-4
F32_WGRAD_DB_UNIT_EXP = -4

# column sums (utv2_colsum): name -> (M, C).  C % 4 == 0, 256 % (C / 4) == 0 and M >= 1024 -> colsum_partial_vec_f32 with 256-row blocks,
# else colsum_partial_f32 with P = min(cdiv(M, 512), 64) row ranges.  The vector route doubles its block rows beyond 256 * 1024 rows: that
# branch needs M > 262144 and stays untested.
COLSUM_CASES = {
    "vec_ragged": (1030, 16),       # 5 blocks, the last one 6 rows
    "scalar_c24": (1030, 24),       # C / 4 = 6 does not divide 256; P = 3
    "scalar_small_m": (600, 16),    # M < 1024; P = 2
    "scalar_c72": (70, 72),         # P = 1, two 64-channel blocks, the second 8 wide
}
COLSUM_UNIT_EXP = -6


def f32_wgrad_splits(M, K, Kred):
    """utv2_conv2d_wgrad_splits (conv.hip) restated"""
    chunks = -(-M // 16)
    tiles = -(-K // 128) * -(-Kred // 128)
    return max(1, min(-(-1024 // tiles), max(chunks // 8, 1), 256))


def colsum_route(M, C):
    """("vec", blocks, rows per block) or ("scalar", P, rows per range): the dispatch of utv2_colsum restated"""
    if C % 4 == 0 and C // 4 <= 256 and 256 % (C // 4) == 0 and M >= 1024:
        rows = 256
        while -(-M // rows) > 1024:
            rows *= 2
        return "vec", -(-M // rows), rows
    P = max(1, min(-(-M // 512), 64))
    return "scalar", P, -(-M // P)


def _out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def f32_fwd_operands(C, K, geom, seed=0):
    """dict of CPU fp32 operands of one (channel case, geometry): x integers * 2^-3, w integers * 2^-5 (f32_operand_bits), scale two-bit
    multipliers of unit 2^-1, bias / residual / acc0 (the output's content before an accumulate launch, non-zero) on the grid 2^-9"""
    N, H, W, k, s, p = geom
    bx, bw = f32_operand_bits(k * k * C)
    g = torch.Generator().manual_seed(seed)
    OH, OW = _out_hw(H, W, k, s, p)
    shp = (N, OH, OW, K)
    return dict(x=dyadic((N, H, W, C), bx, -3, g), w=dyadic((K, k * k * C), bw, -5, g), scale=small_scale((K,), g),
                bias=dyadic((K,), 12, -9, g), res=dyadic(shp, 12, -6, g), acc0=dyadic_nonzero(shp, 12, -7, g), unit=-8)


def f32_dgrad_operands(name, seed=1):
    N, H, W, C, K, k, s, p = F32_DGRAD[name]
    bx, bw = f32_operand_bits(k * k * K)
    g = torch.Generator().manual_seed(seed)
    OH, OW = _out_hw(H, W, k, s, p)
    return dict(dy=dyadic((N, OH, OW, K), bx, -3, g), w=dyadic((K, k * k * C), bw, -5, g),
                acc0=dyadic_nonzero((N, H, W, C), 12, -7, g), unit=-8)


def f32_stem_operands(K, image, seed=3):
    """x4 NHWC4 (all four channels non-zero: the kernel multiplies every one), w [K, 208] with the 4 x 49 taps in [0, 196) and arbitrary
    finite values in the padding [196, 208) - its taps 49 .. 51 do not exist, so the kernel feeds zeros against them"""
    N, H, W = image
    g = torch.Generator().manual_seed(seed)
    return dict(x=dyadic((N, H, W, 4), 5, -3, g), w=dyadic((K, 208), 4, -5, g), scale=small_scale((K,), g), bias=dyadic((K,), 9, -9, g))


def f32_stem_ref(o, epilogue, abs_bound=False):
    """fp64 NHWC reference of the stem on f32_stem_operands: a 4-channel 7x7 stride-2 pad-3 conv over the first 196 weight columns"""
    a = (lambda t: t.abs()) if abs_bound else (lambda t: t)
    w = a(o["w"])[:, :196].contiguous()
    if not epilogue:
        return conv_fwd_ref(a(o["x"]), w, 7, 2, 3)
    return conv_fwd_ref(a(o["x"]), w, 7, 2, 3, o["scale"], a(o["bias"]), relu=not abs_bound)


def f32_stem_domain(o, epilogue):
    ref = f32_stem_ref(o, epilogue)
    assert_exact_domain(f32_stem_ref(o, epilogue, abs_bound=True), ref, F32_STEM_UNIT_EXP)
    return ref


def f32_ml_operands(C, K, k, seed=5):
    P = F32_ML_N * sum(h * w for h, w in F32_ML_LEVELS)
    bx, bw = f32_operand_bits(k * k * C)
    g = torch.Generator().manual_seed(seed)
    return dict(x=dyadic((P, C), bx, -3, g), w=dyadic((K, k * k * C), bw, -5, g), scale=small_scale((K,), g), bias=dyadic((K,), 12, -9, g),
                res=dyadic((P, K), 12, -6, g), acc0=dyadic_nonzero((P, K), 12, -7, g),
                dy=dyadic((P, K), 8, -4, g), xr=dyadic((P, C), 8, -3, g, relu_like=True),
                dw0=dyadic_nonzero((K, k * k * C), 12, -4, g), unit=-8)


def f32_wgrad_operands(name, seed=2):
    N, H, W, C, K, k, s, p = F32_WGRAD[name]
    g = torch.Generator().manual_seed(seed)
    OH, OW = _out_hw(H, W, k, s, p)
    return dict(x=dyadic((N, H, W, C), 8, -3, g, relu_like=True), dy=dyadic((N, OH, OW, K), 7, -4, g),
                dw0=dyadic_nonzero((K, k * k * C), 12, -4, g))


def colsum_operands(name, seed=6):
    M, C = COLSUM_CASES[name]
    g = torch.Generator().manual_seed(seed)
    return dyadic((M, C), 13, COLSUM_UNIT_EXP, g), dyadic_nonzero((C,), 12, COLSUM_UNIT_EXP + 2, g)


def colsum_domain(g2d, db0=None):
    ref = _v64(g2d).sum(0)
    bound = _v64(g2d).abs().sum(0)
    if db0 is not None:
        ref, bound = ref + _v64(db0), bound + _v64(db0).abs()
    assert_exact_domain(bound, ref, COLSUM_UNIT_EXP)
    return ref


def relu_clamps_some(pre64):
    """an epilogue case is not vacuous: the value before the ReLU is negative somewhere and positive somewhere"""
    return bool((pre64 < 0).any()) and bool((pre64 > 0).any())


# ----------------------------------------------------------------------------------------------------------------------------------
# grouped 3x3 conv (csrc/conv_grouped.hip).  A forward / dgrad thread owns one channel quad of GPX = 4 consecutive pixels of a row; a wgrad
# thread owns a 4 x 4 block of one tap over one split of the output pixels.
GPX = 4
# (g channels per group, G groups): (4, 3): C = 12, three channel quads (no power of two), every quad its own group; (8, 2): the second quad
# of a group has co % g != 0; (32, 2): eight trips of the inner channel loop
GCONV_GROUPS = [(4, 3), (8, 2), (32, 2)]
# (N, H, W): a single pixel; OW < GPX (3 at stride 1, 2 at stride 2); W = 4 = GPX with H odd; both sides even, W and OW multiples of 4;
# both sides odd and ragged (W = 9, OW = 5 at stride 2), three images
GCONV_SHAPES = [(1, 1, 1), (2, 2, 3), (2, 5, 4), (2, 6, 8), (3, 7, 9)]
# seeds of the forward and the dgrad operands where seed 0 does not give every 16-bit output of the case an exact tie and an inexact value
# in bf16 AND fp16 (test_exact_conv_ref.py asserts it for every case): (g, G, N, H, W, stride) -> (forward seed, dgrad seed)
GCONV_SEEDS = {
    (4, 3, 1, 1, 1, 1): (19, 17), (4, 3, 1, 1, 1, 2): (19, 17),       # 12 output elements
    (4, 3, 2, 2, 3, 2): (0, 1), (4, 3, 2, 5, 4, 2): (1, 0),
    (8, 2, 1, 1, 1, 1): (4, 0), (8, 2, 1, 1, 1, 2): (4, 0),
    (32, 2, 1, 1, 1, 1): (0, 8), (32, 2, 1, 1, 1, 2): (0, 8),
}
GCONV_CASES = {"g%d_G%d_%dx%dx%d_s%d" % (g, G, N, H, W, s): (g, G, N, H, W, s) + GCONV_SEEDS.get((g, G, N, H, W, s), (0, 0))
               for g, G in GCONV_GROUPS for N, H, W in GCONV_SHAPES for s in (1, 2)}
GCONV_UNIT_EXP = -9         # x 2^-3 * w 2^-5 * scale 2^-1 (forward and dgrad)
GCONV_WGRAD_UNIT_EXP = -8   # x 2^-3 * dy 2^-4 * scale 2^-1
GCONV_FWD_VARIANTS = {"plain": (False, False, False), "scale": (True, False, False), "shift": (False, True, False),
                      "scale_shift_relu": (True, True, True)}                    # name -> (scale, shift, relu)
GCONV_DGRAD_VARIANTS = {"plain": (False, False, False), "scale": (True, False, False), "scale_mask": (True, True, False),
                        "scale_mask_residual": (True, True, True)}               # name -> (scale, mask, residual)


def gconv_out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def gconv_wgrad_splits(N, OH, OW, C, G):
    """(splits, per_split) of utv2_gconv3x3_wgrad (conv_grouped.hip) restated"""
    g = C // G
    tpl = (C // 4) * 9 * (g // 4)
    M = N * OH * OW
    s = min(-(-262144 // tpl), (1 << 25) // (C * 9 * g), 256, (M + 31) // 32)
    s = max(s, 1)
    return s, -(-M // s)


def _gconv_bits(g):
    """(bits_x, bits_w): at most 7 (exact in bf16 and fp16); sums of 9 * g products with 12 .. 16 significant bits"""
    return {4: (6, 6), 8: (6, 5), 32: (5, 4)}[g]


def _mask_with_every_kind(shape, generator):
    """a ReLU-input stand-in: positive and negative integers (3 bits) with exact +0.0 and -0.0 planted: element 4 i + 1 is +0.0, 4 i + 3 is
    -0.0 for every other i; the first four elements are (+1, +0.0, -1, -0.0) so that the smallest tensor holds all four kinds"""
    m = dyadic(shape, 3, 0, generator, zero_frac=0.0).reshape(-1)
    m[m == 0] = 1.0
    m[1::8] = 0.0
    m[3::8] = -0.0
    m[0], m[2] = 1.0, -1.0
    return m.reshape(shape)


def gconv_fwd_operands(name):
    g, G, N, H, W, s, seed, _ = GCONV_CASES[name]
    C = g * G
    bx, bw = _gconv_bits(g)
    gen = torch.Generator().manual_seed(seed)
    return dict(x=dyadic((N, H, W, C), bx, -3, gen), w=dyadic((C, 9 * g), bw, -5, gen), scale=small_scale((C,), gen),
                shift=dyadic((C,), 9, GCONV_UNIT_EXP, gen))


def gconv_dgrad_operands(name):
    g, G, N, H, W, s, _, seed = GCONV_CASES[name]
    C = g * G
    bx, bw = _gconv_bits(g)
    OH, OW = gconv_out_hw(H, W, s)
    gen = torch.Generator().manual_seed(1000 + seed)
    return dict(dy=dyadic((N, OH, OW, C), bx, -3, gen), w=dyadic((C, 9 * g), bw, -5, gen), scale=small_scale((C,), gen),
                mask=_mask_with_every_kind((N, H, W, C), gen), res=dyadic((N, H, W, C), 7, GCONV_UNIT_EXP + 3, gen))


def gconv_wgrad_operands(name):
    g, G, N, H, W, s = GCONV_CASES[name][:6]
    C = g * G
    OH, OW = gconv_out_hw(H, W, s)
    gen = torch.Generator().manual_seed(2000)
    return dict(x=dyadic((N, H, W, C), 6, -3, gen), dy=dyadic((N, OH, OW, C), 6, -4, gen), scale=small_scale((C,), gen),
                dw0=dyadic_nonzero((C, 9 * g), 12, GCONV_WGRAD_UNIT_EXP + 2, gen))


def gconv_fwd_domain(name, o, variant):
    """fp64 reference relu?((acc * scale) + shift) of one forward variant, after assert_exact_domain; a ReLU variant clamps some elements"""
    g, G, N, H, W, s = GCONV_CASES[name][:6]
    use_sc, use_sh, relu = GCONV_FWD_VARIANTS[variant]
    sc, sh = (o["scale"] if use_sc else None), (o["shift"] if use_sh else None)
    ref = fwd_domain(o["x"], o["w"], 3, s, 1, GCONV_UNIT_EXP, sc, sh, None, relu, groups=G)
    if relu:
        assert relu_clamps_some(conv_fwd_ref(o["x"], o["w"], 3, s, 1, sc, sh, groups=G)), name
    return ref


def gconv_dgrad_domain(name, o, variant):
    """fp64 reference (mask > 0 ? sum of dy * (w * scale) : 0) + residual of one dgrad variant, after assert_exact_domain; a mask variant
    holds +0.0, -0.0, a negative and a positive value"""
    g, G, N, H, W, s = GCONV_CASES[name][:6]
    use_sc, use_mk, use_rs = GCONV_DGRAD_VARIANTS[variant]
    mk = o["mask"] if use_mk else None
    if use_mk:
        m = mk.reshape(-1)
        pz, nz = (m == 0) & ~torch.signbit(m), (m == 0) & torch.signbit(m)
        assert bool(pz.any()) and bool(nz.any()) and bool((m < 0).any()) and bool((m > 0).any()), name
    return dgrad_domain(o["dy"], o["w"], (N, H, W, g * G), 3, s, 1, GCONV_UNIT_EXP, mk, o["res"] if use_rs else None, None,
                        groups=G, scale=o["scale"] if use_sc else None)


def gconv_wgrad_domain(name, o, use_scale, accumulate):
    g, G, N, H, W, s = GCONV_CASES[name][:6]
    dw, _ = wgrad_domain(o["x"], o["dy"], 3, s, 1, GCONV_WGRAD_UNIT_EXP, o["scale"] if use_scale else None, o["dw0"] if accumulate else None,
                         None, GCONV_WGRAD_UNIT_EXP + 3, groups=G)
    return dw


def has_tie_and_inexact(ref64, h16):
    tie, inexact = tie_and_inexact_share(ref64, h16)
    return tie > 0 and inexact > 0
