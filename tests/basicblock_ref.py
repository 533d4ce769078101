"""Exact-arithmetic operands and the fp64 reference of one frozen identity BasicBlock (csrc/basicblock.hip), built on the method and the
helpers of tests/exact_conv_ref.py (plain module; used by test_basicblock_backbone.py on the CPU and test_basicblock_kernel_gpu.py).

    c1 = h16(relu(conv1(x) s1 + b1)),   y = h16(relu(conv2(c1) s2 + b2 + x))        both convs 3x3 pad 1, 64 -> 64

Grids: x integers 0 .. 7, weights in {-1, 0, 1} -> conv1's sums are integers; s1 in {8, 16, 24, 32, 48}, b1 integers -> c1 is an integer of
up to ~14 bits BEFORE its rounding (neither 16-bit type holds all of them: the rounding of c1 is live, and it is ONE rounding of an exact
value in any summation order) and an integer after it; s2 in {2^-12, 2^-11}, b2 on 2^-2 -> y on 2^-12, of the magnitude of x, so the
residual decides most outputs."""
import torch

from tests import exact_conv_ref as R

SHAPES = [(2, 9, 17), (1, 8, 16)]
C = 64
C1_UNIT_EXP = 0
Y_UNIT_EXP = -12


def basicblock_operands(shape, seed=11):
    N, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 8, (N, H, W, C), generator=g).to(torch.float32)
    return dict(x=x, w1=R.dyadic((C, 9 * C), 1, 0, g, zero_frac=0.5), w2=R.dyadic((C, 9 * C), 1, 0, g, zero_frac=0.5),
                s1=R.small_scale((C,), g, 4), b1=R.dyadic((C,), 8, 0, g),
                s2=R.pow2((C,), -12, -11, g), b2=R.dyadic((C,), 4, -2, g))


def basicblock_ref(x, w1, w2, s1, b1, s2, b2, h16, abs_bound=False, residual=True):
    """fp64 (y, c1) NHWC with c1 rounded once to h16; abs_bound: no rounding (absolute operands: the bound of assert_exact_domain);
    residual=False: the same expression without `+ x`"""
    c1 = R.conv_fwd_ref(x, w1, 3, 1, 1, s1, b1, relu=True)
    if not abs_bound:
        c1 = R.r16(c1, h16)
    y = R.conv_fwd_ref(c1, w2, 3, 1, 1, s2, b2, residual=x if residual else None, relu=True)
    return y, c1


def basicblock_domain(o, h16):
    """(y, c1, y without the residual) fp64 after the preconditions: every stage inside the exact domain, both ReLUs live (at least 10 % of
    c1 and of y zero, at least 10 % positive), the residual decisive (y differs from the expression without `+ x` in more than half of its
    elements, after the rounding to h16)"""
    keys = ("x", "w1", "w2", "s1", "b1", "s2", "b2")
    y, c1 = basicblock_ref(*[o[k] for k in keys], h16)
    y0, _ = basicblock_ref(*[o[k] for k in keys], h16, residual=False)
    ab = {k: v.abs() for k, v in o.items()}
    by, bc1 = basicblock_ref(*[ab[k] for k in keys], h16, abs_bound=True)
    R.assert_on_grid(o["b1"], C1_UNIT_EXP, "b1")
    R.assert_exact_domain(bc1, R.conv_fwd_ref(o["x"], o["w1"], 3, 1, 1, o["s1"], o["b1"], relu=True), C1_UNIT_EXP)
    for k in ("b2", "x"):
        R.assert_on_grid(o[k], Y_UNIT_EXP, k)
    R.assert_exact_domain(by * (1 + 2.0 ** -8), y, Y_UNIT_EXP)     # rounding c1 to h16 can raise it by half an ulp
    for t, n in ((c1, "c1"), (y, "y")):
        assert float((t == 0).double().mean()) >= 0.1 and float((t > 0).double().mean()) >= 0.1, n
    a, b = R.to_out(y, h16), R.to_out(y0, h16)
    assert float((a != b).double().mean()) > 0.5
    return y, c1, y0
