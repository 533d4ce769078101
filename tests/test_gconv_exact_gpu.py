"""The grouped 3x3 conv kernels (csrc/conv_grouped.hip: forward, dgrad, split-pixel wgrad and its reduce) on operands for which fp32
accumulation is EXACT (tests/exact_conv_ref.py), with fp32 operands and with 16-bit operands in both builds of the library: an fp32 output
equals the fp64 reference of torch's grouped conv bit for bit, a 16-bit output equals ONE round-to-nearest-even of it.  No tolerance, whole
tensors.  The shapes reach a single pixel, OW < GPX, widths that are and are not multiples of the 4-pixel thread tile, even sides at stride 2,
a channel-quad count that is no power of two and wgrad splits that begin mid-row and mid-image."""
import pytest
import torch

from tests import exact_conv_ref as R

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture(params=["fp32", "bf16", "fp16"])
def op_dtype(request):
    """element type of the operands: fp32, or the 16-bit type of either build"""
    from ubteacher import hip
    hip.set_h16("fp16" if request.param == "fp16" else "bf16")
    try:
        yield F32 if request.param == "fp32" else hip.h16_dtype()
    finally:
        hip.set_h16("bf16")


def _eq(got, ref64, dt):
    g = got.cpu()
    want = R.to_out(ref64, dt).view(g.shape)
    same = torch.equal(g, want)
    if not same:       # what differs, for the log
        bad = (g.float() != want.float()).nonzero()
        print("mismatch: %d of %d elements, first at %s: got %r want %r" % (len(bad), g.numel(), bad[0].tolist(),
              float(g[tuple(bad[0])]), float(want[tuple(bad[0])])))
    return same


def _dev(t, dt):
    d = t.cuda().to(dt)
    assert torch.equal(d.float().cpu(), t)          # the operand is exact in its element type (signed zeros compare equal)
    return d


@pytest.mark.parametrize("name", list(R.GCONV_CASES))
def test_forward_is_exact(name, op_dtype):
    from ubteacher import hip
    g, G, N, H, W, s = R.GCONV_CASES[name][:6]
    o = R.gconv_fwd_operands(name)
    x, w = _dev(o["x"], op_dtype), _dev(o["w"], op_dtype)
    for variant, (use_sc, use_sh, relu) in R.GCONV_FWD_VARIANTS.items():
        ref = R.gconv_fwd_domain(name, o, variant)
        for dt in {F32, op_dtype}:
            if dt != F32:
                assert R.has_tie_and_inexact(ref, dt), (variant, dt)
            y = hip.gconv3x3_fwd(x, w, G, s, o["scale"].cuda() if use_sc else None, o["shift"].cuda() if use_sh else None, relu=relu,
                                 out_dtype=dt)
            assert y.dtype == dt and _eq(y, ref, dt), (variant, dt)


@pytest.mark.parametrize("name", list(R.GCONV_CASES))
def test_dgrad_is_exact(name, op_dtype):
    from ubteacher import hip
    g, G, N, H, W, s = R.GCONV_CASES[name][:6]
    o = R.gconv_dgrad_operands(name)
    dy, w = _dev(o["dy"], op_dtype), _dev(o["w"], op_dtype)
    for variant, (use_sc, use_mk, use_rs) in R.GCONV_DGRAD_VARIANTS.items():
        ref = R.gconv_dgrad_domain(name, o, variant)
        for dt in {F32, op_dtype}:
            if dt != F32:
                assert R.has_tie_and_inexact(ref, dt), (variant, dt)
            mk = _dev(o["mask"], dt) if use_mk else None
            if use_mk:       # +0.0, -0.0 and the negative values arrive as such, and all of them zero the gradient
                m = mk.cpu().float().reshape(-1)
                assert bool(((m == 0) & torch.signbit(m)).any()) and bool(((m == 0) & ~torch.signbit(m)).any()) and bool((m < 0).any())
                if not use_rs:
                    assert bool((ref.reshape(-1)[m <= 0] == 0).all()) and bool((ref.reshape(-1)[m > 0] != 0).any())
            dx = hip.gconv3x3_dgrad(dy, w, G, s, (N, H, W, g * G), scale=o["scale"].cuda() if use_sc else None, mask=mk,
                                    residual=_dev(o["res"], dt) if use_rs else None, out_dtype=dt)
            assert dx.dtype == dt and _eq(dx, ref, dt), (variant, dt)


@pytest.mark.parametrize("name", list(R.GCONV_CASES))
def test_wgrad_is_exact_and_deterministic(name, op_dtype):
    from ubteacher import hip
    g, G, N, H, W, s = R.GCONV_CASES[name][:6]
    C = g * G
    OH, OW = R.gconv_out_hw(H, W, s)
    if (N, H, W) == (3, 7, 9):
        splits = hip.load().utv2_gconv3x3_wgrad_splits(N, OH, OW, C, G)
        per_split = -(-N * OH * OW // splits)
        assert splits >= 2 and OW % per_split != 0 and (OH * OW) % per_split != 0
        if s == 1:      # 6 splits of 32 pixels: they begin mid-row and mid-image
            assert per_split % OW != 0 and per_split % (OH * OW) != 0
        else:           # 60 pixels in 2 splits of 30 = 6 rows of 5: the second split begins mid-image (an image is 4 rows)
            assert per_split % (OH * OW) != 0
    o = R.gconv_wgrad_operands(name)
    x, dy = _dev(o["x"], op_dtype), _dev(o["dy"], op_dtype)
    for use_sc in (False, True):
        sc = o["scale"].cuda() if use_sc else None
        runs = []
        for _ in range(2):
            dw = torch.full((C, 9 * g), 3.0, device="cuda")
            hip.gconv3x3_wgrad(x, dy, dw, G, s, scale=sc, accumulate=False)
            runs.append(dw.cpu())
        assert torch.equal(runs[0], runs[1])                     # fixed split order, no atomics
        assert _eq(runs[0], R.gconv_wgrad_domain(name, o, use_sc, False), F32), ("store", use_sc)
        dw = o["dw0"].cuda()
        hip.gconv3x3_wgrad(x, dy, dw, G, s, scale=sc, accumulate=True)
        assert _eq(dw, R.gconv_wgrad_domain(name, o, use_sc, True), F32), ("accumulate", use_sc)
