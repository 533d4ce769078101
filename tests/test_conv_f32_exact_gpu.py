"""The fp32 implicit-GEMM convs (csrc/conv.hip: conv_igemm_f32<BN, MODE, ML>, conv_wgrad_f32<VEC, ML>, reduce_slabs_f32, both colsum kernels,
weight_flip_transpose_f32) on operands for which fp32 accumulation is EXACT (tests/exact_conv_ref.py): every fp32 output equals the fp64
reference bit for bit and the stem's 16-bit output equals one round-to-nearest-even of it.  No tolerance and no row subsets: one dropped,
duplicated or misplaced term, an epilogue step out of order or an ignored `accumulate` fails torch.equal.  The shapes are the smallest that
reach each template instance and each epilogue; the rule that selects each one stands beside its table in exact_conv_ref.py.  Not reached:
the block-row doubling of the vector colsum route (M > 262144 rows)."""
import pytest
import torch

from tests import exact_conv_ref as R

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture(params=["bf16", "fp16"])
def h16(request):
    from ubteacher import hip
    hip.set_h16(request.param)
    try:
        yield hip.h16_dtype()
    finally:
        hip.set_h16("bf16")


def _eq(got, ref64, dt=F32):
    """the whole tensor equals the exact value (fp32) / its single rounding (16-bit)"""
    g = got.cpu()
    want = R.to_out(ref64, dt).view(g.shape)
    same = torch.equal(g, want)
    if not same:       # what differs, for the log
        bad = (g.float() != want.float()).nonzero()
        print("mismatch: %d of %d elements, first at %s: got %r want %r" % (len(bad), g.numel(), bad[0].tolist(),
              float(g[tuple(bad[0])]), float(want[tuple(bad[0])])))
    return same


# -------------------------------------------------------------------------------------------------------------------------------
# forward: every (tile width, gather mode, epilogue) x every geometry x {plain, epilogue} x {store, accumulate}
@pytest.mark.parametrize("geom", R.F32_GEOMS, ids=lambda g: "n%d_%dx%d_k%d_s%d_p%d" % g)
@pytest.mark.parametrize("name", list(R.F32_CASES))
def test_forward_is_exact(name, geom):
    from ubteacher import hip
    C, K = R.F32_CASES[name]
    N, H, W, k, s, p = geom
    o = R.f32_fwd_operands(C, K, geom)
    u = o["unit"]
    kw = dict(stride=s, pad=p, kh=k, kw=k)
    x, w = o["x"].cuda(), o["w"].cuda()
    ref = R.fwd_domain(o["x"], o["w"], k, s, p, u)
    assert _eq(hip.conv2d_fwd(x, w, **kw), ref), "plain"
    epi = (o["scale"], o["bias"], o["res"])
    ref = R.fwd_domain(o["x"], o["w"], k, s, p, u - 1, *epi, True)
    assert R.relu_clamps_some(R.conv_fwd_ref(o["x"], o["w"], k, s, p, *epi))
    assert _eq(hip.conv2d_fwd(x, w, o["scale"].cuda(), o["bias"].cuda(), o["res"].cuda(), relu=True, **kw), ref), "scale + bias + residual + relu"
    # accumulate onto a non-zero output: the earlier content is added after the epilogue (after the ReLU)
    ref = R.fwd_domain(o["x"], o["w"], k, s, p, u, acc0=o["acc0"])
    assert _eq(hip.conv2d_fwd(x, w, out=o["acc0"].cuda(), accumulate=True, **kw), ref), "accumulate"
    ref = R.fwd_domain(o["x"], o["w"], k, s, p, u - 1, *epi, True, acc0=o["acc0"])
    assert not torch.equal(ref, torch.relu(ref))          # the addend is outside the ReLU
    y = hip.conv2d_fwd(x, w, o["scale"].cuda(), o["bias"].cuda(), o["res"].cuda(), relu=True, out=o["acc0"].cuda(), accumulate=True, **kw)
    assert _eq(y, ref), "epilogue + accumulate"


# -------------------------------------------------------------------------------------------------------------------------------
# dgrad: the same kernels over dY with the flipped / transposed weight image and the input-dilation predicate
@pytest.mark.parametrize("name", list(R.F32_DGRAD))
def test_dgrad_is_exact(name):
    from ubteacher import hip
    N, H, W, C, K, k, s, p = R.F32_DGRAD[name]
    o = R.f32_dgrad_operands(name)
    wt = hip.weight_flip_transpose(o["w"].cuda(), K, k, k, C)
    assert torch.equal(wt.cpu(), R.flip_transpose_ref(o["w"], K, k, C))
    ref = R.dgrad_domain(o["dy"], o["w"], (N, H, W, C), k, s, p, o["unit"])
    assert float(ref.abs().max()) > 0
    assert _eq(hip.conv2d_dgrad(o["dy"].cuda(), wt, (N, H, W, C), s, p, k, k), ref), "store"
    ref = R.dgrad_domain(o["dy"], o["w"], (N, H, W, C), k, s, p, o["unit"], acc0=o["acc0"])
    assert _eq(hip.conv2d_dgrad(o["dy"].cuda(), wt, (N, H, W, C), s, p, k, k, out=o["acc0"].cuda(), accumulate=True), ref), "accumulate"


@pytest.mark.parametrize("K,k,C", R.F32_FLIP)
def test_weight_flip_transpose_is_exact(K, k, C):
    from ubteacher import hip
    w = torch.arange(K * k * k * C, dtype=F32).view(K, k * k * C) + 1.0      # every element its own value
    assert torch.equal(hip.weight_flip_transpose(w.cuda(), K, k, k, C).cpu(), R.flip_transpose_ref(w, K, k, C))


# -------------------------------------------------------------------------------------------------------------------------------
# the image stem: MODE 1, fp32 and 16-bit output on both builds
@pytest.mark.parametrize("image", R.F32_STEM_IMAGES, ids=lambda i: "n%d_%dx%d" % i)
@pytest.mark.parametrize("K", R.F32_STEM_K)
def test_stem_is_exact(K, image, h16):
    from ubteacher import hip
    o = R.f32_stem_operands(K, image)
    x, w = o["x"].cuda(), o["w"].cuda()
    ref0, ref1 = R.f32_stem_domain(o, False), R.f32_stem_domain(o, True)
    assert R.relu_clamps_some(R.conv_fwd_ref(o["x"], o["w"][:, :196].contiguous(), 7, 2, 3, o["scale"], o["bias"]))
    for dt in (F32, h16):
        if dt != F32:
            assert R.has_tie_and_inexact(ref0, dt) and R.has_tie_and_inexact(ref1, dt)
        y0 = hip.conv2d_stem_fwd(x, w, None, None, 2, 3, 7, 7, False, dt)
        assert y0.dtype == dt and _eq(y0, ref0, dt), (dt, "plain")
        y1 = hip.conv2d_stem_fwd(x, w, o["scale"].cuda(), o["bias"].cuda(), 2, 3, 7, 7, True, dt)
        assert _eq(y1, ref1, dt), (dt, "scale + bias + relu")


# -------------------------------------------------------------------------------------------------------------------------------
# multi-level convs: one launch over all levels and images
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", list(R.F32_ML))
def test_multi_level_forward_dgrad_and_wgrad_are_exact(name, k):
    from ubteacher import hip
    C, K = R.F32_ML[name]
    lv, N, pad = R.F32_ML_LEVELS, R.F32_ML_N, k // 2
    o = R.f32_ml_operands(C, K, k)
    u = o["unit"]
    x, w = o["x"].cuda(), o["w"].cuda()
    assert _eq(hip.conv2d_ml_fwd(x, w, lv, N, k=k, pad=pad), R.ml_fwd_domain(o["x"], o["w"], lv, N, k, pad, u)), "plain"
    epi = (o["scale"], o["bias"], o["res"])
    assert R.relu_clamps_some(R.ml_fwd_ref(o["x"], o["w"], lv, N, k, pad, *epi))
    ref = R.ml_fwd_domain(o["x"], o["w"], lv, N, k, pad, u - 1, *epi, True)
    assert _eq(hip.conv2d_ml_fwd(x, w, lv, N, o["scale"].cuda(), o["bias"].cuda(), o["res"].cuda(), k=k, pad=pad, relu=True), ref), "epilogue"
    ref = R.ml_fwd_domain(o["x"], o["w"], lv, N, k, pad, u - 1, *epi, True, acc0=o["acc0"])
    y = hip.conv2d_ml_fwd(x, w, lv, N, o["scale"].cuda(), o["bias"].cuda(), o["res"].cuda(), k=k, pad=pad, relu=True, out=o["acc0"].cuda(),
                          accumulate=True)
    assert _eq(y, ref), "epilogue + accumulate"
    # dgrad: utv2_conv2d_ml_fwd needs the reduction channels to be a multiple of 16, so the layer whose dgrad runs here is the transposed
    # one: forward C_f = K -> K_f = C, its dY has C columns (reduction k*k*C), its dX has K
    wf = o["w"].view(K, k, k, C).permute(3, 1, 2, 0).reshape(C, k * k * K).contiguous()
    wt = hip.weight_flip_transpose(wf.cuda(), C, k, k, K)
    ref = R.ml_dgrad_domain(o["x"], wf, lv, N, k, pad, K, u)
    assert _eq(hip.conv2d_ml_dgrad(x, wt, lv, N, k, pad), ref), "dgrad"
    # wgrad: accumulate off, then onto a non-zero dyadic gradient
    xr, dy = o["xr"], o["dy"]
    dw = torch.full((K, k * k * C), 3.0, device="cuda")
    hip.conv2d_ml_wgrad(xr.cuda(), dy.cuda(), dw, lv, N, k, pad, accumulate=False)
    assert _eq(dw, R.ml_wgrad_domain(xr, dy, lv, N, k, pad, R.F32_WGRAD_UNIT_EXP, db_unit_exp=R.F32_WGRAD_DB_UNIT_EXP)[0]), "wgrad"
    dw = o["dw0"].cuda()
    hip.conv2d_ml_wgrad(xr.cuda(), dy.cuda(), dw, lv, N, k, pad, accumulate=True)
    ref = R.ml_wgrad_domain(xr, dy, lv, N, k, pad, R.F32_WGRAD_UNIT_EXP, None, o["dw0"], None, R.F32_WGRAD_DB_UNIT_EXP)[0]
    assert _eq(dw, ref), "wgrad + accumulate"


# -------------------------------------------------------------------------------------------------------------------------------
# weight gradients: two pixel splits, the last chunk partial
@pytest.mark.parametrize("name", list(R.F32_WGRAD))
def test_wgrad_is_exact(name):
    from ubteacher import hip
    N, H, W, C, K, k, s, p = R.F32_WGRAD[name]
    o = R.f32_wgrad_operands(name)
    OH, OW = o["dy"].shape[1:3]
    M = N * OH * OW
    splits = hip.load().utv2_conv2d_wgrad_splits(N, OH, OW, K, k * k * C)
    assert splits >= 2 and M % 16 != 0 and (-(-M // 16)) % splits != 0, (splits, M)      # >= 2 splits, a partial last chunk, uneven splits
    x, dy = o["x"].cuda(), o["dy"].cuda()
    dw = torch.full((K, k * k * C), 3.0, device="cuda")
    hip.conv2d_wgrad(x, dy, dw, s, p, k, k, accumulate=False)
    ref = R.wgrad_domain(o["x"], o["dy"], k, s, p, R.F32_WGRAD_UNIT_EXP, db_unit_exp=R.F32_WGRAD_DB_UNIT_EXP)[0]
    assert float(ref.abs().max()) > 0 and _eq(dw, ref), "store"
    dw = o["dw0"].cuda()
    hip.conv2d_wgrad(x, dy, dw, s, p, k, k, accumulate=True)
    ref = R.wgrad_domain(o["x"], o["dy"], k, s, p, R.F32_WGRAD_UNIT_EXP, None, o["dw0"], None, R.F32_WGRAD_DB_UNIT_EXP)[0]
    assert _eq(dw, ref), "accumulate"


# -------------------------------------------------------------------------------------------------------------------------------
# column sums
@pytest.mark.parametrize("name", list(R.COLSUM_CASES))
def test_colsum_is_exact(name):
    from ubteacher import hip
    M, C = R.COLSUM_CASES[name]
    g2d, db0 = R.colsum_operands(name)
    db = torch.full((C,), 3.0, device="cuda")
    hip.colsum(g2d.cuda(), db, accumulate=False)
    assert _eq(db, R.colsum_domain(g2d)), "store"
    db = db0.cuda()
    hip.colsum(g2d.cuda(), db, accumulate=True)
    assert _eq(db, R.colsum_domain(g2d, db0)), "accumulate"
