"""CPU self-test of tests/exact_conv_ref.py: the operands of every route of test_conv_exact_gpu.py are inside the exact domain, fp32
accumulation of them is order independent, the 16-bit expectations exercise the rounding, and the fp64 reference itself meets the Gaussian
criteria of the fp16 leg."""
import pytest
import torch
import torch.nn.functional as F

from tests import exact_conv_ref as R

H16S = [torch.bfloat16, torch.float16]


def _out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def _fwd_case_ref(name):
    """the epilogue-case reference of one NHWC route (whole tensor, or the stratified rows of the M > 30000 cases)"""
    N, H, W, C, K, k, s, p, _, _, _ = R.NHWC_CASES[name]
    x, w2, u = R.nhwc_operands(name)
    OH, OW = _out_hw(H, W, k, s, p)
    M = N * OH * OW
    sc, bi, res = R.epilogue_operands(K, (M, K), u, 1)
    rows = R.subset_rows(M, 256) if name in R.BIG_M else torch.arange(M)
    plain = R.rows_domain(x, w2, k, s, p, rows, u)
    return R.rows_domain(x, w2, k, s, p, rows, u - 1, sc, bi, res, True), plain


@pytest.mark.parametrize("name", sorted(R.NHWC_CASES))
def test_nhwc_route_operands_are_inside_the_exact_domain(name):
    ref, plain = _fwd_case_ref(name)
    assert float(plain.abs().max()) > 0
    for h16 in H16S:
        tie, inexact = R.tie_and_inexact_share(ref, h16)
        assert tie > 0.01 and inexact > 0.01, (h16, tie, inexact)      # the rounding test is not vacuous


def test_every_big_m_case_is_named():
    for name, c in R.NHWC_CASES.items():
        N, H, W, C, K, k, s, p = c[:8]
        OH, OW = _out_hw(H, W, k, s, p)
        assert (N * OH * OW > 30000) == (name in R.BIG_M), name


def test_dilated_dgrad_and_wide_operands_are_inside_the_exact_domain():
    N, H, W, C, K, k, s, p = R.DGRAD_DILATED
    g = torch.Generator().manual_seed(4)
    OH, OW = _out_hw(H, W, k, s, p)
    dy = R.dyadic((N, OH, OW, K), 3, -3, g)
    w2 = R.dyadic((K, k * k * C), 3, -5, g)
    R.dgrad_domain(dy, w2, (N, H, W, C), k, s, p, -8)
    # the dgrad reference is the gradient autograd computes
    x = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, R._w64(w2, k, C), None, s, p).backward(R._x64(dy))
    assert torch.equal(x.grad.permute(0, 2, 3, 1), R.conv_dgrad_ref(dy, w2, (N, H, W, C), k, s, p))
    # fp32 x with 12 .. 16 significant bits, rounded on load
    N, H, W, C, K, k, s, p = R.NHWC_CASES["generic128"][:8]
    xw = R.dyadic_wide((N, H, W, C), -14, g)
    f = xw[xw != 0].abs().view(torch.int32)
    sig = 24 - (f & -f).float().log2().round() + 0    # 24 - trailing zeros of the mantissa pattern (the implicit bit included)
    assert float(sig.min()) >= 12 and float(sig.max()) <= 16
    wq = R.dyadic((K, k * k * C), 3, -5, g)
    for h16 in H16S:
        xr = xw.to(h16).float()
        assert not torch.equal(xr, xw)
        R.fwd_domain(xr, wq, k, s, p, R.wide_unit_exp(-14, h16) - 5)


@pytest.mark.parametrize("name", sorted(R.ML_CASES))
def test_multi_level_route_operands_are_inside_the_exact_domain(name):
    level_hw, N, C, K, bx, bw = R.ML_CASES[name]
    g = torch.Generator().manual_seed(5)
    P = N * sum(h * w for h, w in level_hw)
    x = R.dyadic((P, C), bx, -3, g)
    w2 = R.dyadic((K, 9 * C), bw, -5, g)
    sc, bi, res = R.epilogue_operands(K, (P, K), -8, 2)
    ref = R.ml_fwd_domain(x, w2, level_hw, N, 3, 1, -9, sc, bi, res, True)
    assert tuple(ref.shape) == (P, K)


@pytest.mark.parametrize("name", sorted(R.WGRAD_128) + sorted(R.WGRAD_PP))
def test_wgrad_operands_are_inside_the_exact_domain(name):
    N, H, W, C, K, k, s, p = {**R.WGRAD_128, **R.WGRAD_PP}[name]
    x, dy, rs, dw0, db0 = R.wgrad_operands(N, H, W, C, K, k, s, p)
    R.wgrad_domain(x, dy, k, s, p, R.WGRAD_UNIT_EXP, rs, dw0, db0, R.WGRAD_DB_UNIT_EXP)


def test_wgrad_tower_operands_are_inside_the_exact_domain():
    level_hw, N, C, K = R.WGRAD_PP_TOWER
    x, dy, rs, dw0, db0 = R.wgrad_ml_operands(level_hw, N, C, K)
    R.ml_wgrad_domain(x, dy, level_hw, N, 3, 1, R.WGRAD_UNIT_EXP, rs, dw0, db0, R.WGRAD_DB_UNIT_EXP)


@pytest.mark.parametrize("h16", H16S)
@pytest.mark.parametrize("shortcut", [False, True])
@pytest.mark.parametrize("shape", R.BOTTLENECK_SHAPES)
def test_bottleneck_chain_is_inside_the_exact_domain(shape, shortcut, h16):
    o = R.bottleneck_operands(shape, shortcut)
    y, c1, c2, sc = R.bottleneck_domain(o, h16)
    assert float(y.max()) > 0 and float(c1.max()) > 0 and float(c2.max()) > 0
    assert float(y.max()) < 60000 and float(c2.max()) < 60000       # nothing overflows fp16 at a 16-bit store


@pytest.mark.parametrize("h16", H16S)
@pytest.mark.parametrize("hw", R.STEM_CANVASES + R.STEM_POOL_HW)
def test_stem_operands_are_inside_the_exact_domain(hw, h16):
    H, W = hw
    ims = R.stem_images(hw, 2)
    x = torch.stack([(im - 128.0) / 64.0 for im in ims]).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(x.to(h16).float(), x)
    w208, sc, sh = R.stem_weights()
    w2 = R.stem_taps(w208)
    assert torch.equal(w2.to(h16).float(), w2)
    ref = R.stem_ref(x, w2, sc, sh)
    bound = R.conv_fwd_ref(x.abs(), w2.abs(), 7, 2, 3, sc, sh.abs())
    R.assert_exact_domain(bound, ref, R.STEM_UNIT_EXP)
    tie, inexact = R.tie_and_inexact_share(ref, h16)
    assert inexact > 0.01, (tie, inexact)


@pytest.mark.parametrize("name", ["v2_64_bk32", "v2_128_bk32"])
def test_fp32_accumulation_is_order_independent_inside_the_domain(name):
    """an fp32 CPU conv equals the fp64 reference bit for bit, and so does the same conv with the reduction axis permuted"""
    N, H, W, C, K, k, s, p = R.NHWC_CASES[name][:8]
    x, w2, u = R.nhwc_operands(name)
    ref = R.fwd_domain(x, w2, k, s, p, u)
    xc = x.permute(0, 3, 1, 2).contiguous()
    wc = w2.view(K, k, k, C).permute(0, 3, 1, 2).contiguous()
    y32 = F.conv2d(xc, wc, None, s, p).permute(0, 2, 3, 1)
    assert y32.dtype == torch.float32 and torch.equal(y32.double(), ref)
    perm = torch.randperm(C, generator=torch.Generator().manual_seed(1))
    y32p = F.conv2d(xc[:, perm].contiguous(), wc[:, perm].flip(0).contiguous(), None, s, p).permute(0, 2, 3, 1).flip(3)
    assert torch.equal(y32p.double(), ref)
    # the im2col GEMM in another order again (taps outermost), accumulated tap by tap in fp32
    rows = torch.arange(ref.shape[0] * ref.shape[1] * ref.shape[2])
    xp = F.pad(x, (0, 0, p, p, p, p))
    OH, OW = ref.shape[1:3]
    n, oh, ow = rows // (OH * OW), (rows // OW) % OH, rows % OW
    acc = torch.zeros(rows.numel(), K)
    for t in reversed(range(k * k)):
        acc += xp[n, oh * s + t // k, ow * s + t % k] @ w2[:, t * C:(t + 1) * C].t()
    assert torch.equal(acc.double().view(ref.shape), ref)
    assert torch.equal(R.conv_rows_ref(x, w2, k, s, p, rows).view(ref.shape), ref)


def test_to_out_rejects_a_value_that_fp32_cannot_hold():
    with pytest.raises(AssertionError):
        R.to_out(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64), torch.float16)
    with pytest.raises(AssertionError):
        R.assert_exact_domain(torch.tensor([2.0 ** 24], dtype=torch.float64), torch.tensor([1.0], dtype=torch.float64), 0)


def test_tie_share_counts_exact_ties_only():
    v = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -9, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8)], dtype=torch.float64)
    tie, inexact = R.tie_and_inexact_share(v, torch.bfloat16)      # bf16 spacing at 1 is 2^-7: 2^-8 is a tie, 2^-9 is not
    assert (tie, inexact) == (3 / 5, 4 / 5)


@pytest.mark.parametrize("name", sorted(set(R.NHWC_CASES) - set(R.BIG_M)))
def test_fp64_reference_rounded_to_fp16_meets_the_gaussian_criteria(name):
    """section D's criteria hold for the reference itself: an fp16 output that is one rounding of the fp64 value passes close16 with
    2^-11, and an fp32 one passes relerr < 2e-4"""
    x, w2, b, res = R.gaussian_operands(name)
    N, H, W, C, K, k, s, p = R.NHWC_CASES[name][:8]
    ref = R.conv_fwd_ref(x, w2, k, s, p, None, b, res, True)
    assert R.close16(ref.to(torch.float16), ref, 2.0 ** -11)
    assert R.relerr(ref.float(), ref) < 2e-4


def test_multi_level_64_wide_case_gets_no_geometry_table():
    """the 64-wide multi-level tile is reached only by a `plain` call (ml_fwd_g): the wrapper builds a geometry table - which makes the
    call not plain - when K % 4 == 0 and the output pitch K is a multiple of 8; the ml64 case must not meet that, its neighbour must"""
    K64, K40 = R.ML_CASES["ml64"][3], R.ML_CASES["ml128_k40"][3]
    assert K64 <= 64 and K64 % 4 == 0 and K64 % 8 != 0
    assert K40 <= 64 and K40 % 8 == 0


@pytest.mark.parametrize("name", ["ml64", "ml128", "n96_72_ragged"])
def test_fp64_multi_level_reference_rounded_to_fp16_meets_the_gaussian_criteria(name):
    level_hw, N, C, K = R.ML_CASES[name][:4]
    x, w2, b, res = R.gaussian_ml_operands(name)
    ref = R.ml_fwd_ref(x, w2, level_hw, N, 3, 1, None, b, res, True)
    assert R.close16(ref.to(torch.float16), ref, 2.0 ** -11) and R.relerr(ref.float(), ref) < 2e-4


# ----------------------------------------------------------------------------------------------------------------------------------
# the fp32 implicit-GEMM and grouped-conv tables (test_conv_f32_exact_gpu.py, test_gconv_exact_gpu.py)
@pytest.mark.parametrize("name", sorted(R.F32_CASES))
def test_f32_forward_cases_are_inside_the_exact_domain_and_obey_their_dispatch_rules(name):
    C, K = R.F32_CASES[name]
    assert ("bn64" in name) == (K <= 64) and ("m0" in name) == (C % 16 == 0) and ("scalar" in name) == (K % 4 != 0)
    for geom in R.F32_GEOMS:
        N, H, W, k, s, p = geom
        o = R.f32_fwd_operands(C, K, geom)
        epi = (o["scale"], o["bias"], o["res"])
        assert float(R.fwd_domain(o["x"], o["w"], k, s, p, o["unit"]).abs().max()) > 0
        R.fwd_domain(o["x"], o["w"], k, s, p, o["unit"], acc0=o["acc0"])
        R.fwd_domain(o["x"], o["w"], k, s, p, o["unit"] - 1, *epi, True)
        ref = R.fwd_domain(o["x"], o["w"], k, s, p, o["unit"] - 1, *epi, True, acc0=o["acc0"])
        assert R.relu_clamps_some(R.conv_fwd_ref(o["x"], o["w"], k, s, p, *epi)) and bool((o["acc0"] != 0).all())
        assert not torch.equal(ref, torch.relu(ref))


def test_f32_geometries_cover_both_row_tile_cases():
    Ms = {g: g[0] * R._out_hw(g[1], g[2], g[3], g[4], g[5])[0] * R._out_hw(g[1], g[2], g[3], g[4], g[5])[1] for g in R.F32_GEOMS}
    assert Ms[(2, 9, 7, 3, 1, 1)] == 126 and Ms[(2, 9, 8, 3, 1, 1)] == 144
    assert {(g[3], g[4]) for g in R.F32_GEOMS} == {(3, 1), (3, 2), (1, 1), (1, 2)}
    assert all(b * 6 * (2 ** a[0] - 1) * (2 ** a[1] - 1) < 2 ** 23 for b in (12, 16, 20, 32, 108, 288) for a in [R.f32_operand_bits(b)])


@pytest.mark.parametrize("name", sorted(R.F32_DGRAD))
def test_f32_dgrad_cases_are_inside_the_exact_domain_and_obey_their_dispatch_rules(name):
    N, H, W, C, K, k, s, p = R.F32_DGRAD[name]
    assert ("m0" in name) == (K % 16 == 0) and ("scalar" in name) == (C % 4 != 0) and ("s2" in name) == (s == 2) and ("bn128" in name) == (C > 64)
    o = R.f32_dgrad_operands(name)
    R.dgrad_domain(o["dy"], o["w"], (N, H, W, C), k, s, p, o["unit"])
    ref = R.dgrad_domain(o["dy"], o["w"], (N, H, W, C), k, s, p, o["unit"], acc0=o["acc0"])
    # the reference is the gradient autograd computes
    x = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, R._w64(o["w"], k, C), None, s, p).backward(R._x64(o["dy"]))
    assert torch.equal(x.grad.permute(0, 2, 3, 1) + o["acc0"].double(), ref)


@pytest.mark.parametrize("h16", H16S)
@pytest.mark.parametrize("image", R.F32_STEM_IMAGES)
@pytest.mark.parametrize("K", R.F32_STEM_K)
def test_f32_stem_cases_are_inside_the_exact_domain_and_exercise_the_rounding(K, image, h16):
    o = R.f32_stem_operands(K, image)
    assert K % 4 == 0 and o["w"].shape[1] == 208 and bool((o["w"][:, 196:] != 0).any()) and bool((o["x"][..., 3] != 0).any())
    for epilogue in (False, True):
        assert R.has_tie_and_inexact(R.f32_stem_domain(o, epilogue), h16), (K, image, h16, epilogue)
    assert R.relu_clamps_some(R.conv_fwd_ref(o["x"], o["w"][:, :196].contiguous(), 7, 2, 3, o["scale"], o["bias"]))


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", sorted(R.F32_ML))
def test_f32_multi_level_cases_are_inside_the_exact_domain(name, k):
    C, K = R.F32_ML[name]
    assert C % 16 == 0 and K % 4 == 0 and (name == "ml64") == (K <= 64)
    lv, N, pad = R.F32_ML_LEVELS, R.F32_ML_N, k // 2
    o = R.f32_ml_operands(C, K, k)
    epi = (o["scale"], o["bias"], o["res"])
    R.ml_fwd_domain(o["x"], o["w"], lv, N, k, pad, o["unit"])
    R.ml_fwd_domain(o["x"], o["w"], lv, N, k, pad, o["unit"] - 1, *epi, True, acc0=o["acc0"])
    assert R.relu_clamps_some(R.ml_fwd_ref(o["x"], o["w"], lv, N, k, pad, *epi))
    wf = o["w"].view(K, k, k, C).permute(3, 1, 2, 0).reshape(C, k * k * K).contiguous()
    ref = R.ml_dgrad_domain(o["x"], wf, lv, N, k, pad, K, o["unit"])
    # the per-level transposed conv equals the stride-1 conv of dY with the flipped / transposed weight image
    assert torch.equal(ref, R.ml_fwd_ref(o["x"], R.flip_transpose_ref(wf, C, k, K), lv, N, k, k - 1 - pad))
    R.ml_wgrad_domain(o["xr"], o["dy"], lv, N, k, pad, R.F32_WGRAD_UNIT_EXP, None, o["dw0"], None, R.F32_WGRAD_DB_UNIT_EXP)
    assert R.f32_wgrad_splits(N * sum(h * w for h, w in lv), K, k * k * C) == 1


@pytest.mark.parametrize("name", sorted(R.F32_WGRAD))
def test_f32_wgrad_cases_are_inside_the_exact_domain_and_split_twice(name):
    N, H, W, C, K, k, s, p = R.F32_WGRAD[name]
    assert ("vec" in name) == (C % 4 == 0 and K % 4 == 0)
    o = R.f32_wgrad_operands(name)
    assert tuple(o["dy"].shape) == (2, 12, 11, K)
    M = 264
    splits = R.f32_wgrad_splits(M, K, k * k * C)
    assert splits == 2 and -(-M // 16) == 17 and M % 16 == 8
    R.wgrad_domain(o["x"], o["dy"], k, s, p, R.F32_WGRAD_UNIT_EXP, None, o["dw0"], None, R.F32_WGRAD_DB_UNIT_EXP)


@pytest.mark.parametrize("name", sorted(R.COLSUM_CASES))
def test_colsum_cases_are_inside_the_exact_domain_and_obey_their_dispatch_rules(name):
    M, C = R.COLSUM_CASES[name]
    g2d, db0 = R.colsum_operands(name)
    R.colsum_domain(g2d)
    R.colsum_domain(g2d, db0)
    route, parts, rows = R.colsum_route(M, C)
    assert (route == "vec") == name.startswith("vec")
    want = {"vec_ragged": (5, 256), "scalar_c24": (3, 344), "scalar_small_m": (2, 300), "scalar_c72": (1, 70)}[name]
    assert (parts, rows) == want and (name != "vec_ragged" or M % rows == 6)


def _per_group(fn, G):
    """the grouped operation as G ungrouped ones over the channel slices, concatenated on the channel axis"""
    return torch.cat([fn(i) for i in range(G)], dim=-1)


@pytest.mark.parametrize("name", sorted(R.GCONV_CASES))
def test_gconv_cases_are_inside_the_exact_domain_and_match_a_per_group_loop(name):
    g, G, N, H, W, s = R.GCONV_CASES[name][:6]
    C = g * G
    assert g % 4 == 0 and (g, G) in R.GCONV_GROUPS
    sl = lambda i: slice(i * g, (i + 1) * g)
    o = R.gconv_fwd_operands(name)
    for variant in R.GCONV_FWD_VARIANTS:
        ref = R.gconv_fwd_domain(name, o, variant)
        for h16 in H16S:
            assert R.has_tie_and_inexact(ref, h16), (variant, h16)
    loop = _per_group(lambda i: R.conv_fwd_ref(o["x"][..., sl(i)], o["w"][sl(i)], 3, s, 1, o["scale"][sl(i)], o["shift"][sl(i)], None, True), G)
    assert torch.equal(loop, R.gconv_fwd_domain(name, o, "scale_shift_relu"))
    for t in (o["x"], o["w"]):
        assert all(torch.equal(t.to(h).float(), t) for h in H16S)
    o = R.gconv_dgrad_operands(name)
    for variant in R.GCONV_DGRAD_VARIANTS:
        ref = R.gconv_dgrad_domain(name, o, variant)
        for h16 in H16S:
            assert R.has_tie_and_inexact(ref, h16), (variant, h16)
    for t in (o["dy"], o["w"], o["mask"], o["res"]):
        assert all(torch.equal(t.to(h).float(), t) for h in H16S)
    ws = o["w"] * o["scale"][:, None]
    loop = _per_group(lambda i: R.conv_dgrad_ref(o["dy"][..., sl(i)], ws[sl(i)], (N, H, W, g), 3, s, 1, o["mask"][..., sl(i)],
                                                 o["res"][..., sl(i)]), G)
    assert torch.equal(loop, R.gconv_dgrad_domain(name, o, "scale_mask_residual"))
    o = R.gconv_wgrad_operands(name)
    for use_sc in (False, True):
        R.gconv_wgrad_domain(name, o, use_sc, False)
    got = R.gconv_wgrad_domain(name, o, True, True)
    loop = torch.cat([R.conv_wgrad_ref(o["x"][..., sl(i)], o["dy"][..., sl(i)], 3, s, 1, o["scale"][sl(i)], o["dw0"][sl(i)])[0] for i in range(G)])
    assert torch.equal(loop, got)


def test_gconv_shapes_reach_the_thread_tile_edges_and_the_split_boundaries():
    hw = {(H, W, s): R.gconv_out_hw(H, W, s) for _, H, W in R.GCONV_SHAPES for s in (1, 2)}
    assert hw[(2, 3, 1)][1] < R.GPX and hw[(1, 1, 2)] == (1, 1)
    assert hw[(6, 8, 2)] == (3, 4) and hw[(6, 8, 1)][1] % R.GPX == 0 and hw[(7, 9, 2)][1] % R.GPX != 0
    for g, G in R.GCONV_GROUPS:
        C = g * G
        (s1, per1), (s2, per2) = R.gconv_wgrad_splits(3, 7, 9, C, G), R.gconv_wgrad_splits(3, 4, 5, C, G)
        assert (s1, per1) == (6, 32) and per1 % 9 != 0 and per1 % 63 != 0        # stride 1: splits begin mid-row and mid-image
        assert (s2, per2) == (2, 30) and per2 % 20 != 0                          # stride 2: the second split begins mid-image
    assert (12 // 4) & (12 // 4 - 1) != 0                                        # (4, 3): three channel quads


@pytest.mark.gpu
def test_restated_split_counts_equal_the_library():
    from ubteacher import hip
    lib = hip.load()
    for N, H, W, C, K, k, s, p in R.F32_WGRAD.values():
        OH, OW = R._out_hw(H, W, k, s, p)
        assert lib.utv2_conv2d_wgrad_splits(N, OH, OW, K, k * k * C) == R.f32_wgrad_splits(N * OH * OW, K, k * k * C)
    for C, K in R.F32_ML.values():
        for k in (1, 3):
            P = R.F32_ML_N * sum(h * w for h, w in R.F32_ML_LEVELS)
            assert lib.utv2_conv2d_wgrad_splits(1, 1, P, K, k * k * C) == R.f32_wgrad_splits(P, K, k * k * C)
    for g, G, N, H, W, s in [c[:6] for c in R.GCONV_CASES.values()]:
        OH, OW = R.gconv_out_hw(H, W, s)
        assert lib.utv2_gconv3x3_wgrad_splits(N, OH, OW, g * G, G) == R.gconv_wgrad_splits(N, OH, OW, g * G, G)[0]
