"""Every 16-bit conv route, in both builds of the kernel library (h16_t = __bf16 / _Float16), on operands for which fp32 accumulation is
EXACT (tests/exact_conv_ref.py): the kernel's fp32 output equals the fp64 reference bit for bit and a 16-bit output equals one
round-to-nearest-even of it, whatever the tile shape, split-K order or wave schedule.  No tolerance: one dropped, duplicated or misplaced
term, or a second rounding at a 16-bit store, fails torch.equal.  The shapes are the smallest that reach each kernel of launch_igemm16 /
wgrad_bf16_impl (csrc/conv_bf16.hip); the rule that selects each one stands beside it in exact_conv_ref.py.  The last section repeats the
route table with Gaussian operands on the fp16 build under the project's own tolerance criteria."""
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


def _eq(got, ref64, dt, rows=None):
    """the whole tensor (or its stratified rows) equals the single rounding of the exact value"""
    got = got.reshape(-1, got.shape[-1]) if rows is not None else got
    g = got[rows.to(got.device)].cpu() if rows is not None else got.cpu()
    want = R.to_out(ref64, dt).view(g.shape)
    same = torch.equal(g, want)
    if not same:       # what differs, for the log
        bad = (g.float() != want.float()).nonzero()
        print("mismatch: %d of %d elements, first at %s: got %r want %r" % (len(bad), g.numel(), bad[0].tolist(),
              float(g[tuple(bad[0])]), float(want[tuple(bad[0])])))
    return same


def _out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def _pack_bits(t):
    b = (t.float() > 0).reshape(t.shape[:-1] + (t.shape[-1] // 8, 8)).to(torch.int32)
    return (b << torch.arange(8, device=t.device, dtype=torch.int32)).sum(-1).to(torch.uint8)


def _fwd_refs(name, x, w2, u, sc, bi, res):
    """(rows or None, plain reference, epilogue reference) of one NHWC case - the precondition is asserted inside"""
    N, H, W, C, K, k, s, p = R.NHWC_CASES[name][:8]
    if name in R.BIG_M:
        OH, OW = _out_hw(H, W, k, s, p)
        rows = R.subset_rows(N * OH * OW, 256)
        return rows, R.rows_domain(x, w2, k, s, p, rows, u), R.rows_domain(x, w2, k, s, p, rows, u - 1, sc, bi, res.view(-1, K), True)
    return None, R.fwd_domain(x, w2, k, s, p, u), R.fwd_domain(x, w2, k, s, p, u - 1, sc, bi, res, True)


# -------------------------------------------------------------------------------------------------------------------------------
# B. forward and dgrad through every route
@pytest.mark.parametrize("name", list(R.NHWC_CASES))
def test_forward_routes_are_exact(name, h16):
    from ubteacher import hip
    N, H, W, C, K, k, s, p, x_f32 = R.NHWC_CASES[name][:9]
    x, w2, u = R.nhwc_operands(name)
    OH, OW = _out_hw(H, W, k, s, p)
    sc, bi, res = R.epilogue_operands(K, (N, OH, OW, K), u, 1)
    rows, ref0, ref1 = _fwd_refs(name, x, w2, u, sc, bi, res)
    xd = x.cuda().to(F32 if x_f32 else h16)
    w16 = w2.cuda().to(h16)
    assert torch.equal(w16.float().cpu(), w2) and torch.equal(xd.float().cpu(), x)
    for dt in (F32, h16):
        y0 = hip.conv2d_fwd_bf16(xd, w16, stride=s, pad=p, kh=k, kw=k, out_dtype=dt)
        assert y0.dtype == dt and _eq(y0, ref0, dt, rows), (name, dt, "plain")
        y1 = hip.conv2d_fwd_bf16(xd, w16, scale=sc.cuda(), bias=bi.cuda(), residual=res.cuda().to(dt), stride=s, pad=p, kh=k, kw=k,
                                 relu=True, out_dtype=dt)
        assert _eq(y1, ref1, dt, rows), (name, dt, "scale + bias + residual + relu")


@pytest.mark.parametrize("name", [n for n in R.NHWC_CASES if n not in R.BIG_M] + ["pp_persistent_rem", "rs_rem"])
def test_dgrad_routes_are_exact(name, h16):
    """the dgrad of every case (the same kernels over dY with the flipped / transposed weight image; stride 2: the dilated gather of the
    generic kernel).  pp_persistent_rem / rs_rem: C >= 256 output channels, so their dgrads run on the 256-tile kernels too."""
    from ubteacher import hip
    N, H, W, C, K, k, s, p, x_f32, bx, bw = R.NHWC_CASES[name]
    g = torch.Generator().manual_seed(11)
    OH, OW = _out_hw(H, W, k, s, p)
    dy = R.dyadic((N, OH, OW, K), bx, -3, g)
    w2 = R.dyadic((K, k * k * C), bw, -5, g)
    wt16 = hip.weight_flip_transpose_bf16(w2.cuda(), K, k, k, C)
    wt_ref = R.flip_transpose_ref(w2, K, k, C)
    assert torch.equal(wt16.cpu(), wt_ref.to(h16))
    if name in R.BIG_M:
        rows = R.subset_rows(N * H * W, 256)
        ref = R.rows_domain(dy, wt_ref, k, 1, k - 1 - p, rows, -8)       # stride 1: dgrad = the conv over dY with pad k - 1 - pad
    else:
        rows, ref = None, R.dgrad_domain(dy, w2, (N, H, W, C), k, s, p, -8)
    dyd = dy.cuda().to(F32 if x_f32 else h16)
    for dt in (F32, h16):
        dx = hip.conv2d_dgrad_bf16(dyd, wt16, (N, H, W, C), s, p, k, k, out_dtype=dt)
        assert dx.dtype == dt and _eq(dx, ref, dt, rows), (name, dt)


def test_dilated_gather_dgrad_is_exact(h16):
    from ubteacher import hip
    N, H, W, C, K, k, s, p = R.DGRAD_DILATED
    g = torch.Generator().manual_seed(4)
    OH, OW = _out_hw(H, W, k, s, p)
    dy = R.dyadic((N, OH, OW, K), 3, -3, g)
    w2 = R.dyadic((K, k * k * C), 3, -5, g)
    ref = R.dgrad_domain(dy, w2, (N, H, W, C), k, s, p, -8)
    wt16 = hip.weight_flip_transpose_bf16(w2.cuda(), K, k, k, C)
    for xdt in (F32, h16):
        for dt in (F32, h16):
            assert _eq(hip.conv2d_dgrad_bf16(dy.cuda().to(xdt), wt16, (N, H, W, C), s, p, k, k, out_dtype=dt), ref, dt), (xdt, dt)


def test_fp32_operand_is_rounded_once_on_load(h16):
    """the generic kernel takes an fp32 x and rounds it to the 16-bit type while staging: x with 12 .. 16 significant bits, the reference
    rounds it with torch first"""
    from ubteacher import hip
    N, H, W, C, K, k, s, p = R.NHWC_CASES["generic128"][:8]
    g = torch.Generator().manual_seed(4)
    x = R.dyadic_wide((N, H, W, C), -14, g)
    w2 = R.dyadic((K, k * k * C), 3, -5, g)
    xr = x.to(h16).float()
    assert float((xr != x).float().mean()) > 0.5
    ref = R.fwd_domain(xr, w2, k, s, p, R.wide_unit_exp(-14, h16) - 5)
    for dt in (F32, h16):
        assert _eq(hip.conv2d_fwd_bf16(x.cuda(), w2.cuda().to(h16), stride=s, pad=p, kh=k, kw=k, out_dtype=dt), ref, dt), dt


@pytest.mark.parametrize("name", list(R.ML_CASES))
def test_multi_level_routes_are_exact(name, h16):
    from ubteacher import hip
    level_hw, N, C, K, bx, bw = R.ML_CASES[name]
    g = torch.Generator().manual_seed(5)
    P = N * sum(h * w for h, w in level_hw)
    x = R.dyadic((P, C), bx, -3, g)
    w2 = R.dyadic((K, 9 * C), bw, -5, g)
    sc, bi, res = R.epilogue_operands(K, (P, K), -8, 2)
    ref0 = R.ml_fwd_domain(x, w2, level_hw, N, 3, 1, -8)
    ref1 = R.ml_fwd_domain(x, w2, level_hw, N, 3, 1, -9, sc, bi, res, True)
    xd, w16 = x.cuda().to(h16), w2.cuda().to(h16)
    for dt in (F32, h16):
        assert _eq(hip.conv2d_ml_fwd_bf16(xd, w16, level_hw, N, k=3, pad=1, out_dtype=dt), ref0, dt), (name, dt, "plain")
        y1 = hip.conv2d_ml_fwd_bf16(xd, w16, level_hw, N, scale=sc.cuda(), bias=bi.cuda(), residual=res.cuda().to(dt), k=3, pad=1, relu=True,
                                    out_dtype=dt)
        assert _eq(y1, ref1, dt), (name, dt, "epilogue")
        if K % 8 == 0 and K <= 96:
            # the 96-wide tile (and the 128-wide one at K = 40) writing K columns of a wider matrix: the columns beyond K keep their bytes
            wide = torch.full((P, 128), 7.0, dtype=dt, device="cuda")
            hip.conv2d_ml_fwd_bf16(xd, w16, level_hw, N, k=3, pad=1, out=wide[:, :K])
            assert _eq(wide[:, :K], ref0, dt) and bool((wide[:, K:] == 7.0).all()), (name, dt, "padded columns")


def _decode_and_table_outputs(name):
    """(y without table, y with table) of one NHWC_CASES / ML_CASES entry on the selected build: the C entry point called directly, once
    with rowinfo null - the tile prologue decodes its rows (conv_geom.h) - and once with the geometry table of the same conv"""
    import ctypes
    from ubteacher import hip
    h16 = hip.h16_dtype()
    ys = []
    if name in R.NHWC_CASES:
        N, H, W, C, K, k, s, p = R.NHWC_CASES[name][:8]
        x, w2, _ = R.nhwc_operands(name)
        OH, OW = _out_hw(H, W, k, s, p)
        xd, w16 = x.cuda().to(h16), w2.cuda().to(h16)
        for ri in (None, hip.rowinfo_nhwc(N, H, W, OH, OW, s, p, k, k, xd.device)):
            y = torch.full((N, OH, OW, K), float("nan"), dtype=h16, device="cuda")
            hip.call("utv2_conv2d_nhwc_fwd_bf16_bits", hip._p(xd), 1, hip._p(w16), hip._p(y), 1, None, None, None, None, None, N, H, W, C, K,
                     k, k, s, p, 1, OH, OW, 0, 0, hip._p(ri), None, None, None, hip._stream())
            ys.append(y)
    else:
        level_hw, N, C, K, bx, bw = R.ML_CASES[name]
        g = torch.Generator().manual_seed(5)
        P = N * sum(h * w for h, w in level_hw)
        xd, w16 = R.dyadic((P, C), bx, -3, g).cuda().to(h16), R.dyadic((K, 9 * C), bw, -5, g).cuda().to(h16)
        Hs, Ws = hip._iarr([h for h, _ in level_hw]), hip._iarr([w for _, w in level_hw])
        for ri in (None, hip.rowinfo_ml(N, level_hw, 1, 3, xd.device)):
            y = torch.full((P, K), float("nan"), dtype=h16, device="cuda")
            hip.call("utv2_conv2d_ml_fwd_bf16_g", hip._p(xd), 1, C, hip._p(w16), hip._p(y), 1, K, None, None, None, len(level_hw),
                     ctypes.cast(Hs, hip.c_p), ctypes.cast(Ws, hip.c_p), N, C, K, 3, 3, 1, 0, 0, 1, None, hip._p(ri), hip._stream())
            ys.append(y)
    torch.cuda.synchronize()
    return ys


# name -> the kernel whose prologue decodes; the environment of a fresh child process when a switch (read once per process) must differ
_PROLOGUE_CASES = {
    "v2_64_bk32": None,        # 3x3 stride 1 pad 1 on the 128 x 64 v2 tile: M = 81, one partial row tile
    "strided_bk64": None,      # 3x3 stride 2 pad 1 (v2<128, ., 64>), 130 row tiles, the last one partial
    "n96_72_ragged": None,     # two levels, 3x3: level 1 starts at row 10368 = 40.5 tiles of 256 rows (v2<96, true, 32>)
    "pp_one_tile": {"UTV2_PP_RS": "0"},   # the smallest ping-pong case, kept off the row-span kernel
}


@pytest.mark.parametrize("name", list(_PROLOGUE_CASES))
def test_tile_prologue_decode_equals_geometry_table(name, h16):
    """The Python wrappers pass the geometry table wherever they can, so the in-kernel row decode of the v2 and ping-pong prologues runs only
    for the image stem and under UTV2_CONV_ROWINFO=0.  It shares its formulas with the table builder (csrc/conv_geom.h): with and without
    the table the same conv must give the same bits."""
    env = _PROLOGUE_CASES[name]
    if env is None:
        y_decode, y_table = _decode_and_table_outputs(name)
        assert not bool(torch.isnan(y_table.float()).any())
        assert torch.equal(y_decode, y_table), name
        return
    import os
    import subprocess
    import sys
    from ubteacher import hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path[:0] = [%r, %r]; import torch; from ubteacher import hip; hip.set_h16(%r); "
            "from tests.test_conv_exact_gpu import _decode_and_table_outputs as f; a, b = f(%r); "
            "assert not bool(torch.isnan(b.float()).any()); assert torch.equal(a, b); print('same bits')"
            % (root, os.path.dirname(os.path.dirname(os.path.abspath(hip.__file__))), hip.H16[0], name))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "same bits" in out.stdout, out.stderr[-2000:]


@pytest.mark.parametrize("canvases", [R.STEM_CANVASES])
def test_image_stem_is_exact(canvases, h16):
    from ubteacher import hip
    ims = [R.stem_images(hw, 1, seed=3 + i)[0] for i, hw in enumerate(canvases)]
    x16, _ = hip.preprocess_images([im.cuda() for im in ims], R.STEM_MEAN, R.STEM_STD, 32, bf16_stem=True)
    assert x16.dtype == h16
    w208, sc, sh = R.stem_weights()
    w16s = hip.stem_weight_image(w208.cuda())
    xs = x16.cpu()
    xs.canvas = x16.canvas
    xi, w2 = R.stem_operands(xs, w16s.cpu())
    assert torch.equal(w2, R.stem_taps(w208).to(h16))      # the packed weight image holds the 7x7x3 taps where the kernel reads them
    R.assert_on_grid(xi, -6, "the stored image")
    ref = R.stem_ref(xi, w2, sc, sh)
    R.assert_exact_domain(R.conv_fwd_ref(xi.float().abs(), w2.float().abs(), 7, 2, 3, sc, sh.abs()), ref, R.STEM_UNIT_EXP)
    for dt in (F32, h16):
        assert _eq(hip.conv2d_stem_fwd_bf16(x16, w16s, sc.cuda(), sh.cuda(), True, dt), ref, dt), dt


@pytest.mark.parametrize("hw", R.STEM_POOL_HW)
def test_fused_stem_pool_is_exact(hw, h16):
    """fused kernel == stem conv then max pool == the fp64 chain with the stem output rounded once"""
    from ubteacher import hip
    ims = R.stem_images(hw, 2)
    x16, _ = hip.preprocess_images([im.cuda() for im in ims], R.STEM_MEAN, R.STEM_STD, 2, bf16_stem=True)
    w208, sc, sh = R.stem_weights()
    w16s = hip.stem_weight_image(w208.cuda())
    xs = x16.cpu()
    xs.canvas = x16.canvas
    xi, w2 = R.stem_operands(xs, w16s.cpu())
    assert torch.equal(w2, R.stem_taps(w208).to(h16))
    conv64 = R.stem_ref(xi, w2, sc, sh)
    R.assert_exact_domain(R.conv_fwd_ref(xi.float().abs(), w2.float().abs(), 7, 2, 3, sc, sh.abs()), conv64, R.STEM_UNIT_EXP)
    want = R.maxpool_ref(R.r16(conv64, h16))
    fused = hip.stem_pool_fwd_bf16(x16, w16s, sc.cuda(), sh.cuda())
    chain = hip.maxpool3x3s2(hip.conv2d_stem_fwd_bf16(x16, w16s, sc.cuda(), sh.cuda(), True, h16))
    assert _eq(fused, want, h16) and _eq(chain, want, h16) and torch.equal(fused, chain)


@pytest.mark.parametrize("shortcut", [False, True])
@pytest.mark.parametrize("shape", R.BOTTLENECK_SHAPES)
def test_fused_bottleneck_is_exact(shape, shortcut, h16):
    """fused kernel == the three / four conv launches == the fp64 chain with c1, c2 and the shortcut rounded once each"""
    from ubteacher import hip
    o = R.bottleneck_operands(shape, shortcut)
    y64, c1_64, c2_64, _ = R.bottleneck_domain(o, h16)
    d = {k: (v.cuda().to(h16) if k[0] in "xw" else v.cuda()) for k, v in o.items()}
    assert all(torch.equal(d[k].float().cpu(), o[k]) for k in d)
    kw = dict(wsc=d["wsc"], ssc=d["ssc"], bsc=d["bsc"]) if shortcut else {}
    y = hip.bottleneck_fwd_bf16(d["x"], d["w1"], d["w2"], d["w3"], d["s1"], d["b1"], d["s2"], d["b2"], d["s3"], d["b3"], **kw)
    c1 = hip.conv2d_fwd_bf16(d["x"], d["w1"], scale=d["s1"], bias=d["b1"], relu=True)
    c2 = hip.conv2d_fwd_bf16(c1, d["w2"], scale=d["s2"], bias=d["b2"], relu=True, kh=3, kw=3, pad=1)
    r = hip.conv2d_fwd_bf16(d["x"], d["wsc"], scale=d["ssc"], bias=d["bsc"]) if shortcut else d["x"]
    y3 = hip.conv2d_fwd_bf16(c2, d["w3"], scale=d["s3"], bias=d["b3"], relu=True, residual=r)
    assert _eq(c1, c1_64, h16) and _eq(c2, c2_64, h16)
    assert _eq(y, y64, h16) and _eq(y3, y64, h16) and torch.equal(y, y3)


# -------------------------------------------------------------------------------------------------------------------------------
# mask and ReLU epilogues
@pytest.mark.parametrize("name", ["v2_64_bk32", "v2_128_bk32", "pp_one_tile"])
def test_relu_bit_plane_and_masked_dgrad_are_exact(name, h16):
    """64-wide, 128-wide and 256-tile epilogues: the forward's bit plane is `stored output > 0`; a dgrad with mask, residual and post_mask -
    as 16-bit tensors and as bit planes - equals the fp64 expression post > 0 ? ((mask > 0 ? dx : 0) + residual) : 0"""
    from ubteacher import hip
    N, H, W, C, K, k, s, p = R.NHWC_CASES[name][:8]
    x, w2, u = R.nhwc_operands(name)
    OH, OW = _out_hw(H, W, k, s, p)
    sc, bi, res = R.epilogue_operands(K, (N, OH, OW, K), u, 1)
    ref = R.fwd_domain(x, w2, k, s, p, u - 1, sc, bi, res, True)
    bits = hip.relu_bits_buffer((N, OH, OW, K), "cuda")
    bits.fill_(0xA5)
    y = hip.conv2d_fwd_bf16(x.cuda().to(h16), w2.cuda().to(h16), scale=sc.cuda(), bias=bi.cuda(), residual=res.cuda().to(h16), stride=s,
                            pad=p, kh=k, kw=k, relu=True, out_dtype=h16, relu_bits=bits)
    assert _eq(y, ref, h16)
    assert torch.equal(bits.cpu(), _pack_bits(R.to_out(ref, h16)))
    assert 0.1 < float((ref > 0).double().mean()) < 0.9
    # dgrad of a K -> C layer of the same geometry class: output channels = the case's K (so the same tile width), reduction = its C
    g = torch.Generator().manual_seed(12)
    Cd, Kd = K, C
    Kd = max(Kd, 32)
    dy = R.dyadic((N, OH, OW, Kd), 3, -3, g)
    wf = R.dyadic((Kd, k * k * Cd), 3, -5, g)
    wt16 = hip.weight_flip_transpose_bf16(wf.cuda(), Kd, k, k, Cd)
    shp = (N, OH, OW, Cd)
    mk = R.dyadic(shp, 3, 0, g, relu_like=True)
    pm = R.dyadic(shp, 3, 0, g, relu_like=True)
    rs = R.dyadic(shp, 7, -4, g)
    pd = k // 2
    want = R.dgrad_domain(dy, wf, shp, k, 1, pd, -8, mask=mk, residual=rs, post_mask=pm)
    m16, p16, r16_ = mk.cuda().to(h16), pm.cuda().to(h16), rs.cuda().to(h16)
    a = hip.conv2d_dgrad_bf16(dy.cuda().to(h16), wt16, shp, 1, pd, k, k, out_dtype=h16, mask=m16, residual=r16_, post_mask=p16)
    b = hip.conv2d_dgrad_bf16(dy.cuda().to(h16), wt16, shp, 1, pd, k, k, out_dtype=h16, mask_bits=_pack_bits(m16), residual=r16_,
                              post_mask_bits=_pack_bits(p16))
    assert _eq(a, want, h16) and _eq(b, want, h16)
    f = hip.conv2d_dgrad_bf16(dy.cuda().to(h16), wt16, shp, 1, pd, k, k, out_dtype=F32, mask=mk.cuda(), residual=rs.cuda(), post_mask=pm.cuda())
    assert _eq(f, want, F32)


# -------------------------------------------------------------------------------------------------------------------------------
# weight gradients
def _wgrad_check(hip, x, dy2d, ri, C, K, k, rs, dw0, db0, ref_fn):
    """dw / db with accumulate off and no rowscale; then rowscale (powers of two) and accumulate=True onto non-zero dyadic dw / db"""
    dw = torch.full((K, k * k * C), 3.0, device="cuda")
    db = torch.full((K,), 3.0, device="cuda")
    hip.conv2d_wgrad_bf16(x, dy2d, dw, ri, C, k, k, accumulate=False, db=db)
    w0, b0 = ref_fn(None, None, None)
    ok = _eq(dw, w0, F32) and _eq(db, b0, F32)
    dw, db = dw0.cuda().clone(), db0.cuda().clone()
    hip.conv2d_wgrad_bf16(x, dy2d, dw, ri, C, k, k, accumulate=True, db=db, rowscale=rs.cuda())
    w1, b1 = ref_fn(rs, dw0, db0)
    return ok and _eq(dw, w1, F32) and _eq(db, b1, F32)


@pytest.mark.parametrize("pair", ["f32-f32", "h16-h16", "h16-f32", "f32-h16"])
@pytest.mark.parametrize("name", list(R.WGRAD_128))
def test_wgrad_128_tile_is_exact(name, pair, h16):
    from ubteacher import hip
    N, H, W, C, K, k, s, p = R.WGRAD_128[name]
    x, dy, rs, dw0, db0 = R.wgrad_operands(N, H, W, C, K, k, s, p)
    xdt, dydt = [F32 if t == "f32" else h16 for t in pair.split("-")]
    ri = hip.rowinfo_nhwc(N, H, W, dy.shape[1], dy.shape[2], s, p, k, k, "cuda")
    ref = lambda r, a, b: R.wgrad_domain(x, dy, k, s, p, R.WGRAD_UNIT_EXP, r, a, b, R.WGRAD_DB_UNIT_EXP)
    assert _wgrad_check(hip, x.cuda().to(xdt), dy.cuda().to(dydt).reshape(-1, K), ri, C, K, k, rs, dw0, db0, ref)


@pytest.mark.parametrize("name", list(R.WGRAD_PP))
def test_wgrad_256_tile_is_exact(name, h16):
    from ubteacher import hip
    N, H, W, C, K, k, s, p = R.WGRAD_PP[name]
    x, dy, rs, dw0, db0 = R.wgrad_operands(N, H, W, C, K, k, s, p)
    ri = hip.rowinfo_nhwc(N, H, W, dy.shape[1], dy.shape[2], s, p, k, k, "cuda")
    ref = lambda r, a, b: R.wgrad_domain(x, dy, k, s, p, R.WGRAD_UNIT_EXP, r, a, b, R.WGRAD_DB_UNIT_EXP)
    assert _wgrad_check(hip, x.cuda().to(h16), dy.cuda().to(h16).reshape(-1, K), ri, C, K, k, rs, dw0, db0, ref)


def test_wgrad_256_tile_multi_level_tower_is_exact(h16):
    from ubteacher import hip
    level_hw, N, C, K = R.WGRAD_PP_TOWER
    x, dy, rs, dw0, db0 = R.wgrad_ml_operands(level_hw, N, C, K)
    assert x.shape[0] >= 16 * 64
    ri = hip.rowinfo_ml(N, level_hw, 1, 3, "cuda")
    ref = lambda r, a, b: R.ml_wgrad_domain(x, dy, level_hw, N, 3, 1, R.WGRAD_UNIT_EXP, r, a, b, R.WGRAD_DB_UNIT_EXP)
    assert _wgrad_check(hip, x.cuda().to(h16), dy.cuda().to(h16), ri, C, K, 3, rs, dw0, db0, ref)


# -------------------------------------------------------------------------------------------------------------------------------
# conversions
def _rounding_probe(h16):
    """fp32 vector of ties, their fp32 neighbours, signed zeros, infinities, a NaN; fp16: the overflow boundary and the subnormal range"""
    keep = 8 if h16 == torch.bfloat16 else 11
    base = torch.tensor([1.0, 1.5, 3.0, 100.0, 0.0078125, 1.0 - 2.0 ** -keep], dtype=torch.float64)
    half = 2.0 ** -keep
    ties = torch.cat([base * (1 + half * m) for m in (1, 3)])           # half way between two h16 values (even and odd low bit)
    f = ties.to(F32)
    assert torch.equal(f.double(), ties)
    ints = f.view(torch.int32)
    v = torch.cat([f, (ints + 1).view(F32), (ints - 1).view(F32)])
    v = torch.cat([v, -v, torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan")])])
    if h16 == torch.float16:
        edge = torch.tensor([65472.0, 65504.0, 65519.99, 65520.0, 65536.0, 1e6])
        sub = torch.arange(0, 2050, dtype=torch.float64) * 2.0 ** -25    # multiples and half multiples of 2^-24, up to the first normals
        v = torch.cat([v, edge, -edge, sub.to(F32), -sub.to(F32)])
    pad = (-v.numel()) % 8
    return torch.cat([v, torch.zeros(pad)])


def _same_or_nan(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a.float(), 9.0).view(torch.int32),
                                                                     torch.nan_to_num(b.float(), 9.0).view(torch.int32))


def test_conversions_round_once_to_nearest_even(h16):
    from ubteacher import hip
    v = _rounding_probe(h16)
    n = v.numel()
    want = v.to(h16)
    out = torch.empty(n, dtype=h16, device="cuda")
    hip.f32_to_bf16(v.cuda(), out)
    assert _same_or_nan(out.cpu(), want)
    assert _same_or_nan(hip.pad_cols_bf16(v.cuda().view(1, n), n + 8).cpu()[0, :n], want)
    assert float(hip.pad_cols_bf16(v.cuda().view(1, n), n + 8)[0, n:].float().abs().max()) == 0.0
    assert _same_or_nan(hip.pad_cols_bf16(want.cuda().view(1, n), n + 8).cpu()[0, :n], want)
    # the dgrad weight image: [K, 1, 1, C] -> [C, K]; without a scale, and with one applied BEFORE the single rounding
    K, C = 8, n // 8
    w = v.view(K, C)
    assert _same_or_nan(hip.weight_flip_transpose_bf16(w.cuda(), K, 1, 1, C).cpu(), w.t().contiguous().to(h16))
    g = torch.Generator().manual_seed(1)
    w3 = torch.randn(24, 9 * 16, generator=g)
    s3 = torch.rand(24, generator=g) + 0.5
    got = hip.weight_flip_transpose_bf16(w3.cuda(), 24, 3, 3, 16, s3.cuda())
    assert torch.equal(got.cpu(), R.flip_transpose_ref(w3 * s3[:, None], 24, 3, 16).to(h16))     # fp32 product, one rounding


# -------------------------------------------------------------------------------------------------------------------------------
# C. fp16-only edges
FP16_EDGE = [65472.0, 65504.0, 65520.0, 65536.0, 70000.0]      # largest finite below the maximum, the maximum, the tie that goes to inf, above


@pytest.fixture
def fp16_build():
    """the fp16 build alone: these edges are properties of the fp16 number format (bf16 has fp32's exponent range)"""
    from ubteacher import hip
    hip.set_h16("fp16")
    try:
        yield hip.h16_dtype()
    finally:
        hip.set_h16("bf16")


@pytest.mark.parametrize("name", ["v2_128_bk32", "pp_one_tile"])
def test_fp16_store_overflow_forward(name, fp16_build):
    """results at and around the fp16 maximum at a 16-bit store (128-tile and 256-tile epilogues): 65520 is the tie that rounds to +inf;
    the fp32 output of the same launch stays finite and exact"""
    h16 = fp16_build
    from ubteacher import hip
    N, H, W, C, K, k, s, p, _, bx, bw = R.NHWC_CASES[name]
    g = torch.Generator().manual_seed(15)
    # grid 2^-2: a sum beyond 65536 still has its 24 bits (17 integer + 2 fraction); conv values of a few hundred around the maximum
    x, w2, u = R.dyadic((N, H, W, C), bx, 0, g), R.dyadic((K, k * k * C), bw, -2, g), -2
    edge = torch.tensor(FP16_EDGE + [-v for v in FP16_EDGE])
    w2[:10] = 0.0                                   # channels 0 .. 9: the bias alone
    bi = torch.full((K,), 65504.0)                  # the others: the conv values around +- the maximum
    bi[K // 2:] = -65504.0
    bi[:10] = edge
    ref = R.fwd_domain(x, w2, k, s, p, u, None, bi)
    want = R.to_out(ref, h16)
    assert all(bool((ref[..., i] == float(edge[i])).all()) for i in range(10))
    assert bool(torch.isinf(want[..., 2]).all()) and bool(torch.isfinite(want[..., 1]).all()) and 0.2 < float(torch.isinf(want).float().mean()) < 0.8
    xd, w16 = x.cuda().to(h16), w2.cuda().to(h16)
    assert _eq(hip.conv2d_fwd_bf16(xd, w16, bias=bi.cuda(), stride=s, pad=p, kh=k, kw=k, out_dtype=h16), ref, h16)
    y32 = hip.conv2d_fwd_bf16(xd, w16, bias=bi.cuda(), stride=s, pad=p, kh=k, kw=k, out_dtype=F32)
    assert bool(torch.isfinite(y32).all()) and _eq(y32, ref, F32)


@pytest.mark.parametrize("route,N,H,W,C,K", [("128", 1, 9, 9, 136, 64), ("256", 1, 130, 127, 512, 1024)])
def test_fp16_store_overflow_dgrad(route, N, H, W, C, K, fp16_build):
    """the same at a dgrad's store (no bias there: two products, 65504 + b): v2<128> and the 256-tile ping-pong kernel (1x1, reduction
    1024, 512 output channels, 130 tiles).  What the loss scaler's found-inf logic relies on."""
    h16 = fp16_build
    from ubteacher import hip
    g = torch.Generator().manual_seed(13)
    dy = R.dyadic((N, H, W, K), 3, 0, g)
    w2 = R.dyadic((K, C), 3, -5, g)
    dy[..., :2] = 1.0
    adds = [-32.0, 0.0, 16.0, 32.0, 4496.0]
    w2[:, :10] = 0.0
    w2[0, :10] = torch.tensor([65504.0] * 5 + [-65504.0] * 5)
    w2[1, :10] = torch.tensor(adds + [-v for v in adds])
    ref = R.dgrad_domain(dy, w2, (N, H, W, C), 1, 1, 0, -5)
    edge = torch.tensor(FP16_EDGE + [-v for v in FP16_EDGE], dtype=torch.float64)
    assert all(bool((ref[..., i] == edge[i]).all()) for i in range(10))
    wt16 = hip.weight_flip_transpose_bf16(w2.cuda(), K, 1, 1, C)
    assert bool(torch.isfinite(wt16).all())
    want = R.to_out(ref, h16)
    assert bool(torch.isinf(want[..., 2]).all()) and bool(torch.isfinite(want[..., 1]).all())
    assert _eq(hip.conv2d_dgrad_bf16(dy.cuda().to(h16), wt16, (N, H, W, C), 1, 0, 1, 1, out_dtype=h16), ref, h16)
    d32 = hip.conv2d_dgrad_bf16(dy.cuda().to(h16), wt16, (N, H, W, C), 1, 0, 1, 1, out_dtype=F32)
    assert bool(torch.isfinite(d32).all()) and _eq(d32, ref, F32)


@pytest.mark.parametrize("name", ["v2_128_bk32", "pp_one_tile"])
def test_fp16_subnormal_operands_and_results(name, fp16_build):
    """x made of fp16 subnormals (integers * 2^-24 below 2^-14) against normal weights: exact in fp32, and the MFMA does NOT flush them
    (measured on gfx950) - the expectation is the fp64 reference on the operands as they are.  Then results that land in the
    fp16 subnormal range at a 16-bit store: one rounding to the subnormal grid."""
    h16 = fp16_build
    from ubteacher import hip
    N, H, W, C, K, k, s, p, _, bx, bw = R.NHWC_CASES[name]
    g = torch.Generator().manual_seed(14)
    x = R.dyadic((N, H, W, C), 7, -24, g)
    w2 = R.dyadic((K, k * k * C), bw, 0, g)
    assert float(x.abs().max()) < 2.0 ** -14 and torch.equal(x.to(h16).float(), x)
    ref = R.fwd_domain(x, w2, k, s, p, -24)
    flushed = R.conv_fwd_ref(torch.zeros_like(x), w2, k, s, p)
    assert not torch.equal(ref, flushed)
    y32 = hip.conv2d_fwd_bf16(x.cuda().to(h16), w2.cuda().to(h16), stride=s, pad=p, kh=k, kw=k, out_dtype=F32)
    assert _eq(y32, ref, F32)
    # results in the subnormal range of the store: normal operands, products on the grid 2^-30, sums of a few 2^-20
    x2 = R.dyadic((N, H, W, C), bx, -13, g)
    w3 = R.dyadic((K, k * k * C), bw, -17, g)
    ref2 = R.fwd_domain(x2, w3, k, s, p, -30)
    want = R.to_out(ref2, h16)
    sub = (want != 0) & (want.abs().float() < 2.0 ** -14)
    assert float(sub.float().mean()) > 0.5 and float((want.double() != ref2).double().mean()) > 0.3
    assert _eq(hip.conv2d_fwd_bf16(x2.cuda().to(h16), w3.cuda().to(h16), stride=s, pad=p, kh=k, kw=k, out_dtype=h16), ref2, h16)


# -------------------------------------------------------------------------------------------------------------------------------
# D. Gaussian operands on the fp16 build (the bf16 equivalents are test_conv_bf16_gpu.py)
@pytest.mark.parametrize("name", list(R.NHWC_CASES))
def test_fp16_build_with_gaussian_operands(name, fp16_build):
    """randn operands rounded to fp16 against the fp64 reference, with the project's criteria: fp32 output relerr < 2e-4, 16-bit output
    close16 with the half ulp of fp16 (2^-11)"""
    h16 = fp16_build
    from ubteacher import hip
    N, H, W, C, K, k, s, p, x_f32 = R.NHWC_CASES[name][:9]
    x, w2, b, res = R.gaussian_operands(name)
    if name in R.BIG_M:
        OH, OW = _out_hw(H, W, k, s, p)
        rows = R.subset_rows(N * OH * OW, 256)
        ref = R._epilogue(R.conv_rows_ref(x, w2, k, s, p, rows), None, b, res.view(-1, K)[rows], True)
    else:
        rows, ref = None, R.conv_fwd_ref(x, w2, k, s, p, None, b, res, True)
    xd, w16 = x.cuda().to(F32 if x_f32 else h16), w2.cuda().to(h16)
    pick = lambda t: (t.reshape(-1, K)[rows.cuda()] if rows is not None else t).cpu()
    y32 = pick(hip.conv2d_fwd_bf16(xd, w16, bias=b.cuda(), residual=res.cuda(), stride=s, pad=p, kh=k, kw=k, relu=True, out_dtype=F32))
    e = R.relerr(y32, ref)
    print(name, "fp32 relerr %.3g" % e)
    assert e < 2e-4
    y16 = pick(hip.conv2d_fwd_bf16(xd, w16, bias=b.cuda(), residual=res.cuda().to(h16), stride=s, pad=p, kh=k, kw=k, relu=True, out_dtype=h16))
    assert R.close16(y16, ref, 2.0 ** -11)
    if K % 8 == 0 and name not in R.BIG_M:
        g = torch.Generator().manual_seed(3)
        dy = torch.randn(N, *_out_hw(H, W, k, s, p), K, generator=g).half().float()
        refd = R.conv_dgrad_ref(dy, w2, (N, H, W, C), k, s, p)
        wt16 = hip.weight_flip_transpose_bf16(w2.cuda(), K, k, k, C)
        dyd = dy.cuda().to(F32 if x_f32 else h16)
        assert R.relerr(hip.conv2d_dgrad_bf16(dyd, wt16, (N, H, W, C), s, p, k, k, out_dtype=F32).cpu(), refd) < 2e-4
        assert R.close16(hip.conv2d_dgrad_bf16(dyd, wt16, (N, H, W, C), s, p, k, k, out_dtype=h16).cpu(), refd, 2.0 ** -11)


@pytest.mark.parametrize("name", list(R.WGRAD_128) + list(R.WGRAD_PP))
def test_fp16_build_weight_gradients_with_gaussian_operands(name, fp16_build):
    h16 = fp16_build
    from ubteacher import hip
    N, H, W, C, K, k, s, p = {**R.WGRAD_128, **R.WGRAD_PP}[name]
    g = torch.Generator().manual_seed(2)
    OH, OW = _out_hw(H, W, k, s, p)
    x = torch.randn(N, H, W, C, generator=g).half().float()
    dy = torch.randn(N, OH, OW, K, generator=g).half().float()
    dw64, db64 = R.conv_wgrad_ref(x, dy, k, s, p)
    ri = hip.rowinfo_nhwc(N, H, W, OH, OW, s, p, k, k, "cuda")
    dw, db = torch.zeros(K, k * k * C, device="cuda"), torch.zeros(K, device="cuda")
    hip.conv2d_wgrad_bf16(x.cuda().to(h16), dy.cuda().to(h16).reshape(-1, K), dw, ri, C, k, k, accumulate=False, db=db)
    assert R.relerr(dw.cpu(), dw64) < 2e-4 and R.relerr(db.cpu(), db64) < 2e-5


@pytest.mark.parametrize("name", list(R.ML_CASES))
def test_fp16_build_multi_level_routes_with_gaussian_operands(name, fp16_build):
    h16 = fp16_build
    from ubteacher import hip
    level_hw, N, C, K = R.ML_CASES[name][:4]
    x, w2, b, res = R.gaussian_ml_operands(name)
    ref = R.ml_fwd_ref(x, w2, level_hw, N, 3, 1, None, b, res, True)
    xd, w16 = x.cuda().to(h16), w2.cuda().to(h16)
    y32 = hip.conv2d_ml_fwd_bf16(xd, w16, level_hw, N, bias=b.cuda(), residual=res.cuda(), k=3, pad=1, relu=True, out_dtype=F32)
    assert R.relerr(y32.cpu(), ref) < 2e-4
    y16 = hip.conv2d_ml_fwd_bf16(xd, w16, level_hw, N, bias=b.cuda(), residual=res.cuda().to(h16), k=3, pad=1, relu=True, out_dtype=h16)
    assert R.close16(y16.cpu(), ref, 2.0 ** -11)


def test_fp16_build_stem_with_gaussian_operands(fp16_build):
    """the image stem and the fused stem + pool on randn weights and the canvases of test_stem_bf16, fp16 build"""
    h16 = fp16_build
    from ubteacher import hip
    g = torch.Generator().manual_seed(7)
    ims = [torch.randn(3, 50, 70, generator=g) * 50 + 100, torch.randn(3, 64, 61, generator=g) * 50 + 100]
    x16, _ = hip.preprocess_images([i.cuda() for i in ims], [103.53, 116.28, 123.675], [57.0, 58.0, 59.0], 32, bf16_stem=True)
    w208 = torch.zeros(64, 208)
    w208[:, :196].view(64, 7, 7, 4)[..., :3] = torch.randn(64, 7, 7, 3, generator=g) * 0.05
    sc, sh = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1
    w16s = hip.stem_weight_image(w208.cuda())
    xs = x16.cpu()
    xs.canvas = x16.canvas
    xi, _ = R.stem_operands(xs, w16s.cpu())
    ref = R.stem_ref(xi, R.stem_taps(w208).half(), sc, sh)
    assert R.relerr(hip.conv2d_stem_fwd_bf16(x16, w16s, sc.cuda(), sh.cuda(), True, F32).cpu(), ref) < 2e-4
    y16 = hip.conv2d_stem_fwd_bf16(x16, w16s, sc.cuda(), sh.cuda(), True, h16)
    assert R.close16(y16.cpu(), ref, 2.0 ** -11)
    # the fused kernel rounds the conv output once and takes exact maxima: within the criterion of the pooled reference
    assert R.close16(hip.stem_pool_fwd_bf16(x16, w16s, sc.cuda(), sh.cuda()).cpu(), R.maxpool_ref(ref), 2.0 ** -11)


def test_fp16_build_wgrad_tower_with_gaussian_operands(fp16_build):
    h16 = fp16_build
    from ubteacher import hip
    level_hw, N, C, K = R.WGRAD_PP_TOWER
    g = torch.Generator().manual_seed(5)
    P = N * sum(h * w for h, w in level_hw)
    x = torch.randn(P, C, generator=g).half().float()
    dy = torch.randn(P, K, generator=g).half().float()
    dw64, db64 = R.ml_wgrad_ref(x, dy, level_hw, N, 3, 1)
    dw, db = torch.zeros(K, 9 * C, device="cuda"), torch.zeros(K, device="cuda")
    hip.conv2d_wgrad_bf16(x.cuda().to(h16), dy.cuda().to(h16), dw, hip.rowinfo_ml(N, level_hw, 1, 3, "cuda"), C, 3, 3, accumulate=False, db=db)
    assert R.relerr(dw.cpu(), dw64) < 2e-4 and R.relerr(db.cpu(), db64) < 2e-5


@pytest.mark.parametrize("name", ["many_splits", "pp_3x3"])
def test_fp16_subnormal_output_gradients_in_the_weight_gradient(name, fp16_build):
    """dy made of fp16 subnormals (what a small gradient is under the loss scale) against normal activations, on the 128-tile and the
    256-tile weight-gradient kernels: exact in fp32, expected unflushed"""
    h16 = fp16_build
    from ubteacher import hip
    N, H, W, C, K, k, s, p = {**R.WGRAD_128, **R.WGRAD_PP}[name]
    g = torch.Generator().manual_seed(16)
    OH, OW = _out_hw(H, W, k, s, p)
    x = R.dyadic((N, H, W, C), 3, 0, g, relu_like=True)
    dy = R.dyadic((N, OH, OW, K), 7, -24, g)
    assert float(dy.abs().max()) < 2.0 ** -14 and torch.equal(dy.to(h16).float(), dy)
    dw64, db64 = R.wgrad_domain(x, dy, k, s, p, -24)
    assert float(dw64.abs().max()) > 0
    dw, db = torch.zeros(K, k * k * C, device="cuda"), torch.zeros(K, device="cuda")
    ri = hip.rowinfo_nhwc(N, H, W, OH, OW, s, p, k, k, "cuda")
    hip.conv2d_wgrad_bf16(x.cuda().to(h16), dy.cuda().to(h16).reshape(-1, K), dw, ri, C, k, k, accumulate=False, db=db)
    assert _eq(dw, dw64, F32) and _eq(db, db64, F32)
