"""The glue kernels of csrc/elementwise.hip at their edges, element by element against tests/elementwise_ref64.py: the stem max pool
(forward and backward), the FPN resampling pair, both zero_interleave2x forms, relu_bwd_scale, add, the three preprocess entries,
frozenbn_fold and the flat-arena updates (ema_axpby, sgd_momentum, sgd_momentum_amp, amp_found_inf) - on both 16-bit builds.

Operands sit on a grid where the expected value is exact (see elementwise_ref64.py), so the assertions are equalities: an fp32 output
equals the fp64 reference, a 16-bit output equals ONE rounding of it.  Only preprocess and the fold carry (stated) bounds.

Every kernel here is a grid-stride loop behind a block cap; one case per family is sized past its cap so that the second trip runs.
Not tested: the host switch of the x8 pool to 64-bit indexing at 2^31 elements - it needs a tensor of at least 34 GB."""
import pytest
import torch

from tests import elementwise_ref64 as R
from ubteacher import hip

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32
F64 = torch.float64
REFUSED = (RuntimeError, AssertionError, ValueError, TypeError)


@pytest.fixture(params=["bf16", "fp16"])
def h16(request):
    """both builds of the library: every call of the test goes to the build whose 16-bit type is returned"""
    hip.set_h16(request.param)
    try:
        yield hip.h16_dtype()
    finally:
        hip.set_h16("bf16")


def D(t, dtype=None):
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def agrees(got, ref64, what=""):
    """got (device tensor) == one rounding of the exact reference to got's type, by value, NaN == NaN"""
    want = R.round16(ref64, got.dtype)
    ok = R.same(got.cpu(), want)
    if not ok:
        bad = ~((got.cpu() == want) | (got.cpu().isnan() & want.isnan()))
        print("%s: %d of %d differ, first at %s" % (what, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist()))
    return ok


def _types(pair, h):
    return {"f": F32, "h": h}[pair[0]], {"f": F32, "h": h}[pair[1]]


# ----------------------------------------------------------------------------------------------------------------------------------
# max pool
@pytest.mark.parametrize("pair", ["ff", "fh", "hh"])          # input type, output type; hh: the x8 kernel at C % 8 == 0, else the generic one
def test_maxpool_forward(h16, pair):
    xdt, ydt = _types(pair, h16)
    for i, shape in enumerate(R.POOL_FWD_SHAPES):
        x = R.pool_input(shape, xdt, i)
        ref = R.maxpool_fwd(x)
        R.assert_exact(ref, x)
        y = hip.maxpool3x3s2(D(x, xdt), out_dtype=ydt)
        assert y.dtype == ydt and tuple(y.shape) == R.pool_out_shape(shape)
        assert agrees(y, ref, "pool %s %s" % (pair, shape,))


@pytest.mark.parametrize("pair", ["ff", "fh", "hh"])
def test_maxpool_forward_keeps_nan(h16, pair):
    """a NaN on the first tap, on the last tap, in a border window and over a whole window is the window's maximum, as in ATen
    (`val > maxval || isnan(val)`), so forward and backward name the same pixel"""
    xdt, ydt = _types(pair, h16)
    x = R.pool_nan_input(xdt, 9)
    ref = R.maxpool_fwd(x)
    assert int(ref.isnan().sum()) >= 8
    assert agrees(hip.maxpool3x3s2(D(x, xdt), out_dtype=ydt), ref, "pool nan " + pair)


def test_maxpool_refused_type_pairs(h16):
    x = torch.zeros(1, 4, 4, 8, device=DEV)
    with pytest.raises(REFUSED):
        hip.maxpool3x3s2(x.to(h16), out_dtype=F32)               # no fp32 pool of a 16-bit tensor
    with pytest.raises(REFUSED):
        hip.maxpool3x3s2_bwd(x, torch.zeros(1, 2, 2, 8, device=DEV, dtype=h16))   # no 16-bit gradient of an fp32 pool
    torch.cuda.synchronize()


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("pair", ["ff", "hh", "hf"])          # type of x, type of dpool / dx: every legal pair
def test_maxpool_backward(h16, pair, relu):
    xdt, gdt = _types(pair, h16)
    for i, shape in enumerate(R.POOL_BWD_SHAPES):
        x, d = R.pool_input(shape, xdt, 20 + i), R.pool_grad(shape, gdt, i)
        ref = R.maxpool_bwd(x, d, relu)
        R.assert_exact(ref, d, d, d, d)
        dx = hip.maxpool3x3s2_bwd(D(x, xdt), D(d, gdt), relu=relu)
        assert dx.dtype == gdt and agrees(dx, ref, "pool bwd %s %s relu=%s" % (pair, shape, relu))


@pytest.mark.parametrize("pair", ["ff", "hh", "hf"])
def test_maxpool_backward_nan_goes_where_aten_sends_it(h16, pair):
    xdt, gdt = _types(pair, h16)
    x = R.pool_nan_input(xdt, 9)
    d = R.pool_grad(tuple(x.shape), gdt, 3)
    for relu in (False, True):
        ref = R.maxpool_bwd(x, d, relu)
        assert agrees(hip.maxpool3x3s2_bwd(D(x, xdt), D(d, gdt), relu=relu), ref, "pool bwd nan %s relu=%s" % (pair, relu))


def test_maxpool_backward_of_equal_taps_goes_to_the_first_tap(h16):
    """a constant input: every existing tap of every window ties, so each window's whole gradient lands on its first existing tap,
    pixel (max(2 oh - 1, 0), max(2 ow - 1, 0)) - the strict `>` of the rule the forward and the backward share; at H = W = 4 window
    (1, 1) has all nine taps.  C = 4 and 8, every legal type pair."""
    for pair in ("ff", "hh", "hf"):
        xdt, gdt = _types(pair, h16)
        for C in (4, 8):
            for HW in (3, 4):
                shape = (1, HW, HW, C)
                x = torch.full(shape, 1.5)
                d = R.pool_grad(shape, gdt, 7)
                want = torch.zeros(shape, dtype=F64)
                for oh in range(d.shape[1]):
                    for ow in range(d.shape[2]):
                        want[0, max(2 * oh - 1, 0), max(2 * ow - 1, 0)] += d[0, oh, ow].double()
                ref = R.maxpool_bwd(x, d, False)
                assert torch.equal(ref, want) and int((d != 0).sum()) > 2 * C
                for relu in (False, True):
                    dx = hip.maxpool3x3s2_bwd(D(x, xdt), D(d, gdt), relu=relu)
                    assert agrees(dx, ref, "pool bwd ties %s %s relu=%s" % (pair, shape, relu))


# ----------------------------------------------------------------------------------------------------------------------------------
# FPN resampling
@pytest.mark.parametrize("kind", ["f", "h"])
def test_upsample_add_and_downsample_sum(h16, kind):
    dt = F32 if kind == "f" else h16
    for i, shape in enumerate(R.LATERAL_SHAPES):
        lat, top = R.lateral_operands(shape, dt, 40 + i)
        ref = R.upsample_add(lat, top)
        R.assert_exact(ref, lat, top)
        assert agrees(hip.upsample2x_add(D(lat, dt), D(top, dt)), ref, "upsample %s" % (shape,))
        ref = R.downsample_sum(lat)
        R.assert_exact(ref, lat, lat, lat, lat)
        assert agrees(hip.downsample2x_sum(D(lat, dt)), ref, "downsample %s" % (shape,))
        ref = R.downsample_sum(lat, top)                                      # accumulate onto a non-zero target
        R.assert_exact(ref, lat, lat, lat, lat, top)
        out = D(top, dt)
        assert hip.downsample2x_sum(D(lat, dt), out=out, accumulate=True) is out
        assert agrees(out, ref, "downsample accumulate %s" % (shape,))
        out = D(top, dt)
        hip.downsample2x_sum(D(lat, dt), out=out, accumulate=False)           # ... and over it
        assert agrees(out, R.downsample_sum(lat), "downsample overwrite %s" % (shape,))


def test_resampling_refuses_odd_sizes(h16):
    for dt in (F32, h16):
        for (H, W) in ((3, 4), (4, 3), (5, 5), (1, 2)):
            g = torch.ones(1, H, W, 4, device=DEV, dtype=dt)
            with pytest.raises(REFUSED):
                hip.downsample2x_sum(g)
            with pytest.raises(REFUSED):
                hip.downsample2x_sum(g, out=torch.zeros(1, H // 2, W // 2, 4, device=DEV, dtype=dt), accumulate=True)
            with pytest.raises(REFUSED):
                hip.upsample2x_add(g, torch.ones(1, H // 2, W // 2, 4, device=DEV, dtype=dt))
    torch.cuda.synchronize()


def test_upsample_add_past_the_block_cap(h16):
    """N H W C / 4 = 1.125 * 2^24 quads against 2^16 blocks of 256 threads: the grid-stride loop makes a second trip.  Operands are
    drawn on the device and compared there with ATen's own add of the repeated tensor - one IEEE add and one rounding, as the kernel."""
    N, H, W, C = 1, 2304, 2048, 16
    assert N * H * W * C // 4 > (1 << 16) * 256
    g = torch.Generator(device=DEV).manual_seed(1)
    lat = (torch.randint(-127, 128, (N, H, W, C), generator=g, device=DEV, dtype=torch.int16).to(F32) / 4).to(h16)
    top = (torch.randint(-127, 128, (N, H // 2, W // 2, C), generator=g, device=DEV, dtype=torch.int16).to(F32) / 4).to(h16)
    got = hip.upsample2x_add(lat, top)
    want = lat + top.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    assert got.dtype == h16 and torch.equal(got, want)
    assert float(want[0, -1].float().abs().max()) > 0


# ----------------------------------------------------------------------------------------------------------------------------------
# zero_interleave2x
def _zi8(src, H, W, mask=None, bits=None, add=None):
    """the 8-channel 16-bit kernel through its C entry (the Python wrapper sends the unmasked, add-free case to the generic kernel)"""
    N, _, _, C = src.shape
    out = torch.empty((N, H, W, C), dtype=src.dtype, device=src.device)
    hip.call("utv2_zero_interleave2x_add_nhwc", hip._p(src), hip._p(mask), hip._p(bits), hip._p(add), hip._p(out), N, H, W, C, hip._stream())
    return out


@pytest.mark.parametrize("kind", ["f", "h"])
def test_zero_interleave_generic_kernel(h16, kind):
    dt = F32 if kind == "f" else h16
    for i, (H, W) in enumerate(R.INTERLEAVE_HW):
        for C in (4, 12):
            src, mask, add = R.interleave_operands(2, H, W, C, dt, 60 + i)
            assert agrees(hip.zero_interleave2x(D(src, dt), H, W), R.zero_interleave(src, H, W), "interleave %s" % ((H, W, C),))
            assert agrees(hip.zero_interleave2x(D(src, dt), H, W, mask=D(mask, dt)), R.zero_interleave(src, H, W, mask),
                          "interleave mask %s" % ((H, W, C),))


def test_zero_interleave_x8_kernel(h16):
    """{no mask, tensor mask, bit plane} x {add, no add}; the mask holds -0.0, negative values and NaN, which all stop the value"""
    for i, (H, W) in enumerate(R.INTERLEAVE_HW):
        for C in (8, 16):
            src, mask, add = R.interleave_operands(2, H, W, C, h16, 60 + i)
            s, m, a = D(src, h16), D(mask, h16), D(add, h16)
            bits = D(R.pack_mask_bits(mask))
            for use_add in (False, True):
                a64, ad = (add, a) if use_add else (None, None)
                ref = R.zero_interleave(src, H, W, None, a64)
                R.assert_exact(ref, src, add)
                assert agrees(_zi8(s, H, W, add=ad), ref, "x8 %s add=%s" % ((H, W, C), use_add))
                ref = R.zero_interleave(src, H, W, mask, a64)
                by_mask = _zi8(s, H, W, mask=m, add=ad)
                assert agrees(by_mask, ref, "x8 mask %s add=%s" % ((H, W, C), use_add))
                by_bits = _zi8(s, H, W, bits=bits, add=ad)
                assert torch.equal(by_bits.view(torch.int16), by_mask.view(torch.int16))      # the same bits as the mask it was packed from
                via = hip.zero_interleave2x(s, H, W, mask_bits=bits, add=ad)                     # and through the wrapper
                assert torch.equal(via.view(torch.int16), by_mask.view(torch.int16))
            assert agrees(hip.zero_interleave2x(s, H, W, mask=m), R.zero_interleave(src, H, W, mask), "wrapper mask")


def test_zero_interleave_x8_refuses_two_masks(h16):
    src, mask, _ = R.interleave_operands(1, 6, 4, 8, h16, 1)
    s, m, bits = D(src, h16), D(mask, h16), D(R.pack_mask_bits(mask))
    out = torch.full((1, 6, 4, 8), 3.0, dtype=h16, device=DEV)
    fn = hip.load().utv2_zero_interleave2x_add_nhwc
    rc = fn(hip._p(s), hip._p(m), hip._p(bits), None, hip._p(out), 1, 6, 4, 8, hip._stream())
    torch.cuda.synchronize()
    assert rc != 0 and bool((out == 3.0).all())
    with pytest.raises(REFUSED):                                   # the generic kernel has neither a bit plane nor an add
        hip.zero_interleave2x(D(src, h16)[..., :4].contiguous(), 6, 4, add=out[..., :4].contiguous())


# ----------------------------------------------------------------------------------------------------------------------------------
# relu_bwd_scale and add
@pytest.mark.parametrize("kind", ["f", "h"])
def test_relu_bwd_scale_masks_and_scales(h16, kind):
    """y present / absent x scale present / absent; y = -0.0 and y = NaN give gradient 0"""
    dt = F32 if kind == "f" else h16
    for (M, C) in ((37, 12), (5, 4), (64, 64)):
        dy, y, sc = R.relu_bwd_operands(M, C, dt, 80)
        for use_y in (False, True):
            for use_sc in (False, True):
                ref = R.relu_bwd_scale(dy, y if use_y else None, sc if use_sc else None)
                R.assert_exact(ref, dy * 3)
                got = hip.relu_bwd_scale(D(dy, dt), D(y, dt) if use_y else None, D(sc) if use_sc else None)
                assert got.dtype == dt and agrees(got, ref, "relu_bwd_scale %s y=%s scale=%s" % ((M, C), use_y, use_sc))
                if use_y:
                    assert bool((got.cpu()[y.isnan() | (y == 0)] == 0).all())


def test_relu_bwd_scale_past_the_block_cap(h16):
    """M C / 4 = 1 050 000 quads against 4096 blocks of 256 threads: a second trip whose stride (2^20) is no multiple of the scale's
    period (C / 4 = 3), so the quad of the scale moves on between the trips.  Compared on the first and last 64 rows plus every 97th."""
    M, C = 350000, 12
    assert M * C // 4 > 4096 * 256 and (4096 * 256) % (C // 4) != 0
    dy, y, sc = R.relu_bwd_operands(M, C, F32, 81)
    got = hip.relu_bwd_scale(D(dy), D(y), D(sc)).cpu()
    rows = torch.unique(torch.cat([torch.arange(64), torch.arange(M - 64, M), torch.arange(0, M, 97)]))
    ref = R.relu_bwd_scale(dy[rows], y[rows], sc)
    R.assert_exact(ref, dy[rows] * 3)
    assert R.same(got[rows], R.round16(ref, F32))


def test_add(h16):
    g = torch.Generator().manual_seed(2)
    for n in (1, 3, (1 << 20) * 4 + 3):                             # the last one: five trips of the 4096-block grid
        a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
        da, db = D(a), D(b)
        got = hip.add(da, db)
        assert torch.equal(got, da + db)                            # one IEEE add: ATen's is the same operation
        assert torch.equal(got.cpu(), torch.from_numpy(a.numpy() + b.numpy()))
        out = torch.empty_like(da)
        assert hip.add(da, db, out=out) is out and torch.equal(out, got)


# ----------------------------------------------------------------------------------------------------------------------------------
# flat-arena updates
ARENA_N = [1, 2, 3, 4, 5, 7, 1021, 4 * (1 << 20) + 3, 4 * (1 << 20) + 7]     # the last: a vectorised element past the first trip, and a tail
SENTINEL = 3.0


def _mirror(n, h16, on):
    return torch.full((n,), SENTINEL, dtype=h16, device=DEV) if on else None


def _mirror_ok(mirror, new32):
    """bit-equal to one rounding of the new fp32 value (fp16: values beyond 65504 become inf, tiny ones subnormals)"""
    return R.same(mirror.cpu(), R.round16(new32.double(), mirror.dtype))


@pytest.mark.parametrize("mirror", [False, True])
def test_ema_axpby(h16, mirror):
    for n in ARENA_N:
        t, s, _ = R.arena_operands(n, n % 1000, fp16_edges=True)
        for keep in (0.9996, 0.5):
            want = R.ema_axpby(t, s, keep)
            dt_, ds, mi = D(t), D(s), _mirror(n, h16, mirror)
            hip.ema_axpby(dt_, ds, keep, mirror16=mi)
            assert torch.equal(dt_.cpu(), want) and torch.equal(ds.cpu(), s), "n = %d" % n
            assert mi is None or _mirror_ok(mi, want), "mirror, n = %d" % n
    h = R.round16(want.double(), torch.float16)
    assert bool(torch.isinf(h).any()) and bool(((h != 0) & (h.float().abs() < 6.1e-5)).any())      # the fp16 edges are in play


def test_ema_axpby_refuses_a_misaligned_teacher(h16):
    buf = torch.zeros(17, device=DEV)
    with pytest.raises(REFUSED):
        hip.ema_axpby(buf[1:], torch.ones(16, device=DEV), 0.5)      # a view offset by one float: not 16-byte aligned
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0


@pytest.mark.parametrize("zero_grad", [False, True])
@pytest.mark.parametrize("mirror", [False, True])
def test_sgd_momentum(h16, mirror, zero_grad):
    lr, mo, wd, gs = 0.01, 0.9, 1e-4, 0.125
    for n in ARENA_N:
        p, g, m = R.arena_operands(n, 1 + n % 1000, fp16_edges=True)
        pn, mn = R.sgd_momentum(p, g, m, lr, mo, wd, gs)
        dp, dg, dm, mi = D(p), D(g), D(m), _mirror(n, h16, mirror)
        hip.sgd_momentum(dp, dg, dm, lr, mo, wd, grad_scale=gs, zero_grad=zero_grad, mirror16=mi)
        assert torch.equal(dp.cpu(), pn) and torch.equal(dm.cpu(), mn), "n = %d" % n
        assert torch.equal(dg.cpu(), torch.zeros(n) if zero_grad else g), "grad, n = %d" % n
        assert mi is None or _mirror_ok(mi, pn), "mirror, n = %d" % n


@pytest.mark.parametrize("mirror", [False, True])
def test_sgd_momentum_amp(h16, mirror):
    lr, mo, wd, gs, loss_scale = 0.01, 0.9, 1e-4, 0.25, 1024.0
    for n in ARENA_N:
        p, g, m = R.arena_operands(n, 2 + n % 1000, fp16_edges=True)
        g = g * 37.0                                                   # a scaled gradient: g / 1024 is not the plain test's value
        for flag in (0.0, 1.0):
            st = torch.tensor([loss_scale, flag, 5.0])
            pn, mn = R.sgd_momentum_amp(p, g, m, lr, mo, wd, gs, st)
            dp, dg, dm, ds, mi = D(p), D(g), D(m), D(st), _mirror(n, h16, mirror)
            hip.sgd_momentum_amp(dp, dg, dm, lr, mo, wd, gs, ds, mirror16=mi)
            assert torch.equal(dp.cpu(), pn) and torch.equal(dm.cpu(), mn), "n = %d flag = %g" % (n, flag)
            assert torch.equal(dg.cpu(), g) and torch.equal(ds.cpu(), st)
            if flag:                                                   # found_inf: nothing changes, the mirror included
                assert torch.equal(pn, p) and torch.equal(mn, m)
                assert mi is None or bool((mi == SENTINEL).all())
            else:
                assert mi is None or _mirror_ok(mi, pn), "mirror, n = %d" % n


def test_amp_found_inf(h16):
    """one inf, -inf or NaN at index 0, at the last vectorised element, at each tail index and one index past the first grid-stride trip
    (4096 blocks x 256 threads x 4 floats) sets the flag; finite values up to +-3.4e38 and subnormals do not; nothing clears it"""
    trip = 4096 * 256 * 4
    g0 = torch.Generator().manual_seed(3)
    for n in (1, 2, 3, 5, 6, 7, 4099, 4 * (1 << 20) + 3, 4 * (1 << 20) + 7):
        n4 = n // 4
        pos = {0, n - 1} | set(range(4 * n4, n))
        if n4:
            pos.add(4 * n4 - 1)
        if n > trip:
            pos.add(trip)
        g = torch.randn(n, generator=g0)
        g[::5] = 3.4e38
        g[1::5] = -3.4e38
        g[2::5] = 1e-45
        g[3::5] = -1e-40
        assert not R.found_inf(g)
        dg = D(g)
        st = torch.tensor([1024.0, 0.0, 7.0], device=DEV)
        hip.amp_found_inf(dg, st)
        assert st.tolist() == [1024.0, 0.0, 7.0], "finite gradients, n = %d" % n
        for p in sorted(pos):
            for bad in (float("inf"), float("-inf"), float("nan")):
                keep = float(g[p])
                dg[p] = bad
                st = torch.tensor([1024.0, 0.0, 7.0], device=DEV)
                hip.amp_found_inf(dg, st)
                assert st.tolist() == [1024.0, 1.0, 7.0], "n = %d: %s at %d not seen" % (n, bad, p)
                dg[p] = keep
        st = torch.tensor([1024.0, 1.0, 7.0], device=DEV)
        hip.amp_found_inf(dg, st)                                     # finite again: the flag stays set
        assert st.tolist() == [1024.0, 1.0, 7.0]


EDGE_N = 64
EDGE_SEGMENTS = [(0, 1), (1, 3), (3, 6), (6, 10), (12, 17), (17, 23), (23, 30)]    # lengths 1..7; the tail [30, 64) and [10, 12) are gaps


@pytest.mark.parametrize("mirror", [False, True])
def test_flat_sgd_equals_segmented_sgd_at_chunk_edges(h16, mirror):
    """one arena of 64 floats cut into chunks of 1..7 elements that start at 0, 1, 2 and 3 mod 4 (heads of 0..3 elements, bodies of 0 or 1
    quads, tails of 0..3): the segmented kernel's single-lane head / tail and its 16-byte body give the bytes of the flat kernel - both
    call one update - and of the one-rounding-per-operation reference; plain, under AMP, and skipped under AMP with found_inf set"""
    from ubteacher.params import SegmentTable
    assert [e - s for s, e in EDGE_SEGMENTS] == list(range(1, 8)) and {s % 4 for s, _ in EDGE_SEGMENTS} == {0, 1, 2, 3}
    lr, mo, wd, gs = 0.01, 0.9, 1e-4, 0.25
    tb = SegmentTable(EDGE_N, EDGE_SEGMENTS, [(0, EDGE_N, wd)], DEV)
    g0 = torch.Generator().manual_seed(11)
    p, g, m = (R.grid((EDGE_N,), h16, g0, zero_frac=0.0) for _ in range(3))
    bits16 = lambda t: None if t is None else t.view(torch.int16)
    for state in (None, [1024.0, 0.0, 0.0], [1024.0, 1.0, 0.0]):
        st = None if state is None else torch.tensor(state, device=DEV)
        sp, sg, sm, smi = D(p), D(g), D(m), _mirror(EDGE_N, h16, mirror)
        hip.sgd_segmented(sp, sg, sm, tb, lr, mo, gs, None, 1.0, False, st, mirror16=smi)
        fp, fg, fm, fmi = D(p), D(g), D(m), _mirror(EDGE_N, h16, mirror)
        if st is None:
            hip.sgd_momentum(fp, fg, fm, lr, mo, wd, grad_scale=gs, zero_grad=False, mirror16=fmi)
            pn, mn = R.sgd_momentum(p, g, m, lr, mo, wd, gs)
        else:
            hip.sgd_momentum_amp(fp, fg, fm, lr, mo, wd, gs, st, mirror16=fmi)
            pn, mn = R.sgd_momentum_amp(p, g, m, lr, mo, wd, gs, torch.tensor(state))
        for what, a, b in (("p", sp, fp), ("m", sm, fm)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (what, state)
        assert torch.equal(sg.cpu(), g) and torch.equal(fg.cpu(), g)
        assert torch.equal(sp.cpu().view(torch.int32), pn.view(torch.int32)) and torch.equal(sm.cpu().view(torch.int32), mn.view(torch.int32)), state
        if mirror:
            assert torch.equal(bits16(smi), bits16(fmi)), state
        if state is not None and state[1]:                             # found_inf: all three arrays stay untouched
            assert torch.equal(sp.cpu(), p) and torch.equal(sm.cpu(), m) and torch.equal(fp.cpu(), p) and torch.equal(fm.cpu(), m)
            assert not mirror or (bool((smi == SENTINEL).all()) and bool((fmi == SENTINEL).all()))
        else:
            assert not torch.equal(pn, p) and not torch.equal(mn, m)
            assert not mirror or _mirror_ok(smi, pn)


# ----------------------------------------------------------------------------------------------------------------------------------
# preprocess (all three C entries through hip.preprocess_images)
def _pre_check(got, ref64, what):
    """fp32 layout: two roundings, |got - ref64| <= 1 ulp32(ref64).  16-bit layout: got lies between the roundings of ref64 -+ 1 ulp32.
    Zeros of the reference (the canvas beyond an image, the border, channel 3) are exact zeros.  Returns the largest error in ulp32
    (fp32 layout) or the share of elements that are not the rounding of ref64 itself (16-bit layout).
    Observed on an MI355X, both builds: at most 0.500 ulp32; every 16-bit element is the rounding of the fp64 value."""
    g = got.cpu()
    assert tuple(g.shape) == tuple(ref64.shape), (what, g.shape, ref64.shape)
    u = R.ulp32(ref64)
    assert bool((g[ref64 == 0] == 0).all()) and float(g[..., 3].abs().max()) == 0.0, what
    if g.dtype == F32:
        err = float(((g.double() - ref64).abs() / u).max())
        print("preprocess %s: max error %.3f ulp32" % (what, err))
        assert err <= 1.0, what
        return err
    lo, hi = R.round16(ref64 - u, g.dtype, exact=False), R.round16(ref64 + u, g.dtype, exact=False)
    off = float((g != R.round16(ref64, g.dtype, exact=False)).double().mean())
    print("preprocess %s: %.4f %% of the elements are not the rounding of the fp64 value" % (what, 100 * off))
    assert bool(((g >= lo) & (g <= hi)).all()), what
    return off


PRE_BATCHES = {
    "u8": ([(37, 50), (40, 45)], ["u8", "u8"], 32),
    "f32": ([(37, 50), (40, 45)], ["f32", "f32"], 32),
    "canvas_and_1x1": ([(64, 64), (1, 1)], ["u8", "u8"], 32),        # an image equal to the canvas next to a 1 x 1 image
    "mixed": ([(20, 30), (32, 17), (5, 64)], ["u8", "f32", "u8"], 32),   # mixed source types: one launch per image
    "tiny33": ([(1 + i % 4, 1 + i % 5) for i in range(33)], ["u8", "f32"] * 16 + ["u8"], 4),   # more than 32 images: one launch per image
    "tiny33_u8": ([(1 + i % 4, 1 + i % 5) for i in range(33)], ["u8"] * 33, 4),
    "batch32_f32": ([(1 + i % 7, 2 + i % 6) for i in range(32)], ["f32"] * 32, 8),            # the largest one-launch batch
}


@pytest.mark.parametrize("name", sorted(PRE_BATCHES))
def test_preprocess(h16, name):
    sizes, kinds, div = PRE_BATCHES[name]
    ims = R.images_of(sizes, kinds, 5)
    dims = [D(i) for i in ims]
    x4, got_sizes = hip.preprocess_images(dims, R.PRE_MEAN, R.PRE_STD, div)
    assert got_sizes == sizes and x4.dtype == F32
    _pre_check(x4, R.preprocess(ims, R.PRE_MEAN, R.PRE_STD, div), name + " fp32")
    x16, got_sizes = hip.preprocess_images(dims, R.PRE_MEAN, R.PRE_STD, div, bf16_stem=True)
    assert got_sizes == sizes and x16.dtype == h16 and x16.canvas == R.canvas_of(ims, div)
    _pre_check(x16, R.preprocess_pad(ims, R.PRE_MEAN, R.PRE_STD, div), name + " stem")


def test_preprocess_odd_width_takes_the_fp32_path(h16):
    ims = R.images_of([(5, 7), (4, 3)], ["u8", "f32"], 6)
    out, sizes = hip.preprocess_images([D(i) for i in ims], R.PRE_MEAN, R.PRE_STD, 1, bf16_stem=True)
    assert out.dtype == F32 and tuple(out.shape) == (2, 5, 7, 4) and sizes == [(5, 7), (4, 3)]
    _pre_check(out, R.preprocess(ims, R.PRE_MEAN, R.PRE_STD, 1), "odd width")


@pytest.mark.parametrize("kinds", [["u8", "u8"], ["u8", "f32"]])          # the batched launch, the per-image launches
def test_preprocess_rewrites_the_cached_stem_buffer(h16, kinds):
    """the stem's input buffer is cached per (batch, canvas): after a batch that fills the canvas, a batch of smaller images with the
    same key must leave exact zeros beyond each image and in the whole border"""
    full = R.images_of([(32, 32), (32, 32)], kinds, 7)
    a, _ = hip.preprocess_images([D(i) for i in full], R.PRE_MEAN, R.PRE_STD, 32, bf16_stem=True)
    assert int((a[:, 3:35, 3:35, :3] != 0).sum()) > 6000                # the canvas is full
    small = R.images_of([(20, 30), (1, 1)], kinds, 8)
    b, _ = hip.preprocess_images([D(i) for i in small], R.PRE_MEAN, R.PRE_STD, 32, bf16_stem=True)
    assert b.data_ptr() == a.data_ptr()                              # the same buffer
    ref = R.preprocess_pad(small, R.PRE_MEAN, R.PRE_STD, 32)
    _pre_check(b, ref, "cached stem buffer")
    g = b.cpu()
    assert float(g[0, 3 + 20:, :, :].abs().max()) == 0.0 and float(g[0, :, 3 + 30:, :].abs().max()) == 0.0
    assert float(g[1, 4:, :, :].abs().max()) == 0.0 and float(g[1, :, 4:, :].abs().max()) == 0.0
    assert float(g[:, :3].abs().max()) == 0.0 and float(g[:, :, :3].abs().max()) == 0.0


def test_per_image_stem_path_equals_the_batched_path(h16):
    """the first 32 of 33 tiny images in one batched launch, then all 33 one launch each (more than 32 images), through the same
    kernel: slots 0..31 are byte-identical, the zero border (3 rows above, 3 below, 3 columns left, 5 right) included"""
    sizes, kinds, div = PRE_BATCHES["tiny33_u8"]
    dims = [D(i) for i in R.images_of(sizes, kinds, 5)]
    batched, _ = hip.preprocess_images(dims[:32], R.PRE_MEAN, R.PRE_STD, div, bf16_stem=True)
    each, _ = hip.preprocess_images(dims, R.PRE_MEAN, R.PRE_STD, div, bf16_stem=True)
    assert batched.canvas == each.canvas == (4, 8) and batched.data_ptr() != each.data_ptr()
    assert tuple(batched.shape) == (32, 10, 16, 4) and tuple(each.shape) == (33, 10, 16, 4)
    assert torch.equal(batched.view(torch.int16), each[:32].view(torch.int16))
    inner = each[:, 3:7, 3:11]
    assert int((inner != 0).sum()) == 3 * sum(h * w for h, w in sizes)      # every pixel of every image, nothing beyond it
    border = each.clone()
    border[:, 3:7, 3:11] = 0
    assert not bool(border.view(torch.int16).any())


# ----------------------------------------------------------------------------------------------------------------------------------
# FrozenBN fold
def test_frozenbn_fold(h16):
    """scale within 3 ulp32 of the fp64 value (four rounded operations - add, sqrt, divide, multiply - of which about 2.25 ulp
    propagate); |shift - ref| <= 4 * 2^-24 * (|b| + |mean * scale|); var from 0 to 1e6.
    Observed on an MI355X, both builds: scale at most 1.69 ulp32, shift at most 0.74 of its bound."""
    g = torch.Generator().manual_seed(4)
    worst_scale = worst_shift = 0.0
    for n in (1, 255, 256, 257):
        w, b, mean = (torch.randn(n, generator=g) for _ in range(3))
        var = torch.pow(10.0, torch.rand(n, generator=g) * 12 - 6)
        var[0] = 0.0
        var[-1] = 1e6
        if n > 2:
            var[1] = 1e-30
        sc = torch.full((n + 1,), SENTINEL, device=DEV)
        sh = torch.full((n + 1,), SENTINEL, device=DEV)
        hip.frozenbn_fold(D(w), D(b), D(mean), D(var), sc, sh, eps=1e-5)
        assert float(sc[n]) == SENTINEL and float(sh[n]) == SENTINEL                    # nothing past n
        rsc, rsh = R.frozenbn_fold(w, b, mean, var, 1e-5)
        e_sc = (sc[:n].cpu().double() - rsc).abs() / R.ulp32(rsc)
        bound = 4 * 2.0 ** -24 * (b.double().abs() + (mean.double() * rsc).abs())
        e_sh = (sh[:n].cpu().double() - rsh).abs() / bound
        worst_scale, worst_shift = max(worst_scale, float(e_sc.max())), max(worst_shift, float(e_sh.max()))
        print("frozenbn_fold n = %d: scale %.3f ulp32, shift %.3f of its bound" % (n, float(e_sc.max()), float(e_sh.max())))
        assert float(e_sc.max()) <= 3.0 and float(e_sh.max()) <= 1.0
