"""The BatchNorm + ReLU kernels of the FCOS towers (csrc/batchnorm.hip) through their wrappers, against tests/bn_ref64.py (torch's batch
norm in float64 on the CPU, autograd for the backward).

Shapes: C = 256 and 512 (the paired towers' width); L = 5 levels with one and with two statistic sets per level; set sizes 2, 63, 64, 65
and 4097 rows (stage 1 sums chunks of 64 rows: a set smaller than a wave, one chunk exactly, one row more, 65 chunks for stage 2).
Channel 1 has mean 300 and standard deviation 0.05 (cancellation), channel 2 is constant (var = 0), channel 3 holds -1 / 0 / +1 in equal
numbers with beta = 0, so that its mean is exactly 0 and x * scale + shift is exactly 0 where x is 0 (the mask rule: no gradient there).

Tolerances.
  fp32 mode: the yardstick is torch's own fp32 CPU batch norm (forward and backward) against the same float64 result on the same inputs.
    Per output the kernel's maximum error may be at most 4 x the yardstick's (the summation order differs), with a floor of 2 fp32 ulps
    at the output's magnitude (its largest reference value).
  16-bit modes (both libraries): the float64 restatement is fed the 16-bit inputs as stored; every y and dx element may differ from the
    float64 value rounded to the 16-bit type by at most one representable value.  Statistics and parameter gradients: the fp32 rule.
Every figure is printed before it is asserted (pytest -s shows them)."""
import functools
import types

import pytest
import torch

from tests import bn_ref64 as R

pytestmark = pytest.mark.gpu

SIZES = [2, 63, 64, 65, 4097]
L = len(SIZES)
OUTPUTS = ("y", "mean", "rstd", "running_mean", "running_var", "dx", "dgamma", "dbeta")


def make_sets(nper):
    sets, r = [], 0
    for l in range(L):
        for k in range(nper):
            n = SIZES[(l + 2 * k) % L]
            sets.append((r, n, l))
            r += n
    return sets, r


@functools.lru_cache(maxsize=None)
def inputs(C, nper):
    g = torch.Generator().manual_seed(100 * nper + C)
    sets, P = make_sets(nper)
    x = torch.randn(P, C, generator=g) * 1.5 + 0.3
    x[:, 1] = 300.0 + 0.05 * torch.randn(P, generator=g)
    x[:, 2] = 1.5
    for r0, n, _ in sets:
        v = torch.zeros(n)
        v[:n // 3], v[n // 3:2 * (n // 3)] = 1.0, -1.0
        x[r0:r0 + n, 3] = v[torch.randperm(n, generator=g)]
    dy = torch.randn(P, C, generator=g)
    ga, be = torch.rand(L, C, generator=g) + 0.5, torch.randn(L, C, generator=g) * 0.1
    be[:, 3] = 0.0
    rm, rv = torch.randn(L, C, generator=g) * 0.1, torch.rand(L, C, generator=g) + 0.5
    return dict(sets=sets, P=P, x=x, dy=dy, ga=ga, be=be, rm=rm, rv=rv)


def select(kind):
    from ubteacher import hip, ops
    ops.set_precision(kind)
    return torch.float32 if kind == "fp32" else hip.h16_dtype()


def run_kernels(c, x, dy, training=True):
    """the whole op through the wrappers -> dict of CPU tensors named as bn_ref64.bn_relu names them"""
    from ubteacher import hip
    dev = "cuda"
    st = hip.BnSets(c["sets"], L)
    ga, be, rm, rv = (c[k].to(dev).clone() for k in ("ga", "be", "rm", "rv"))
    xd, dyd = x.to(dev), dy.to(dev)
    mom = hip.bn_stats(xd, st) if training else None
    mean, rstd, scale = hip.bn_finalize(mom, ga, rm, rv, st, R.EPS, R.MOMENTUM, training=training)
    y = hip.bn_apply_relu(xd, mean, scale, be, st)
    out = dict(y=y, mean=mean, rstd=rstd, running_mean=rm, running_var=rv)
    if training:
        dga, dbe = torch.zeros_like(ga), torch.zeros_like(be)
        sums = hip.bn_bwd_sums(dyd, y, xd, mean, rstd, st)
        out.update(dx=hip.bn_bwd_apply(dyd, y, xd, mean, rstd, ga, sums, dga, dbe, st), dgamma=dga, dbeta=dbe)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def check_fp32_rule(name, got, ref, yard, tag):
    ref = ref.double()
    err, yerr = float((got.double() - ref).abs().max()), float((yard.double() - ref).abs().max())
    floor = 2 * R.ulp32(float(ref.abs().max()))
    print("%s %-12s kernel err %.3e  torch fp32 err %.3e  ratio %.3g  floor %.3e" % (tag, name, err, yerr, err / yerr if yerr else float("inf"), floor))
    assert err <= max(4 * yerr, floor), (tag, name, err, yerr, floor)


def check_16bit_rule(name, got, ref, dt, tag):
    steps = R.ulp_steps16(got, ref.to(dt))
    print("%s %-12s elements one 16-bit value off: %d of %d, worst %d" % (tag, name, int((steps == 1).sum()), steps.numel(), int(steps.max())))
    assert int(steps.max()) <= 1, (tag, name, int(steps.max()))


@pytest.mark.parametrize("kind", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("nper", [1, 2])
@pytest.mark.parametrize("C", [256, 512])
def test_training_forward_backward_against_fp64(C, nper, kind):
    c = inputs(C, nper)
    dt = select(kind)
    x, dy = c["x"].to(dt), c["dy"].to(dt)           # the values as stored
    got = run_kernels(c, x, dy)
    again = run_kernels(c, x, dy)
    for k in OUTPUTS:
        assert torch.equal(got[k], again[k]), "two runs differ in %s" % k
    ref = R.bn_relu(x, c["ga"], c["be"], c["rm"], c["rv"], c["sets"], dy=dy)
    yard = R.bn_relu(x, c["ga"], c["be"], c["rm"], c["rv"], c["sets"], dy=dy, dtype=torch.float32)
    tag = "[C=%d sets/level=%d %s]" % (C, nper, kind)
    z = (c["x"][:, 3] == 0)
    assert bool((ref["y"][z, 3] == 0).all()) and bool((got["y"][z, 3] == 0).all()), "channel 3: y is exactly 0 where x is 0"
    for k in OUTPUTS:
        if kind != "fp32" and k in ("y", "dx"):
            check_16bit_rule(k, got[k], ref[k], dt, tag)
        else:
            check_fp32_rule(k, got[k], ref[k], yard[k], tag)
    # the input classes on their own (the figures DESIGN.md quotes): cancellation, constant and exact-zero channels
    if kind == "fp32":
        for ch, label in ((1, "mean300"), (2, "constant"), (3, "exactzero")):
            for k in ("y", "dx"):
                check_fp32_rule("%s/%s" % (k, label), got[k][:, ch], ref[k][:, ch], yard[k][:, ch], tag)


@pytest.mark.parametrize("kind", ["fp32", "bf16", "fp16"])
def test_eval_mode_uses_the_running_statistics_and_writes_none(kind):
    c = inputs(256, 2)
    dt = select(kind)
    x = c["x"].to(dt)
    got = run_kernels(c, x, c["dy"].to(dt), training=False)
    ref = R.bn_relu(x, c["ga"], c["be"], c["rm"], c["rv"], c["sets"], training=False)
    yard = R.bn_relu(x, c["ga"], c["be"], c["rm"], c["rv"], c["sets"], training=False, dtype=torch.float32)
    assert torch.equal(got["running_mean"], c["rm"]) and torch.equal(got["running_var"], c["rv"])
    tag = "[eval %s]" % kind
    if kind == "fp32":
        check_fp32_rule("y", got["y"], ref["y"], yard["y"], tag)
    else:
        check_16bit_rule("y", got["y"], ref["y"], dt, tag)
    for k in ("mean", "rstd"):
        check_fp32_rule(k, got[k], ref[k], yard[k], tag)


@pytest.mark.parametrize("kind", ["fp32", "bf16", "fp16"])
def test_split_entry_points_combine_to_the_whole_batch(kind):
    """two "ranks" hold half of every level's rows: their moments are averaged and their backward sums added on the host in float64 (the
    SyncBN rule), finalize / bwd_apply take them with count_mul = 2 -> BatchNorm over the whole batch, with the BIASED running variance;
    the ranks' parameter gradients (each the mean of the ranks' sums) add up to the whole batch's"""
    from ubteacher import hip
    dt = select(kind)
    C, halves = 256, [2, 63, 64, 65, 4097]
    g = torch.Generator().manual_seed(7)
    P = sum(halves)
    xs = [(torch.randn(P, C, generator=g) * (1 + r) + 0.5 * r).to(dt) for r in range(2)]
    dys = [torch.randn(P, C, generator=g).to(dt) for _ in range(2)]
    ga, be = torch.rand(L, C, generator=g) + 0.5, torch.randn(L, C, generator=g) * 0.1
    rm, rv = torch.randn(L, C, generator=g) * 0.1, torch.rand(L, C, generator=g) + 0.5
    half_sets, whole_sets, r0, w0, order = [], [], 0, 0, []
    for l, n in enumerate(halves):
        half_sets.append((r0, n, l))
        whole_sets.append((w0, 2 * n, l))
        order.append((r0, n))
        r0, w0 = r0 + n, w0 + 2 * n
    whole = lambda ts: torch.cat([torch.cat([t[a:a + n] for t in ts]) for a, n in order])      # per level: rank 0's rows, then rank 1's
    ref = R.bn_relu(whole(xs), ga, be, rm, rv, whole_sets, dy=whole(dys), biased_running=True)
    yard = R.bn_relu(whole(xs), ga, be, rm, rv, whole_sets, dy=whole(dys), biased_running=True, dtype=torch.float32)
    st = hip.BnSets(half_sets, L)
    dev = "cuda"
    xd, dyd = [t.to(dev) for t in xs], [t.to(dev) for t in dys]
    gad, bed = ga.to(dev), be.to(dev)
    moments = sum(hip.bn_stats(t, st).cpu() for t in xd) / 2          # float64 on the host
    outs = []
    for r in range(2):
        rmd, rvd = rm.to(dev).clone(), rv.to(dev).clone()
        mean, rstd, scale = hip.bn_finalize(moments.to(dev), gad, rmd, rvd, st, R.EPS, R.MOMENTUM, count_mul=2, biased_running=True)
        outs.append(dict(y=hip.bn_apply_relu(xd[r], mean, scale, bed, st), mean=mean, rstd=rstd, rm=rmd, rv=rvd))
    sums = sum(hip.bn_bwd_sums(dyd[r], outs[r]["y"], xd[r], outs[r]["mean"], outs[r]["rstd"], st).cpu() for r in range(2)).to(dev)
    dga, dbe = torch.zeros_like(gad), torch.zeros_like(bed)
    dxs = [hip.bn_bwd_apply(dyd[r], outs[r]["y"], xd[r], outs[r]["mean"], outs[r]["rstd"], gad, sums, dga, dbe, st, count_mul=2) for r in range(2)]
    torch.cuda.synchronize()
    got = dict(y=whole([o["y"].cpu() for o in outs]), dx=whole([t.cpu() for t in dxs]), mean=outs[0]["mean"].cpu(), rstd=outs[0]["rstd"].cpu(),
               running_mean=outs[1]["rm"].cpu(), running_var=outs[1]["rv"].cpu(), dgamma=dga.cpu(), dbeta=dbe.cpu())
    tag = "[split %s]" % kind
    for k in OUTPUTS:
        if kind != "fp32" and k in ("y", "dx"):
            check_16bit_rule(k, got[k], ref[k], dt, tag)
        else:
            check_fp32_rule(k, got[k], ref[k], yard[k], tag)
    # the unbiased rule would have given another running variance: the two differ by the factor n / (n - 1), largest for the 4-row set
    unb = R.bn_relu(whole(xs), ga, be, rm, rv, whole_sets)["running_var"]
    assert float((unb[0] - ref["running_var"][0]).abs().max()) > 1e-3


def test_one_row_training_set_raises_before_any_launch():
    from ubteacher import hip, ops
    select("fp32")
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        hip.BnSets([(0, 1, 0)], 1).check_training()
    hip.BnSets([(0, 1, 0)], 1).check_training(count_mul=2)      # two ranks of one row each: two values per channel
    C = 8
    h = lambda v: types.SimpleNamespace(t=torch.full((1, C), v, device="cuda"), g=torch.zeros((1, C), device="cuda"))
    bn = ops.BatchNormReLU(h(1.0), h(0.0), h(0.0), h(1.0), ops.HostCounter())
    bn.count_calls = True
    x =torch.full((1, C), float("nan"), device="cuda")       # never read
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        bn(x, ops.LevelMeta(1, [(1, 1)]))
    assert float(bn.running_mean.t.abs().max()) == 0.0 and bn.counter.value == 0
    bn.training = False                                       # eval mode normalises one row with the running statistics
    assert tuple(bn(torch.ones((1, C), device="cuda"), ops.LevelMeta(1, [(1, 1)])).shape) == (1, C)


BN_ENTRIES = ("stats_partial", "reduce", "finalize", "apply_relu", "bwd_partial", "bwd_apply")
BN_TILE_ENTRIES = ("stats_partial", "apply_relu", "bwd_partial", "bwd_apply")        # the entries that walk the [P, C] activation


def bn_raw(entry, t, sets, nsets=None, P=67, C=8, nlevels=2, count_mul=1, mode=0, **ptr):
    """return code of the raw entry utv2_bn_<entry> on the tensors of `t` (a name in `ptr` replaces that tensor's pointer: an int or None)"""
    import ctypes
    from ubteacher import hip
    p = lambda name: ptr[name] if name in ptr else t[name].data_ptr()
    row0, rows, level = (ctypes.cast(hip._iarr([s[k] for s in sets]), hip.c_p) for k in range(3))
    n, s = len(sets) if nsets is None else nsets, hip._stream()
    args = dict(
        stats_partial=lambda: (p("x"), 0, p("partial"), P, C, n, row0, rows, s),
        reduce=lambda: (p("partial"), p("out"), C, n, rows, 0, s),
        finalize=lambda: (p("out"), p("gamma"), p("rm"), p("rv"), p("mean"), p("rstd"), p("scale"), C, nlevels, n, rows, level, R.EPS, R.MOMENTUM,
                          mode, count_mul, 0, s),
        apply_relu=lambda: (p("x"), p("y"), 0, p("mean"), p("scale"), p("beta"), P, C, nlevels, n, row0, rows, level, s),
        bwd_partial=lambda: (p("dy"), p("y"), p("x"), 0, p("mean"), p("rstd"), p("partial"), P, C, n, row0, rows, s),
        bwd_apply=lambda: (p("dy"), p("y"), p("x"), p("dx"), 0, p("mean"), p("rstd"), p("gamma"), p("out"), p("dgamma"), p("dbeta"), P, C, nlevels,
                           n, row0, rows, level, count_mul, s))[entry]()
    return getattr(hip.load(), "utv2_bn_" + entry)(*args)


def test_argument_gate_rejects_without_launching():
    """every bad argument of the list gives UTV2_EARG (-1000) from every entry it concerns and nothing is launched (all outputs keep
    their fill); one well-formed call per entry returns 0.  What the entries accept although it looks odd is recorded at the end:
    reduce and finalize take any C >= 1 (they touch no quads), a one-row set is fine in eval mode and with count_mul = 2."""
    from ubteacher import hip
    select("fp32")
    FILL = -7.0
    sets, P, C, Lv = [(0, 65, 0), (65, 2, 1)], 67, 8, 2          # three chunks
    f32 = lambda *s: torch.full(s, FILL, device="cuda")
    f64 = lambda *s: torch.full(s, FILL, dtype=torch.float64, device="cuda")
    t = dict(x=f32(P + 1, C), dy=f32(P + 1, C), y=f32(P + 1, C), dx=f32(P + 1, C),      # a spare row: the shifted pointer stays inside
             partial=f64(3, 2, C), out=f64(2, 2, C), mean=f64(2, C), rstd=f64(2, C), scale=f64(2, C),
             gamma=f32(Lv, C), beta=f32(Lv, C), rm=f32(Lv, C), rv=f32(Lv, C), dgamma=f32(Lv, C), dbeta=f32(Lv, C))
    bad = [
        ("nsets 0", BN_ENTRIES, dict(nsets=0)),
        ("nsets 17", BN_ENTRIES, dict(sets=[(2 * i, 2, 0) for i in range(17)])),
        ("a set of 0 rows", BN_ENTRIES, dict(sets=[(0, 65, 0), (65, 0, 1)])),
        ("row0 + rows > P", BN_TILE_ENTRIES, dict(sets=[(0, 65, 0), (65, 3, 1)])),
        ("level == nlevels", ("finalize", "apply_relu", "bwd_apply"), dict(sets=[(0, 65, 0), (65, 2, 2)])),
        ("C 6", BN_TILE_ENTRIES, dict(C=6)),
        ("activation pointer one element off", BN_TILE_ENTRIES, dict(x=t["x"].data_ptr() + 4)),
        ("null partial", ("stats_partial", "reduce", "bwd_partial"), dict(partial=None)),
        ("count_mul 0", ("finalize", "bwd_apply"), dict(count_mul=0)),
        ("mode 2", ("finalize",), dict(mode=2)),
        ("training finalize, rows * count_mul = 1", ("finalize",), dict(sets=[(0, 65, 0), (65, 1, 1)])),
    ]
    for label, entries, kw in bad:
        for e in entries:
            assert bn_raw(e, t, **dict(dict(sets=sets), **kw)) == -1000, (label, e)
    st = hip.BnSets(sets, Lv)
    chunks = hip.load().utv2_bn_chunks
    assert chunks(0, st.p_rows) == -1000 and chunks(17, st.p_rows) == -1000 and chunks(2, None) == -1000 and chunks(2, st.p_rows) == 3
    torch.cuda.synchronize()
    for k, v in t.items():
        assert bool((v == FILL).all()), "a rejected call wrote %s" % k
    for e in BN_ENTRIES:
        assert bn_raw(e, t, sets) == 0, e
    for e in ("reduce", "finalize"):
        assert bn_raw(e, t, sets, C=6) == 0, e
    assert bn_raw("finalize", t, [(0, 65, 0), (65, 1, 1)], mode=1) == 0
    assert bn_raw("finalize", t, [(0, 65, 0), (65, 1, 1)], count_mul=2) == 0
    assert bn_raw("finalize", t, sets, mode=1, out=None) == 0         # eval mode reads no moments
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", ["fp32", "bf16", "fp16"])
def test_nan_activation_stays_nan_as_in_torch(kind):
    """torch's ReLU hands a NaN on (relu(nan) is nan) and gives it no gradient (nan > 0 is false): eval mode, so that the NaN does not
    reach the statistics; the other elements are untouched by it"""
    from ubteacher import hip
    dt = select(kind)
    C = 8
    st = hip.BnSets([(0, 4, 0)], 1)
    x = torch.arange(4 * C, dtype=torch.float32).reshape(4, C) / 8 - 1.0
    x[1, 2], x[3, 5] = float("nan"), float("nan")
    xd = x.to(dt).cuda()
    ga, be, rm, rv = (torch.full((1, C), v, device="cuda") for v in (1.5, 0.25, 0.5, 2.0))
    mean, rstd, scale = hip.bn_finalize(None, ga, rm, rv, st, R.EPS, R.MOMENTUM, training=False)
    y = hip.bn_apply_relu(xd, mean, scale, be, st)
    want = torch.relu(torch.nn.functional.batch_norm(x.to(dt).double().t()[None], rm[0].cpu().double(), rv[0].cpu().double(), ga[0].cpu().double(),
                                                     be[0].cpu().double(), False, R.MOMENTUM, R.EPS))[0].t()
    got = y.cpu().double()
    assert bool(torch.isnan(got[1, 2])) and bool(torch.isnan(got[3, 5])) and int(torch.isnan(got).sum()) == 2 == int(torch.isnan(want).sum())
    ok = ~torch.isnan(want)
    assert float((got[ok] - want[ok]).abs().max()) <= (1e-6 if kind == "fp32" else 2.0 ** -7) * float(want[ok].abs().max())
    dy = torch.ones_like(xd)
    sums = hip.bn_bwd_sums(dy, y, xd, mean, rstd, st).cpu()
    # the masked gradient of a NaN element is 0: it is not counted in sum g; in sum g * xhat it is 0 * nan = nan, as in torch's batch
    # norm backward behind torch's ReLU backward - the NaN channels, and only they, report the NaN in dgamma
    assert bool(torch.isfinite(sums[0, 0]).all())
    assert [bool(v) for v in torch.isnan(sums[0, 1])] == [c in (2, 5) for c in range(C)]
    assert float(sums[0, 0, 2]) == float((want[:, 2] > 0).sum()) and float(sums[0, 0, 5]) == float((want[:, 5] > 0).sum())
