"""The TEST.PRECISE_BN kernels (csrc/bn_precise.hip) through their wrappers against tests/precise_bn_ref64.py.

Shape: 2 levels, C = 8, three iterations of three statistic sets each: levels (0, 1, 0), rows (6, 15, 130), B (2, 2, 1) - level 0 takes two
sets of unequal B per iteration, level 1 one; the 130-row set spans three 64-row chunks of the statistics kernels.  Inputs have |mean| <=
std, so running_var = pop_sq - pop_mean^2 loses no more than a few bits to cancellation.

Bounds.
  state (pop_mean, pop_sq):  1e-12 * max(|value|, pop_sq) - fewer than 100 fp64 operations per element (the moments' sums of <= 130
      terms on the device side differ from numpy's only in their order, the estimator adds ~10 operations per set for 6 sets) at
      1.1e-16 each.
  committed fp32 buffers:    the reference rounded once to fp32, within 1 fp32 ulp.
  mean / rstd / scale:       bit-equal to utv2_bn_finalize mode 0 on the same moments.
Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest
import torch

from tests import precise_bn_ref64 as R

pytestmark = pytest.mark.gpu

L, C = 2, 8
LEVELS, ROWS, IMAGES = (0, 1, 0), (6, 15, 130), (2, 2, 1)
ITERS = 3
EPS = 1e-5


def make_sets():
    sets, r = [], 0
    for l, n in zip(LEVELS, ROWS):
        sets.append((r, n, l))
        r += n
    return sets, r


def select(kind):
    from ubteacher import hip, ops
    ops.set_precision(kind)
    return torch.float32 if kind == "fp32" else hip.h16_dtype()


def inputs(dt):
    g = torch.Generator().manual_seed(17)
    sets, P = make_sets()
    xs = [(torch.randn(P, C, generator=g) * (1.0 + 0.5 * torch.rand(C, generator=g)) + (torch.rand(C, generator=g) - 0.5)).to(dt) for _ in range(ITERS)]
    ga = torch.rand(L, C, generator=g) + 0.5
    rm, rv = torch.randn(L, C, generator=g) * 0.1, torch.rand(L, C, generator=g) + 0.5
    return sets, xs, ga, rm, rv


def reference(sets, xs):
    """the estimator on the inputs as stored, numpy fp64"""
    stream = []
    for x in xs:
        x64 = x.double().numpy()
        for (r0, n, l), B in zip(sets, IMAGES):
            seg = x64[r0:r0 + n]
            m, v = R.moments_to_batch_stats(seg.mean(axis=0), (seg * seg).mean(axis=0), n)
            stream.append((l, m, v, B))
    return R.estimate(L, C, stream)


def ulp32(a):
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("kind", ["fp32", "bf16", "fp16"])
def test_update_and_commit_against_ref64(kind):
    from ubteacher import hip
    dt = select(kind)
    sets, xs, ga, rm0, rv0 = inputs(dt)
    st = hip.BnSets(sets, L).set_images(IMAGES)
    ga_d, rm, rv = ga.cuda(), rm0.cuda(), rv0.cuda()
    state = hip.bn_precise_state(1, L, C, "cuda")
    for x in xs:
        mom = hip.bn_stats(x.cuda(), st)
        mean, rstd, scale = hip.bn_precise_update(mom, ga_d, state[0], st, EPS)
        rm_f, rv_f = rm0.cuda(), rv0.cuda()           # finalize moves its running buffers: give it copies
        fmean, frstd, fscale = hip.bn_finalize(mom, ga_d, rm_f, rv_f, st, EPS, 0.1, training=True)
        for name, a, b in (("mean", mean, fmean), ("rstd", rstd, frstd), ("scale", scale, fscale)):
            assert torch.equal(a.view(torch.int64), b.view(torch.int64)), "%s differs from utv2_bn_finalize mode 0" % name
    torch.cuda.synchronize()
    assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0), "the running buffers are untouched before the commit"
    ref = reference(sets, xs)
    got = state[0].cpu().numpy()
    bound = 1e-12 * np.maximum(np.abs(ref["pop_mean"]), ref["pop_sq"])
    for name, g, w in (("pop_mean", got[:, 0], ref["pop_mean"]), ("pop_sq", got[:, 1], ref["pop_sq"])):
        err = np.abs(g - w)
        print("[%s] %-8s largest error %.3e, as a fraction of its bound %.3g" % (kind, name, float(err.max()), float((err / bound).max())))
        assert bool((err <= bound).all()), (kind, name, float((err / bound).max()))
    assert np.array_equal(got[:, 2], np.repeat(ref["num"][:, None], C, axis=1)), "num: the images seen per level"
    assert list(ref["num"]) == [ITERS * 3.0, ITERS * 2.0]

    hip.bn_precise_commit(state, [rm], [rv])
    torch.cuda.synchronize()
    for name, g, w64 in (("running_mean", rm, ref["running_mean"]), ("running_var", rv, ref["running_var"])):
        g = g.cpu().numpy().astype(np.float64)
        w = w64.astype(np.float32).astype(np.float64)
        steps = np.abs(g - w) / ulp32(w)
        print("[%s] %-12s worst distance to the reference rounded once: %.3g fp32 ulp" % (kind, name, float(steps.max())))
        assert float(steps.max()) <= 1.0, (kind, name, float(steps.max()))
    assert float(rv.min()) > 0

    # bit-reproducible: the whole sequence again
    state2 = hip.bn_precise_state(1, L, C, "cuda")
    for x in xs:
        hip.bn_precise_update(hip.bn_stats(x.cuda(), st), ga_d, state2[0], st, EPS)
    assert torch.equal(state2, state)


def test_commit_leaves_a_level_without_sets_and_writes_every_layer():
    from ubteacher import hip
    select("fp32")
    state = hip.bn_precise_state(3, L, C, "cuda")
    g = torch.Generator().manual_seed(5)
    state[:, 0, 0] = torch.randn(3, C, generator=g, dtype=torch.float64).cuda()
    state[:, 0, 1] = state[:, 0, 0] ** 2 + 1.0 + torch.rand(3, C, generator=g, dtype=torch.float64).cuda()
    state[:, 0, 2] = 4.0                                                   # level 1 of every layer: num = 0
    rms = [torch.full((L, C), 7.0, device="cuda") for _ in range(3)]
    rvs = [torch.full((L, C), 9.0, device="cuda") for _ in range(3)]
    hip.bn_precise_commit(state, rms, rvs)
    torch.cuda.synchronize()
    for k in range(3):
        assert torch.equal(rms[k][0], state[k, 0, 0].float()), k
        assert torch.equal(rvs[k][0], (state[k, 0, 1] - state[k, 0, 0] * state[k, 0, 0]).float()), k
        assert bool((rms[k][1] == 7.0).all()) and bool((rvs[k][1] == 9.0).all()), "a level no set reached keeps its buffers"


def test_argument_errors_launch_nothing():
    """UTV2_EARG (-1000): a set of one row with count_mul 1 (n < 2), B < 1, C % 4 != 0, more than 16 sets; the outputs keep their fill"""
    from ubteacher import hip
    select("fp32")
    FILL = 3.25
    t = {k: torch.full(s, FILL, dtype=torch.float64, device="cuda") for k, s in
         (("moments", (2, 2, C)), ("state", (L, 3, C)), ("mean", (2, C)), ("rstd", (2, C)), ("scale", (2, C)))}
    ga = torch.ones((L, C), device="cuda")
    iarr = lambda v: ctypes.cast((ctypes.c_int * len(v))(*v), ctypes.c_void_p)
    fn = hip.load().utv2_bn_precise_update

    def raw(rows=(65, 2), levels=(0, 1), images=(2, 2), C_=C, count_mul=1, n=2):
        s = torch.cuda.current_stream().cuda_stream
        return fn(t["moments"].data_ptr(), ga.data_ptr(), t["state"].data_ptr(), t["mean"].data_ptr(), t["rstd"].data_ptr(), t["scale"].data_ptr(),
                  C_, L, n, iarr(rows), iarr(levels), iarr(images), EPS, count_mul, 0, s)
    assert raw(rows=(65, 1)) == -1000, "one row with count_mul 1"
    assert raw(images=(2, 0)) == -1000, "B < 1"
    assert raw(C_=6) == -1000 and raw(levels=(0, 2)) == -1000 and raw(count_mul=0) == -1000
    assert raw(rows=(2,) * 17, levels=(0,) * 17, images=(1,) * 17, n=17) == -1000
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        hip.bn_precise_update(t["moments"], ga, t["state"], hip.BnSets([(0, 65, 0), (65, 1, 1)], L).set_images((2, 2)))
    torch.cuda.synchronize()
    for k, v in t.items():
        assert bool((v == FILL).all()), "a rejected call wrote %s" % k
    assert raw(rows=(65, 1), count_mul=2) == 0, "two ranks of one row each: two values per channel"
    commit = hip.load().utv2_bn_precise_commit
    one = (ctypes.c_void_p * 1)(ga.data_ptr())
    assert commit(None, ctypes.cast(one, ctypes.c_void_p), ctypes.cast(one, ctypes.c_void_p), 1, L, C, 0) == -1000
    assert commit(t["state"].data_ptr(), ctypes.cast(one, ctypes.c_void_p), ctypes.cast(one, ctypes.c_void_p), 1, L, 6, 0) == -1000
    assert commit(t["state"].data_ptr(), ctypes.cast(one, ctypes.c_void_p), ctypes.cast(one, ctypes.c_void_p), 0, L, C, 0) == -1000
    torch.cuda.synchronize()
    assert bool((ga == 1.0).all())
