"""SOLVER.CLIP_GRADIENTS / NESTEROV on the device (csrc/elementwise.hip: seg_norm_partial, seg_clip_coef, sgd_seg_f32).

Kernel level: a synthetic arena of 10 007 floats with twelve segments of awkward lengths at unaligned offsets, gaps between some of them
and at the tail, against fp64 torch.  Model level: two clipped steps of the smallest FCOS and Faster-RCNN trainers against
torch.nn.utils.clip_grad_* + torch.optim.SGD in fp64 on the tensors the state_dict exports - which pins the segment mapping of the
paired towers and the fused heads to the reference's key layout.

Tolerances.  Coefficients, rtol 1e-6: the sums are fp64, only the final rounding to fp32 (6e-8) remains; measured worst 5.0e-8.
Updated values: every fp32 operation rounds by at most 2^-24 = 6e-8 of its result; the chain multiplier - coefficient - weight decay -
momentum - learning rate - subtraction is eight roundings (the fp32 constants included), 4.8e-7 of the largest magnitude in the chain
in the worst case: 1e-6 at the kernel test's magnitude 2.  With a clip the chain is smaller than that worst case - the clipped gradient
is at most 1, momentum * old momentum at most 1.8 (half an ulp: 6e-8), the new momentum at most 2.8 (1.2e-7), three roundings at
magnitude <= 1 in front (9e-8), the fp32 momentum constant 5e-8: 3.2e-7 - so the clipped cases are held to ATOL = 5e-7 (measured worst:
2.1e-7 on the momentum, 1.5e-7 on the parameter); the case without a clip (Nesterov alone) sees unclipped gradients of 3 and momenta of
6.6 and keeps 2 * ATOL = 1e-6.  Model level: 5e-7 x the tensor's largest magnitude in the chain (measured worst: 6.0e-8 x)."""
import functools

import pytest
import torch

from tests.utv2_testutil import FixedLoader, cpu_state, make_batch, rcnn_tune, tune_state_for_pseudo_labels

pytestmark = pytest.mark.gpu

N = 10007
LENGTHS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 4099)
GAPS_BEFORE = (3, 0, 2, 1, 0, 5, 0, 7, 3, 0, 1, 2)          # unsegmented elements in front of each segment; the tail is a gap too
WD_BORDER, WDS = 2019, (5e-2, 1e-3)                           # two weight-decay ranges; the border lies in the gap before the last segment
CLIP = 1.0
# the p-norm of each segment's gradient: clipped and unclipped ones, an all-zero one, and one within 1e-3 of CLIP on either side
NORM_TARGETS = (0.3, 5.0, 0.0, 1.7, 0.2, 3.0, 1.0 + 5e-4, 10.0, 0.01, 1.0 - 5e-4, 0.9, 2.5)
LR, MOM, GSCALE = 0.1, 0.9, 0.5
INF = float("inf")
ATOL = 5e-7


def _segments():
    segs, pos = [], 0
    for gap, n in zip(GAPS_BEFORE, LENGTHS):
        segs.append((pos + gap, pos + gap + n))
        pos += gap + n
    assert pos < N and segs[-1][0] > WD_BORDER > segs[-2][1]
    return segs


def _pnorm(x, p):
    return x.abs().max() if p == INF else (x.abs() ** p).sum() ** (1.0 / p)


@functools.lru_cache(maxsize=None)
def _inputs(norm_type):
    """(param, grad, momentum) fp32 on the CPU; grad is what the arena holds BEFORE the multiplier GSCALE, scaled so that the p-norm of
    GSCALE * grad[segment] is NORM_TARGETS[segment]"""
    g = torch.Generator().manual_seed(1234)
    p = torch.rand(N, generator=g, dtype=torch.float64) * 4 - 2
    m = torch.rand(N, generator=g, dtype=torch.float64) * 4 - 2
    gr = torch.randn(N, generator=g, dtype=torch.float64) * 0.3        # the gaps keep this
    for (s, e), t in zip(_segments(), NORM_TARGETS):
        gr[s:e] *= t / (GSCALE * _pnorm(gr[s:e], norm_type))
    return p.float(), gr.float(), m.float()


@functools.lru_cache(maxsize=None)
def _reference(norm_type, clip_type, nesterov):
    """fp64: (coefficients, new param, new momentum) of one step on _inputs(norm_type)"""
    p, gr, m = (t.double() for t in _inputs(norm_type))
    gv = gr * GSCALE
    coefs = torch.ones(len(LENGTHS), dtype=torch.float64)
    for i, (s, e) in enumerate(_segments()):
        coefs[i] = min(1.0, CLIP / (float(_pnorm(gv[s:e], norm_type)) + 1e-6))
        if clip_type == "norm":
            gv[s:e] *= coefs[i]
    if clip_type == "value":
        gv = gv.clamp(-CLIP, CLIP)
    wd = torch.full((N,), WDS[1], dtype=torch.float64)
    wd[:WD_BORDER] = WDS[0]
    gv = gv + wd * p
    mn = MOM * m + gv
    pn = p - LR * (gv + MOM * mn if nesterov else mn)
    return coefs, pn, mn


@functools.lru_cache(maxsize=None)
def _table():
    from ubteacher.params import SegmentTable
    return SegmentTable(N, _segments(), [(0, WD_BORDER, WDS[0]), (WD_BORDER, N, WDS[1])], "cuda")


def _step(norm_type, clip_type, nesterov, clip=CLIP, state=None, grad_mul=1.0, mirror=False, inputs=None):
    """one eager segmented step on fresh device copies: (coef, p, m, mirror16)"""
    from ubteacher import hip
    p, gr, m = (t.cuda().clone() for t in (inputs or _inputs(norm_type)))
    gr *= grad_mul
    m16 = torch.zeros(N, dtype=hip.h16_dtype(), device="cuda") if mirror else None
    tb = _table()
    coef = None
    if clip_type == "norm":
        coef = hip.grad_clip_coef(gr, tb, norm_type, clip, GSCALE, state).clone()
    hip.sgd_segmented(p, gr, m, tb, LR, MOM, GSCALE, clip_type, clip, nesterov, state, mirror16=m16)
    torch.cuda.synchronize()
    return coef, p, m, m16


def test_layout_is_the_awkward_one():
    segs = _segments()
    assert [e - s for s, e in segs] == list(LENGTHS) and N % 4 == 3
    assert sum(1 for s, _ in segs if s % 4) >= 8 and segs[0][0] > 0 and segs[-1][1] < N
    assert any(a[1] == b[0] for a, b in zip(segs, segs[1:])) and any(a[1] < b[0] for a, b in zip(segs, segs[1:]))
    tb = _table()
    assert tb.seg_chunks[-1, 1] == 2                         # the 4099-element segment is two chunks: partials are summed across workgroups


@pytest.mark.parametrize("norm_type", [2.0, 1.0, INF])
def test_coefficients_vs_fp64(norm_type):
    ref, _, _ = _reference(norm_type, "norm", False)
    coef, _, _, _ = _step(norm_type, "norm", False)
    coef = coef.cpu().double()
    rel = ((coef - ref).abs() / ref).max()
    print("coefficients p=%s: worst relative error %.3e" % (norm_type, rel))
    assert (ref < 1).sum() >= 5 and (ref == 1).sum() >= 5    # some segments clip, some do not
    assert ref[2] == 1.0 and coef[2] == 1.0                  # the all-zero segment
    assert ref[6] < 1.0 and ref[9] == 1.0 and abs(float(ref[6]) - 1) < 1e-3    # the two next to the threshold, one on each side
    assert float(rel) <= 1e-6


@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("clip_type, norm_type", [("norm", 2.0), ("norm", 1.0), ("norm", INF), ("value", 2.0), (None, 2.0)])
def test_update_vs_fp64(clip_type, norm_type, nesterov):
    _, pr, mr = _reference(norm_type, clip_type, nesterov)
    _, p, m, _ = _step(norm_type, clip_type, nesterov)
    ep, em = (p.cpu().double() - pr).abs(), (m.cpu().double() - mr).abs()
    print("update clip=%s p=%s nesterov=%s: worst |dp| %.3e |dm| %.3e" % (clip_type, norm_type, nesterov, ep.max(), em.max()))
    atol = ATOL if clip_type is not None else 2 * ATOL
    assert float(ep.max()) <= atol and float(em.max()) <= atol
    # gaps take coefficient 1 (their gradient is not small: a wrong coefficient would show)
    in_seg = torch.zeros(N, dtype=torch.bool)
    for s, e in _segments():
        in_seg[s:e] = True
    assert float(ep[~in_seg].max()) <= atol and float(em[~in_seg].max()) <= atol and int((~in_seg).sum()) > 3000
    if clip_type is not None:    # and the clip is visible at this tolerance: the unclipped update is far away
        _, pu, _ = _reference(norm_type, None, nesterov)
        assert float((pu - pr).abs().max()) > 1e-2


@pytest.mark.parametrize("h16", ["bf16", "fp16"])
def test_mirror16_is_the_rounding_of_the_new_param(h16):
    from ubteacher import hip
    try:
        hip.set_h16(h16)
        for clip_type, nesterov in (("norm", False), ("value", True)):
            _, p, _, m16 = _step(2.0, clip_type, nesterov, mirror=True)
            assert m16.dtype == (torch.bfloat16 if h16 == "bf16" else torch.float16)
            assert torch.equal(m16.view(torch.int16), p.to(m16.dtype).view(torch.int16))
            _, pr, _ = _reference(2.0, clip_type, nesterov)
            assert float((p.cpu().double() - pr).abs().max()) <= ATOL          # either library computes the same fp32 update
    finally:
        hip.set_h16("bf16")


def test_neutral_case_is_bit_identical_to_the_plain_kernels():
    """all coefficients 1 (a huge CLIP_VALUE), Nesterov off: the bits of utv2_sgd_momentum / utv2_sgd_momentum_amp per weight-decay range"""
    from ubteacher import hip
    for amp in (False, True):
        state = torch.tensor([1024.0, 0.0, 0.0], device="cuda") if amp else None
        coef, p, m, m16 = _step(2.0, "norm", False, clip=1e30, state=state, grad_mul=1024.0 if amp else 1.0, mirror=True)
        assert bool((coef == 1).all())
        p0, g0, m0 = (t.cuda().clone() for t in _inputs(2.0))
        if amp:
            g0 *= 1024.0
        r16 = torch.zeros(N, dtype=hip.h16_dtype(), device="cuda")
        for (s, e), wd in zip(((0, WD_BORDER), (WD_BORDER, N)), WDS):
            if amp:
                hip.sgd_momentum_amp(p0[s:e], g0[s:e], m0[s:e], LR, MOM, wd, GSCALE, state, mirror16=r16[s:e])
            else:
                hip.sgd_momentum(p0[s:e], g0[s:e], m0[s:e], LR, MOM, wd, GSCALE, zero_grad=False, mirror16=r16[s:e])
        torch.cuda.synchronize()
        assert torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(m16.view(torch.int16), r16.view(torch.int16)), amp


@pytest.mark.parametrize("norm_type", [2.0, INF])
def test_amp_unscales_before_clipping_and_skips_on_found_inf(norm_type):
    coef, p, m, _ = _step(norm_type, "norm", True)
    state = torch.tensor([1024.0, 0.0, 0.0], device="cuda")
    coef_a, p_a, m_a, _ = _step(norm_type, "norm", True, state=state, grad_mul=1024.0)      # pre-scaled gradients, loss scale 1024
    assert torch.equal(coef_a, coef) and torch.equal(p_a, p) and torch.equal(m_a, m)
    assert state.tolist() == [1024.0, 0.0, 0.0]                                              # the step reads the state, it does not write it
    state[1] = 1.0
    p0, _, m0 = _inputs(norm_type)
    for clip_type in ("norm", "value"):
        _, p_s, m_s, m16 = _step(norm_type, clip_type, True, state=state, grad_mul=1024.0, mirror=True)
        assert torch.equal(p_s.cpu(), p0) and torch.equal(m_s.cpu(), m0) and not bool(m16.view(torch.int16).any())


def test_two_runs_are_bit_identical():
    for norm_type in (2.0, 1.0, INF):
        a, b = _step(norm_type, "norm", True), _step(norm_type, "norm", True)
        assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))


def test_clipped_step_is_capturable_on_one_stream():
    """the norm reduction, the coefficients and the update captured once (no host read, no allocation, nothing uploaded), replayed on
    two gradient fills: the bits of the eager step"""
    from ubteacher import hip
    p0, g0, m0 = _inputs(2.0)
    fills = (g0, torch.flip(g0, (0,)) * 3.0)
    eager = [_step(2.0, "norm", True, mirror=True, inputs=(p0, g, m0)) for g in fills]
    tb = _table()
    p, gr, m = p0.cuda().clone(), g0.cuda().clone(), m0.cuda().clone()
    m16 = torch.zeros(N, dtype=hip.h16_dtype(), device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.grad_clip_coef(gr, tb, 2.0, CLIP, GSCALE, None)
        hip.sgd_segmented(p, gr, m, tb, LR, MOM, GSCALE, "norm", CLIP, True, None, mirror16=m16)
    for g, (coef_e, p_e, m_e, m16_e) in zip(fills, eager):
        p.copy_(p0)
        m.copy_(m0)
        gr.copy_(g)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(tb.coef, coef_e) and torch.equal(p, p_e) and torch.equal(m, m_e)
        assert torch.equal(m16.view(torch.int16), m16_e.view(torch.int16))
    assert not torch.equal(eager[0][0], eager[1][0])          # the two fills clip differently


# ---- model level ---------------------------------------------------------------------------------------------------------------------
H, W = 96, 128


def _trainer(kind, overrides):
    from ubteacher.engine import UBRCNNTeacherTrainer, UBTeacherTrainer
    from ubteacher.presets import get_config
    torch.manual_seed(0)
    if kind == "fcos":
        cfg = get_config("fcos", 1, ["SOLVER.IMG_PER_BATCH_LABEL", 2, "SOLVER.IMG_PER_BATCH_UNLABEL", 2, "SEMISUPNET.BURN_UP_STEP", 0,
                                     "SOLVER.AMP.ENABLED", False, "MODEL.DEVICE", "cuda"] + list(overrides))      # small_fcos_cfg + the solver keys
        prod, orac = make_batch(12, 2, 2, H, W, "cuda")
        tr = UBTeacherTrainer(cfg, data_loader=FixedLoader(prod))
        sd = tune_state_for_pseudo_labels(cpu_state(tr.model), [d["image"] for d in orac[3]])
    else:
        cfg = get_config("rcnn", 1, ["SOLVER.IMG_PER_BATCH_LABEL", 1, "SOLVER.IMG_PER_BATCH_UNLABEL", 1, "SEMISUPNET.BURN_UP_STEP", 0,
                                     "SOLVER.AMP.ENABLED", False, "MODEL.DEVICE", "cuda"] + list(overrides))
        prod, orac = make_batch(31, 1, 1, H, W, "cuda")
        tr = UBRCNNTeacherTrainer(cfg, data_loader=FixedLoader(prod))
        sd = rcnn_tune(cpu_state(tr.model), [d["image"] for d in orac[3]], torch.tensor(cfg.MODEL.PIXEL_MEAN).view(3, 1, 1),
                       torch.tensor(cfg.MODEL.PIXEL_STD).view(3, 1, 1))
    tr.model.load_state_dict(sd)
    tr.model_teacher.load_state_dict(sd)
    tr.iter = 1
    tr.optimizer.param_groups[0]["lr"] = 0.01
    return cfg, tr


def _reference_sgd(before, cfg, lr, grad_scale):
    """[D2-recall] maybe_add_gradient_clipping + build_optimizer on the CPU in fp64: the clipper on each parameter tensor, then
    torch.optim.SGD with the WEIGHT_DECAY / WEIGHT_DECAY_NORM groups.  Returns {key: (new param, magnitude of the chain)}"""
    s = cfg.SOLVER
    params, groups = {}, {"decay": [], "nodecay": []}
    for k, (p, g, m, kind) in before.items():
        q = torch.nn.Parameter(p.clone())
        q.grad = g * grad_scale
        params[k] = q
        groups[kind].append(q)
    sgd = torch.optim.SGD([{"params": ps, "weight_decay": wd} for ps, wd in ((groups["decay"], s.WEIGHT_DECAY),
                                                                              (groups["nodecay"], s.WEIGHT_DECAY_NORM)) if ps],
                          lr=lr, momentum=s.MOMENTUM, nesterov=s.NESTEROV)
    for k, q in params.items():
        sgd.state[q]["momentum_buffer"] = before[k][2].clone()
    clipped = 0
    for q in params.values():
        raw = q.grad.clone()
        if s.CLIP_GRADIENTS.CLIP_TYPE == "norm":
            torch.nn.utils.clip_grad_norm_(q, s.CLIP_GRADIENTS.CLIP_VALUE, s.CLIP_GRADIENTS.NORM_TYPE)
        else:
            torch.nn.utils.clip_grad_value_(q, s.CLIP_GRADIENTS.CLIP_VALUE)
        clipped += int(not torch.equal(raw, q.grad))
    mags = {k: max(float(before[k][0].abs().max()), float(q.grad.abs().max())) for k, q in params.items()}
    sgd.step()
    out = {}
    for k, q in params.items():
        mag = max(mags[k], float(q.detach().abs().max()), float(sgd.state[q]["momentum_buffer"].abs().max()))
        out[k] = (q.detach(), mag)
    return out, clipped


@pytest.mark.parametrize("kind, clip_type, clip_value, nesterov", [("fcos", "norm", 0.01, False), ("rcnn", "norm", 0.01, False),
                                                                   ("fcos", "value", 1e-4, True)])
def test_clipped_model_step_vs_torch_sgd_per_reference_tensor(kind, clip_type, clip_value, nesterov):
    """two fp32 steps (the second with momentum) of the smallest trainer; gradients, parameters and momenta are captured THROUGH the
    state_dict export views just before each update.  Fails without the feature: the unclipped update is orders of magnitude away."""
    cfg, tr = _trainer(kind, ["SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", clip_type,
                              "SOLVER.CLIP_GRADIENTS.CLIP_VALUE", clip_value, "SOLVER.NESTEROV", nesterov])
    opt = tr.optimizer
    inner, seen = opt.step, []

    def step(grad_scale=1.0, amp_state=None):
        assert amp_state is None
        named, mv = tr.model.store.trainable_named(), opt._momentum_views()
        before = {k: (p.detach().double().cpu(), g.detach().double().cpu(), mv[k][1].detach().double().cpu(), mv[k][0].kind)
                  for k, (p, g) in named.items()}
        lr = opt.param_groups[0]["lr"]
        inner(grad_scale=grad_scale, amp_state=amp_state)
        torch.cuda.synchronize()
        after = {k: p.detach().double().cpu() for k, (p, _) in tr.model.store.trainable_named().items()}
        ref, clipped = _reference_sgd(before, cfg, lr, grad_scale)
        worst = (0.0, None)
        for k, (pr, mag) in ref.items():
            assert bool(torch.isfinite(before[k][1]).all()), k
            err = float((after[k] - pr).abs().max())
            worst = max(worst, (err / max(mag, 1e-30), k))
            assert err <= 5e-7 * mag, (k, err, mag)
        moved = sum(int(not torch.equal(after[k], before[k][0])) for k in after)
        print("%s %s step %d: %d tensors, %d clipped, %d moved, worst error %.3e of the magnitude (%s)"
              % (kind, clip_type, len(seen), len(ref), clipped, moved, worst[0], worst[1]))
        seen.append((len(ref), clipped, moved))

    opt.step = step
    tr.run_step_full_semisup()
    tr.run_step_full_semisup()
    assert len(seen) == 2
    for n, clipped, moved in seen:
        assert n > 50 and clipped > n // 2 and moved > n // 2      # most tensors clip, and they all train
    keys = set(tr.model.store.trainable_named())
    fused = {"fcos": ("proposal_generator.fcos_head.cls_tower.0.weight", "proposal_generator.fcos_head.bbox_tower.0.weight",
                      "proposal_generator.fcos_head.bbox_pred_std.weight", "proposal_generator.fcos_head.ctrness.bias"),
             "rcnn": ("proposal_generator.rpn_head.objectness_logits.weight", "proposal_generator.rpn_head.anchor_deltas.bias",
                      "roi_heads.box_predictor.bbox_pred_std.weight", "roi_heads.box_head.fc1.weight")}[kind]
    assert set(fused) <= keys
