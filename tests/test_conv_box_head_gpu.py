"""The conv box head (MODEL.ROI_BOX_HEAD.NUM_CONV > 0, NORM "GN"; Detectron2 v0.6 FastRCNNConvFCHead) on the GPU.

_box_features (RoIAlign -> [3x3 conv without bias -> GroupNorm(32) -> ReLU] x NUM_CONV -> fc + ReLU) and the gradients of every new
parameter and of the FPN features against a composition of F.conv2d / F.group_norm / F.linear in float64 on the Detectron2-layout
tensors of the model's own state_dict(), with the RoIAlign of tests/roi_pooler_ref64.py.  Tolerances are the conv tests':
  fp32    tests/test_conv_gpu.py: 2e-4 of the reference's max-norm (accumulation order only).  The composition runs end to end.
  16-bit  tests/test_conv_bf16_gpu.py: the reference makes the DECLARED roundings (16-bit weights, 16-bit stored activations and
          activation gradients) and nothing else; fp32 results within 2e-4 of the max-norm, 16-bit results within
          2^-8 |ref| + 2e-4 max|ref| (close16).  That bound is the one of ONE op on given operands, so the composition is checked
          link by link: every layer of the chain _box_features ran is restated on the operands the product itself stored (the input
          it read, the gradient it was handed).  End to end the bound cannot hold for any correct implementation: a value that lands
          on the other side of a 16-bit rounding boundary (accumulation order decides) moves by one ulp, the next conv spreads that
          over 9 x 128 outputs, each of which crosses its own boundary with a probability of a few per cent - five storage points
          later (measured, MI355X) the bf16 features differ by 2.9e-3 and conv1's weight gradient by 1e-2 of the max-norm while every
          single layer is within 2e-7 (parameter gradients) and one rounding (stored tensors) of its float64 restatement.
Then whole steps: one semi-supervised training step with the 4conv1fc GN head (fp32 and AMP), teacher inference, and the default head
(NUM_CONV 0) unchanged by the new keys."""
import pytest
import torch
import torch.nn.functional as F

from tests import roi_pooler_ref64 as R64
from tests.utv2_testutil import FixedLoader, make_batch

pytestmark = pytest.mark.gpu

HEAD = ["MODEL.ROI_BOX_HEAD.NUM_CONV", 2, "MODEL.ROI_BOX_HEAD.NUM_FC", 1, "MODEL.ROI_BOX_HEAD.NORM", "GN",
        "MODEL.ROI_BOX_HEAD.CONV_DIM", 128, "MODEL.ROI_BOX_HEAD.FC_DIM", 64]
HEAD_4CONV1FC = ["MODEL.ROI_BOX_HEAD.NUM_CONV", 4, "MODEL.ROI_BOX_HEAD.NUM_FC", 1, "MODEL.ROI_BOX_HEAD.NORM", "GN"]
N, P_SLOTS, C_IN, S = 2, 16, 256, 7
LEVEL_HW = ((16, 16), (8, 8), (4, 4), (2, 2))       # p2 .. p5 of a 64 x 64 image
PRE = "roi_heads.box_head."


def relerr(a, b):
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-12)


def close16(y, ref):
    tol = 2.0 ** -8 * ref.abs() + 2e-4 * ref.abs().max()
    return bool(((y - ref).abs() <= tol).all())


def make_inputs():
    g = torch.Generator().manual_seed(5)
    feats = [torch.randn(N, C_IN, h, w, generator=g) for h, w in LEVEL_HW]
    xy = torch.rand(N, P_SLOTS, 2, generator=g) * 40
    wh = torch.rand(N, P_SLOTS, 2, generator=g) * 30 + 2
    boxes = torch.cat((xy, (xy + wh).clamp(max=64.0)), dim=2)
    for i, half in enumerate((60.0, 120.0, 230.0)):      # boxes past the 64 x 64 image: one for each of the levels p3, p4, p5
        boxes[i % N, 5 + i] = torch.tensor([32 - half, 32 - half, 32 + half, 32 + half])
    valid = (torch.rand(N, P_SLOTS, generator=g) > 0.25).to(torch.uint8)
    valid[:, 5:8] = 1
    valid[0, 3] = valid[1, 0] = 0
    gout = torch.randn(N * P_SLOTS, 64, generator=g) * valid.reshape(-1, 1)      # the loss leaves padding slots without gradient
    return feats, boxes, valid, gout


def reference(sd, feats, boxes, valid, gout):
    """float64 composition on Detectron2-layout tensors -> (features [R, FC], {key: gradient}, [feature gradients NCHW])"""
    f64 = [f.double().requires_grad_(True) for f in feats]
    par = {k: v.double().requires_grad_(True) for k, v in sd.items() if k.startswith(PRE)}
    batch = torch.arange(N).repeat_interleave(P_SLOTS)
    x = R64.roi_pooler(f64, boxes.reshape(-1, 4).double(), batch, S, "ROIAlignV2", 0, roi_valid=valid.reshape(-1))
    for k in (1, 2):
        p = PRE + "conv%d" % k
        x = F.conv2d(x, par[p + ".weight"], None, 1, 1)
        x = F.relu(F.group_norm(x, 32, par[p + ".norm.weight"], par[p + ".norm.bias"], 1e-5))
    x = F.relu(F.linear(x.flatten(1), par[PRE + "fc1.weight"], par[PRE + "fc1.bias"]))
    (x * gout.double()).sum().backward()
    return x.detach(), {k: v.grad for k, v in par.items()}, [torch.zeros_like(f) if f.grad is None else f.grad for f in f64]


class _Tap:
    """a layer of the head that keeps (layer, input, output) of its call, with the gradients of both retained"""

    def __init__(self, layer, log):
        self.layer, self.log = layer, log

    def __call__(self, x):
        y = self.layer(x)
        for t in (x, y):
            if t.requires_grad and not t.is_leaf:
                t.retain_grad()
        self.log.append((self.layer, x, y))
        return y


def _nchw(t):
    return t.detach().double().cpu().permute(0, 3, 1, 2)


def _same(got, ref, stored16, what):
    """a stored 16-bit tensor: close16; an fp32 result: 2e-4 of the max-norm"""
    e = relerr(got, ref)
    print("  %-46s relerr %.3g" % (what, e))
    assert close16(got, ref) if stored16 else e < 2e-4, (what, e)


def check_links(log, sd, named, dt):
    """every layer _box_features ran against its float64 restatement on the operands the product stored"""
    from ubteacher import ops
    r16 = lambda t: t.to(dt).double()  # noqa: E731
    convs = [k for k in sd if k.startswith(PRE + "conv") and k.endswith(".weight") and ".norm." not in k]
    ci = gi = 0
    for layer, x, y in log:
        g = y.grad
        assert g is not None and x.grad is not None
        if isinstance(layer, ops.RoiGroupNormReLU):
            p = convs[gi][:-len(".weight")] + ".norm"
            gi += 1
            a = _nchw(x).requires_grad_(True)
            ga, be = sd[p + ".weight"].double().requires_grad_(True), sd[p + ".bias"].double().requires_grad_(True)
            ref = F.relu(F.group_norm(a, 32, ga, be, 1e-5))
            ref.backward(_nchw(g))
            _same(_nchw(y), ref.detach(), True, p + " output")
            _same(_nchw(x.grad), a.grad, True, p + " input gradient")
            _same(named[p + ".weight"][1].detach().double().cpu(), ga.grad, False, "d " + p + ".weight")
            _same(named[p + ".bias"][1].detach().double().cpu(), be.grad, False, "d " + p + ".bias")
        elif layer.k == 3:
            p = convs[ci][:-len(".weight")]
            ci += 1
            a = r16(_nchw(x)).requires_grad_(True)          # the MFMA operand: x as stored (conv2..) or rounded while staged (conv1)
            w = r16(sd[p + ".weight"]).requires_grad_(True)
            ref = F.conv2d(a, w, None, 1, 1)
            ref.backward(_nchw(g))
            _same(_nchw(y), ref.detach(), True, p + " output")
            _same(_nchw(x.grad), a.grad, x.dtype == dt, p + " input gradient")
            _same(named[p + ".weight"][1].detach().double().cpu(), w.grad, False, "d " + p + ".weight")
        else:
            p = PRE + "fc1"
            R = x.shape[0]
            a = x.detach().double().cpu().view(R, S, S, -1).permute(0, 3, 1, 2).reshape(R, -1).requires_grad_(True)      # D2's CHW order
            w, b = r16(sd[p + ".weight"]).requires_grad_(True), sd[p + ".bias"].double().requires_grad_(True)
            ref = F.relu(F.linear(a, w, b))
            (ref * (g.detach().double().cpu().view(R, -1) * (r16(ref.detach()) > 0))).sum().backward()     # the ReLU mask of the stored output
            _same(y.detach().double().cpu().view(R, -1), ref.detach(), True, p + " output")
            _same(x.grad.double().cpu().view(R, S, S, -1).permute(0, 3, 1, 2).reshape(R, -1), a.grad, True, p + " input gradient")
            _same(named[p + ".weight"][1].detach().double().cpu(), w.grad, False, "d " + p + ".weight")
            _same(named[p + ".bias"][1].detach().double().cpu(), b.grad, False, "d " + p + ".bias")
    assert ci == 2 and gi == 2 and len(log) == 5


@pytest.mark.parametrize("kind", ["fp32", "bf16", "fp16"])
def test_box_features_and_gradients_against_float64(kind):
    from ubteacher import hip, ops
    from ubteacher.modeling.rcnn import StandardROIHeadsPseudoLab
    from ubteacher.params import ParamStore
    from ubteacher.presets import get_config
    ops.set_precision(kind)
    dt = None if kind == "fp32" else hip.h16_dtype()
    cfg = get_config("rcnn", 1, ["MODEL.DEVICE", "cuda"] + HEAD)
    torch.manual_seed(0)
    store = ParamStore()
    head = StandardROIHeadsPseudoLab(cfg, store, C_IN)
    store.finalize("cuda")
    g = torch.Generator().manual_seed(9)
    for k, v in store.state_dict().items():       # norm parameters off their initial 1 / 0
        if ".norm." in k:
            v.copy_((torch.rand(v.shape, generator=g) + 0.5 if k.endswith("weight") else torch.randn(v.shape, generator=g) * 0.2).cuda())
    store.touch()
    sd = {k: v.detach().cpu().clone() for k, v in store.state_dict().items()}
    assert tuple(sd[PRE + "conv2.weight"].shape) == (128, 128, 3, 3) and tuple(sd[PRE + "fc1.weight"].shape) == (64, 128 * S * S)
    feats, boxes, valid, gout = make_inputs()
    if dt is not None:
        gout = gout.to(dt).float()
    log = []
    head.convs = [(_Tap(c, log), _Tap(n, log)) for c, n in head.convs]
    head.fcs = [_Tap(fc, log) for fc in head.fcs]

    fg = [f.permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True) for f in feats]
    out = head._box_features(fg, boxes.cuda(), valid.cuda())
    assert out.dtype == (torch.float32 if dt is None else dt) and tuple(out.shape) == (N * P_SLOTS, 64)
    out.backward(gout.cuda().to(out.dtype))
    torch.cuda.synchronize()
    named = store.trainable_named()
    print("box head %s" % kind)
    if dt is None:
        want, wgrad, wfeat = reference(sd, feats, boxes, valid, gout)
        _same(out.detach().double().cpu(), want, False, "features")
        for k, ref in wgrad.items():
            assert float(ref.abs().max()) > 0
            _same(named[k][1].detach().double().cpu(), ref, False, "d " + k)
    else:
        check_links(log, sd, named, dt)
        # the first link: RoIAlign (fp32 in, fp32 out) and the feature gradients from the gradient conv1 handed back
        roi = log[0][1]
        f64 = [f.double().requires_grad_(True) for f in feats]
        ref = R64.roi_pooler(f64, boxes.reshape(-1, 4).double(), torch.arange(N).repeat_interleave(P_SLOTS), S, "ROIAlignV2", 0,
                             roi_valid=valid.reshape(-1))
        ref.backward(_nchw(roi.grad))
        _same(_nchw(roi), ref.detach(), False, "RoIAlign output")
        wfeat = [torch.zeros_like(f) if f.grad is None else f.grad for f in f64]
    for i, ref in enumerate(wfeat):
        _same(fg[i].grad.double().cpu().permute(0, 3, 1, 2), ref, False, "d feature level %d" % i)
    # padding slots: all-zero rows into the head, finite all the way
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(f.grad).all()) for f in fg)
    assert all(bool(torch.isfinite(y).all()) and bool(torch.isfinite(x.grad).all()) for _, x, y in log)


def _step_cfg(opts, amp):
    from ubteacher.presets import get_config
    cfg = get_config("rcnn", 1, ["SOLVER.IMG_PER_BATCH_LABEL", 1, "SOLVER.IMG_PER_BATCH_UNLABEL", 1, "SEMISUPNET.BURN_UP_STEP", 0,
                                 "MODEL.DEVICE", "cuda"] + list(opts))
    cfg.SOLVER.AMP.ENABLED = amp
    return cfg


def _one_step(opts, amp=False):
    """a trainer on a fixed 96 x 128 batch after one run_step_full_semisup -> (trainer, losses, gradient arena before the update, batch)"""
    from ubteacher import ops
    from ubteacher.engine import UBRCNNTeacherTrainer
    torch.manual_seed(0)
    prod, _ = make_batch(31, 1, 1, 96, 128, "cuda")
    tr = UBRCNNTeacherTrainer(_step_cfg(opts, amp), data_loader=FixedLoader(prod))
    tr.iter = 1
    g = torch.Generator().manual_seed(99)
    src = lambda n, m, device: torch.rand(n, m, generator=g).to(device)  # noqa: E731
    tr.model.proposal_generator.sample_keys = src
    tr.model.roi_heads.sample_keys = src
    grads = {}
    step = tr.optimizer.step

    def spy(*a, **kw):
        ops.join_wgrad_stream()
        grads["arena"] = tr.model.store.grad.clone()
        return step(*a, **kw)

    tr.optimizer.step = spy
    tr.run_step_full_semisup()
    rec = {k: v for k, v in tr.flush_metrics().items() if k.startswith("loss")}
    torch.cuda.synchronize()
    return tr, rec, grads["arena"], prod


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "amp"])
def test_training_step_and_inference_with_4conv1fc_gn(amp):
    import math
    tr, rec, grad, prod = _one_step(HEAD_4CONV1FC, amp)
    assert rec and all(math.isfinite(v) for v in rec.values()), rec
    st = tr.model.store
    seen = 0
    for h in st.handles:
        if h.exports and h.exports[0][0].startswith(PRE + "conv"):
            gh = grad[h.offset:h.offset + h.numel]
            assert bool(torch.isfinite(gh).all()) and float(gh.abs().max()) > 0, h.exports[0][0]
            seen += 1
    assert seen == 12       # 4 x (weight, norm.weight, norm.bias)
    # the teacher moved with the EMA that opens the next step
    before = tr.model_teacher.store.flat.clone()
    tr.iter = 2
    tr.run_step_full_semisup()
    torch.cuda.synchronize()
    sd_t, key = tr.model_teacher.state_dict(), PRE + "conv3.weight"
    h = next(h for h in tr.model_teacher.store.handles if h.exports and h.exports[0][0] == key)
    assert not torch.equal(before[h.offset:h.offset + h.numel], sd_t[key].permute(0, 2, 3, 1).reshape(-1))
    # teacher inference
    with torch.no_grad():
        res = tr.model_teacher.inference([dict(d) for d in prod[3]])
    assert len(res) == 1
    boxes = res[0]["instances"].pred_boxes.tensor
    assert bool(torch.isfinite(boxes).all()) and bool(torch.isfinite(res[0]["instances"].scores).all())


def test_default_head_is_untouched_by_the_new_keys():
    """NUM_CONV 0 ignores NORM and CONV_DIM: the same state-dict keys, the same first-step losses to the bit"""
    a, rec_a, _, _ = _one_step([])
    b, rec_b, _, _ = _one_step(["MODEL.ROI_BOX_HEAD.NUM_CONV", 0, "MODEL.ROI_BOX_HEAD.NORM", "GN", "MODEL.ROI_BOX_HEAD.CONV_DIM", 128])
    assert list(a.model.state_dict()) == list(b.model.state_dict())
    assert [tuple(h.shape) for h in a.model.store.handles] == [tuple(h.shape) for h in b.model.store.handles]
    assert rec_a == rec_b and len(rec_a) >= 4
