"""The conv autograd node (ubteacher/ops.py: _ConvFn, _BottleneckFn and the stage functions they drive) makes, for every case and
precision kind below, the C-ABI calls and the gradient bits it made at the commit that tests/golden/conv_backward_parent.json names.
The fixture is written by tests/golden/gen_golden_conv_backward_parent.py, which imports the cases and inputs from this module.

What a (case, kind) holds:
  * trace: one line per hip.call made between the start of backward() and the end of the weight-gradient join (the trainer's
    _backward: side streams on, FanIn.check, join) - the entry point's name and its arguments; integers and floats verbatim, pointers
    (include/utv2.h, through hip._SIGS) as "p" / "0", the trailing stream as "s<ordinal of its first appearance in this trace>" - main
    stream and weight-gradient lanes are told apart without recording a handle.  hip.call is replaced through monkeypatch in the
    test itself.  The geometry-table cache (hip._rowinfo_cache) and the lane assignment start empty in every case, so that a trace does
    not depend on the tests that ran before.
  * digests: SHA-256 of the bytes of every gradient the backward produced (dx, the residual's, the arena's w.g / bias.g / Scale / GroupNorm
    gradients, the ColPair / FanIn buffers as they arrive in dx).
Inputs and parameters come from the integer formula of tests/test_norm_kernels_parent_bits_gpu.py (`dyadic`): no random-number
generator's version enters a layer case.  The weight-gradient schedules are deterministic (test_weight_gradient_schedules_bit_identical),
so bits can be compared.

Layer cases are the smallest shapes at which a route still has a partial tile or an edge: NHWC N = 2 on 8 x 8 (9 x 9 for the stride-2
layers: an odd edge), level-first N = 2 on levels (5,7), (3,4), (2,2): P = 102 rows, the last 64- and 128-row tiles are partial.
Two whole-backward cases (one backward of the small FCOS and Faster-RCNN steps of test_fcos_step_gpu.py / test_rcnn_step_gpu.py, 2 + 2
images) reach the fused bottleneck, the bit planes and GradHandoff in their natural wiring; they hold the trace and the digests of the
gradient arena, whole and per top-level module (the generator runs them twice and keeps the digests the two runs agree on: all of
them at the fixture's commit).

test_epi_plain_switch_takes_the_unfused_dgrad: UTV2_EPI_PLAIN=0 (an A/B switch the library reads once per process: a fresh child) makes
utv2_conv2d_ml_fwd_bf16_gnb refuse; hip.gnb_eligible mirrors that, so the paired-tower case runs the unfused dgrad."""
import ctypes
import functools
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "unbiased-teacher-v2_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from tests.test_norm_kernels_parent_bits_gpu import dyadic, select  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_backward_parent.json")
KINDS = ("fp32", "bf16", "fp16")
LEVELS = [(5, 7), (3, 4), (2, 2)]
N = 2
STEP_H, STEP_W = 96, 128


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


class Recorder:
    """stands in for hip.call: records (while `on`) and forwards"""

    def __init__(self, hip):
        self.real, self.sigs, self.on, self.lines, self.streams = hip.call, hip._SIGS, False, [], {}
        txt = re.sub(r"/\*.*?\*/", "", open(hip.HEADER_PATH).read(), flags=re.S)
        self.has_stream = {m.group(1): "utv2_stream_t" in m.group(2).split(",")[-1]
                           for m in re.finditer(r"\b(utv2_\w+)\s*\(([^;{]*?)\)\s*;", txt, flags=re.S)}

    def __call__(self, name, *args):
        if self.on:
            argt = self.sigs[name][1]
            assert len(argt) == len(args), name
            out = [name]
            for i, (a, t) in enumerate(zip(args, argt)):
                if t is ctypes.c_void_p:
                    v = a.value if isinstance(a, ctypes.c_void_p) else a
                    if i == len(args) - 1 and self.has_stream[name]:
                        out.append("s%d" % self.streams.setdefault(v or 0, len(self.streams)))
                    else:
                        out.append("p" if v else "0")
                elif t is ctypes.c_float or t is ctypes.c_double:
                    out.append(repr(float(a)))
                else:
                    out.append(str(int(a)))
            self.lines.append(" ".join(out))
        return self.real(name, *args)


# ---- parameters and inputs ------------------------------------------------------------------------------------------------------
def _fill(h, k, mul=1.0 / 32, add=0.0):
    h.t.copy_((dyadic(h.numel, k).reshape(h.shape) * mul + add).to(h.t.device))


def _act(shape, k, dt, relu=False, grad=True):
    n = 1
    for s in shape:
        n *= s
    x = dyadic(n, k).reshape(shape)
    if relu:
        x = torch.relu(x)
    return x.to(dt).cuda().requires_grad_(grad)


def _dy(y, k):
    """the incoming gradient of an output: 1/64 of the formula's values (fp16 products stay far from its range)"""
    return (dyadic(y.numel(), k).reshape(y.shape) / 64).to(y.dtype).cuda()


class _Net:
    """a ParamStore with its FrozenBN folder: layers are declared, then finish() allocates and fills the arena from the formula"""

    def __init__(self):
        from ubteacher.modeling.backbone import BNFolder
        from ubteacher.params import ParamStore
        self.store = ParamStore()
        self.folder = BNFolder(self.store)
        self.around_075 = []

    def conv_bn(self, cin, cout, k, stride, pad, relu, groups=1):
        from ubteacher.modeling.backbone import _conv_bn
        return _conv_bn(self.store, self.folder, "l%d" % len(self.store.handles), cin, cout, k, stride, pad, relu, True, groups=groups)

    def conv(self, cin, cout, k, stride, pad, relu=False, **kw):
        from ubteacher import ops
        w = self.store.new((cout, k * k * cin), "decay")
        b = self.store.new((cout,), "decay")
        return ops.Conv(w, cin, cout, k, stride, pad, bias=b, relu=relu, **kw)

    def gn(self, C, groups):
        from ubteacher import ops
        gamma, beta = self.store.new((C,), "nodecay"), self.store.new((C,), "nodecay")
        self.around_075.append(gamma)
        return ops.GroupNormReLU(gamma, beta, groups, 1e-5, True)

    def finish(self):
        self.store.finalize("cuda")
        for i, h in enumerate(self.store.handles):
            if h.kind in ("bn_w", "bn_v") or any(h is g for g in self.around_075):
                _fill(h, 101 + i, 1.0 / 8, 0.75)          # FrozenBN weight / running variance, GroupNorm gamma: in [0.5, 1)
            else:
                _fill(h, 101 + i, 1.0 / 32)
        self.folder.materialize()
        self.folder.fold()
        return self

    def grads(self):
        return {"param%02d_%s" % (i, h.kind): h.g for i, h in enumerate(self.store.handles) if h.g is not None}


def _meta():
    from ubteacher import ops
    return ops.LevelMeta(N, LEVELS)


# ---- layer cases: name -> fn(dt) -> (outputs, their gradients, {name: gradient tensor} after backward) ------------------------------
def _nhwc(cin, cout, k, stride, pad, hw, bn, relu=False, residual=False, premask=False):
    def case(dt):
        net = _Net()
        layer = net.conv_bn(cin, cout, k, stride, pad, relu) if bn else net.conv(cin, cout, k, stride, pad, relu)
        layer.premask_input = premask
        net.finish()
        x = _act((N, hw, hw, cin), 1, dt, relu=premask)
        oh = (hw + 2 * pad - k) // stride + 1
        res = _act((N, oh, oh, cout), 2, dt) if residual else None
        y = layer(x, residual=res)
        return [y], [_dy(y, 3)], lambda: dict(net.grads(), dx=x.grad, **({"gres": res.grad} if residual else {}))
    return case


def _grouped(stride, premask, out_fp32=False):
    def case(dt):
        net = _Net()
        layer = net.conv_bn(64, 64, 3, stride, 1, True, groups=8)
        layer.premask_input, layer.out_fp32 = premask, out_fp32     # out_fp32: an fp32 gradient arrives at 16-bit weights
        net.finish()
        x = _act((N, 9, 9, 64), 1, dt, relu=premask)
        y = layer(x)
        return [y], [_dy(y, 3)], lambda: dict(net.grads(), dx=x.grad)
    return case


class _SyncStub:
    """stands in for utils.grad_sync.GradBuckets (data parallel): counts the handles each notification names"""

    def __init__(self):
        self.seen = []

    def on_forward(self, handles):
        self.seen.append(len(handles))

    def on_backward_done(self, handles):
        self.seen.append(100 + len(handles))


def _grad_sync(dt):
    """a grouped FrozenBN conv into a biased 3x3 conv with ops.GRAD_SYNC set: both backwards report their handles"""
    from ubteacher import ops
    ops.GRAD_SYNC[0] = stub = _SyncStub()      # _fresh_host_state registered the slot: the monkeypatch's undo restores it
    net = _Net()
    a, b = net.conv_bn(64, 64, 3, 1, 1, True, groups=8), net.conv(64, 64, 3, 1, 1)
    net.finish()
    x = _act((N, 8, 8, 64), 1, dt)
    y = b(a(x))
    return [y], [_dy(y, 3)], lambda: dict(net.grads(), dx=x.grad, notified=torch.tensor(stub.seen, dtype=torch.int32))


def _box_head(net, C, discrete):
    """the bbox prediction conv and its per-level Scale handles as modeling/fcos.py builds them"""
    from ubteacher import ops
    from ubteacher.modeling import fcos
    reg_max = 16 if discrete else 0          # MODEL.FCOS.REG_MAX / hip.REG_CONT
    R4 = 4 * (reg_max + 1)
    bs = fcos.BOX_STRIDE if discrete else fcos.BOX_STRIDE_CONT
    wb, bb = net.store.new((bs, 9 * C), "decay"), net.store.new((bs,), "decay")
    head = ops.Conv(wb, C, bs, 3, 1, 1, bias=bb, colscale=R4, out_fp32=True)
    head.dgrad_pad_small = not discrete
    return head, [net.store.new((1,), "decay") for _ in LEVELS]


def _set_scales(scales):
    for l, h in enumerate(scales):
        h.t.fill_(1.0 + 0.25 * l)


def _bbox_pred(discrete, input_grad=True):
    def case(dt):
        net = _Net()
        head, scales = _box_head(net, 128, discrete)
        net.finish()
        _set_scales(scales)
        meta = _meta()
        x = _act((meta.P, 128), 1, dt, grad=input_grad)
        y = head(x, meta=meta, colscale_handle=scales)
        return [y], [_dy(y, 3)], lambda: dict(net.grads(), **({"dx": x.grad} if input_grad else {}))
    return case


def _levels(cin, cout, relu=False, out_fp32=False, fanin=False):
    def case(dt):
        from ubteacher import ops
        net = _Net()
        layer = net.conv(cin, cout, 3, 1, 1, relu, out_fp32=out_fp32)
        net.finish()
        meta = _meta()
        x = _act((meta.P, cin), 1, dt)
        if fanin and ops.fanin_enabled():      # as RoIAlign's backward does before the RPN conv's dgrad runs (16-bit modes only)
            x._utv2_fanin = ops.FanIn(meta, 2)
            buf, _ = x._utv2_fanin.store(cin, dt, x.device)
            buf.copy_(_dy(buf, 5))
        y = layer(x, meta=meta)
        return [y], [_dy(y, 3)], lambda: dict(net.grads(), dx=x.grad)
    return case


def _matrix_1x1(dt):
    """the RPN's prediction conv (modeling/rcnn.py): 1x1 on the level-first ReLU output of the RPN conv, fp32 output, premasked input"""
    net = _Net()
    layer = net.conv(64, 16, 1, 1, 0, out_fp32=True)
    layer.premask_input = True
    net.finish()
    meta = _meta()
    x = _act((meta.P, 64), 1, dt, relu=True)
    y = layer(x, meta=meta)
    return [y], [_dy(y, 3)], lambda: dict(net.grads(), dx=x.grad)


def _paired_tower(dt):
    """two depths of the paired FCOS towers at C = 128 (conv -> GroupNorm(32) -> ReLU; depth 1 grouped, its dgrad on the GroupNorm-backward
    route), split_cols, and the two prediction convs (80 classes; the discrete box head with its Scales) as the halves' consumers"""
    from ubteacher import ops
    C = 128
    net = _Net()
    layers = []
    for i in range(2):
        w, b = net.store.new((2 * C, 9 * C), "decay"), net.store.new((2 * C,), "decay")
        conv = ops.Conv(w, C, 2 * C, 3, 1, 1, bias=b, groups=1 if i == 0 else 2)
        conv.defer_wgrad = True
        layers.append(ops.pair_conv_gn(conv, net.gn(2 * C, 32)))
        if i > 0:
            ops.chain_gn_conv(layers[i - 1][1], conv)
    cls = net.conv(C, 80, 3, 1, 1, out_fp32=True)
    head, scales = _box_head(net, C, True)
    net.finish()
    _set_scales(scales)
    meta = _meta()
    x = _act((meta.P, C), 1, dt)
    t = x
    for conv, gn in layers:
        t = gn(conv(t, meta=meta), meta)
    tc, tb = ops.split_cols(t)
    logits, box = cls(tc, meta=meta), head(tb, meta=meta, colscale_handle=scales)
    return [logits, box], [_dy(logits, 3), _dy(box, 7)], lambda: dict(net.grads(), dx=x.grad)


LAYER_CASES = {
    "nhwc_1x1_s1_64_64_bn_relu_res": _nhwc(64, 64, 1, 1, 0, 8, bn=True, relu=True, residual=True),
    "nhwc_1x1_s1_64_256_bn": _nhwc(64, 256, 1, 1, 0, 8, bn=True),
    "nhwc_1x1_s2_64_128_bn_premask": _nhwc(64, 128, 1, 2, 0, 9, bn=True, premask=True),
    "nhwc_3x3_s2_64_64_bias": _nhwc(64, 64, 3, 2, 1, 9, bn=False),
    "nhwc_3x3_s2_64_40_bias": _nhwc(64, 40, 3, 2, 1, 9, bn=False),
    "nhwc_3x3_s1_64_64_bias_relu": _nhwc(64, 64, 3, 1, 1, 8, bn=False, relu=True),
    "nhwc_3x3_s1_64_80_bias": _nhwc(64, 80, 3, 1, 1, 8, bn=False),
    "grouped_s1": _grouped(1, False),
    "grouped_s1_premask": _grouped(1, True),
    "grouped_s2": _grouped(2, False),
    "grouped_s2_premask": _grouped(2, True),
    "grouped_s1_out_fp32": _grouped(1, False, out_fp32=True),
    "grad_sync_notified": _grad_sync,
    "paired_tower": _paired_tower,
    "levels_3x3_128_80_bias": _levels(128, 80, out_fp32=True),
    "bbox_pred_discrete": _bbox_pred(True),
    "bbox_pred_continuous": _bbox_pred(False),
    "bbox_pred_discrete_no_input_grad": _bbox_pred(True, input_grad=False),
    "levels_3x3_64_64_relu_fanin": _levels(64, 64, relu=True, fanin=True),
    "matrix_1x1_64_16_premask": _matrix_1x1,
}


def _fresh_host_state(mp):
    """what a trace would otherwise inherit from earlier tests of the process"""
    from ubteacher import hip, ops
    mp.setattr(hip, "_rowinfo_cache", {})
    mp.setitem(ops._WGRAD, "lane_of", {})
    mp.setitem(ops._WGRAD, "next", 0)
    mp.setattr(ops, "GRAD_SYNC", [None])
    for k in [k for k in os.environ if k.startswith("UTV2_") and k not in ("UTV2_LIB_DIR", "UTV2_TEST_THREADS")]:
        mp.delenv(k)


def _recorded_backward(rec, run):
    from ubteacher import ops
    rec.on = True
    ops.wgrad_side_stream(True)
    try:
        run()
        ops.FanIn.check()
    finally:
        ops.wgrad_side_stream(False)
        ops.join_wgrad_stream()
        rec.on = False
    torch.cuda.synchronize()


def layer_record(name, kind, mp):
    """mp: a pytest MonkeyPatch (the test's fixture; the generator makes its own)"""
    from ubteacher import hip
    _fresh_host_state(mp)
    rec = Recorder(hip)
    mp.setattr(hip, "call", rec)
    outs, douts, grads = LAYER_CASES[name](select(kind))
    _recorded_backward(rec, lambda: torch.autograd.backward(outs, douts))
    return {"trace": rec.lines, "digests": {k: digest(v) for k, v in grads().items() if v is not None}}


# ---- whole-backward cases ---------------------------------------------------------------------------------------------------------
_TUNED = {}


def _trainer(model, kind, mp):
    """the trainer of tests/test_fcos_step_gpu.py / test_rcnn_step_gpu.py on their 2 + 2 batch, in precision `kind`"""
    from tests.utv2_testutil import FixedLoader, cpu_state, make_batch, rcnn_tune, small_fcos_cfg, tune_state_for_pseudo_labels
    from ubteacher.presets import get_config
    if kind != "fp32":
        mp.setenv("UTV2_PRECISION", kind)
    torch.manual_seed(0)
    if model == "fcos":
        from ubteacher.engine import UBTeacherTrainer as Trainer
        cfg = small_fcos_cfg()
        prod, orac = make_batch(12, 2, 2, STEP_H, STEP_W, "cuda")
    else:
        from ubteacher.engine import UBRCNNTeacherTrainer as Trainer
        cfg = get_config("rcnn", 1, ["SOLVER.IMG_PER_BATCH_LABEL", 2, "SOLVER.IMG_PER_BATCH_UNLABEL", 2, "SEMISUPNET.BURN_UP_STEP", 0,
                                     "MODEL.DEVICE", "cuda"])
        prod, orac = make_batch(31, 2, 2, STEP_H, STEP_W, "cuda")
    cfg.SOLVER.AMP.ENABLED = kind != "fp32"
    tr = Trainer(cfg, data_loader=FixedLoader(prod))
    if model not in _TUNED:     # the same seeded initial state in every kind: tuned once (the oracle's CPU forward)
        images = [d["image"] for d in orac[3]]
        if model == "fcos":
            _TUNED[model] = tune_state_for_pseudo_labels(cpu_state(tr.model), images)
        else:
            _TUNED[model] = rcnn_tune(cpu_state(tr.model), images, torch.tensor(cfg.MODEL.PIXEL_MEAN).view(3, 1, 1),
                                      torch.tensor(cfg.MODEL.PIXEL_STD).view(3, 1, 1))
    tr.model.load_state_dict(_TUNED[model])
    tr.model_teacher.load_state_dict(_TUNED[model])
    if model == "rcnn":
        g = torch.Generator().manual_seed(99)
        tr.model.proposal_generator.sample_keys = tr.model.roi_heads.sample_keys = lambda n, m, device: torch.rand(n, m, generator=g).to(device)
    tr.iter = 1
    tr.optimizer.param_groups[0]["lr"] = 1e-3
    return tr


def step_record(model, kind, mp):
    from ubteacher import hip
    _fresh_host_state(mp)
    rec = Recorder(hip)
    mp.setattr(hip, "call", rec)
    tr = _trainer(model, kind, mp)
    digests = {}
    inner = tr._backward

    def backward(losses):
        _fresh_host_state(mp)          # the forward filled the geometry cache: the backward's trace starts from an empty one
        rec.on = True
        try:
            inner(losses)
        finally:
            rec.on = False
        torch.cuda.synchronize()
        store = tr.model.store
        digests["arena"] = digest(store.grad)
        groups = {}
        for key, (_, g) in store.trainable_named().items():
            groups.setdefault(".".join(key.split(".")[:2]), []).append(g.reshape(-1).float())
        for prefix, gs in groups.items():
            digests[prefix] = digest(torch.cat(gs))
    tr._backward = backward
    tr.run_step_full_semisup()
    torch.cuda.synchronize()
    assert "arena" in digests
    return {"trace": rec.lines, "digests": digests}


# ---- the tests -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


def check(cid, kind, got):
    want = fixture()[cid][kind]
    for i, (a, b) in enumerate(zip(got["trace"], want["trace"])):
        assert a == b, "%s %s: call %d is\n  %s\nthe fixture's commit made\n  %s" % (cid, kind, i, a, b)
    assert len(got["trace"]) == len(want["trace"]), (cid, kind, got["trace"][len(want["trace"]):], want["trace"][len(got["trace"]):])
    missing = sorted(k for k in want["digests"] if k not in got["digests"])
    assert not missing, (cid, kind, missing)
    differ = sorted(k for k in want["digests"] if got["digests"][k] != want["digests"][k])
    assert not differ, "%s %s: other bytes than the fixture's commit in %s" % (cid, kind, differ)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(LAYER_CASES))
def test_layer_backward_is_the_fixture_commits(name, kind, monkeypatch):
    got = layer_record(name, kind, monkeypatch)
    assert sorted(got["digests"]) == sorted(fixture()[name][kind]["digests"]), (name, kind)
    check(name, kind, got)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("model", ["fcos", "rcnn"])
def test_whole_backward_is_the_fixture_commits(model, kind, monkeypatch):
    check("step_" + model, kind, step_record(model, kind, monkeypatch))


def _child(out_path):
    """the paired-tower case, forward and backward, in the environment the parent test set: what it raised, how often the fused entry
    point was called, the digests"""
    from ubteacher import hip
    mp = pytest.MonkeyPatch()
    res = {"error": None, "gnb_calls": 0, "digests": {}}
    try:
        keep = {k: os.environ[k] for k in ("UTV2_EPI_PLAIN", "UTV2_GN_BWD_FUSE") if k in os.environ}
        _fresh_host_state(mp)
        for k, v in keep.items():
            mp.setenv(k, v)
        rec = Recorder(hip)
        mp.setattr(hip, "call", rec)
        outs, douts, grads = _paired_tower(select("fp16"))
        _recorded_backward(rec, lambda: torch.autograd.backward(outs, douts))
        res["gnb_calls"] = sum(l.startswith("utv2_conv2d_ml_fwd_bf16_gnb ") for l in rec.lines)
        res["digests"] = {k: digest(v) for k, v in grads().items()}
    except Exception as e:  # noqa: BLE001
        res["error"] = "%s: %s" % (type(e).__name__, e)
    finally:
        mp.undo()
    with open(out_path, "w") as f:
        json.dump(res, f)


def test_epi_plain_switch_takes_the_unfused_dgrad(tmp_path):
    """UTV2_EPI_PLAIN=0 with the default UTV2_GN_BWD_FUSE=1: no exception, no utv2_conv2d_ml_fwd_bf16_gnb call, and the gradients of a
    second child with UTV2_GN_BWD_FUSE=0 (default epilogues), bit for bit.  At the fixture's commit the first child raised
    "utv2_conv2d_ml_fwd_bf16_gnb failed with code ..." (hip.gnb_eligible did not know the switch: ADVICE.md round 6, item 3)."""
    res = {}
    for tag, env in (("plain0", {"UTV2_EPI_PLAIN": "0"}), ("fuse0", {"UTV2_GN_BWD_FUSE": "0"})):
        out = str(tmp_path / (tag + ".json"))
        e = {k: v for k, v in os.environ.items() if k not in ("UTV2_EPI_PLAIN", "UTV2_GN_BWD_FUSE")}
        e.update(env)
        p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), out], env=e, capture_output=True, text=True)
        assert p.returncode == 0, (tag, p.returncode, p.stderr[-2000:])
        with open(out) as f:
            res[tag] = json.load(f)
        assert res[tag]["error"] is None, (tag, res[tag]["error"])
        assert res[tag]["gnb_calls"] == 0, (tag, res[tag]["gnb_calls"])
    assert res["plain0"]["digests"] and res["plain0"]["digests"] == res["fuse0"]["digests"]


if __name__ == "__main__":
    _child(sys.argv[1])
