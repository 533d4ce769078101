"""ResNet-18 / 34 / 50 / 101 / 152 and ResNeXt + FPN on the HIP conv path.

Behavioural spec: Detectron2 v0.6 ResNet (DEPTH, RES2_OUT_CHANNELS, NUM_GROUPS, WIDTH_PER_GROUP, STRIDE_IN_1X1, FrozenBN, FREEZE_AT) and FPN
[D2-recall, SURVEY.md appendix C]; FCOS top block: reference ubteacher/modeling/backbone/fpn.py:11-78
(P6 = conv3x3 s2 (P5), P7 = conv3x3 s2 (relu(P6))).  State-dict keys follow Detectron2's
(`bottom_up.stem.conv1.weight`, `bottom_up.res3.0.conv1.norm.running_mean`, `fpn_lateral3.weight`,
`top_block.p6.weight`, ...) so checkpoints stay interchangeable.

MI355X mapping: every conv is one implicit-GEMM launch with FrozenBN/ReLU/residual fused in
the epilogue (a grouped ResNeXt conv2: one launch of csrc/conv_grouped.hip for all groups); stem+res2 (frozen) run outside autograd; the image batch enters as NHWC4.
"""
import math
import os

import torch

from .. import hip, ops
from ..d2.registry import BACKBONE_REGISTRY


def _nchw_view(cout, cin, k):
    """[cout, k*k*cin] arena matrix -> [cout, cin, k, k]-shaped strided view (state_dict surface)."""
    def fn(t):
        return t.view(cout, k, k, cin).permute(0, 3, 1, 2)
    return fn


def _msra_init(cout, cin, k):
    def fn(t):  # kaiming_normal_(mode="fan_out", nonlinearity="relu")
        std = math.sqrt(2.0 / (cout * k * k))
        t.normal_(0.0, std)
    return fn


def _xavier_init(cout, cin, k):
    def fn(t):  # c2_xavier_fill: kaiming_uniform_(a=1)  -> bound = sqrt(3 / fan_in)
        bound = math.sqrt(3.0 / (cin * k * k))
        t.uniform_(-bound, bound)
    return fn


class FrozenBN:
    """Four per-channel buffers; folded to scale/shift by one launch for all layers (utv2_frozenbn_fold)."""

    def __init__(self, store, prefix, c):
        self.w = store.new((c,), "bn_w", lambda t: t.fill_(1.0)).export(prefix + ".weight")
        self.b = store.new((c,), "bn_b", lambda t: t.zero_()).export(prefix + ".bias")
        self.m = store.new((c,), "bn_m", lambda t: t.zero_()).export(prefix + ".running_mean")
        # D2 FrozenBatchNorm2d initialises running_var to 1 - eps so that an affine-only checkpoint (R-50.pkl has no running
        # statistics) yields scale == weight exactly [D2-recall]
        self.v = store.new((c,), "bn_v", lambda t: t.fill_(1.0 - 1e-5)).export(prefix + ".running_var")
        self.c = c
        self.scale = None
        self.shift = None


class BNFolder:
    def __init__(self, store):
        self.store = store
        self.layers = []
        self.scale_all = None

    def add(self, bn):
        self.layers.append(bn)
        return bn

    def materialize(self):
        st = self.store
        s0, e0 = st.ranges["bn_w"]
        n = e0 - s0
        self.n = n
        self.scale_all = torch.empty(n, dtype=torch.float32, device=st.flat.device)
        self.shift_all = torch.empty(n, dtype=torch.float32, device=st.flat.device)
        for bn in self.layers:
            o = bn.w.offset - s0
            bn.scale = self.scale_all[o: o + bn.c]
            bn.shift = self.shift_all[o: o + bn.c]

    def fold(self, eps=1e-5):
        if self.n == 0:
            return
        st = self.store
        hip.frozenbn_fold(st.region("bn_w"), st.region("bn_b"), st.region("bn_m"), st.region("bn_v"),
                          self.scale_all, self.shift_all, eps)


def _conv_bn(store, folder, prefix, cin, cout, k, stride, pad, relu, trainable, groups=1):
    kind = "decay" if trainable else "frozen"
    cg = cin // groups      # input channels per group: the weight is [cout, k * k * cg] ([cout, cg, k, k] in the state dict)
    w = store.new((cout, k * k * cg), kind, _msra_init(cout, cg, k)).export(prefix + ".weight", _nchw_view(cout, cg, k))
    bn = folder.add(FrozenBN(store, prefix + ".norm", cout))
    return ops.Conv(w, cg, cout, k, stride, pad, bias=None, bn=bn, relu=relu, trainable=trainable, groups=groups)


class Bottleneck:
    def __init__(self, store, folder, prefix, cin, cout, mid, stride, trainable, groups=1, stride_in_1x1=True):
        # STRIDE_IN_1X1: the stride sits on conv1 (True) or on the 3x3 conv2 (False); the shortcut always carries it
        s1, s3 = (stride, 1) if stride_in_1x1 else (1, stride)
        self.conv1 = _conv_bn(store, folder, prefix + ".conv1", cin, mid, 1, s1, 0, True, trainable)
        self.conv2 = _conv_bn(store, folder, prefix + ".conv2", mid, mid, 3, s3, 1, True, trainable, groups=groups)
        self.conv3 = _conv_bn(store, folder, prefix + ".conv3", mid, cout, 1, 1, 0, True, trainable)  # relu after add
        self.shortcut = None
        if cin != cout:
            self.shortcut = _conv_bn(store, folder, prefix + ".shortcut", cin, cout, 1, stride, 0, False, trainable)
        # backward of the fused AMP node (ops._BottleneckFn): input_relu - the gradient returned for the input is masked by input > 0
        # in the dgrad epilogue; grad_premasked - every consumer of this block's output does the same, so no mask pass of its own.
        # Both are switched on by the FPN builder, which knows all consumers of the stage outputs.
        self.input_relu = False
        self.grad_premasked = False

    def __call__(self, x):
        return ops.bottleneck(self, x)


class BasicBlock:
    """Detectron2 BasicBlock (R-18 / R-34): conv1 3x3 (carries the stride) + FrozenBN + ReLU, conv2 3x3 + FrozenBN, a 1x1 shortcut conv +
    FrozenBN only where the channel count changes (the first block of res3 / res4 / res5), relu(conv2 + shortcut)."""

    def __init__(self, store, folder, prefix, cin, cout, stride, trainable):
        self.conv1 = _conv_bn(store, folder, prefix + ".conv1", cin, cout, 3, stride, 1, True, trainable)
        self.conv2 = _conv_bn(store, folder, prefix + ".conv2", cout, cout, 3, 1, 1, True, trainable)  # relu after add
        self.shortcut = None
        if cin != cout:
            self.shortcut = _conv_bn(store, folder, prefix + ".shortcut", cin, cout, 1, stride, 0, False, trainable)

    def __call__(self, x):
        return ops.basic_block(self, x)


# Detectron2 build_resnet_backbone: blocks per stage; 18 / 34 are built from BasicBlock, the others from Bottleneck
RESNET_DEPTHS = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3), 50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}
BASIC_BLOCK_DEPTHS = (18, 34)


def resnet_spec(cfg):
    """(blocks per stage, groups, width per group, stride_in_1x1) of cfg.MODEL.RESNETS, or NotImplementedError naming the key of a
    configuration this backbone does not build (it would otherwise be built as something else without a word).  The BasicBlock depths
    (cfg.MODEL.RESNETS.DEPTH in BASIC_BLOCK_DEPTHS) come with RES2_OUT_CHANNELS 64, one group of width 64 (Detectron2's assertions)."""
    r = cfg.MODEL.RESNETS
    if r.DEPTH not in RESNET_DEPTHS:
        raise NotImplementedError("MODEL.RESNETS.DEPTH %r: only the depths %s are built" % (r.DEPTH, sorted(RESNET_DEPTHS)))
    basic = r.DEPTH in BASIC_BLOCK_DEPTHS
    if basic and r.RES2_OUT_CHANNELS != 64:
        raise NotImplementedError("MODEL.RESNETS.DEPTH %r is built from BasicBlocks and needs MODEL.RESNETS.RES2_OUT_CHANNELS 64 (got %r)"
                                  % (r.DEPTH, r.RES2_OUT_CHANNELS))
    if any(bool(d) for d in r.DEFORM_ON_PER_STAGE):
        raise NotImplementedError("MODEL.RESNETS.DEFORM_ON_PER_STAGE %r: deformable convolutions are not built" % (list(r.DEFORM_ON_PER_STAGE),))
    if r.RES5_DILATION != 1:
        raise NotImplementedError("MODEL.RESNETS.RES5_DILATION %r: only 1 is built" % (r.RES5_DILATION,))
    if r.NORM != "FrozenBN":
        raise NotImplementedError("MODEL.RESNETS.NORM %r: only FrozenBN is built" % (r.NORM,))
    if not basic and r.RES2_OUT_CHANNELS != 256:
        raise NotImplementedError("MODEL.RESNETS.RES2_OUT_CHANNELS %r: the bottleneck depths are built with 256 only (64 goes with DEPTH 18 / 34)"
                                  % (r.RES2_OUT_CHANNELS,))
    if r.STEM_OUT_CHANNELS != 64:
        raise NotImplementedError("MODEL.RESNETS.STEM_OUT_CHANNELS %r: only 64 is built" % (r.STEM_OUT_CHANNELS,))
    if cfg.MODEL.FPN.NORM != "":
        raise NotImplementedError("MODEL.FPN.NORM %r: only '' (no norm) is built" % (cfg.MODEL.FPN.NORM,))
    if cfg.MODEL.FPN.FUSE_TYPE != "sum":
        raise NotImplementedError("MODEL.FPN.FUSE_TYPE %r: only 'sum' is built" % (cfg.MODEL.FPN.FUSE_TYPE,))
    groups, wpg = int(r.NUM_GROUPS), int(r.WIDTH_PER_GROUP)
    if basic and groups != 1:
        raise NotImplementedError("MODEL.RESNETS.NUM_GROUPS %r: DEPTH %r (BasicBlocks) takes 1 only" % (groups, r.DEPTH))
    if basic and wpg != 64:
        raise NotImplementedError("MODEL.RESNETS.WIDTH_PER_GROUP %r: DEPTH %r (BasicBlocks) takes 64 only" % (wpg, r.DEPTH))
    if groups > 1 and wpg % 4:
        raise NotImplementedError("MODEL.RESNETS.WIDTH_PER_GROUP %r: the grouped conv kernels take a multiple of 4 channels per group" % wpg)
    return RESNET_DEPTHS[r.DEPTH], groups, wpg, bool(r.STRIDE_IN_1X1)


class ResNet:
    """Detectron2 build_resnet_backbone: bottleneck ResNets / ResNeXts (DEPTH 50 / 101 / 152, NUM_GROUPS x WIDTH_PER_GROUP bottleneck
    width of res2, doubling per stage; only conv2 is grouped; STRIDE_IN_1X1) and, with basic=True, the BasicBlock ResNets (DEPTH 18 / 34).
    Stage output widths are res2_out * 2^i.  FrozenBN, FREEZE_AT."""

    def __init__(self, store, folder, prefix, out_features, freeze_at=2, num_blocks=(3, 4, 6, 3), groups=1, width_per_group=64,
                 stride_in_1x1=True, basic=False, res2_out=256):
        self.out_features = out_features
        # stem on the NHWC4 image: [64][7*7*4 -> padded to 208]
        def stem_init(t):
            t.zero_()
            w = torch.empty(64, 7, 7, 3, device=t.device).normal_(0.0, math.sqrt(2.0 / (64 * 49)))
            t.view(64, 208)[:, :196].view(64, 7, 7, 4)[..., :3].copy_(w)
        stem_train = freeze_at < 1
        self.stem_w = store.new((64, 208), "decay" if stem_train else "frozen", stem_init).export(
            prefix + ".stem.conv1.weight", lambda t: torch.as_strided(t, (64, 3, 7, 7), (208, 1, 28, 4), t.storage_offset()))
        self.stem_bn = folder.add(FrozenBN(store, prefix + ".stem.conv1.norm", 64))
        self.stem = ops.Conv(self.stem_w, 4, 64, 7, 2, 3, bn=self.stem_bn, relu=True, trainable=stem_train, kred=208)
        self.stages = []
        self.channels = {}
        cin = 64
        for si, nblocks in enumerate(num_blocks):
            name, mid, cout = "res%d" % (si + 2), groups * width_per_group * 2 ** si, res2_out * 2 ** si
            trainable = freeze_at < si + 2
            blocks = []
            for b in range(nblocks):
                stride = 2 if (b == 0 and name != "res2") else 1
                bp = "%s.%s.%d" % (prefix, name, b)
                if basic:
                    blocks.append(BasicBlock(store, folder, bp, cin, cout, stride, trainable))
                else:
                    blocks.append(Bottleneck(store, folder, bp, cin, cout, mid, stride, trainable, groups, stride_in_1x1))
                cin = cout
            self.stages.append((name, blocks, trainable))
            self.channels[name] = cout
        self.strides = {"res2": 4, "res3": 8, "res4": 16, "res5": 32}

    def __call__(self, x4):
        outs = {}
        if self.stem.trainable and torch.is_grad_enabled():
            # MODEL.BACKBONE.FREEZE_AT < 1: the stem trains (ops._StemFn; the image comes as fp32 NHWC4 in every precision mode)
            assert x4.dtype == torch.float32 and x4.shape[-1] == 4, "a trainable stem takes the fp32 NHWC4 image"
            x = ops.stem(self.stem, x4)
            for name, blocks, trainable in self.stages:
                for b in blocks:
                    x = b(x)
                if name in self.out_features:
                    outs[name] = x
            return outs
        # frozen stem + pool run outside autograd; under AMP the bf16 activation pipeline starts at the stem's output
        sc, sh = self.stem.scale_shift()
        if x4.dtype == hip.h16_dtype():  # AMP: 16-bit MFMA stem on the zero-bordered 16-bit image
            v = (self.stem_w.store.version, hip.H16[0])
            if getattr(self, "_w16s_version", None) != v:
                self._w16s = hip.stem_weight_image(self.stem_w.t)
                self._w16s_version = v
            if os.environ.get("UTV2_FUSED_STEM_POOL", "1") != "0" and self._w16s.shape[0] == 64:
                x = hip.stem_pool_fwd_bf16(x4, self._w16s, sc, sh)      # conv + FrozenBN + ReLU + max pool, the conv output stays in LDS
            else:
                x = hip.maxpool3x3s2(hip.conv2d_stem_fwd_bf16(x4, self._w16s, sc, sh, True, hip.h16_dtype()))
        else:
            x = hip.maxpool3x3s2(hip.conv2d_stem_fwd(x4, self.stem_w.t, sc, sh, 2, 3, 7, 7, True, ops.act_dtype()))
        for name, blocks, trainable in self.stages:
            if trainable:
                for b in blocks:
                    x = b(x)
            else:
                with torch.no_grad():
                    for b in blocks:
                        x = b(x)
            if name in self.out_features:
                outs[name] = x
        return outs


def ResNet50(store, folder, prefix, out_features, freeze_at=2):
    """the R-50 of the shipped configs (kept importable under its old name)"""
    return ResNet(store, folder, prefix, out_features, freeze_at)


def build_resnet(cfg, store, folder, prefix):
    blocks, groups, wpg, s1x1 = resnet_spec(cfg)
    r = cfg.MODEL.RESNETS
    return ResNet(store, folder, prefix, r.OUT_FEATURES, cfg.MODEL.BACKBONE.FREEZE_AT, blocks, groups, wpg, s1x1,
                  basic=r.DEPTH in BASIC_BLOCK_DEPTHS, res2_out=int(r.RES2_OUT_CHANNELS))


def _conv_bias(store, prefix, cin, cout, k, stride, pad, init, relu=False):
    w = store.new((cout, k * k * cin), "decay", init(cout, cin, k)).export(prefix + ".weight", _nchw_view(cout, cin, k))
    b = store.new((cout,), "decay", lambda t: t.zero_()).export(prefix + ".bias")
    return ops.Conv(w, cin, cout, k, stride, pad, bias=b, relu=relu, trainable=True)


class FPN:
    """lateral 1x1 + top-down nearest x2 sum + output 3x3 (FUSE_TYPE sum, NORM '')."""

    def __init__(self, store, folder, cfg, top_block_kind):
        self.bottom_up = build_resnet(cfg, store, folder, "backbone.bottom_up")
        self.in_features = list(cfg.MODEL.FPN.IN_FEATURES)
        oc = cfg.MODEL.FPN.OUT_CHANNELS
        self.out_channels = oc
        self.lateral, self.output = {}, {}
        for f in self.in_features:
            stage = int(math.log2(self.bottom_up.strides[f]))
            self.lateral[f] = _conv_bias(store, "backbone.fpn_lateral%d" % stage, self.bottom_up.channels[f], oc, 1, 1, 0, _xavier_init)
            self.output[f] = _conv_bias(store, "backbone.fpn_output%d" % stage, oc, oc, 3, 1, 1, _xavier_init)
        # Gradient pre-masking (ops.premask_on): a stage output is consumed by the next block / next stage's first block and by this
        # stage's lateral only, and all of them mask the gradient they return by (output > 0) in their dgrad epilogue - so the fused
        # bottlenecks of the trainable stages skip the mask pass at the top of their backward.  BasicBlock stages (R-18 / R-34) run as
        # plain ops.Conv nodes, each of which masks its own incoming gradient: nothing is pre-masked for them, blocks or laterals.
        for name, blocks, trainable in self.bottom_up.stages:
            if trainable and all(isinstance(blk, Bottleneck) for blk in blocks):
                for blk in blocks:
                    blk.input_relu = True
                    blk.grad_premasked = True
                if name in self.lateral:
                    self.lateral[name].premask_input = True
        self.top_block_kind = top_block_kind
        self.levels_fp32 = False  # every consumer of the level buffer (tower / RPN convs, RoIAlign) takes bf16 under AMP
        self.top = []
        if top_block_kind == "p6p7":
            self.top = [_conv_bias(store, "backbone.top_block.p6", oc, oc, 3, 2, 1, _xavier_init),
                        _conv_bias(store, "backbone.top_block.p7", oc, oc, 3, 2, 1, _xavier_init)]
        elif top_block_kind == "p6":
            self.top = [_conv_bias(store, "backbone.top_block.p6", oc, oc, 3, 2, 1, _xavier_init)]
        stages = [int(math.log2(self.bottom_up.strides[f])) for f in self.in_features]
        self.out_names = ["p%d" % s for s in stages]
        last = stages[-1]
        ntop = {"p6p7": 2, "p6": 1, "maxpool": 1, "none": 0}[top_block_kind]
        self.out_names += ["p%d" % (last + 1 + i) for i in range(ntop)]
        self.size_divisibility = self.bottom_up.strides[self.in_features[-1]]

    def __call__(self, x4):
        """Returns {p_l: NHWC level tensor}.  All levels are rows of ONE level-first buffer
        (`results["_levelfirst"] = (big [P,C], LevelMeta)`) so shared heads run one launch for all levels."""
        feats = self.bottom_up(x4)
        N = x4.shape[0]
        C = self.out_channels
        hw = {}
        for f in self.in_features:
            hw["p%d" % int(math.log2(self.bottom_up.strides[f]))] = (feats[f].shape[1], feats[f].shape[2])
        last = "p%d" % int(math.log2(self.bottom_up.strides[self.in_features[-1]]))
        nlast = int(last[1:])
        h, w = hw[last]
        for i in range(len(self.out_names) - len(self.in_features)):
            h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1   # conv3x3 s2 p1 == max_pool(k1,s2) output size
            hw["p%d" % (nlast + 1 + i)] = (h, w)
        meta = ops.LevelMeta(N, [hw[k] for k in self.out_names])
        big = torch.empty((meta.P, C), dtype=torch.float32 if self.levels_fp32 else ops.act_dtype(), device=x4.device)
        slot = {k: meta.alias_view(big, i) for i, k in enumerate(self.out_names)}
        results = {}
        prev = None
        for f in reversed(self.in_features):
            lat = self.lateral[f](feats[f])
            if prev is not None:
                lat = ops.upsample2x_add(lat, prev)
            prev = lat
            name = "p%d" % int(math.log2(self.bottom_up.strides[f]))
            results[name] = self.output[f](lat, out=slot[name])
        if self.top_block_kind == "p6p7":
            p6 = self.top[0](results[last], out=slot["p%d" % (nlast + 1)])
            p7 = self.top[1](ops.relu(p6), out=slot["p%d" % (nlast + 2)])
            results["p%d" % (nlast + 1)] = p6
            results["p%d" % (nlast + 2)] = p7
        elif self.top_block_kind == "p6":
            results["p%d" % (nlast + 1)] = self.top[0](results[last], out=slot["p%d" % (nlast + 1)])
        elif self.top_block_kind == "maxpool":
            # LastLevelMaxPool: max_pool2d(kernel 1, stride 2) == strided subsample
            results["p%d" % (nlast + 1)] = ops.subsample2_into(results[last], slot["p%d" % (nlast + 1)])
        out = {k: results[k] for k in self.out_names}
        levels = [out[k] for k in self.out_names]
        if torch.is_grad_enabled() and any(t.requires_grad for t in levels):
            bigt = ops.assemble(big, [(r0, r1, tuple(t.shape)) for (r0, r1), t in zip(meta.rows, levels)], levels)
        else:
            bigt = big
        out["_levelfirst"] = (bigt, meta)
        return out


@BACKBONE_REGISTRY.register()
def build_fcos_resnet_fpn_backbone(cfg, store, folder):
    tl = cfg.MODEL.FCOS.TOP_LEVELS
    return FPN(store, folder, cfg, {2: "p6p7", 1: "p6", 0: "none"}[tl])


@BACKBONE_REGISTRY.register()
def build_resnet_fpn_backbone(cfg, store, folder):
    return FPN(store, folder, cfg, "maxpool")
