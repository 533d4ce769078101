"""Golden vectors of the FCOS head under MODEL.FCOS.NORM "BN", "SyncBN" and "none": the reference's own FCOSHead executed here (CPU, build
container only; the shims of gen_golden.py, which this script imports and does not edit; Detectron2's NaiveSyncBatchNorm is not among
them: a world of one makes it nn.BatchNorm2d [D2-recall], which is the stand-in below).

  fcos_norm.npz   seed, three inputs (5 tiny levels, N = 2, C = 256), and per NORM value: the head outputs of two training calls (labeled,
                  then unlabeled) and one eval call, the running statistics and num_batches_tracked after each training call, and the sorted
                  key list of state_dict() (with shapes).  In a world of one "SyncBN" is "BN" to the bit: the script asserts that every
                  SyncBN array equals its BN counterpart and stores the flag `SyncBN_same_as_BN` in their place.  No weights: the product's head built under the same seed has the same
                  initialisation, which the reference head is loaded with; the norm layers' weight / bias are then perturbed by
                  perturb_norm_params() (the test repeats it), so that gamma and beta take part.

    python tests/golden/gen_golden_fcos_norm.py
"""
import os
import re
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import gen_golden as G  # noqa: E402

SEED = 20240
LEVEL_HW = [(3, 4), (2, 3), (2, 2), (1, 3), (1, 2)]
N, C = 2, 256
NORMS = ("BN", "SyncBN", "none")
PREFIX = "proposal_generator.fcos_head."


def perturb_norm_params(sd, seed):
    """the per-level norm layers' weight and bias of a head state dict (keys ..._tower.K.L.weight / .bias), in sorted key order"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k in sorted(sd):
            if re.search(r"_tower\.\d+\.\d+\.(weight|bias)$", k):
                sd[k] += 0.2 * torch.randn(sd[k].shape, generator=g)


def product_head_state(norm):
    """(the product's configuration - the reference's own keys and defaults -, state dict of the product's FCOSHead (CPU arena)
    initialised under SEED)"""
    saved = {k: v for k, v in sys.modules.items() if k == "ubteacher" or k.startswith("ubteacher.")}
    for k in saved:
        del sys.modules[k]
    pkg = os.path.join(ROOT, "unbiased-teacher-v2_amd")
    sys.path.insert(0, pkg)
    try:
        from ubteacher.modeling.fcos import FCOSHead
        from ubteacher.params import ParamStore
        from ubteacher.presets import get_config
        cfg = get_config("fcos", 1, ["MODEL.DEVICE", "cpu", "MODEL.FCOS.NORM", norm])
        store = ParamStore()
        torch.manual_seed(SEED)
        FCOSHead(cfg, store, C, PREFIX[:-1])
        store.finalize(torch.device("cpu"))
        return cfg, {k: v.detach().clone().contiguous() for k, v in store.state_dict().items()}
    finally:
        sys.path.remove(pkg)
        for k in [k for k in sys.modules if k == "ubteacher" or k.startswith("ubteacher.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def main():
    G.install_shims()
    sys.modules["detectron2.layers"].NaiveSyncBatchNorm = type("NaiveSyncBatchNorm", (torch.nn.BatchNorm2d,), {})   # world of one
    fcos_mod = G._load("ubteacher.modeling.fcos.fcos", G.REF + "/ubteacher/modeling/fcos/fcos.py")
    g = torch.Generator().manual_seed(SEED)
    d = {"seed": np.int64(SEED), "level_hw": np.array(LEVEL_HW, dtype=np.int64)}
    calls = ("labeled", "unlabeled", "eval")
    feats = {c: [torch.randn(N, C, h, w, generator=g) for h, w in LEVEL_HW] for c in calls}
    for c in calls:
        for l in range(len(LEVEL_HW)):
            d["x_%s_%d" % (c, l)] = G.npy(feats[c][l])
    for norm in NORMS:
        cfg, init = product_head_state(norm)
        shapes = [types.SimpleNamespace(channels=C, stride=s) for s in cfg.MODEL.FCOS.FPN_STRIDES]
        head = fcos_mod.FCOSHead(cfg, shapes)
        sd = {PREFIX + k: v for k, v in head.state_dict().items()}
        keys = sorted(sd)
        d["%s_keys" % norm] = np.array(keys)
        shp = np.full((len(keys), 4), -1, dtype=np.int64)
        for i, k in enumerate(keys):
            shp[i, :sd[k].dim()] = list(sd[k].shape)
        d["%s_shapes" % norm] = shp
        assert sorted(init) == keys, (sorted(set(init) ^ set(keys))[:6])
        perturb_norm_params(init, SEED + 1)
        head.load_state_dict({k[len(PREFIX):]: v for k, v in init.items()}, strict=True)
        for c in calls:
            head.train(c != "eval")
            with torch.no_grad():
                out = head(feats[c])
            assert len(out) == 6, "the shipped recipe has KL_LOSS: logits, reg, std, ctrness, top_feats, bbox_towers"
            for name, lst in zip(("logits", "reg", "std", "ctr"), out[:4]):
                for l, t in enumerate(lst):
                    d["%s_%s_%s_%d" % (norm, c, name, l)] = G.npy(t)
            if c != "eval" and norm != "none":
                st = head.state_dict()
                for tower in ("cls_tower", "bbox_tower"):
                    n = cfg.MODEL.FCOS.NUM_CLS_CONVS if tower == "cls_tower" else cfg.MODEL.FCOS.NUM_BOX_CONVS
                    for kind in ("running_mean", "running_var"):
                        d["%s_%s_%s_%s" % (norm, c, tower, kind)] = G.npy(torch.stack(
                            [torch.stack([st["%s.%d.%d.%s" % (tower, 3 * i + 1, l, kind)] for l in range(len(LEVEL_HW))]) for i in range(n)]))
                nbt = {int(v) for k, v in st.items() if k.endswith("num_batches_tracked")}
                assert len(nbt) == 1
                d["%s_%s_num_batches_tracked" % (norm, c)] = np.int64(nbt.pop())
    dup = [k for k in d if k.startswith("SyncBN_") and not k.endswith(("_keys", "_shapes"))]
    for k in dup:
        assert np.array_equal(d[k], d["BN_" + k[len("SyncBN_"):]]), k
        del d[k]
    d["SyncBN_same_as_BN"] = np.bool_(True)
    path = os.path.join(HERE, "fcos_norm.npz")
    np.savez_compressed(path, **d)
    print("fcos_norm.npz:", len(d), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
