"""Milliseconds per TEST.PRECISE_BN iteration on one MI355X: FCOS R-50, MODEL.FCOS.NORM "BN", fp16, 4 + 4 images of 1333 x 800.

  new       engine.precise_bn.update_bn_stats: the statistics-only forward (backbone, FPN, towers up to their last BatchNorm) with the
            estimator on the device, one commit launch and one host synchronisation at the end of the update;
  baseline  in the same process, with code the commit before this feature already had: the layers' momentum set to 1.0, the
            training-mode `model` forward of the same two calls under no_grad (as fvcore's update_bn_stats runs the model) with its
            losses computed - the unlabeled call has no ground truth in the synthetic loader and runs as branch "raw" - the running
            buffers read back after each call and averaged on the host (precise_bn.PopulationStatistics).

    python tools/bench_precise_bn.py [--iters 20] [--warmup 3] [--rounds 3] [--out profiles/precise_bn.json]

The two alternate for `rounds` rounds; the figure is the median round's wall time per iteration (perf_counter around a synchronised
update).  One JSON line at the end, also written to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "unbiased-teacher-v2_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def fresh(batch):
    return tuple([dict(d) for d in part] for part in batch)


def run_new(model, batch, iters):
    from ubteacher.engine.precise_bn import update_bn_stats
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    update_bn_stats(model, (fresh(batch) for _ in range(iters)), iters)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def run_baseline(model, batch, iters):
    from ubteacher.engine.precise_bn import PopulationStatistics, get_bn_modules
    bns = get_bn_modules(model)
    L, C = bns[0].gamma.t.shape
    est = [PopulationStatistics(L, C) for _ in bns]
    for b in bns:
        b.momentum = 1.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:
        with torch.no_grad():
            for _ in range(iters):
                lq, lk, uq, _ = fresh(batch)
                for call, branch in ((lq + lk, "labeled"), (uq, "raw")):
                    losses = model(call, branch=branch)
                    for e, b in zip(est, bns):
                        m, v = b.running_mean.t.cpu().numpy(), b.running_var.t.cpu().numpy()      # the host read of every call
                        for l in range(L):
                            e.update(l, m[l], v[l], len(call))
                    del losses
            for e, b in zip(est, bns):
                m, v = e.result()
                b.running_mean.t.copy_(torch.from_numpy(m.astype(np.float32)))
                b.running_var.t.copy_(torch.from_numpy(v.astype(np.float32)))
    finally:
        for b in bns:
            b.momentum = 0.1
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--label", type=int, default=4)
    ap.add_argument("--unlabel", type=int, default=4)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1333)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "precise_bn.json"))
    a = ap.parse_args()
    os.environ["UTV2_PRECISION"] = a.precision
    from ubteacher.data.synthetic import SyntheticTwoCropLoader
    from ubteacher.engine import UBTeacherTrainer
    from ubteacher.presets import get_config
    cfg = get_config("fcos", 1, ["SOLVER.IMG_PER_BATCH_LABEL", a.label, "SOLVER.IMG_PER_BATCH_UNLABEL", a.unlabel, "SOLVER.AMP.ENABLED",
                                 a.precision != "fp32", "MODEL.DEVICE", "cuda", "MODEL.FCOS.NORM", "BN", "TEST.PRECISE_BN.ENABLED", True])
    torch.manual_seed(0)
    loader = SyntheticTwoCropLoader(cfg, height=a.height, width=a.width)
    tr = UBTeacherTrainer(cfg, data_loader=loader)
    assert tr._precise_bn is not None
    batch = loader.batches[0]
    run_new(tr.model, batch, a.warmup)
    run_baseline(tr.model, batch, a.warmup)
    new, base = [], []
    for _ in range(a.rounds):
        new.append(run_new(tr.model, batch, a.iters))
        base.append(run_baseline(tr.model, batch, a.iters))
        print("round: new %.2f ms / iteration, baseline %.2f ms / iteration" % (new[-1], base[-1]), flush=True)
    res = {"workload": "fcos_r50_bn_%dp%d_%dx%d_%s" % (a.label, a.unlabel, a.width, a.height, a.precision), "device": torch.cuda.get_device_name(0),
           "iters_per_round": a.iters, "rounds": a.rounds,
           "precise_bn_ms_per_iter": round(statistics.median(new), 3), "precise_bn_ms_per_iter_rounds": [round(v, 3) for v in new],
           "baseline_ms_per_iter": round(statistics.median(base), 3), "baseline_ms_per_iter_rounds": [round(v, 3) for v in base],
           "baseline": "momentum 1.0, training-mode model forward of both calls under no_grad with losses, buffers read back per call, host fp64 average"}
    res["speedup"] = round(res["baseline_ms_per_iter"] / res["precise_bn_ms_per_iter"], 3)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
