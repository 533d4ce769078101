"""Step rate of the deeper / grouped backbones and the grouped-conv kernels against their HBM bound.

    python tools/bench_backbone.py steps   [--steps K --warmup W --out profiles/backbone_steps.json]
        FCOS and Faster-RCNN run_step_full_semisup at 4 + 4 images of 1333x800 (the synthetic loader of bench.py), in f16 and bf16,
        for R-50 (the reference point, same process), R-101 and X-101-32x8d: step images/sec (host clock around synchronised steps).
    python tools/bench_backbone.py kernels [--reps R --out profiles/backbone_gconv.json]
        the grouped conv2 launches of X-101-32x8d at the per-stage shapes of that step (forward on 12 images, dgrad and wgrad on 8; 16-bit
        operands, stride 1): kernel time from device events, bytes computed from the shapes, fraction of the 6.3 TB/s HBM bound.
        Under `rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/bench_backbone.py kernels --trace-order` the launches run
        in a fixed order, and `python tools/bench_backbone.py table --trace DIR/.../run_kernel_trace.csv` turns the trace into the same table
        with the profiler's kernel times.
    python tools/bench_backbone.py basicblock [--reps R --rounds N --out profiles/basicblock_kernel.json]
        the fused frozen BasicBlock launch (csrc/basicblock.hip) against the two conv launches it replaces at the res2 shape of the benchmark
        (8 images, 200 x 336 x 64), both 16-bit builds: device events around R launches back to back, the two versions alternating for N
        rounds (median and range over the rounds), bytes from the shapes, achieved bytes/s.
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "unbiased-teacher-v2_amd"))

HBM_TBS = 6.3            # achievable HBM rate (MI355X, float4 copy)
BACKBONES = {
    "R-18": ["MODEL.RESNETS.DEPTH", 18, "MODEL.RESNETS.RES2_OUT_CHANNELS", 64],
    "R-34": ["MODEL.RESNETS.DEPTH", 34, "MODEL.RESNETS.RES2_OUT_CHANNELS", 64],
    "R-50": [],
    "R-101": ["MODEL.RESNETS.DEPTH", 101],
    "X-101-32x8d": ["MODEL.RESNETS.DEPTH", 101, "MODEL.RESNETS.NUM_GROUPS", 32, "MODEL.RESNETS.WIDTH_PER_GROUP", 8,
                    "MODEL.RESNETS.STRIDE_IN_1X1", False],
}
# X-101-32x8d conv2 per stage on the padded 1344x800 canvas: (stage, H, W, C, groups)
GCONV_SHAPES = [("res2", 200, 336, 256, 32), ("res3", 100, 168, 512, 32), ("res4", 50, 84, 1024, 32), ("res5", 25, 42, 2048, 32)]


def step_rate(kind, backbone, dtype, steps, warmup, label=4, unlabel=4):
    import torch
    import bench
    from ubteacher.engine import UBRCNNTeacherTrainer, UBTeacherTrainer
    from ubteacher.presets import get_config
    cfg = get_config(kind, 1, ["SOLVER.IMG_PER_BATCH_LABEL", label, "SOLVER.IMG_PER_BATCH_UNLABEL", unlabel, "SEMISUPNET.BURN_UP_STEP", 0,
                               "SOLVER.AMP.ENABLED", True, "MODEL.DEVICE", "cuda"] + BACKBONES[backbone])
    torch.manual_seed(0)
    bench.set_amp_type(dtype)
    tr = (UBRCNNTeacherTrainer if kind == "rcnn" else UBTeacherTrainer)(cfg)
    tr.iter, tr.log_period = 1, 10 ** 9
    tr.optimizer.param_groups[0]["lr"] = 1e-12
    (bench.tune_rcnn_for_pseudo_labels if kind == "rcnn" else bench.tune_for_pseudo_labels)(tr, tr._data_loader.batches[0])
    for _ in range(warmup):
        tr.run_step_full_semisup()
        tr.iter += 1
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.run_step_full_semisup()
        tr.iter += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    losses = {k: v for k, v in tr.flush_metrics().items() if k.startswith("loss")}
    del tr
    torch.cuda.empty_cache()
    return {"model": kind, "backbone": backbone, "dtype": dtype, "step_images_per_sec": (label + unlabel) * steps / dt,
            "ms_per_step": 1e3 * dt / steps, "steps": steps, "warmup": warmup, "images": "%d + %d of 1333x800" % (label, unlabel),
            "losses": losses}


def launch_bytes(op, n, H, W, C, G, esize=2):
    """bytes a launch must move at least: every operand once (the 3x3 halo re-read from caches is not counted)"""
    act = n * H * W * C * esize
    wgt = C * 9 * (C // G)
    if op == "fwd":
        return 2 * act + wgt * esize
    if op == "dgrad":          # dy in, dx out, the producer's 16-bit ReLU output read for the mask
        return 3 * act + wgt * esize
    return 2 * act + wgt * 4   # wgrad: x and dy in, the fp32 gradient rows out


def _gconv_launches(reps):
    """(op, stage, n, H, W, C, G, callable) of the timed launches"""
    import torch
    from ubteacher import hip
    dt = hip.h16_dtype()
    out = []
    for stage, H, W, C, G in GCONV_SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        x12 = torch.randn(12, H, W, C, device="cuda", generator=g).relu().to(dt)
        x8, dy8 = x12[:8].contiguous(), torch.randn(8, H, W, C, device="cuda", generator=g).to(dt)
        w = (torch.randn(C, 9 * C // G, device="cuda", generator=g) * 0.05).to(dt)
        sc, sh = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
        dw = torch.zeros(C, 9 * C // G, device="cuda")
        out.append(("fwd", stage, 12, H, W, C, G, lambda x=x12, w=w, sc=sc, sh=sh, G=G: hip.gconv3x3_fwd(x, w, G, 1, sc, sh, True)))
        out.append(("dgrad", stage, 8, H, W, C, G, lambda dy=dy8, w=w, sc=sc, m=x8, G=G: hip.gconv3x3_dgrad(dy, w, G, 1, tuple(m.shape), sc, m)))
        out.append(("wgrad", stage, 8, H, W, C, G, lambda x=x8, dy=dy8, dw=dw, sc=sc, G=G: hip.gconv3x3_wgrad(x, dy, dw, G, 1, sc)))
    return out


def kernels(reps, dtype):
    import torch
    import bench
    from ubteacher import hip
    bench.set_amp_type(dtype)
    hip.set_h16("fp16" if dtype == "f16" else "bf16")
    rows = []
    for op, stage, n, H, W, C, G, fn in _gconv_launches(reps):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = 1e3 * e0.elapsed_time(e1) / reps
        rows.append(_row(op, stage, n, H, W, C, G, us, "device events, %d launches back to back" % reps))
    return rows


BASICBLOCK_SHAPE = (8, 200, 336, 64)     # res2 of R-18 / R-34 on the padded 1344x800 canvas, 4 + 4 images


def basicblock(reps, rounds):
    """fused launch against the two-launch chain, alternating; bytes each must move at least: fused x + y, chain x + c1 (conv1) and
    c1 + x + y (conv2) - weights (147 KB) and the halo re-reads from caches are not counted"""
    import statistics
    import torch
    from ubteacher import hip
    N, H, W, C = BASICBLOCK_SHAPE
    act = N * H * W * C * 2
    rows = []
    for kind in ("bf16", "fp16"):
        hip.set_h16(kind)
        dt = hip.h16_dtype()
        g = torch.Generator(device="cuda").manual_seed(0)
        x = (torch.randn(N, H, W, C, device="cuda", generator=g).relu() * 0.7).to(dt)
        w1, w2 = [(torch.randn(C, 9 * C, device="cuda", generator=g) * 0.05).to(dt) for _ in range(2)]
        s1, s2 = [torch.rand(C, device="cuda", generator=g) + 0.5 for _ in range(2)]
        b1, b2 = [torch.randn(C, device="cuda", generator=g) * 0.2 for _ in range(2)]
        y, c1, y2 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)

        def fused():
            hip.basicblock_fwd_bf16(x, w1, w2, s1, b1, s2, b2, out=y)

        def chain():
            hip.conv2d_fwd_bf16(x, w1, scale=s1, bias=b1, relu=True, kh=3, kw=3, pad=1, out=c1)
            hip.conv2d_fwd_bf16(c1, w2, scale=s2, bias=b2, relu=True, kh=3, kw=3, pad=1, residual=x, out=y2)

        for fn in (fused, chain):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        differing = float((y != y2).float().mean())
        times = {"fused": [], "chain": []}
        for _ in range(rounds):
            for name, fn in (("fused", fused), ("chain", chain)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(1e3 * e0.elapsed_time(e1) / reps)
        for name, nbytes in (("fused", 2 * act), ("chain", 5 * act)):
            us = statistics.median(times[name])
            rows.append({"op": name, "dtype": kind, "shape": list(BASICBLOCK_SHAPE), "us_median": us, "us_min": min(times[name]),
                         "us_max": max(times[name]), "bytes": nbytes, "achieved_TBps": nbytes / us / 1e6,
                         "flops": (2 * 9 * C * C * N * H * W) * 2, "share_of_elements_differing_from_chain": differing,
                         "time_source": "device events, %d launches back to back, %d alternating rounds" % (reps, rounds)})
        hip.set_h16("bf16")
    return rows


def _row(op, stage, n, H, W, C, G, us, source):
    b = launch_bytes(op, n, H, W, C, G)
    bound_us = b / (HBM_TBS * 1e12) * 1e6
    return {"op": op, "stage": stage, "images": n, "H": H, "W": W, "C": C, "g": C // G, "kernel_us": us, "bytes": b,
            "hbm_bound_us": bound_us, "fraction_of_hbm_bound": bound_us / us, "time_source": source}


def table(trace, reps):
    """rows of the kernel trace written under `kernels --trace-order` (dispatch order = _gconv_launches order, 1 + reps launches each;
    a wgrad is two kernels, the partial sums and the split reduction, summed)"""
    with open(trace) as f:
        recs = [r for r in csv.DictReader(f) if "gconv3x3" in r.get("Kernel_Name", "")]
    recs.sort(key=lambda r: int(r["Start_Timestamp"]))
    rows, i = [], 0
    for op, stage, n, H, W, C, G in [(op, st, n, H, W, C, G) for st, H, W, C, G in GCONV_SHAPES
                                     for op, n in (("fwd", 12), ("dgrad", 8), ("wgrad", 8))]:
        per = 2 if op == "wgrad" else 1
        chunk = recs[i:i + per * (1 + reps)][per:]           # the first launch of a shape is its warm-up
        i += per * (1 + reps)
        ns = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in chunk)
        rows.append(_row(op, stage, n, H, W, C, G, ns / 1e3 / reps, "rocprofv3 kernel trace, %d launches" % reps))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["steps", "kernels", "table", "basicblock"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--dtypes", default="f16,bf16")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--models", default="fcos,rcnn")
    ap.add_argument("--backbones", default=",".join(BACKBONES))
    ap.add_argument("--trace-order", action="store_true", help="(kernels) run without the event timing pass: one warm-up + reps launches")
    ap.add_argument("--trace", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.what == "steps":
        res = []
        for dtype in a.dtypes.split(","):
            for kind in a.models.split(","):
                for bb in a.backbones.split(","):
                    r = step_rate(kind, bb, dtype, a.steps, a.warmup)
                    print(json.dumps(r), flush=True)
                    res.append(r)
        out = {"what": "step images/sec, 4 + 4 images of 1333x800 per step", "results": res}
    elif a.what == "basicblock":
        out = {"what": "fused frozen BasicBlock launch against the two conv launches it replaces, res2 of R-18 / R-34 at 4 + 4 images",
               "results": basicblock(a.reps, a.rounds)}
        for r in out["results"]:
            print("%-5s %-4s %8.1f us (%.1f .. %.1f)  %.2f TB/s of the bytes its shapes require" % (
                r["op"], r["dtype"], r["us_median"], r["us_min"], r["us_max"], r["achieved_TBps"]))
    elif a.what == "kernels":
        if a.trace_order:
            import torch
            from ubteacher import hip
            hip.set_h16("fp16" if a.dtype == "f16" else "bf16")
            for op, stage, n, H, W, C, G, fn in _gconv_launches(a.reps):
                for _ in range(1 + a.reps):
                    fn()
            torch.cuda.synchronize()
            return
        out = {"what": "grouped conv2 launches of X-101-32x8d (%s operands): kernel time against the %.1f TB/s HBM bound of the bytes the "
                       "shapes require" % (a.dtype, HBM_TBS), "rows": kernels(a.reps, a.dtype)}
    else:
        out = {"what": "grouped conv2 launches of X-101-32x8d: rocprofv3 kernel time against the %.1f TB/s HBM bound" % HBM_TBS,
               "rows": table(a.trace, a.reps)}
    for r in out.get("rows", []):
        print("%-5s %-5s n=%-2d C=%-4d g=%-2d %9.1f us  bound %7.1f us  %.3f of bound" % (
            r["op"], r["stage"], r["images"], r["C"], r["g"], r["kernel_us"], r["hbm_bound_us"], r["fraction_of_hbm_bound"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
