"""The conv box head (MODEL.ROI_BOX_HEAD.NUM_CONV 4, NUM_FC 1, NORM "GN": Detectron2's "4conv1fc") next to the default 2-fc head:

  * the two per-ROI GroupNorm kernels alone at R = 6144, HW = 49, C = 256: device events around `rep` back-to-back launches, bytes
    moved (forward: x read, y written; backward: dy and x read, dx written) over time;
  * run_step_full_semisup of UBRCNNTeacherTrainer on the synthetic 4 + 4 batch with either head, bf16 and f32, the two heads alternating.

    python tools/bench_box_head.py [--steps 10] [--warmup 3] [--rep 50] [--label 4] [--unlabel 4] [--no-step]

The synthetic detector is not tuned for pseudo labels here (the tuning helper restates the fc head): the ROI batch has its fixed size
either way, so the box head's work per step does not depend on it.  One JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "unbiased-teacher-v2_amd"))
import torch  # noqa: E402

HEADS = (("2fc", []), ("4conv1fc_gn", ["MODEL.ROI_BOX_HEAD.NUM_CONV", 4, "MODEL.ROI_BOX_HEAD.NUM_FC", 1, "MODEL.ROI_BOX_HEAD.NORM", "GN"]))


def kernels(rep, result):
    from ubteacher import hip, ops
    R, HW, C, G = 6144, 49, 256, 32
    for mode in ("fp32", "bf16"):
        ops.set_precision(mode)
        dt = torch.float32 if mode == "fp32" else hip.h16_dtype()
        g = torch.Generator(device="cuda").manual_seed(0)
        x = torch.randn(R, HW, C, device="cuda", generator=g).to(dt)
        dy = torch.randn(R, HW, C, device="cuda", generator=g).to(dt)
        ga, be = torch.rand(C, device="cuda") + 0.5, torch.zeros(C, device="cuda")
        dga, dbe = torch.zeros_like(ga), torch.zeros_like(be)
        _, mean, rstd = hip.groupnorm_roi_fwd(x, ga, be, G)
        esz = x.element_size()
        for name, fn, nbytes in (("fwd", lambda: hip.groupnorm_roi_fwd(x, ga, be, G), 2 * x.numel() * esz),
                                 ("bwd", lambda: hip.groupnorm_roi_bwd(dy, x, mean, rstd, ga, be, dga, dbe, G), 3 * x.numel() * esz)):
            ts = []
            for rnd in range(4):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                fn()
                torch.cuda.synchronize()
                e0.record()
                for _ in range(rep):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    ts.append(e0.elapsed_time(e1) / rep * 1e3)
            t = statistics.median(ts)
            print("groupnorm_roi_%s %s R=%d HW=%d C=%d: %.1f us (min %.1f max %.1f), %.1f MB -> %.2f TB/s"
                  % (name, mode, R, HW, C, t, min(ts), max(ts), nbytes / 1e6, nbytes / t / 1e6))
            result["gn_roi_%s_%s_us" % (name, mode)] = round(t, 2)
            result["gn_roi_%s_%s_TBps" % (name, mode)] = round(nbytes / t / 1e6, 3)
    ops.set_precision("fp32")


def steps(args, result):
    from ubteacher.engine import UBRCNNTeacherTrainer
    from ubteacher.presets import get_config
    for dtype in ("bf16", "f32"):
        if dtype == "f32":
            os.environ.pop("UTV2_PRECISION", None)
        else:
            os.environ["UTV2_PRECISION"] = "bf16"
        trainers = {}
        for name, keys in HEADS:
            cfg = get_config("rcnn", 1, ["SOLVER.IMG_PER_BATCH_LABEL", args.label, "SOLVER.IMG_PER_BATCH_UNLABEL", args.unlabel,
                                         "SEMISUPNET.BURN_UP_STEP", 0, "SOLVER.AMP.ENABLED", dtype != "f32", "MODEL.DEVICE", "cuda"] + keys)
            torch.manual_seed(0)
            tr = UBRCNNTeacherTrainer(cfg, data_loader=None)
            tr.iter = 1
            tr.log_period = 10 ** 9
            tr.optimizer.param_groups[0]["lr"] = 1e-12
            trainers[name] = tr
        times = {name: [] for name in trainers}
        for rnd in range(3):                       # round 0 warms both heads up
            for name, tr in trainers.items():
                n = args.warmup if rnd == 0 else args.steps
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    tr.run_step_full_semisup(); tr.iter += 1
                torch.cuda.synchronize()
                if rnd:
                    times[name].append((time.perf_counter() - t0) / n * 1e3)
        for name in trainers:
            t = statistics.median(times[name])
            print("step %s %-12s %.2f ms (%s)" % (dtype, name, t, ", ".join("%.2f" % v for v in times[name])))
            result["step_%s_%s_ms" % (dtype, name)] = round(t, 3)
        del trainers
        torch.cuda.empty_cache()
    os.environ.pop("UTV2_PRECISION", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rep", type=int, default=50)
    ap.add_argument("--label", type=int, default=4)
    ap.add_argument("--unlabel", type=int, default=4)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    result = {"label": args.label, "unlabel": args.unlabel, "steps": args.steps}
    kernels(args.rep, result)
    if not args.no_step:
        steps(args, result)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
