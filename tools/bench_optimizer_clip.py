"""The optimizer step alone at the R-50 FCOS arena size: ArenaSGD with SOLVER.CLIP_GRADIENTS off (the two plain launches) against the
segmented path (norm clipping: norm reduction + coefficients + one update launch; value clipping / Nesterov: the update launch), in the
fp32 step and in the fp16 AMP step (found_inf scan, 16-bit mirror written by the update, loss-scale update).

    python tools/bench_optimizer_clip.py [--rounds 5] [--rep 200]

Device events around `rep` back-to-back steps, the variants alternating within a round; the median over the rounds is reported, with
the bytes each variant has to move (per trainable element: param r/w, momentum r/w, gradient r = 20 B; AMP: + 4 B found_inf scan + 2 B
mirror; norm clipping: + 4 B, the extra gradient read) and one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "unbiased-teacher-v2_amd"))
import torch  # noqa: E402

VARIANTS = (("off", []),
            ("norm2", ["SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "norm"]),
            ("norm_inf", ["SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "norm",
                          "SOLVER.CLIP_GRADIENTS.NORM_TYPE", float("inf")]),
            ("value", ["SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "value"]),
            ("nesterov", ["SOLVER.NESTEROV", True]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rep", type=int, default=200)
    args = ap.parse_args()
    from ubteacher import ops
    from ubteacher.engine.trainer import ArenaSGD
    from ubteacher.modeling import build_model
    from ubteacher.presets import get_config

    base = ["MODEL.DEVICE", "cuda", "SOLVER.BASE_LR", 1e-9]     # a vanishing rate: hundreds of steps on one random gradient stay finite
    torch.manual_seed(0)
    model = build_model(get_config("fcos", 1, base))
    st = model.store
    n = st.n_train
    result = {"trainable_elements": n, "rep": args.rep, "rounds": args.rounds}
    for mode in ("fp32", "fp16"):
        ops.set_precision(mode)
        amp_state = None
        if mode == "fp16":
            st.bf16(st.handles[0])                               # the 16-bit mirror exists and is fresh: the update keeps it so
            amp_state = torch.tensor([65536.0, 0.0, 0.0], device="cuda")
        # (the momentum arena belongs to the store: the variants share the one the last constructor allocated)
        opts = {name: ArenaSGD(get_config("fcos", 1, base + keys), model) for name, keys in VARIANTS}
        st.grad.normal_(0.0, 1e-3)
        if amp_state is not None:
            st.grad.mul_(65536.0)
        times = {name: [] for name in opts}
        for rnd in range(args.rounds + 1):                       # round 0 warms every variant up
            for name, o in opts.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                o.step(grad_scale=1.0, amp_state=amp_state)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.rep):
                    o.step(grad_scale=1.0, amp_state=amp_state)
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    times[name].append(e0.elapsed_time(e1) / args.rep * 1e3)
        assert bool(torch.isfinite(st.flat).all())
        if mode == "fp16":
            assert st.mirror16(need_fresh=True) is not None and float(amp_state[1]) == 0.0
        off = statistics.median(times["off"])
        for name in opts:
            t = statistics.median(times[name])
            per = 20 + (6 if mode == "fp16" else 0) + (4 if name.startswith("norm") else 0)
            print("%s %-9s %8.1f us/step (min %.1f max %.1f)  %5.2f x off   %2d B/element -> %.2f TB/s"
                  % (mode, name, t, min(times[name]), max(times[name]), t / off, per, per * n / t / 1e6))
            result["%s_%s_us" % (mode, name)] = round(t, 2)
            result["%s_%s_ratio" % (mode, name)] = round(t / off, 3)
    ops.set_precision("fp32")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
