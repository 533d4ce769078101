"""tests/golden/conv_backward_parent.json: per case and precision kind, the C-ABI calls the conv autograd node makes during backward and
the SHA-256 of every gradient it produces, as the checked-out commit makes them on the GPU.  Results only: the cases, the inputs and
the recorder live in tests/test_conv_backward_parent_gpu.py, which this script imports and which asserts the file.

RUN IT ON THE COMMIT WHOSE BEHAVIOUR IS MEANT (build that commit's libraries first) and name it with --commit.  The whole-backward
cases run twice: a digest the two runs do not agree on would be left out, and said (none was at da1f718).

    python tests/golden/gen_golden_conv_backward_parent.py --commit <hash> [--out tests/golden/conv_backward_parent.json]
    python tests/golden/gen_golden_conv_backward_parent.py --coverage     # lines of the backward-stage functions the cases execute
"""
import argparse
import inspect
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "unbiased-teacher-v2_amd"))

from tests import test_conv_backward_parent_gpu as T  # noqa: E402

# functions of ubteacher/ops.py whose lines --coverage lists (those that exist in the checked-out tree)
STAGES = ("backward", "_grad_in", "_backward_grouped", "_per_group", "_dgrad_levels", "_wgrad_levels", "_dgrad_nhwc", "_wgrad_nhwc", "_dgrad16")


def _run(fn, *args):
    mp = pytest.MonkeyPatch()
    try:
        return fn(*args, mp)
    finally:
        mp.undo()


def records(twice=True):
    cases = {}
    for name in sorted(T.LAYER_CASES):
        cases[name] = {kind: _run(T.layer_record, name, kind) for kind in T.KINDS}
    for model in ("fcos", "rcnn"):
        cases["step_" + model] = {}
        for kind in T.KINDS:
            a = _run(T.step_record, model, kind)
            b = _run(T.step_record, model, kind) if twice else a
            assert a["trace"] == b["trace"], (model, kind, "two runs made different calls")
            unstable = sorted(k for k in a["digests"] if a["digests"][k] != b["digests"][k])
            if unstable:
                print("step_%s %s: not reproducible run to run, left out: %s" % (model, kind, unstable))
            a["digests"] = {k: v for k, v in a["digests"].items() if k not in unstable}
            cases["step_" + model][kind] = a
    return cases


def coverage():
    """run every case with a line tracer installed where the backward runs (autograd's own thread) and list, per stage function, the
    lines that were never executed"""
    from ubteacher import ops
    found = {}
    for name in STAGES:
        fn = getattr(ops, name, None) or getattr(ops._ConvFn, name, None)
        if fn is not None:
            found[fn.__code__] = (name, fn)
    hit = set()

    def tracer(frame, event, arg):
        if frame.f_code not in found:
            return None
        if event == "line":
            hit.add((frame.f_code, frame.f_lineno))
        return tracer

    def traced(inner):
        def backward(ctx, *a):
            sys.settrace(tracer)
            try:
                return inner(ctx, *a)
            finally:
                sys.settrace(None)
        return staticmethod(backward)

    for cls in (ops._ConvFn, ops._BottleneckFn):
        cls.backward = traced(cls.backward)
    records(twice=False)
    for code, (name, fn) in sorted(found.items(), key=lambda kv: kv[0].co_firstlineno):
        src, first = inspect.getsourcelines(fn)
        lines = sorted({l for _, _, l in code.co_lines() if l is not None and l > first})
        missed = [l for l in lines if (code, l) not in hit]
        print("%-18s %3d lines, %3d executed, not executed: %s" % (name, len(lines), len(lines) - len(missed),
                                                                   "; ".join("%d: %s" % (l, src[l - first].strip()[:90]) for l in missed) or "-"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", help="the commit whose code and kernels are checked out and built")
    ap.add_argument("--out", default=T.FIXTURE)
    ap.add_argument("--coverage", action="store_true")
    args = ap.parse_args()
    if args.coverage:
        return coverage()
    assert args.commit, "--commit is required"
    cases = records()
    with open(args.out, "w") as f:
        json.dump({"commit": args.commit, "cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases, %d traced calls" % (args.out, len(cases), sum(len(r["trace"]) for c in cases.values() for r in c.values())))


if __name__ == "__main__":
    main()
