"""bench.py on a configuration with further keys merged in: `python tools/bench_with_opts.py KEY VALUE [KEY VALUE ...] -- <bench.py
arguments>`.  bench.py builds its configurations itself and has no option for that; this driver appends the pairs to the options of
every `ubteacher.presets.get_config` call and then runs `bench.main` in the same process, so protocol, workload and output line are
bench.py's own.  Used for the MODEL.FCOS.THRESH_WITH_CTR timing of DESIGN.md section 18:

    python tools/bench_with_opts.py MODEL.FCOS.THRESH_WITH_CTR True -- --gpus 1 --steps 50 --warmup 10 --model fcos --dtype f16

Values are read as Python literals where they are one (True, 50, 0.05), else as strings.  One GPU only: more ranks are spawned as new
processes, which would not see the wrapper."""
import ast
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unbiased-teacher-v2_amd")]


def main(argv):
    if "--" not in argv:
        raise SystemExit(__doc__)
    cut = argv.index("--")
    pairs, rest = argv[:cut], argv[cut + 1:]
    if len(pairs) % 2:
        raise SystemExit("KEY VALUE pairs expected before `--`")
    extra = []
    for k, v in zip(pairs[0::2], pairs[1::2]):
        try:
            v = ast.literal_eval(v)
        except (ValueError, SyntaxError):
            pass
        extra += [k, v]
    import bench
    from ubteacher import presets
    if bench.parse_args(rest).gpus != 1:
        raise SystemExit("bench_with_opts: --gpus 1 only")
    inner = presets.get_config

    def get_config(family="fcos", sup=1, opts=()):
        return inner(family, sup, list(opts) + extra)
    presets.get_config = get_config
    bench.main(rest)


if __name__ == "__main__":
    main(sys.argv[1:])
