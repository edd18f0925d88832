"""What group records (option 24, "group_records") do to one training step of 16-bit box attention: forward + backward
through Functions in the reference's own shape (bench.reference_style_functions on the compiled e2edet_ops module),
model-like inputs, 8 input sets cycled, 300 steps between two HIP events after 20 warm-up steps, three repeats a process.

    python tools/group_records_step.py [--key24 V] [--label NAME] [--tree DIR] [--cells C2,C2p,C3pp,C5p]
                                       [--dtypes bf16,f16] [--steps K] [--warmup W] [--repeats R] [--slots]
                                       [--set NAME=V ...]
    python tools/group_records_step.py --ab PARENT_DIR [--processes 3] [--limit SECONDS] [--log FILE] [...]
    python tools/group_records_step.py --table FILE

--tree DIR: import boxer_amd from DIR (a build of the parent commit; --key24 -1 leaves the option alone, for a build
that has no key 24).  One JSON line per (cell, dtype) with the repeats' us per step; --slots adds the library's per-launch
averages (forward / point gradients / accumulate / binning, HIP events around the kernels over 50 further steps).

--ab: the A/B of DESIGN.md 4.2.3.  Processes of the parent build and of this build with key 24 = 2 alternate, --processes
of each, ONE process on the GPU at a time, each under its own time limit; the run stops at the first process that fails.
Raw lines and the table go to --log (profiles/group_records_step.log).  A cell PASSES if this build's slowest repeat is
faster than the parent's fastest: only then may group records become the default of that shape class."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = 8
DTYPES = {"bf16": "bfloat16", "f16": "float16"}


def time_cell(torch, bench, mod, _lib, cell, dtype, steps, warmup, repeats, slots):
    ref_box, _ = bench.reference_style_functions(mod)
    calls = []
    for s in range(SETS):
        inp = bench.make_inputs(cell, dtype, "cuda", family="model", seed=s)
        v, lg, ag = (inp[k].detach().clone().requires_grad_() for k in ("value", "loc", "attn"))
        calls.append((v, inp["shapes"], inp["lsi"], lg, ag, inp["grad_out"]))
    state = {"i": 0}

    def step():
        v, sh, ls, lg, ag, go = calls[state["i"] % SETS]
        state["i"] += 1
        v.grad = lg.grad = ag.grad = None
        ref_box.apply(v, sh, ls, lg, ag, 64).backward(go)

    for _ in range(bench.PREHEAT_STEPS):
        step()
    us = []
    for _ in range(repeats):
        for _ in range(warmup):
            step()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(steps):
            step()
        b.record()
        torch.cuda.synchronize()
        us.append(round(a.elapsed_time(b) * 1e3 / steps, 2))
    per_launch = None
    if slots:
        _lib.profile_begin()
        try:
            for _ in range(50):
                step()
            torch.cuda.synchronize()
        finally:
            prof = _lib.profile_end()
        per_launch = {k: round(v["ms"] * 1e3, 2) for k, v in prof.items() if v["ms"] is not None}
    return us, per_launch


def measure(args):
    sys.path.insert(0, os.path.abspath(args.tree))
    if ROOT not in sys.path:
        sys.path.append(ROOT)
    import torch
    import boxer_amd
    from boxer_amd import _ext, _lib
    import bench
    assert os.path.dirname(os.path.abspath(boxer_amd.__file__)) == os.path.join(os.path.abspath(args.tree), "boxer_amd")
    torch.autograd.set_multithreading_enabled(False)       # (as bench.make_step: the backward on the calling thread)
    if args.key24 >= 0:
        _lib.set_option("group_records", args.key24)
    for kv in args.set or ():                              # further option keys by name (boxer_amd._lib.OPTIONS)
        name, value = kv.split("=")
        _lib.set_option(name, int(value))
    mod = _ext.load()
    for cell in args.cells.split(","):
        for name in args.dtypes.split(","):
            dtype = getattr(torch, DTYPES[name])
            us, per_launch = time_cell(torch, bench, mod, _lib, cell, dtype, args.steps, args.warmup, args.repeats, args.slots)
            row = {"build": args.label, "key24": args.key24, "set": args.set or [], "cell": cell, "dtype": name, "us_per_step": us,
                   "steps": args.steps, "input_sets": SETS}
            if per_launch:
                row["us_per_launch"] = per_launch
            print(json.dumps(row), flush=True)


def table(rows):
    """rows: the JSON lines of an A/B -> markdown lines and {(cell, dtype): passed}."""
    cells = {}
    for r in rows:
        cells.setdefault((r["cell"], r["dtype"]), {}).setdefault(r["build"], []).extend(r["us_per_step"])
    out = ["| cell | type | parent, us (min .. max) | this build, key 24 = 2, us (min .. max) | passes |", "|---|---|---|---|---|"]
    passed = {}
    for (cell, dtype), by in sorted(cells.items()):
        if "parent" not in by or "this" not in by:
            continue
        p, t = by["parent"], by["this"]
        passed[(cell, dtype)] = max(t) < min(p)
        out.append("| %s | %s | %.1f .. %.1f | %.1f .. %.1f | %s |" % (cell, dtype, min(p), max(p), min(t), max(t),
                                                                  "yes" if passed[(cell, dtype)] else "no"))
    return out, passed


def ab(args):
    log = open(args.log, "a") if args.log else None

    def emit(line):
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    rows = []
    common = ["--cells", args.cells, "--dtypes", args.dtypes, "--steps", str(args.steps), "--warmup", str(args.warmup),
              "--repeats", str(args.repeats)] + (["--slots"] if args.slots else [])
    for i in range(args.processes):
        for label, tree, key in (("parent", args.ab, -1), ("this", ROOT, 2)):
            cmd = [sys.executable, os.path.abspath(__file__), "--label", label, "--tree", tree, "--key24", str(key)] + common
            if label == "this":
                cmd += [a for kv in args.set or () for a in ("--set", kv)]
            try:
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                emit("# process %d (%s) ran into its time limit of %d s: stopped" % (i, label, args.limit))
                return 1
            if res.returncode != 0:
                emit("# process %d (%s) failed with status %d: stopped\n%s" % (i, label, res.returncode, res.stderr[-2000:]))
                return 1
            for line in res.stdout.splitlines():
                if line.startswith("{"):
                    emit(line)
                    rows.append(json.loads(line))
    lines, passed = table(rows)
    for line in lines:
        emit(line)
    emit("# passed: %s" % (", ".join("%s %s" % k for k, ok in sorted(passed.items()) if ok) or "none"))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--key24", type=int, default=2)
    ap.add_argument("--label", default="this")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--cells", default="C2,C2p,C3pp,C5p")
    ap.add_argument("--dtypes", default="bf16,f16")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--set", action="append", metavar="NAME=V", help="set another option key, e.g. bin_chunk=512")
    ap.add_argument("--slots", action="store_true", help="add the per-launch averages of the library's timing slots")
    ap.add_argument("--ab", metavar="PARENT_DIR", help="alternate processes of the parent build there and of this build")
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="--ab: time limit of one process, seconds")
    ap.add_argument("--log", help="--ab: append raw lines and the table to this file")
    ap.add_argument("--table", metavar="FILE", help="print the table of the JSON lines in FILE")
    args = ap.parse_args()
    if args.table:
        rows = [json.loads(l) for l in open(args.table) if l.startswith("{")]
        print("\n".join(table(rows)[0]))
        return 0
    return ab(args) if args.ab else measure(args)


if __name__ == "__main__":
    sys.exit(main())
