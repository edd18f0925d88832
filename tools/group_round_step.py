"""A/B of the group-record accumulate's round against a build of the parent commit, measured as
tools/group_records_step.py measures a step (reference-style Functions, 8 input sets cycled, 300 steps between two HIP
events, three repeats a process) -- its sibling for two builds that BOTH know option key 24: every build runs with the key
left alone, so each cell takes the record kind that is its shape class's default.

    python tools/group_round_step.py --ab PARENT_DIR [--variant NAME=TREE ...] [--processes 3] [--cells C2,C2p,C3pp,C5p]
                                     [--dtypes bf16,f16] [--slots] [--limit SECONDS] [--log FILE]

Processes of the parent build, of this build and of every --variant (a tree whose boxer_amd holds a tuning build of the
library under the product's name, next to a copy of the package: the compiled operator module loads the library beside
it) alternate, --processes of each, ONE process on the GPU at a time, each under its own time limit;
the run stops at the first process that fails.  A cell PASSES for a build if its slowest repeat is faster than the parent's
fastest; for the cells that do not take the kernel the rule is read the other way: the build's fastest repeat must not be
slower than the parent's slowest."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = os.path.join(ROOT, "tools", "group_records_step.py")


def table(rows, builds):
    cells = {}
    for r in rows:
        cells.setdefault((r["cell"], r["dtype"]), {}).setdefault(r["build"], []).extend(r["us_per_step"])
    out = ["| cell | type | build | us (min .. max) | parent, us (min .. max) | faster | not slower |", "|---|---|---|---|---|---|---|"]
    for (cell, dtype), by in sorted(cells.items()):
        p = by.get("parent")
        for b in builds:
            t = by.get(b)
            if not p or not t or b == "parent":
                continue
            out.append("| %s | %s | %s | %.1f .. %.1f | %.1f .. %.1f | %s | %s |" % (
                cell, dtype, b, min(t), max(t), min(p), max(p), "yes" if max(t) < min(p) else "no",
                "yes" if min(t) <= max(p) else "no"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", metavar="PARENT_DIR", required=True)
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=TREE")
    ap.add_argument("--no-this", action="store_true", help="only the parent and the variants")
    ap.add_argument("--cells", default="C2,C2p,C3pp,C5p")
    ap.add_argument("--dtypes", default="bf16,f16")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--slots", action="store_true")
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--log")
    args = ap.parse_args()
    log = open(args.log, "a") if args.log else None

    def emit(line):
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    builds = [("parent", os.path.abspath(args.ab))] + ([] if args.no_this else [("this", ROOT)])
    for kv in args.variant:
        name, tree = kv.split("=", 1)
        builds.append((name, os.path.abspath(tree)))
    common = ["--key24", "-1", "--cells", args.cells, "--dtypes", args.dtypes, "--steps", str(args.steps), "--warmup",
              str(args.warmup), "--repeats", str(args.repeats)] + (["--slots"] if args.slots else [])
    rows = []
    for i in range(args.processes):
        for label, tree in builds:
            env = dict(os.environ)
            env.pop("BOXATTN_HIP_LIB", None)
            cmd = [sys.executable, STEP, "--label", label, "--tree", tree] + common
            try:
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit, env=env)
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
    for line in table(rows, [b[0] for b in builds]):
        emit(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
