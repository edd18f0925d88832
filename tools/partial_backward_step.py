"""What a backward that computes only the gradients autograd asks for saves: forward + backward through
``BoxAttnFunction`` / ``BoxAttnBF16Function`` at the encoder (C2) and decoder (C3'') shapes, float32 and bf16,
for three ``requires_grad`` patterns -- every input ("all"), everything but ``value`` ("points": a frozen
memory), ``value`` only ("value": frozen attention heads).

    python tools/partial_backward_step.py [--steps K] [--warmup W] [--repeats R] [--family test] [--tree DIR] [--out FILE]
    python tools/partial_backward_step.py --check NEW.jsonl --against PARENT.jsonl [PARENT2.jsonl ...] [--same-pattern]

Protocol (measuring guide): 8 input sets cycled, bench.PREHEAT_STEPS untimed steps, W warm-up steps, then K steps
between two HIP events on the op's stream; R repeats per configuration, all kept.  ``--tree``: time another built
checkout of the project (the parent commit) with this very script -- the pass condition is stated against the
parent, in the same session:

  * a partial pattern must not be slower than the PARENT's "all" pattern at the same shape and type,
  * this build's "all" pattern must be within the parent's own spread of the parent's,

where the spread is max - min over the parent's repeated "all" runs (all files given to --against).  --check
prints the table and exits 1 if a row misses.  ``--same-pattern`` (a change that must leave every step as it is: the
parent has the partial backward too) holds every row against the parent's row of the SAME pattern instead: this
build's fastest repeat must not be slower than the parent's slowest."""
import argparse
import json
import os
import sys

PATTERNS = {"all": (True, True, True), "points": (False, True, True), "value": (True, False, False)}
SETS = 8


def measure(args):
    root = os.path.abspath(args.tree or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, root)
    import torch
    import bench
    import boxer_amd
    assert os.path.dirname(os.path.abspath(boxer_amd.__file__)) == os.path.join(root, "boxer_amd"), boxer_amd.__file__
    torch.autograd.set_multithreading_enabled(False)       # (bench.make_step, entry "function": see there)
    out = open(args.out, "a") if args.out else None

    def timed(workload, dtype, pattern):
        fn = boxer_amd.BoxAttnBF16Function if dtype == torch.bfloat16 else boxer_amd.BoxAttnFunction
        sets = []
        for seed in range(SETS):
            inp = bench.make_inputs(workload, dtype, "cuda", family=args.family, seed=seed)
            leaves = [inp[k].detach().clone().requires_grad_(need)
                      for k, need in zip(("value", "loc", "attn"), PATTERNS[pattern])]
            sets.append((leaves, inp["shapes"], inp["lsi"], inp["grad_out"]))
        state = {"i": 0}

        def step():
            (v, loc, attn), sh, ls, go = sets[state["i"] % SETS]
            state["i"] += 1
            v.grad = loc.grad = attn.grad = None
            fn.apply(v, sh, ls, loc, attn, 64).backward(go)
        for _ in range(bench.PREHEAT_STEPS):
            step()
        runs = []
        for _ in range(args.repeats):
            for _ in range(args.warmup):
                step()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(args.steps):
                step()
            b.record()
            torch.cuda.synchronize()
            runs.append(round(a.elapsed_time(b) * 1e3 / args.steps, 2))
        return runs

    for workload in args.workloads.split(","):
        for name, dtype in (("bf16", torch.bfloat16), ("f32", torch.float32)):
            for pattern in PATTERNS:
                shape = workload if args.family == "model" else workload + "/" + args.family
                line = json.dumps({"tree": args.label or os.path.basename(root), "workload": shape, "dtype": name,
                                   "pattern": pattern, "us_per_step": timed(workload, dtype, pattern),
                                   "steps": args.steps, "input_sets": SETS})
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()


def load(paths):
    rows = {}
    for path in paths:
        with open(path) as fh:
            for line in fh:
                if line.startswith("{"):
                    r = json.loads(line)
                    rows.setdefault((r["workload"], r["dtype"], r["pattern"]), []).extend(r["us_per_step"])
    return rows


def check(args):
    new, parent = load([args.check]), load(args.against)
    bad = 0
    print("| shape | type | pattern | parent %s, us (min .. max) | this build, us (min .. max) | bound | |"
          % ("same pattern" if args.same_pattern else "all"))
    print("|---|---|---|---|---|---|---|")
    for (workload, dtype, pattern), runs in sorted(new.items()):
        base = parent[(workload, dtype, pattern if args.same_pattern else "all")]
        spread = max(base) - min(base)
        # each side by the fastest of its repeats (the least disturbed one); the parent's spread is the noise margin
        # -- i.e. the fastest repeat of this build against the SLOWEST all-gradients repeat of the parent
        bound = min(base) + spread
        ok = min(runs) <= bound
        bad += not ok
        print("| %s | %s | %s | %.1f .. %.1f | %.1f .. %.1f | %.1f | %s |" % (
            workload, dtype, pattern, min(base), max(base), min(runs), max(runs), bound, "ok" if ok else "SLOWER"))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--workloads", default="C2,C3pp")
    ap.add_argument("--family", default="model", choices=["model", "test"],
                    help="bench.make_inputs family: model-like boxes, or uniformly random (non-local) locations")
    ap.add_argument("--tree", help="root of another built checkout to time instead of this one")
    ap.add_argument("--label", help="name of the tree in the output lines")
    ap.add_argument("--out", help="append the JSON lines to this file")
    ap.add_argument("--check", help="JSON lines of this build: evaluate the pass condition ...")
    ap.add_argument("--against", nargs="+", help="... against these JSON lines of the parent commit")
    ap.add_argument("--same-pattern", action="store_true", help="--check: against the parent's row of the same pattern")
    args = ap.parse_args()
    sys.exit(check(args) if args.check else measure(args))


if __name__ == "__main__":
    main()
