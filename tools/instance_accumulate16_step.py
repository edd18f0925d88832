"""One training step of 16-bit instance attention (forward + backward through InstanceAttnBF16Function /
InstanceAttnF16Function) under a setting of option 23 ("inst_acc16": 1 the VALU list walk, 2 grad_value on the matrix
cores), timed with HIP events: model-like inputs (bench.make_inputs), 8 input sets cycled, 300 steps after 20 warm-up
steps, three repeats a process.

    python tools/instance_accumulate16_step.py [--key23 V] [--label NAME] [--tree DIR] [--cells C3,C3k8,C3p]
                                               [--dtypes bf16,f16] [--batches 1,2] [--steps K] [--warmup W] [--repeats R]

--tree DIR: import boxer_amd from DIR (a build of another commit; --key23 -1 leaves the option alone, for a build that
has no key 23).  One JSON line per (cell, dtype, batch) with the repeats' us per step.  The A/B of DESIGN.md 4.2.2
alternates processes of the parent build, this build with key 23 = 2 and this build with key 23 = 1, three of each
(profiles/instance_accumulate16_step.log)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = 8
C2P = [(100, 167), (50, 84), (25, 42), (13, 21)]
# cell -> bench workload (C3k8: k = 8 on the C2' levels, 77 k points a slice -- added to bench's table in this process)
CELLS = {"C3": "C3", "C3k8": "C3k8", "C3p": "C3p"}


def time_cell(bench, boxer_amd, cell, dtype, batch, steps, warmup, repeats):
    fn = boxer_amd.InstanceAttnBF16Function if dtype == torch.bfloat16 else boxer_amd.InstanceAttnF16Function
    calls = []
    for s in range(SETS):
        inp = bench.make_inputs(CELLS[cell], dtype, "cuda", family="model", batch=batch, seed=s)
        v, lg, ag = (inp[k].detach().clone().requires_grad_() for k in ("value", "loc", "attn"))
        wg = inp["level_w"].detach().clone().requires_grad_()
        ms = int(round(inp["dims"]["P"] ** 0.5))
        calls.append((v, inp["shapes"], inp["lsi"], lg, ag, wg, ms, inp["grad_out"], inp["grad_mask"]))
    state = {"i": 0}

    def step():
        v, sh, ls, lg, ag, wg, ms, go, gm = calls[state["i"] % SETS]
        state["i"] += 1
        v.grad = lg.grad = ag.grad = wg.grad = None
        out, mask = fn.apply(v, sh, ls, lg, ag, wg, ms, 64)
        torch.autograd.backward([out, mask], [go, gm.view_as(mask)])

    us = []
    for _ in range(repeats):
        for _ in range(warmup):
            step()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            step()
        b.record()
        torch.cuda.synchronize()
        us.append(round(a.elapsed_time(b) * 1e3 / steps, 2))
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--key23", type=int, default=2)
    ap.add_argument("--label", default="this")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--cells", default="C3,C3k8,C3p")
    ap.add_argument("--dtypes", default="bf16,f16")
    ap.add_argument("--batches", default="1,2")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    if ROOT not in sys.path:
        sys.path.append(ROOT)
    import boxer_amd
    from boxer_amd import _lib
    import bench
    bench.WORKLOADS.setdefault("C3k8", (C2P, 300, 64, "instance"))
    torch.autograd.set_multithreading_enabled(False)       # (as bench.make_step: the backward on the calling thread)
    if args.key23 >= 0:
        _lib.set_option("inst_acc16", args.key23)
    for cell in args.cells.split(","):
        for name in args.dtypes.split(","):
            dtype = {"bf16": torch.bfloat16, "f16": torch.float16}[name]
            for batch in (int(b) for b in args.batches.split(",")):
                us = time_cell(bench, boxer_amd, cell, dtype, batch, args.steps, args.warmup, args.repeats)
                levels, lq, P, _ = bench.WORKLOADS[CELLS[cell]]
                print(json.dumps({"build": args.label, "key23": args.key23, "cell": cell, "dtype": name, "B": batch,
                                  "points_per_slice": lq * len(levels) * P, "us_per_step": us, "steps": args.steps,
                                  "input_sets": SETS}), flush=True)


if __name__ == "__main__":
    main()
