"""The float16 storage mode against bf16 on the same GPU, same process, same protocol as bench.py's headline:
C2 (encoder, box attention) and C3' (instance attention, mask decoder), one training step of the compiled drop-in
through the reference-style Functions (bench.make_step(entry="reference")), 8 input sets cycled, bench.run_timed.

    python tools/f16_step.py [--steps K] [--warmup W] [--workloads C2,C3p]

Prints one JSON line per (workload, dtype) and the f16 / bf16 ratio per workload."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402

SETS = 8


def time_step(workload, dtype, steps, warmup):
    steps_k = [bench.make_step(bench.make_inputs(workload, dtype, "cuda", seed=s), entry="reference")
               for s in range(SETS)]
    state = {"i": 0}

    def step():
        steps_k[state["i"] % SETS]()
        state["i"] += 1
    for _ in range(bench.PREHEAT_STEPS):
        step()
    elapsed = bench.run_timed(step, steps, warmup, torch.cuda.synchronize)
    return elapsed / steps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workloads", default="C2,C3p")
    args = ap.parse_args()
    for w in args.workloads.split(","):
        us = {}
        # interleaved twice (bf16, f16, bf16, f16): clock and thermal drift hit both alike; the faster of each kept
        for rep in range(2):
            for name, dtype in (("bf16", torch.bfloat16), ("f16", torch.float16)):
                t = time_step(w, dtype, args.steps, args.warmup)
                us[name] = min(us.get(name, t), t)
        for name in ("bf16", "f16"):
            print(json.dumps({"workload": w, "dtype": name, "us_per_step": round(us[name], 2),
                              "steps": args.steps, "input_sets": SETS}))
        print(json.dumps({"workload": w, "f16_over_bf16": round(us["f16"] / us["bf16"], 4)}))


if __name__ == "__main__":
    main()
