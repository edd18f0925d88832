"""What instance attention's inference forward costs from boxes and 2x2 logits: the three launches (``ops.box_grid_forward``
-> ``ops.instance_weights_forward`` -> ``ops.instance_attn_forward``, or ``ops.box_attn_forward`` for the flavour without
mask -- the module with ``fused_boxes`` off) against the one call ``ops.instance_attn_forward_boxes`` (the flag on), on
the C2' levels (100x167, 50x84, 25x42, 13x21), H = 8, C = 32, L = 4, k = 14, for Lq in {100, 300, 900}, B in {1, 2},
float32 / bf16 / f16, with and without mask_out.

    python tools/boxes_forward_step.py [--calls K] [--warmup W] [--repeats R] [--out FILE] [--only LEG]
    python tools/boxes_forward_step.py --table FILE [FILE ...]

Inputs as tools/inference_forward_step.py: windows cx, cy ~ U(0.05, 0.95), w, h ~ U(0.05, 0.5), box
offsets N(0, 1), logits N(0, 1).  Protocol of DESIGN.md 4.1: 8 input sets cycled, W warm-up calls, then K calls between
two HIP events on the op's stream; the two legs alternate, R repeats each, all kept.  Run it in three processes;
``--table`` then prints, per cell, the three launches' FASTEST repeat and the one call's SLOWEST.  ``--only three|one``
runs one leg alone, K calls per cell once: the process to put under a kernel trace for the kernel-only sums."""
import argparse
import json
import os
import sys

LEVELS = [(100, 167), (50, 84), (25, 42), (13, 21)]
H, C, K = 8, 32, 14
LQS, BATCHES = (100, 300, 900), (1, 2)
SETS = 8


def measure(args):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from boxer_amd import ops
    from boxer_amd.modules import _kernel_offsets
    dev = torch.device("cuda")
    shapes = torch.tensor(LEVELS, dtype=torch.long, device=dev)
    lsi = torch.cat((shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1]))
    S, L, P = int(shapes.prod(1).sum()), len(LEVELS), K * K
    kidx = _kernel_offsets(K, K).to(dev).contiguous()
    out = open(args.out, "a") if args.out else None

    def inputs(B, Lq, dtype, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        ctr = 0.05 + 0.9 * torch.rand(B, Lq, 2, device=dev, generator=g)
        wh = 0.05 + 0.45 * torch.rand(B, Lq, 2, device=dev, generator=g)
        return (torch.randn(B, S, H, C, device=dev, generator=g).to(dtype), torch.cat((ctr, wh), -1).contiguous(),
                torch.randn(B, Lq, H, L, 4, device=dev, generator=g),
                torch.randn(B, Lq, H, L, 2, 2, device=dev, generator=g))

    def three(v, ref, off, logits, mask):
        grid = ops.box_grid_forward(ref, off, kidx, None, 0)
        spatial, level = ops.instance_weights_forward(logits, K, need_level=mask)
        if mask:
            return ops.instance_attn_forward(v, shapes, lsi, grid, spatial, level, 64)
        return ops.box_attn_forward(v, shapes, lsi, grid, spatial.view(*spatial.shape[:4], P), 64)

    def one(v, ref, off, logits, mask):
        return ops.instance_attn_forward_boxes(v, shapes, lsi, ref, off, kidx, None, logits, K, mask)

    legs = {"three": three, "one": one}
    if args.only:
        legs = {args.only: legs[args.only]}
    for name, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16), ("f16", torch.float16)):
        for mask in (True, False):
            for Lq in LQS:
                for B in BATCHES:
                    sets = [inputs(B, Lq, dtype, seed) for seed in range(SETS)]
                    assert ops.forward_boxes_ok(sets[0][0], L, Lq, K)
                    runs = {leg: [] for leg in legs}
                    for _ in range(1 if args.only else args.repeats):
                        for leg, fn in legs.items():                           # the legs alternate
                            for i in range(args.warmup):
                                fn(*sets[i % SETS], mask)
                            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            torch.cuda.synchronize()
                            a.record()
                            for i in range(args.calls):
                                fn(*sets[i % SETS], mask)
                            b.record()
                            torch.cuda.synchronize()
                            runs[leg].append(round(a.elapsed_time(b) * 1e3 / args.calls, 2))
                    line = json.dumps({"dtype": name, "mask": int(mask), "Lq": Lq, "B": B, "us_per_call": runs,
                                       "calls": args.calls, "input_sets": SETS, "pid": os.getpid()})
                    print(line, flush=True)
                    if out:
                        out.write(line + "\n")
                        out.flush()


def table(paths):
    rows = {}
    for path in paths:
        with open(path) as fh:
            for line in fh:
                if line.startswith("{"):
                    r = json.loads(line)
                    for leg, runs in r["us_per_call"].items():
                        rows.setdefault((r["dtype"], r["mask"], r["Lq"], r["B"]), {}).setdefault(leg, []).extend(runs)
    print("| type | mask_out | Lq | B | three launches, us (fastest .. slowest) | one call, us (fastest .. slowest) | "
          "slowest one / fastest three |")
    print("|---|---|---|---|---|---|---|")
    for key in sorted(rows):
        t, o = rows[key].get("three", [float("nan")]), rows[key].get("one", [float("nan")])
        print("| %s | %s | %d | %d | %.1f .. %.1f | %.1f .. %.1f | %.2f |" % (
            key[0], "yes" if key[1] else "no", key[2], key[3], min(t), max(t), min(o), max(o), max(o) / min(t)))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=("three", "one"), help="one leg alone, once per cell (for a kernel trace)")
    ap.add_argument("--out", help="append the JSON lines to this file")
    ap.add_argument("--table", nargs="+", help="print the table of these JSON-lines files")
    args = ap.parse_args()
    sys.exit(table(args.table) if args.table else measure(args))


if __name__ == "__main__":
    main()
