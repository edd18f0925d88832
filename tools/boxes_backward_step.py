"""What instance attention's training step (forward + backward) costs from boxes and 2x2 logits, at the mask model's
shape: the C2' / C3' levels (100x167, 50x84, 25x42, 13x21), H = 8, C = 32, L = 4, Lq = 300, k = 14, B in {1, 2},
float32 / bf16 / f16, gradients for value, reference windows, box offsets and logits.
  points  today's fastest configuration: ``BoxGridFunction`` -> ``InstanceWeightsFunction`` ->
          ``InstanceAttn{,BF16,F16}Function`` (the module with ``fused_grid`` and ``fused_pointwise``);
  boxes   ``InstanceAttnBoxesFunction`` (the module with ``fused_boxes_train``).
Both legs are built from the same sources; the "points" leg is code the "boxes" leg did not touch.

    python tools/boxes_backward_step.py [--steps K] [--warmup W] [--repeats R] [--out FILE] [--only LEG]
                                        [--dtype f32|bf16|f16] [--batch B]
    python tools/boxes_backward_step.py --table FILE [FILE ...]

Inputs as tools/boxes_forward_step.py: windows cx, cy ~ U(0.05, 0.95), w, h ~ U(0.05, 0.5), box offsets N(0, 1),
logits N(0, 1), upstream gradients N(0, 1) in the storage type.  8 input sets cycled, W warm-up steps, then K steps
between two HIP events on the op's stream; the legs alternate, R repeats each, all kept.  After the timing, one step per
leg alone with the caching allocator's peak counter reset: ``torch.cuda.max_memory_allocated`` of that step and what
it adds to the bytes allocated before it (the inputs of all sets and the library's cached workspaces).  ``--table``
prints, per cell, the points leg's FASTEST repeat and the boxes leg's SLOWEST.  ``--only points|boxes`` runs one leg
alone, K steps per cell once: the process to put under a kernel trace (``--dtype`` / ``--batch``: one cell of the grid)."""
import argparse
import json
import os
import sys

LEVELS = [(100, 167), (50, 84), (25, 42), (13, 21)]
H, C, K, LQ = 8, 32, 14, 300
BATCHES = (1, 2)
SETS = 8


def measure(args):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import boxer_amd as ba
    from boxer_amd import ops
    from boxer_amd.modules import _kernel_offsets
    dev = torch.device("cuda")
    shapes = torch.tensor(LEVELS, dtype=torch.long, device=dev)
    lsi = torch.cat((shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1]))
    S, L, P = int(shapes.prod(1).sum()), len(LEVELS), K * K
    kidx = _kernel_offsets(K, K).to(dev).contiguous()
    out = open(args.out, "a") if args.out else None

    def inputs(B, dtype, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        ctr = 0.05 + 0.9 * torch.rand(B, LQ, 2, device=dev, generator=g)
        wh = 0.05 + 0.45 * torch.rand(B, LQ, 2, device=dev, generator=g)
        leaves = (torch.randn(B, S, H, C, device=dev, generator=g).to(dtype), torch.cat((ctr, wh), -1).contiguous(),
                  torch.randn(B, LQ, H, L, 4, device=dev, generator=g),
                  torch.randn(B, LQ, H, L, 2, 2, device=dev, generator=g))
        grads = (torch.randn(B, LQ, H * C, device=dev, generator=g).to(dtype),
                 torch.randn(B, LQ, K, K, H * C, device=dev, generator=g).to(dtype))
        return tuple(t.requires_grad_() for t in leaves), grads

    def points(fn, value, ref, off, logits):
        grid = ba.BoxGridFunction.apply(ref, off, kidx, None, 0)
        spatial, level = ba.InstanceWeightsFunction.apply(logits, K, True)
        return fn.apply(value, shapes, lsi, grid, spatial, level, K, 64)

    def boxes(fn, value, ref, off, logits):
        return ba.InstanceAttnBoxesFunction.apply(value, shapes, lsi, ref, off, kidx, None, logits, K)

    def step(leg, fn, leaves, grads):
        return torch.autograd.grad(leg(fn, *leaves), leaves, grads)

    legs = {"points": points, "boxes": boxes}
    if args.only:
        legs = {args.only: legs[args.only]}
    for name, dtype, fn in (("f32", torch.float32, ba.InstanceAttnFunction),
                            ("bf16", torch.bfloat16, ba.InstanceAttnBF16Function),
                            ("f16", torch.float16, ba.InstanceAttnF16Function)):
        if args.dtype and args.dtype != name:
            continue
        for B in BATCHES if not args.batch else (args.batch,):
            sets = [inputs(B, dtype, seed) for seed in range(SETS)]
            assert ops.forward_boxes_ok(sets[0][0][0], L, LQ, K) and ops.backward_boxes_ok(sets[0][0][0], L, LQ, K)
            runs = {leg: [] for leg in legs}
            for _ in range(1 if args.only else args.repeats):
                for leg, body in legs.items():                                 # the legs alternate
                    for i in range(args.warmup):
                        step(body, fn, *sets[i % SETS])
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    a.record()
                    for i in range(args.steps):
                        step(body, fn, *sets[i % SETS])
                    b.record()
                    torch.cuda.synchronize()
                    runs[leg].append(round(a.elapsed_time(b) * 1e3 / args.steps, 2))
            peak, added = {}, {}
            for leg, body in legs.items():
                torch.cuda.synchronize()
                before = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                grads = step(body, fn, *sets[0])
                torch.cuda.synchronize()
                peak[leg] = torch.cuda.max_memory_allocated()
                added[leg] = peak[leg] - before
                del grads
            line = json.dumps({"dtype": name, "Lq": LQ, "B": B, "us_per_step": runs, "max_memory_allocated": peak,
                               "peak_bytes_over_start": added, "steps": args.steps, "input_sets": SETS,
                               "pid": os.getpid()})
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del sets


def table(paths):
    rows, mem = {}, {}
    for path in paths:
        with open(path) as fh:
            for line in fh:
                if line.startswith("{"):
                    r = json.loads(line)
                    key = (r["dtype"], r["B"])
                    for leg, runs in r["us_per_step"].items():
                        rows.setdefault(key, {}).setdefault(leg, []).extend(runs)
                    for leg, n in r["peak_bytes_over_start"].items():
                        mem.setdefault(key, {}).setdefault(leg, []).append(n)
    print("| type | B | points, us a step (fastest .. slowest) | boxes, us a step (fastest .. slowest) | "
          "slowest boxes / fastest points | peak MB over start, points | boxes |")
    print("|---|---|---|---|---|---|---|")
    nan = [float("nan")]
    for key in sorted(rows):
        p, b = rows[key].get("points", nan), rows[key].get("boxes", nan)
        mp, mb = mem[key].get("points", nan), mem[key].get("boxes", nan)
        print("| %s | %d | %.1f .. %.1f | %.1f .. %.1f | %.2f | %.1f | %.1f |" % (
            key[0], key[1], min(p), max(p), min(b), max(b), max(b) / min(p), max(mp) / 1e6, max(mb) / 1e6))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=("points", "boxes"), help="one leg alone, once per cell (for a kernel trace)")
    ap.add_argument("--dtype", choices=("f32", "bf16", "f16"), help="this storage type only")
    ap.add_argument("--batch", type=int, help="this batch size only")
    ap.add_argument("--out", help="append the JSON lines to this file")
    ap.add_argument("--table", nargs="+", help="print the table of these JSON-lines files")
    args = ap.parse_args()
    sys.exit(table(args.table) if args.table else measure(args))


if __name__ == "__main__":
    main()
