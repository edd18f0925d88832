"""What box attention's inference forward costs from boxes and L*P logits: the three launches (``ops.box_grid_forward`` ->
``ops.softmax_forward`` -> ``ops.box_attn_forward`` with the host tables, so encoder shapes take the window-staged
forward -- the module with every other fusion on and ``fused_boxes`` off) against the one call
``ops.box_attn_forward_boxes`` (the flag on), H = 8, C = 32, 2 x 2 points a level, float32 / bf16 / f16, on
  decoder shapes   C2 levels and C2' levels with Lq 300 at B 1 and 2; C5 (468 x 468, Lq 1 000, one level, learned
                   rotation) at B 1;
  encoder shapes   C2 (Lq = S) at B 1 and 2; C5' (234 x 234, 117 x 117, Lq = S, fixed angle) at B 1.

    python tools/box_boxes_forward_step.py [--calls K] [--warmup W] [--repeats R] [--out FILE]
    python tools/box_boxes_forward_step.py --table FILE [FILE ...]

Decoder inputs as tools/boxes_forward_step.py: windows cx, cy ~ U(0.05, 0.95), w, h ~ U(0.05, 0.5); encoder inputs:
query i is pixel i, its window the pixel's centre and four pixels of its level; angles ~ U(-0.5, 0.5), box offsets
N(0, 1), logits N(0, 1).  Protocol of DESIGN.md 4.1: 8 input sets cycled, W warm-up calls, then K calls between two HIP
events on the op's stream; the two legs alternate, R repeats each, all kept.  Run it in two processes; ``--table`` then
prints, per cell, the three launches' FASTEST repeat and the one call's SLOWEST."""
import argparse
import json
import os
import sys

C2 = [(100, 100), (50, 50), (25, 25), (13, 13)]
C2P = [(100, 167), (50, 84), (25, 42), (13, 21)]
C5 = [(468, 468)]
C5P = [(234, 234), (117, 117)]
H, C, KS = 8, 32, 2
SETS = 8
# name, levels, Lq (None: one query a pixel), B, angle_mode
CELLS = [("C2 dec", C2, 300, 1, 0), ("C2 dec", C2, 300, 2, 0), ("C2' dec", C2P, 300, 1, 0), ("C2' dec", C2P, 300, 2, 0),
         ("C5", C5, 1000, 1, 1), ("C2 enc", C2, None, 1, 0), ("C2 enc", C2, None, 2, 0), ("C5' enc", C5P, None, 1, 2)]


def measure(args):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from boxer_amd import _lib, ops
    from boxer_amd.modules import _kernel_offsets
    dev = torch.device("cuda")
    P = KS * KS
    out = open(args.out, "a") if args.out else None

    def tables(levels):
        shapes = torch.tensor(levels, dtype=torch.long, device=dev)
        return shapes, torch.cat((shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1])), int(shapes.prod(1).sum())

    def windows(levels, B, Lq, g):
        if Lq is not None:
            ctr = 0.05 + 0.9 * torch.rand(B, Lq, 2, device=dev, generator=g)
            wh = 0.05 + 0.45 * torch.rand(B, Lq, 2, device=dev, generator=g)
            return torch.cat((ctr, wh), -1)
        rows = []
        for hl, wl in levels:
            ys, xs = torch.meshgrid(torch.arange(hl, device=dev), torch.arange(wl, device=dev), indexing="ij")
            rows.append(torch.stack([(xs.reshape(-1) + 0.5) / wl, (ys.reshape(-1) + 0.5) / hl,
                                     torch.full((hl * wl,), 4.0 / wl, device=dev),
                                     torch.full((hl * wl,), 4.0 / hl, device=dev)], -1))
        return torch.cat(rows, 0)[None].expand(B, -1, -1)

    for cell, levels, lq, B, mode in CELLS:
        shapes, lsi, S = tables(levels)
        L, Lq = len(levels), lq if lq is not None else S
        V = 5 if mode == 1 else 4
        kidx = _kernel_offsets(KS, KS if mode == 0 else 2).to(dev).contiguous()

        def inputs(dtype, seed):
            g = torch.Generator(device=dev).manual_seed(seed)
            ref = windows(levels, B, lq, g)
            if mode:
                ref = torch.cat((ref, torch.rand(B, Lq, 1, device=dev, generator=g) - 0.5), -1)
            return (torch.randn(B, S, H, C, device=dev, generator=g).to(dtype), ref.float().contiguous(),
                    torch.randn(B, Lq, H, L, V, device=dev, generator=g),
                    torch.randn(B, Lq, H, L * P, device=dev, generator=g))

        def three(v, ref, off, logits):
            grid = ops.box_grid_forward(ref, off, kidx, None, mode)
            attn = ops.softmax_forward(logits)
            return ops.box_attn_forward(v, shapes, lsi, grid, attn.view(B, Lq, H, L, P), 64)

        def one(v, ref, off, logits):
            return ops.box_attn_forward_boxes(v, shapes, lsi, ref, off, kidx, None, logits, mode)

        for name, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16), ("f16", torch.float16)):
            sets = [inputs(dtype, seed) for seed in range(SETS)]
            assert ops.box_forward_boxes_ok(sets[0][0], L, Lq, P)
            probe = torch.empty(B, Lq, H, L, P, 2, device=dev)
            route = _lib.FWD_FAMILIES[ops.forward_route(sets[0][0], probe, shapes, lsi)]
            del probe
            runs = {"three": [], "one": []}
            for _ in range(args.repeats):
                for leg, fn in (("three", three), ("one", one)):               # the legs alternate
                    for i in range(args.warmup):
                        fn(*sets[i % SETS])
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    a.record()
                    for i in range(args.calls):
                        fn(*sets[i % SETS])
                    b.record()
                    torch.cuda.synchronize()
                    runs[leg].append(round(a.elapsed_time(b) * 1e3 / args.calls, 2))
            line = json.dumps({"cell": cell, "dtype": name, "Lq": Lq, "B": B, "angle_mode": mode, "three_route": route,
                               "us_per_call": runs, "calls": args.calls, "input_sets": SETS, "pid": os.getpid()})
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del sets


def table(paths):
    rows = {}
    for path in paths:
        with open(path) as fh:
            for line in fh:
                if line.startswith("{"):
                    r = json.loads(line)
                    key = (r["cell"], r["B"], r["dtype"], r["Lq"], r["three_route"])
                    for leg, runs in r["us_per_call"].items():
                        rows.setdefault(key, {}).setdefault(leg, []).extend(runs)
    print("| shape | B | type | Lq | three launches' forward | three launches, us (fastest .. slowest) | "
          "one call, us (fastest .. slowest) | slowest one / fastest three |")
    print("|---|---|---|---|---|---|---|---|")
    for key in sorted(rows):
        t, o = rows[key]["three"], rows[key]["one"]
        print("| %s | %d | %s | %d | %s | %.1f .. %.1f | %.1f .. %.1f | %.2f |" % (
            key[0], key[1], key[2], key[3], key[4], min(t), max(t), min(o), max(o), max(o) / min(t)))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", help="append the JSON lines to this file")
    ap.add_argument("--table", nargs="+", help="print the table of these JSON-lines files")
    args = ap.parse_args()
    sys.exit(table(args.table) if args.table else measure(args))


if __name__ == "__main__":
    main()
