"""What box attention's inference forward costs on ENCODER shapes (one query a pixel, H = 8, C = 32, 2 x 2 points a level,
float32 / bf16 / f16), three ways:
  (a) three   the three launches ``ops.box_grid_forward`` -> ``ops.softmax_forward`` -> ``ops.box_attn_forward`` with the
              host tables: the window-staged forward (asserted);
  (b) one     ``ops.box_attn_forward_boxes``: the row gather from boxes and logits (``fused_boxes``);
  (c) staged  ``ops.box_attn_forward_boxes_staged``: the window-staged forward from boxes and logits (``fused_boxes`` +
              ``fused_boxes_staged``)
on C2 (100 x 100 .. 13 x 13) and C2' (100 x 167 .. 13 x 21) at B 1 and 2 and C5' (234 x 234, 117 x 117, fixed angle) at
B 1.

    python tools/box_boxes_staged_forward_step.py [--calls K] [--warmup W] [--repeats R] [--out FILE]
    python tools/box_boxes_staged_forward_step.py --table FILE [FILE ...]

Inputs and protocol as tools/box_boxes_forward_step.py (query i is pixel i, its window the pixel's centre and four pixels
of its level; angles ~ U(-0.5, 0.5), box offsets N(0, 1), logits N(0, 1); 8 input sets cycled, W warm-up calls, then K
calls between two HIP events on the op's stream); the THREE legs alternate inside one process, R repeats each, all
kept.  Run it in two processes; ``--table`` then prints, per cell, every leg's fastest and slowest repeat and the
verdict: (c) wins a cell only if its SLOWEST repeat is below the FASTEST repeat of both (a) and (b)."""
import argparse
import json
import os
import sys

C2 = [(100, 100), (50, 50), (25, 25), (13, 13)]
C2P = [(100, 167), (50, 84), (25, 42), (13, 21)]
C5P = [(234, 234), (117, 117)]
H, C, KS = 8, 32, 2
SETS = 8
LEGS = ("three", "one", "staged")
# name, levels, B, angle_mode
CELLS = [("C2 enc", C2, 1, 0), ("C2 enc", C2, 2, 0), ("C2' enc", C2P, 1, 0), ("C2' enc", C2P, 2, 0), ("C5' enc", C5P, 1, 2)]


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

    def windows(levels, B):
        rows = []
        for hl, wl in levels:
            ys, xs = torch.meshgrid(torch.arange(hl, device=dev), torch.arange(wl, device=dev), indexing="ij")
            rows.append(torch.stack([(xs.reshape(-1) + 0.5) / wl, (ys.reshape(-1) + 0.5) / hl,
                                     torch.full((hl * wl,), 4.0 / wl, device=dev),
                                     torch.full((hl * wl,), 4.0 / hl, device=dev)], -1))
        return torch.cat(rows, 0)[None].expand(B, -1, -1)

    for cell, levels, B, mode in CELLS:
        shapes, lsi, S = tables(levels)
        L, Lq = len(levels), S
        V = 5 if mode == 1 else 4
        kidx = _kernel_offsets(KS, KS if mode == 0 else 2).to(dev).contiguous()

        def inputs(dtype, seed):
            g = torch.Generator(device=dev).manual_seed(seed)
            ref = windows(levels, B)
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

        def staged(v, ref, off, logits):
            return ops.box_attn_forward_boxes_staged(v, shapes, lsi, ref, off, kidx, None, logits, mode)

        fns = {"three": three, "one": one, "staged": staged}
        for name, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16), ("f16", torch.float16)):
            sets = [inputs(dtype, seed) for seed in range(SETS)]
            assert ops.box_forward_boxes_ok(sets[0][0], L, Lq, P)
            assert ops.box_forward_boxes_staged_ok(sets[0][0], shapes, lsi, Lq, P)
            probe = torch.empty(B, Lq, H, L, P, 2, device=dev)
            route = _lib.FWD_FAMILIES[ops.forward_route(sets[0][0], probe, shapes, lsi)]
            del probe
            assert route == "staged", route
            runs = {leg: [] for leg in LEGS}
            for _ in range(args.repeats):
                for leg in LEGS:                                               # the legs alternate
                    fn = fns[leg]
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
                    key = (r["cell"], r["B"], r["dtype"])
                    for leg, runs in r["us_per_call"].items():
                        rows.setdefault(key, {}).setdefault(leg, []).extend(runs)
    print("| shape | B | type | (a) three launches, us | (b) one call, row gather, us | (c) one call, window-staged, us | "
          "slowest (c) / fastest (a) | slowest (c) / fastest (b) | verdict |")
    print("|---|---|---|---|---|---|---|---|---|")
    for key in sorted(rows):
        t, o, s = (rows[key][leg] for leg in LEGS)
        print("| %s | %d | %s | %.1f .. %.1f | %.1f .. %.1f | %.1f .. %.1f | %.2f | %.2f | %s |" % (
            key + (min(t), max(t), min(o), max(o), min(s), max(s), max(s) / min(t), max(s) / min(o),
                   "wins" if max(s) < min(t) and max(s) < min(o) else "no win")))
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
