"""What box attention's training step (forward + backward) costs from boxes and L*P logits, H = 8, C = 32, 2 x 2 points a
level, float32 / bf16 / f16, gradients for value, reference windows, box offsets and logits, on
  decoder shapes   C2 levels with Lq 300 at B 1 and 2; C5 (468 x 468, Lq 1 000, one level, learned rotation) at B 1;
  encoder shapes   C2 (Lq = S) at B 1 and 2; C5' (234 x 234, 117 x 117, Lq = S, fixed angle) at B 1.
  points  today's fastest configuration: ``BoxGridFunction`` -> ``LogitSoftmaxFunction`` ->
          ``BoxAttn{,BF16,F16}Function`` (the module with ``fused_grid`` and ``fused_pointwise``);
  boxes   ``BoxAttnBoxesFunction`` (the module with ``fused_boxes_train``);
  value   ``BoxAttnBoxesValueFunction`` called directly (the module takes it with ``fused_boxes_value`` where Lq < S
          only: the encoder cells are measured here although the module would not route them).
The legs are built from the same sources; the "points" leg is code the other two did not touch.

    python tools/box_boxes_backward_step.py [--steps K] [--warmup W] [--repeats R] [--out FILE] [--only LEG]
                                            [--dtype f32|bf16|f16] [--cell NAME] [--batch B]
    python tools/box_boxes_backward_step.py --table FILE [FILE ...]

Inputs as tools/box_boxes_forward_step.py; upstream gradients N(0, 1) in the storage type.  8 input sets cycled, W
warm-up steps, then K steps between two HIP events on the op's stream; the legs alternate, R repeats each, all kept.
After the timing, one step per leg alone with the caching allocator's peak counter reset:
``torch.cuda.max_memory_allocated`` of that step, what it adds to the bytes allocated before it (the inputs of all sets;
the library's cached workspaces are released first, so each leg's figure holds its own), and the bytes the forward
saved for the backward beyond the inputs' own storages.  ``--table`` prints, per cell, the points leg's FASTEST repeat
and the boxes and value legs' SLOWEST.  ``--only points|boxes|value`` runs one leg alone, K steps per cell once: the process to put
under a kernel trace."""
import argparse
import json
import os
import sys

C2 = [(100, 100), (50, 50), (25, 25), (13, 13)]
C5 = [(468, 468)]
C5P = [(234, 234), (117, 117)]
H, C, KS = 8, 32, 2
SETS = 8
# name, levels, Lq (None: one query a pixel), B, angle_mode
CELLS = [("C2 dec", C2, 300, 1, 0), ("C2 dec", C2, 300, 2, 0), ("C5", C5, 1000, 1, 1), ("C2 enc", C2, None, 1, 0),
         ("C2 enc", C2, None, 2, 0), ("C5' enc", C5P, None, 1, 2)]


def measure(args):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import boxer_amd as ba
    from boxer_amd import ops
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
        if (args.cell and args.cell != cell) or (args.batch and args.batch != B):
            continue
        shapes, lsi, S = tables(levels)
        L, Lq = len(levels), lq if lq is not None else S
        V = 5 if mode == 1 else 4
        kidx = _kernel_offsets(KS, KS if mode == 0 else 2).to(dev).contiguous()

        def inputs(dtype, seed):
            g = torch.Generator(device=dev).manual_seed(seed)
            ref = windows(levels, B, lq, g)
            if mode:
                ref = torch.cat((ref, torch.rand(B, Lq, 1, device=dev, generator=g) - 0.5), -1)
            leaves = (torch.randn(B, S, H, C, device=dev, generator=g).to(dtype), ref.float().contiguous(),
                      torch.randn(B, Lq, H, L, V, device=dev, generator=g),
                      torch.randn(B, Lq, H, L * P, device=dev, generator=g))
            gout = torch.randn(B, Lq, H * C, device=dev, generator=g).to(dtype)
            return tuple(t.requires_grad_() for t in leaves), gout

        def points(fn, value, ref, off, logits):
            grid = ba.BoxGridFunction.apply(ref, off, kidx, None, mode)
            attn = ba.LogitSoftmaxFunction.apply(logits).view(B, Lq, H, L, P)
            return fn.apply(value, shapes, lsi, grid, attn, 64)

        def boxes(fn, value, ref, off, logits):
            return ba.BoxAttnBoxesFunction.apply(value, shapes, lsi, ref, off, kidx, None, logits, mode)

        def step(leg, fn, leaves, gout):
            return torch.autograd.grad(leg(fn, *leaves), leaves, gout)

        def saved_bytes(node, seen, tensors):
            """Bytes of the tensors the graph below ``node`` keeps for its backward (each storage once; the leaves'
            own storages, which live anyway, are not counted)."""
            if node is None or node in seen:
                return
            seen.add(node)
            for name in dir(node):
                if name.startswith("_saved_"):
                    t = getattr(node, name)
                    if isinstance(t, torch.Tensor):
                        tensors[t.untyped_storage().data_ptr()] = t.untyped_storage().nbytes()
            if hasattr(node, "saved_tensors"):
                for t in node.saved_tensors:
                    if t is not None:
                        tensors[t.untyped_storage().data_ptr()] = t.untyped_storage().nbytes()
            for nxt, _ in node.next_functions:
                saved_bytes(nxt, seen, tensors)

        def value(fn, value, ref, off, logits):
            return ba.BoxAttnBoxesValueFunction.apply(value, shapes, lsi, ref, off, kidx, None, logits, mode)

        legs = {"points": points, "boxes": boxes, "value": value}
        if args.only:
            legs = {args.only: legs[args.only]}
        for name, dtype, fn in (("f32", torch.float32, ba.BoxAttnFunction), ("bf16", torch.bfloat16, ba.BoxAttnBF16Function),
                                ("f16", torch.float16, ba.BoxAttnF16Function)):
            if args.dtype and args.dtype != name:
                continue
            sets = [inputs(dtype, seed) for seed in range(SETS)]
            assert ops.box_forward_boxes_ok(sets[0][0][0], L, Lq, P) and ops.box_backward_boxes_ok(sets[0][0][0], L, Lq, P)
            assert "value" not in legs or ops.box_backward_boxes_value_ok(sets[0][0][0], L, Lq, P)
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
            peak, added, saved = {}, {}, {}
            for leg, body in legs.items():
                torch.cuda.synchronize()
                ops.release_workspaces()                   # both legs start without the other's cached workspaces
                before = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                leaves, gout = sets[0]
                result = body(fn, *leaves)
                own = {t.untyped_storage().data_ptr() for t in leaves}
                kept = {}
                saved_bytes(result.grad_fn, set(), kept)
                saved[leg] = sum(n for p, n in kept.items() if p not in own)
                grads = torch.autograd.grad(result, leaves, gout)
                torch.cuda.synchronize()
                peak[leg] = torch.cuda.max_memory_allocated()
                added[leg] = peak[leg] - before
                del grads, result, kept
            line = json.dumps({"cell": cell, "dtype": name, "Lq": Lq, "B": B, "angle_mode": mode, "us_per_step": runs,
                               "max_memory_allocated": peak, "peak_bytes_over_start": added,
                               "saved_for_backward_bytes": saved, "steps": args.steps, "input_sets": SETS,
                               "pid": os.getpid()})
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del sets


def table(paths):
    rows, mem, kept = {}, {}, {}
    for path in paths:
        with open(path) as fh:
            for line in fh:
                if line.startswith("{"):
                    r = json.loads(line)
                    key = (r["cell"], r["B"], r["dtype"], r["Lq"])
                    for leg, runs in r["us_per_step"].items():
                        rows.setdefault(key, {}).setdefault(leg, []).extend(runs)
                    for leg, n in r["peak_bytes_over_start"].items():
                        mem.setdefault(key, {}).setdefault(leg, []).append(n)
                    for leg, n in r["saved_for_backward_bytes"].items():
                        kept.setdefault(key, {}).setdefault(leg, []).append(n)
    print("| shape | B | type | Lq | points, us a step (fastest .. slowest) | boxes, us a step (fastest .. slowest) | "
          "value, us a step (fastest .. slowest) | slowest boxes / fastest points | slowest value / slowest boxes | "
          "peak MB over start, points | boxes | value | saved for backward MB, points | boxes | value |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    nan = [float("nan")]
    for key in sorted(rows):
        p, b, v = (rows[key].get(leg, nan) for leg in ("points", "boxes", "value"))
        mp, mb, mv = (mem[key].get(leg, nan) for leg in ("points", "boxes", "value"))
        kp, kb, kv = (kept[key].get(leg, nan) for leg in ("points", "boxes", "value"))
        print("| %s | %d | %s | %d | %.1f .. %.1f | %.1f .. %.1f | %.1f .. %.1f | %.2f | %.2f | %.1f | %.1f | %.1f | %.1f "
              "| %.1f | %.1f |" % (key[0], key[1], key[2], key[3], min(p), max(p), min(b), max(b), min(v), max(v),
                                   max(b) / min(p), max(v) / max(b), max(mp) / 1e6, max(mb) / 1e6, max(mv) / 1e6,
                                   max(kp) / 1e6, max(kb) / 1e6, max(kv) / 1e6))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=("points", "boxes", "value"), help="one leg alone, once per cell (for a kernel trace)")
    ap.add_argument("--dtype", choices=("f32", "bf16", "f16"), help="this storage type only")
    ap.add_argument("--cell", help="this shape only (e.g. 'C2 dec')")
    ap.add_argument("--batch", type=int, help="this batch size only")
    ap.add_argument("--out", help="append the JSON lines to this file")
    ap.add_argument("--table", nargs="+", help="print the table of these JSON-lines files")
    args = ap.parse_args()
    sys.exit(table(args.table) if args.table else measure(args))


if __name__ == "__main__":
    main()
