"""What box attention's training step (forward + backward) costs from boxes and L*P logits, H = 8, C = 32, 2 x 2 points a
level, float32 / bf16 / f16, gradients for value, reference windows, box offsets and logits, on
  decoder shapes   C2 levels with Lq 300 at B 1 and 2; C5 (468 x 468, Lq 1 000, one level, learned rotation) at B 1;
  encoder shapes   C2 (Lq = S) at B 1 and 2; C5' (234 x 234, 117 x 117, Lq = S, fixed angle) at B 1.
  points  today's fastest configuration: ``BoxGridFunction`` -> ``LogitSoftmaxFunction`` ->
          ``BoxAttn{,BF16,F16}Function`` (the module with ``fused_grid`` and ``fused_pointwise``);
  boxes   ``BoxAttnBoxesFunction`` (the module with ``fused_boxes_train``);
  value   ``BoxAttnBoxesValueFunction`` called directly (the module takes it with ``fused_boxes_value`` where Lq < S
          only: the encoder cells are measured here although the module would not route them);
  staged  ``BoxAttnBoxesStagedFunction`` (the module with ``fused_boxes_train`` + ``fused_boxes_train_staged``): the
          encoder cells only (C2 at B 1 and 2, C2' -- 100 x 167 .. 13 x 21 -- at B 2, C5'), where both staged calls
          have their kernel.
The legs are built from the same sources; the "points" leg is code the others did not touch.

    python tools/box_boxes_backward_step.py [--steps K] [--warmup W] [--repeats R] [--out FILE] [--only LEG]
                                            [--dtype f32|bf16|f16] [--cell NAME] [--batch B] [--launch]
    python tools/box_boxes_backward_step.py --table FILE [FILE ...]

``--launch`` measures, on the encoder cells, the DEVICE time of the parameter-gradient launch alone, three ways on the
same operands: ``staged`` ``ops.box_attn_backward_boxes_staged``; ``gather`` ``ops.box_attn_backward_boxes``
(bwd2_boxes_kernel); ``three`` the launches the staged one replaces, ``ops.box_attn_backward(want=2)`` on the
window-staged route (asserted) + ``ops.box_grid_backward`` + ``ops.softmax_backward``, their per-point inputs made
outside the timed region.  The K calls of a repeat are enqueued behind ~30 ms of matrix products, so the two HIP events
around them see the device's time, not the host's; the legs alternate, R repeats each, all kept.

Inputs as tools/box_boxes_forward_step.py; upstream gradients N(0, 1) in the storage type.  8 input sets cycled, W
warm-up steps, then K steps between two HIP events on the op's stream; the legs alternate, R repeats each, all kept.
After the timing, one step per leg alone with the caching allocator's peak counter reset:
``torch.cuda.max_memory_allocated`` of that step, what it adds to the bytes allocated before it (the inputs of all sets;
the library's cached workspaces are released first, so each leg's figure holds its own), and the bytes the forward
saved for the backward beyond the inputs' own storages.  ``--table`` prints, per cell, the points leg's FASTEST repeat
and the other legs' SLOWEST, and for ``--launch`` lines the verdict: the staged launch wins a cell only if its
SLOWEST repeat is below the FASTEST repeat of both others.  ``--only points|boxes|value|staged`` runs one leg alone, K steps per cell once: the process to put
under a kernel trace."""
import argparse
import json
import os
import sys

C2 = [(100, 100), (50, 50), (25, 25), (13, 13)]
C5 = [(468, 468)]
C5P = [(234, 234), (117, 117)]
C2P = [(100, 167), (50, 84), (25, 42), (13, 21)]
H, C, KS = 8, 32, 2
SETS = 8
# name, levels, Lq (None: one query a pixel), B, angle_mode
CELLS = [("C2 dec", C2, 300, 1, 0), ("C2 dec", C2, 300, 2, 0), ("C5", C5, 1000, 1, 1), ("C2 enc", C2, None, 1, 0),
         ("C2 enc", C2, None, 2, 0), ("C2' enc", C2P, None, 2, 0), ("C5' enc", C5P, None, 1, 2)]
LEGS = ("points", "boxes", "value", "staged")
LAUNCH_LEGS = ("three", "gather", "staged")


def launch_cell(args, out, cell, B, mode, shapes, lsi, S, L, kidx, inputs):
    """--launch: the device time of the parameter-gradient launch of one encoder cell, three ways (module docstring)."""
    import torch
    from boxer_amd import _lib, ops
    P, Lq = KS * KS, S
    spin = torch.randn(8192, 8192, device="cuda")
    for name, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16), ("f16", torch.float16)):
        if args.dtype and args.dtype != name:
            continue
        sets = []
        for seed in range(SETS):
            (value, ref, off, logits), gout = inputs(dtype, seed)
            value, ref, off, logits = (t.detach() for t in (value, ref, off, logits))
            grid = ops.box_grid_forward(ref, off, kidx, None, mode)
            attn = ops.softmax_forward(logits)
            sets.append((value, ref, off, logits, gout, grid, attn))
        v0, grid0 = sets[0][0], sets[0][5]
        assert ops.box_backward_boxes_ok(v0, L, Lq, P) and ops.box_backward_boxes_staged_ok(v0, shapes, lsi, Lq, P)
        route = _lib.FWD_FAMILIES[ops.forward_route(v0, grid0, shapes, lsi)]
        assert route == "staged", route

        def three(value, ref, off, logits, gout, grid, attn):
            _, gloc, gattn = ops.box_attn_backward(value, shapes, lsi, grid, attn.view(B, Lq, H, L, P), gout, 64, want=2)
            ops.box_grid_backward(ref, off, kidx, None, mode, gloc, need_ref_grad=True)
            ops.softmax_backward(attn, gattn.view(attn.shape), torch.float32)

        def gather(value, ref, off, logits, gout, grid, attn):
            ops.box_attn_backward_boxes(value, shapes, lsi, ref, off, kidx, None, logits, mode, gout, need_ref_grad=True)

        def staged(value, ref, off, logits, gout, grid, attn):
            ops.box_attn_backward_boxes_staged(value, shapes, lsi, ref, off, kidx, None, logits, mode, gout,
                                               need_ref_grad=True)

        fns = {"three": three, "gather": gather, "staged": staged}
        runs = {leg: [] for leg in LAUNCH_LEGS}
        for _ in range(args.repeats):
            for leg in LAUNCH_LEGS:                                        # the legs alternate
                fn = fns[leg]
                for i in range(args.warmup):
                    fn(*sets[i % SETS])
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                for _ in range(4):                                         # the device is busy while the host enqueues
                    torch.mm(spin, spin)
                a.record()
                for i in range(args.steps):
                    fn(*sets[i % SETS])
                b.record()
                torch.cuda.synchronize()
                runs[leg].append(round(a.elapsed_time(b) * 1e3 / args.steps, 2))
        line = json.dumps({"cell": cell, "dtype": name, "Lq": Lq, "B": B, "angle_mode": mode, "three_route": route,
                           "launch_us_per_call": runs, "calls": args.steps, "input_sets": SETS, "pid": os.getpid()})
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        del sets


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

        def staged(fn, value, ref, off, logits):
            return ba.BoxAttnBoxesStagedFunction.apply(value, shapes, lsi, ref, off, kidx, None, logits, mode)

        if args.launch:
            if lq is None:
                launch_cell(args, out, cell, B, mode, shapes, lsi, S, L, kidx, inputs)
            continue
        legs = {"points": points, "boxes": boxes, "value": value}
        if lq is None:                                     # one query a pixel: the window-staged Function
            legs["staged"] = staged
        if args.only and args.only not in legs:
            continue
        if args.only:
            legs = {args.only: legs[args.only]}
        for name, dtype, fn in (("f32", torch.float32, ba.BoxAttnFunction), ("bf16", torch.bfloat16, ba.BoxAttnBF16Function),
                                ("f16", torch.float16, ba.BoxAttnF16Function)):
            if args.dtype and args.dtype != name:
                continue
            sets = [inputs(dtype, seed) for seed in range(SETS)]
            assert ops.box_forward_boxes_ok(sets[0][0][0], L, Lq, P) and ops.box_backward_boxes_ok(sets[0][0][0], L, Lq, P)
            assert "value" not in legs or ops.box_backward_boxes_value_ok(sets[0][0][0], L, Lq, P)
            assert "staged" not in legs or (ops.box_forward_boxes_staged_ok(sets[0][0][0], shapes, lsi, Lq, P) and
                                            ops.box_backward_boxes_staged_ok(sets[0][0][0], shapes, lsi, Lq, P))
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
    rows, mem, kept, launch = {}, {}, {}, {}
    for path in paths:
        with open(path) as fh:
            for line in fh:
                if line.startswith("{"):
                    r = json.loads(line)
                    key = (r["cell"], r["B"], r["dtype"], r["Lq"])
                    for leg, runs in r.get("launch_us_per_call", {}).items():
                        launch.setdefault(key, {}).setdefault(leg, []).extend(runs)
                    for leg, runs in r.get("us_per_step", {}).items():
                        rows.setdefault(key, {}).setdefault(leg, []).extend(runs)
                    for leg, n in r.get("peak_bytes_over_start", {}).items():
                        mem.setdefault(key, {}).setdefault(leg, []).append(n)
                    for leg, n in r.get("saved_for_backward_bytes", {}).items():
                        kept.setdefault(key, {}).setdefault(leg, []).append(n)
    nan = [float("nan")]
    span = lambda v: "%.1f .. %.1f" % (min(v), max(v))
    if rows:
        print("| shape | B | type | Lq | " + " | ".join("%s, us a step (fastest .. slowest)" % leg for leg in LEGS) +
              " | slowest boxes / fastest points | slowest value / slowest boxes | slowest staged / fastest boxes | "
              "slowest staged / fastest points | peak MB over start, " + " | ".join(LEGS) +
              " | saved for backward MB, " + " | ".join(LEGS) + " |")
        print("|" + "---|" * (16 + len(LEGS)))
        for key in sorted(rows):
            p, b, v, s = (rows[key].get(leg, nan) for leg in LEGS)
            print("| %s | %d | %s | %d | %s | %s | %s | %s | %.2f | %.2f | %.2f | %.2f | %s | %s |" % (
                key[0], key[1], key[2], key[3], span(p), span(b), span(v), span(s), max(b) / min(p), max(v) / max(b),
                max(s) / min(b), max(s) / min(p),
                " | ".join("%.1f" % (max(mem[key].get(leg, nan)) / 1e6) for leg in LEGS),
                " | ".join("%.1f" % (max(kept[key].get(leg, nan)) / 1e6) for leg in LEGS)))
    if launch:
        print("| shape | B | type | three launches (point gradients + grid + softmax), us | row gather (bwd2_boxes_kernel), us "
              "| window-staged from boxes, us | slowest staged / fastest three | slowest staged / fastest gather | verdict |")
        print("|---|---|---|---|---|---|---|---|---|")
        for key in sorted(launch):
            t, g, s = (launch[key].get(leg, nan) for leg in LAUNCH_LEGS)
            print("| %s | %d | %s | %s | %s | %s | %.2f | %.2f | %s |" % (
                key[0], key[1], key[2], span(t), span(g), span(s), max(s) / min(t), max(s) / min(g),
                "wins" if max(s) < min(t) and max(s) < min(g) else "no win"))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=LEGS, help="one leg alone, once per cell (for a kernel trace)")
    ap.add_argument("--launch", action="store_true",
                    help="the device time of the parameter-gradient launch on the encoder cells, three ways")
    ap.add_argument("--dtype", choices=("f32", "bf16", "f16"), help="this storage type only")
    ap.add_argument("--cell", help="this shape only (e.g. 'C2 dec')")
    ap.add_argument("--batch", type=int, help="this batch size only")
    ap.add_argument("--out", help="append the JSON lines to this file")
    ap.add_argument("--table", nargs="+", help="print the table of these JSON-lines files")
    args = ap.parse_args()
    sys.exit(table(args.table) if args.table else measure(args))


if __name__ == "__main__":
    main()
