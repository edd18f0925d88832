"""What the mask model's inference forward costs: box attention with few queries and a k x k grid per level --
``InstanceAttention`` with ``inferencing`` set, the mask decoder's layers -- forward only, through
``ops.box_attn_forward``, on the C2' levels (100x167, 50x84, 25x42, 13x21), H = 8, C = 32, L = 4, for
Lq in {100, 300, 900}, P in {16, 36, 64, 196}, B in {1, 2}, float32 / bf16 / f16.

    python tools/inference_forward_step.py [--tree DIR] [--label NAME] [--wide-box V] [--calls K] [--warmup W]
                                           [--repeats R] [--out FILE]
    python tools/inference_forward_step.py --check NEW.jsonl --against PARENT.jsonl

Inputs are model-like decoder inputs: windows cx, cy ~ U(0.05, 0.95), w, h ~ U(0.05, 0.5), box
offsets N(0, 1), the grid through the module's own ``_where_to_attend``, spatial weights from
``InstanceWeightsFunction(need_level=False)`` on N(0, 1) logits.  Protocol (measuring guide): 8 input sets cycled,
W warm-up calls, then K calls between two HIP events on the op's stream; R repeats per configuration, all kept.
``--tree``: time another built checkout of the project (the parent commit) with this very script; ``--wide-box V``:
set option key 22 (this build only: 1 = the row-gather kernel, the parent's route).  Run the trees alternating, a
process each, several times; ``--check`` then prints the table of (type, P) cells: a cell keeps the wave-per-pair
route only if this build's SLOWEST repeat is below the parent's FASTEST at every (Lq, B) of the cell."""
import argparse
import json
import os
import sys

LEVELS = [(100, 167), (50, 84), (25, 42), (13, 21)]
H, C = 8, 32
LQS, POINTS, BATCHES = (100, 300, 900), (16, 36, 64, 196), (1, 2)
SETS = 8


def measure(args):
    root = os.path.abspath(args.tree or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, root)
    import torch
    import boxer_amd
    from boxer_amd import _lib, ops
    from boxer_amd.functions import InstanceWeightsFunction
    assert os.path.dirname(os.path.abspath(boxer_amd.__file__)) == os.path.join(root, "boxer_amd"), boxer_amd.__file__
    if args.wide_box is not None:
        _lib.set_option("wide_box", args.wide_box)
    dev = torch.device("cuda")
    shapes = torch.tensor(LEVELS, dtype=torch.long, device=dev)
    lsi = torch.cat((shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1]))
    S, L = int(shapes.prod(1).sum()), len(LEVELS)
    out = open(args.out, "a") if args.out else None

    modules = {}

    def inputs(B, Lq, P, dtype, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        k = int(round(P ** 0.5))
        m = modules.setdefault(k, boxer_amd.InstanceAttention(H * C, L, H, k).to(dev))
        ctr = 0.05 + 0.9 * torch.rand(B, Lq, 2, device=dev, generator=g)
        wh = 0.05 + 0.45 * torch.rand(B, Lq, 2, device=dev, generator=g)
        offsets = torch.randn(B, Lq, H, L, 4, device=dev, generator=g)
        m._box_offsets = lambda query, ref_windows, n_vars: offsets
        with torch.no_grad():
            loc = m._where_to_attend(ctr, None, torch.cat((ctr, wh), -1))
            logits = torch.randn(B, Lq, H, L, 2, 2, device=dev, generator=g)
            attn = InstanceWeightsFunction.apply(logits, k, False)[0]
        value = torch.randn(B, S, H, C, device=dev, generator=g).to(dtype)
        assert loc.shape == (B, Lq, H, L, P, 2) and attn.shape == (B, Lq, H, L, k, k)
        return value, loc.contiguous(), attn.contiguous()

    def timed(B, Lq, P, dtype):
        sets = [inputs(B, Lq, P, dtype, seed) for seed in range(SETS)]
        state = {"i": 0}

        def step():
            v, loc, attn = sets[state["i"] % SETS]
            state["i"] += 1
            return ops.box_attn_forward(v, shapes, lsi, loc, attn, 64)
        runs = []
        for _ in range(args.repeats):
            for _ in range(args.warmup):
                step()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(args.calls):
                step()
            b.record()
            torch.cuda.synchronize()
            runs.append(round(a.elapsed_time(b) * 1e3 / args.calls, 2))
        route = None
        if hasattr(ops, "forward_route"):
            route = _lib.FWD_FAMILIES[ops.forward_route(sets[0][0], sets[0][1], shapes, lsi)]
        return runs, route

    label = args.label or os.path.basename(root)
    for name, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16), ("f16", torch.float16)):
        for P in POINTS:
            for Lq in LQS:
                for B in BATCHES:
                    runs, route = timed(B, Lq, P, dtype)
                    line = json.dumps({"tree": label, "dtype": name, "P": P, "Lq": Lq, "B": B, "route": route,
                                       "us_per_call": runs, "calls": args.calls, "input_sets": SETS})
                    print(line, flush=True)
                    if out:
                        out.write(line + "\n")
                        out.flush()


def load(paths, tree=None):
    rows = {}
    for path in paths:
        with open(path) as fh:
            for line in fh:
                if line.startswith("{"):
                    r = json.loads(line)
                    if tree is None or r["tree"] == tree:
                        rows.setdefault((r["dtype"], r["P"], r["Lq"], r["B"]), []).extend(r["us_per_call"])
    return rows


def check(args):
    new, parent = load([args.check], args.new_label), load(args.against, args.parent_label)
    print("| type | P | Lq | B | parent, us (min .. max) | this build, us (min .. max) | |")
    print("|---|---|---|---|---|---|---|")
    cells = {}
    for key in sorted(new):
        base, runs = parent[key], new[key]
        ok = max(runs) < min(base)                 # the slowest repeat of this build below the parent's fastest
        cells.setdefault(key[:2], []).append(ok)
        print("| %s | %d | %d | %d | %.1f .. %.1f | %.1f .. %.1f | %s |" % (
            *key, min(base), max(base), min(runs), max(runs), "faster" if ok else "not faster"))
    print()
    for (dtype, P), oks in sorted(cells.items()):
        print("cell %s P=%d: %s (%d of %d shapes faster)" % (dtype, P, "wave per pair" if all(oks) else "row gather",
                                                            sum(oks), len(oks)))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tree", help="root of another built checkout to time instead of this one")
    ap.add_argument("--label", help="name of the tree in the output lines")
    ap.add_argument("--wide-box", type=int, help="value of option key 22 for the run")
    ap.add_argument("--out", help="append the JSON lines to this file")
    ap.add_argument("--check", help="JSON lines of this build: print the table of cells ...")
    ap.add_argument("--against", nargs="+", help="... against these JSON lines of the parent commit")
    ap.add_argument("--new-label", help="--check: only the lines of this tree label in the --check file")
    ap.add_argument("--parent-label", help="--check: only the lines of this tree label in the --against files")
    args = ap.parse_args()
    sys.exit(check(args) if args.check else measure(args))


if __name__ == "__main__":
    main()
