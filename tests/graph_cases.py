"""Steps captured in a HIP graph and replayed on new inputs: the two ways a step meets its capture (warmed up on the
stream it is captured on, or captured on a stream that has run nothing), loading another input set into the captured
tensors, the host tables of boxer_amd.ops whose entries must not come from a graph's private pool, the second input
sets of the from-boxes problems, and the driver every test of tests/test_gpu_graph_replay.py runs."""
import functools

import numpy as np
import torch

import boxes_cases
import error_bounds as eb

MODES = ("same_stream", "new_stream")
WARM_UP = 3


def capture(step, mode):
    """-> (graph, what ``step`` returned inside the capture: the outputs every replay overwrites).

    "same_stream": WARM_UP calls of ``step`` on a side stream, then the capture on THAT stream: whatever boxer_amd.ops
    keys by the stream handle (state buffer, workspace, parked plans, locality) is what the warm-up left.
    "new_stream": warm-up on the current stream, capture on a stream that has run nothing (bench.graph_step): everything
    keyed by the stream is created while the stream captures.
    No environment variable, no queue count: the graph runs under what the machine sets."""
    assert mode in MODES, mode
    current = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    if mode == "same_stream":
        side.wait_stream(current)
        with torch.cuda.stream(side):
            for _ in range(WARM_UP):
                step()
    else:
        for _ in range(WARM_UP):
            step()
    torch.cuda.synchronize()
    side.wait_stream(current)
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            kept = step()
    current.wait_stream(side)
    return graph, kept


def _pairs(static, new):
    if isinstance(static, dict):
        for k, t in static.items():
            if k in new:
                yield from _pairs(t, new[k])
    elif isinstance(static, (list, tuple)):
        assert len(static) == len(new), (len(static), len(new))
        for s, n in zip(static, new):
            yield from _pairs(s, n)
    elif isinstance(static, torch.Tensor):
        yield static, new


def load(static, new):
    """Copy the input set ``new`` into the captured tensors ``static`` (dictionaries, lists or tuples of tensors, the
    same keys and shapes; anything else in them is left alone): every tensor, the locations, weights, boxes, offsets
    and logits included.  The addresses stay."""
    with torch.no_grad():
        for s, n in _pairs(static, new):
            if s is not n:
                assert isinstance(n, torch.Tensor) and s.shape == n.shape, (tuple(s.shape), getattr(n, "shape", None))
                s.copy_(n)


def clone(inputs, leaves=()):
    """The captured tensors of an input set: every tensor cloned, those named in ``leaves`` requiring a gradient."""
    out = {}
    for k, t in inputs.items():
        if isinstance(t, torch.Tensor):
            t = t.detach().clone()
            if k in leaves:
                t.requires_grad_()
        out[k] = t
    return out


def tables_snapshot():
    """The key sets of the tables boxer_amd.ops keeps per stream and shape."""
    from boxer_amd import ops
    return {name: frozenset(getattr(ops, name)) for name in ("_STATE", "_WORKSPACE", "_PARKED", "_LOCALITY")}


def replay_on(mode, step, static, sets, order, check, after_capture=None, around_replay=None):
    """The pattern of every test: capture ``step`` (which reads ``static``) on ``sets[order[0]]``, replay on each set of
    ``order`` in turn with a synchronisation after each, and hand what the graph produced to ``check(index of the set,
    outputs, what)``.  ``around_replay(position in order, replay)`` runs the replay itself where a test reads counters
    around it.  "new_stream" adds the lifetime checks: the capture leaves the tables of boxer_amd.ops as the warm-up
    left them, and after the graph is gone and the cached buffers are dropped an eager step on the default stream still
    satisfies ``check``."""
    from boxer_amd import ops
    load(static, sets[order[0]])
    if mode == "new_stream":
        step()                                   # (the default stream's entries exist before the snapshot)
        torch.cuda.synchronize()
    before = tables_snapshot()
    graph, kept = capture(step, mode)
    if mode == "new_stream":
        assert tables_snapshot() == before, "the capture left an entry in a table of boxer_amd.ops: %r -> %r" % (
            before, tables_snapshot())
    if after_capture is not None:
        after_capture()

    def replay():
        graph.replay()
        torch.cuda.synchronize()
    for pos, i in enumerate(order):
        load(static, sets[i])
        if around_replay is not None:
            around_replay(pos, replay)
        else:
            replay()
        check(i, kept, "%s, replay %d on set %d" % (mode, pos, i))
        if after_capture is not None:
            after_capture()
    if mode == "new_stream":
        del graph, kept, replay
        ops.release_workspaces()
        last = min(1, len(sets) - 1)
        load(static, sets[last])
        out = step()
        torch.cuda.synchronize()
        check(last, out, "eager on the default stream after the graph is gone, set %d" % last)


# ------------------------------------------------------------------ the input sets of the per-point steps
ORDER_ABBCA = (0, 1, 1, 2, 0)


def onepass_sets(lq, dtype):
    """test_gpu_onepass.test_ranges_planned_by_other_data_are_redone on point_cases.LEVELS4: A samples the top-left corner
    of the maps, B the bottom-right corner (nearly every block with records outgrows the range A's counts planned), C
    the locations as they are."""
    import point_cases
    base = point_cases.make_onepass_case(point_cases.LEVELS4, lq, dtype=dtype, seed=5)
    return [dict(base, loc=(base["loc"] * 0.3).contiguous()), dict(base, loc=(base["loc"] * 0.3 + 0.65).contiguous()), base]


def instance_sets(shape, dtype, seeds):
    """point_cases.instance_problem of ``shape`` from each seed, as error_bounds.reference_of takes it ("f32" takes the
    bf16 numbers, as point_cases.shape_a_input)."""
    import point_cases
    from route_vocab import DTYPES
    sets = []
    for seed in seeds:
        g = point_cases.instance_problem(dtype=DTYPES["bf16" if dtype == "f32" else dtype], seed=seed, **shape)
        sets.append(dict(g, kind="instance", attn=g["spatial_w"]))
    return sets


# ------------------------------------------------------------------ the second input sets of the from-boxes problems
# Another seed of the same builder: like the first set it holds collapsed boxes and rows wholly outside the map (the
# builders place them).  (builder, its arguments) -> (what is added to the builder's seed, the share of sample points
# within EDGE_PX + slack of a bilinear cell edge that the float64 model finds for that seed, on the CPU; the cap is
# boxes_cases.EDGE_CAP).
SECOND_SEED = {
    ("box_boxes_problem", "model", 32, 0, 4, False, True): (3000017, 0.0),
    ("box_boxes_problem", "model", 32, 1, 5, False, True): (3000017, 0.0),
    ("box_boxes_problem", "encoder", 32, 0, 4, False, True): (3000017, 0.0),
    ("box_boxes_problem", "encoder", 32, 1, 5, False, True): (3000017, 0.0),
    ("staged_problem", "four_levels", "local", 1, 5, True, False): (3000017, 0.000515),
    ("staged_problem", "tiny_levels", "scattered", 0, 4, False, True): (3000017, 0.0),
    ("inst_boxes_problem", "five_levels", 32, 4, False, True): (3000017, 0.0),
    ("inst_boxes_problem", "five_levels", 32, 14, False, True): (3000017, 0.0),
}


def reseeded(builder, bump, *key):
    """``builder(*key)`` with ``bump`` added to the seed it makes from its arguments (past its cache)."""
    make = np.random.default_rng
    np.random.default_rng = lambda seed: make(seed + bump)
    try:
        return getattr(builder, "__wrapped__", builder)(*key)
    finally:
        np.random.default_rng = make


def second_problem(builder, *key):
    return reseeded(builder, SECOND_SEED[(builder.__name__,) + key][0], *key)


def second_upstream(shape, seed=101):
    """An upstream gradient every storage type holds exactly, from another seed than the first set's (100)."""
    return boxes_cases.every_type(np.random.default_rng(seed).standard_normal(shape))


def exact(g):
    """``g`` with a value every storage type holds exactly: one float64 model serves the three types."""
    return dict(g, value=boxes_cases.every_type(g["value"]))


def _box_set(g, gout):
    g = exact(g)
    return dict(g=g, gout=gout, ref=eb.boxes_reference(*boxes_cases.bwd_model_args(g), grad_out=gout),
                grad_value=boxes_cases.model_of(g, gout))


@functools.lru_cache(maxsize=None)
def box_sets(route, geometry, flavour, family=None):
    """The two input sets of a box step from boxes with their float64 models: ``route`` "gather" (the problems of
    boxes_cases.bwd_problem at C = 32) or "staged" (boxes_cases.staged_bwd_case of ``family``) -> [{g, gout, ref:
    boxes_reference's planes, grad_value: model_of's planes}, the same from the second seed]."""
    (angle_mode, ref_dim), per_head, with_vr = flavour
    if route == "gather":
        first = boxes_cases.bwd_problem(geometry, 32, flavour)
        builder, key = boxes_cases.box_boxes_problem, (geometry, 32, angle_mode, ref_dim, per_head, with_vr)
    else:
        builder, key = boxes_cases.staged_problem, (geometry, family, angle_mode, ref_dim, per_head, with_vr)
        first = boxes_cases.staged_bwd_case(*key)
    B, S, H, C, L, Lq, P = first["dims"]
    return [_box_set(first, boxes_cases.bwd_upstream(first)),
            _box_set(second_problem(builder, *key), second_upstream((B, Lq, H * C)))]


def inst_value_model(g, k, gout, gmask):
    """grad_value's planes of the instance step from boxes: boxes_cases.model_of with the two weight sets of
    error_bounds.instance_weights_reference (``gmask`` None: the mask output took no part, box flavour on the spatial
    weights)."""
    value = eb.f64(g["value"])
    B, S, H, C = value.shape
    loc, dloc = eb.grid_reference(g["ref"], g["off"], boxes_cases.kernel_offsets(k), g["vr"], 0)
    Lq, P = loc.shape[1], loc.shape[4]
    sw, lw, dsw, dlw = eb.instance_weights_reference(g["logits"], k, True)
    shapes, lsi = eb.f64(g["shapes"]).astype(np.int64), eb.f64(g["lsi"]).astype(np.int64)
    if gmask is None:
        r = eb._reference(value, shapes, lsi, loc, [sw], [eb.f64(gout).reshape(B, Lq, H, C)], False, slack=dloc, dws=[dsw])
    else:
        r = eb._reference(value, shapes, lsi, loc, [sw, lw],
                          [eb.f64(gout).reshape(B, Lq, H, C), eb.f64(gmask).reshape(B, Lq, P, H, C)], True, slack=dloc,
                          dws=[dsw, dlw])
    return r["grad_value"]


def _inst_set(g, k, gout, gmask):
    g = exact(g)
    ref = eb.boxes_reference("instance", g["value"], g["shapes"], g["lsi"], g["ref"], g["off"],
                             boxes_cases.kernel_offsets(k), g["vr"], g["logits"], 0, k, gout, gmask)
    return dict(g=g, gout=gout, gmask=gmask, ref=ref, grad_value=inst_value_model(g, k, gout, gmask))


@functools.lru_cache(maxsize=None)
def inst_sets(geometry, k, per_head, with_vr, with_mask):
    """The two input sets of the instance step from boxes (boxes_cases.inst_problem at C = 32) with their float64
    models; ``with_mask``: the mask output takes part in the loss."""
    key = (geometry, 32, k, per_head, with_vr)
    first = boxes_cases.inst_problem(*key)
    B, S, H, C, L, Lq = first["dims"]
    gout, gmask = boxes_cases.inst_upstream(first, k)
    gout2, gmask2 = second_upstream((B, Lq, H * C)), second_upstream((B, Lq, k * k, H * C), seed=102)
    return [_inst_set(first, k, gout, gmask if with_mask else None),
            _inst_set(second_problem(boxes_cases.inst_boxes_problem, *key), k, gout2, gmask2 if with_mask else None)]
