// The reference's compiled operator module, rebuilt on the C ABI of include/boxattn.h.
//
// BoxeR's Functions import a pybind11 module `e2edet.ops` with four functions
// (e2edet/module/ops/src/vision.cpp:7-12; signatures box_attn/box_attn.h:29-83,
// instance_attn/instance_attn.h:32-92).  This file is that module for MI355X: the same four
// names, argument lists and return values on at::Tensor, and nothing inside but argument checks
// (CHECK_INPUT of box_attn.cu:9-11,24-28; the batch / im2col_step assertion of box_attn.cu:42)
// and pointer marshalling into libboxattn_hip.so -- the stub a maintainer of the reference
// would compile instead of its src/ directory.  Host code only: no
// kernels here, built with the host compiler against torch's headers
// (`python setup.py build_ext --inplace`, or __graft_entry__.build()).
//
// float32 / float64 as in the reference; bfloat16 and float16 `value` (with float32 locations /
// weights) are the storage modes this library adds.  Each family of C entry points is called from
// ONE place: with_storage picks the struct of `value`'s storage type (element types, entry points),
// and the two sequences box and instance attention share -- forward, backward_ws -- take the
// call itself as a lambda.
#include <torch/extension.h>

#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/hip/HIPGraphsC10Utils.h>

#include <algorithm>
#include <cstdint>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <tuple>
#include <type_traits>
#include <vector>

#include "boxattn.h"

namespace e2edet {
namespace {

// One call: the tensors the shared sequences need (w1: instance attention's level weights, NULL for box attention),
// the dimensions, the device pointers of the two level tables and the stream.
struct Call {
    const at::Tensor &value, &shapes, &lsi, &loc, &w0;
    const at::Tensor *w1;
    int B, S, H, C, L, Lq, P;
    const int64_t *sh, *ls;
    void *stream;
};

void check_input(const at::Tensor &t, const char *name)
{
    TORCH_CHECK(t.is_cuda(), name, " must be a CUDA tensor: Not implemented on the CPU");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

bool is_h16(const at::Tensor &value)       // 16-bit storage
{
    return value.scalar_type() == at::kBFloat16 || value.scalar_type() == at::kHalf;
}

// The reference's CHECK_INPUT block plus the shape relations its kernels silently assume.
Call prepare(const at::Tensor &value, const at::Tensor &shapes, const at::Tensor &lsi, const at::Tensor &loc,
             const at::Tensor &w0, const at::Tensor *w1, int im2col_step)
{
    check_input(value, "value");
    check_input(shapes, "spatial_shapes");
    check_input(lsi, "level_start_index");
    check_input(loc, "sampling_loc");
    for (const at::Tensor *w : {&w0, w1})
        if (w) check_input(*w, "attn_weight");
    const auto vt = value.scalar_type();
    const bool h16 = is_h16(value);
    TORCH_CHECK(vt == at::kFloat || vt == at::kDouble || h16,
                "box_attn: unsupported dtype (float32, float64, bfloat16, float16)");
    TORCH_CHECK(shapes.scalar_type() == at::kLong && lsi.scalar_type() == at::kLong,
                "spatial_shapes / level_start_index must be int64");
    TORCH_CHECK(value.dim() == 4 && loc.dim() == 6 && loc.size(5) == 2,
                "expected value (B,S,H,C) and sampling_loc (B,Lq,H,L,P,2)");
    Call c = {value, shapes, lsi, loc, w0, w1};
    c.B = (int)value.size(0); c.S = (int)value.size(1); c.H = (int)value.size(2);
    c.C = (int)value.size(3); c.L = (int)shapes.size(0);
    c.Lq = (int)loc.size(1); c.P = (int)loc.size(4);
    TORCH_CHECK(loc.size(0) == c.B && loc.size(2) == c.H && loc.size(3) == c.L && lsi.numel() == c.L,
                "sampling_loc / spatial_shapes do not match value");
    const auto wt = h16 ? at::kFloat : vt;     // 16-bit storage: fp32 geometry
    TORCH_CHECK(loc.scalar_type() == wt, "sampling_loc must be ",
                h16 ? "float32 for bfloat16 / float16 value" : "of value's dtype");
    const int64_t n_w = (int64_t)c.B * c.Lq * c.H * c.L * c.P;
    for (const at::Tensor *w : {&w0, w1}) {
        if (!w) continue;
        TORCH_CHECK(w->numel() == n_w, "attention weights must have B*Lq*H*L*P elements");
        TORCH_CHECK(w->scalar_type() == wt, "attention weights must have sampling_loc's dtype");
    }
    const int64_t step = std::min<int64_t>(c.B, im2col_step);
    if (c.B > 0)
        TORCH_CHECK(step > 0 && c.B % step == 0, "batch(", c.B, ") must divide im2col_step(", step, ")");
    c.sh = shapes.data_ptr<int64_t>();
    c.ls = lsi.data_ptr<int64_t>();
    return c;
}

void check_rc(int rc, const char *what)
{
    TORCH_CHECK(rc == 0, what, " failed with hipError ", rc);
}

void *current_stream(const at::Tensor &t)
{
    return (void *)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.get_device()).stream();
}

// ---- what a training step must not pay for on every call (boxer_amd/ops.py keeps the same three things):
//  * host copies of the two level tables: one device -> host copy (a synchronisation) per TENSOR, not per call --
//    BoxeR hands the same two tensors to every layer of every step;
//  * the backward's scratch: one tensor per (device, stream), grown as needed (0.1-0.3 GB at BoxeR-R50 shapes);
//  * the plan: a forward whose inputs require a gradient runs the *_fwd_train_* entry and PARKS the plan; the
//    backward -- which the reference's Function calls with nothing but the saved tensors
//    (box_attention_func.py:24-64) -- finds it under (stream, dimensions, location / weight addresses + versions).
std::mutex g_mu;

struct TableEntry {
    c10::weak_intrusive_ptr<c10::TensorImpl> impl;     // the tensor object the copy was made of ...
    uint32_t version;                                  // ... and its version counter then
    std::shared_ptr<const std::vector<int64_t>> data;
};
std::map<const c10::TensorImpl *, TableEntry> g_tables;
constexpr size_t kTableCap = 64;

uint32_t version_of(const at::Tensor &t)
{
    return t.is_inference() ? 0u : (uint32_t)t._version();
}

// Host copy of a small int64 device table, cached on the tensor OBJECT: an address alone may be a new tensor's (the
// weak reference tells a live object from a recycled address), a version tells an in-place update.
std::shared_ptr<const std::vector<int64_t>> host_table(const at::Tensor &t)
{
    const c10::TensorImpl *key = t.unsafeGetTensorImpl();
    const uint32_t ver = version_of(t);
    {
        std::lock_guard<std::mutex> g(g_mu);
        const auto it = g_tables.find(key);
        if (it != g_tables.end()) {
            const auto alive = it->second.impl.lock();
            if (alive && alive.get() == key && it->second.version == ver) return it->second.data;
            g_tables.erase(it);
        }
    }
    const at::Tensor h = t.cpu().contiguous();         // (the one synchronising copy)
    auto data = std::make_shared<const std::vector<int64_t>>(h.data_ptr<int64_t>(), h.data_ptr<int64_t>() + h.numel());
    std::lock_guard<std::mutex> g(g_mu);
    if (g_tables.size() >= kTableCap) g_tables.clear();
    g_tables.erase(key);
    g_tables.emplace(key, TableEntry{c10::weak_intrusive_ptr<c10::TensorImpl>(t.getIntrusivePtr()), ver, data});
    return data;
}
struct HostTables {
    std::shared_ptr<const std::vector<int64_t>> shapes, lsi;
    explicit HostTables(const Call &c) : shapes(host_table(c.shapes)), lsi(host_table(c.lsi)) {}
    const int64_t *sh() const { return shapes->data(); }
    const int64_t *ls() const { return lsi->data(); }
};

typedef std::pair<int, void *> StreamKey;               // (device index, stream handle)
std::map<StreamKey, at::Tensor> g_workspace;
// (device, stream, B, S, H, C, L, Lq, P, storage type, hash of the level shapes): ABI 8 keeps the record ranges of the
// backward's one-pass fill in the state buffer -- one buffer per geometry
typedef std::tuple<int, void *, int, int, int, int, int, int, int, int, uint64_t> StateKey;
struct StateEntry { at::Tensor buf; bool fresh; };      // fresh: zeroed, not yet handed to the library (BOXATTN_HINT_FRESH_STATE)
std::map<StateKey, StateEntry> g_state;
constexpr size_t kStateCap = 1024;

// a tensor created while the stream captures a graph lives in the graph's private pool: it serves the call, but must
// not outlive the graph in a process-wide table (boxer_amd/ops.py has the same guard)
bool capturing()
{
    return c10::hip::currentStreamCaptureStatusMayInitCtx() != c10::hip::CaptureStatus::None;
}

// the backward's scratch of this stream (contents only live inside one call; calls on a stream never overlap)
at::Tensor workspace(const Call &c, const HostTables &h)
{
    const size_t bytes = std::max<size_t>(
        boxattn_bwd_workspace_bytes(is_h16(c.value), c.B, c.S, c.H, c.C, c.L, c.Lq, c.P, h.sh(), h.ls()), 256);
    const StreamKey key(c.value.get_device(), c.stream);
    const bool keep = !capturing();
    std::lock_guard<std::mutex> g(g_mu);
    const auto it = g_workspace.find(key);
    if (it != g_workspace.end() && (size_t)it->second.numel() >= bytes) return it->second;
    at::Tensor ws = at::empty({(int64_t)bytes}, c.value.options().dtype(at::kByte));
    if (keep) g_workspace[key] = ws;
    return ws;
}
// the library's state buffer of this (stream, geometry): zeroed once; every call leaves its tickets zero and the
// record ranges of the next backward's one-pass fill.  Adds the fresh-state bit to *hints -- the only hint this
// module ever gives.
at::Tensor state(const Call &c, const HostTables &h, int *hints)
{
    const size_t bytes = boxattn_state_bytes(c.B, c.S, c.H, c.C, c.L, c.Lq, c.P, h.sh(), h.ls());
    uint64_t geo = 1469598103934665603ull;
    for (int i = 0; i < 2 * c.L; ++i) geo = (geo ^ (uint64_t)h.sh()[i]) * 1099511628211ull;
    const StateKey key(c.value.get_device(), c.stream, c.B, c.S, c.H, c.C, c.L, c.Lq, c.P, (int)c.value.scalar_type(), geo);
    const bool keep = !capturing();
    std::lock_guard<std::mutex> g(g_mu);
    const auto it = g_state.find(key);
    if (it != g_state.end() && (size_t)it->second.buf.numel() >= bytes) {
        if (it->second.fresh) *hints |= BOXATTN_HINT_FRESH_STATE;
        it->second.fresh = false;
        return it->second.buf;
    }
    at::Tensor st = at::zeros({(int64_t)bytes}, c.value.options().dtype(at::kByte));
    *hints |= BOXATTN_HINT_FRESH_STATE;
    if (keep) {
        if (g_state.size() >= kStateCap) g_state.clear();
        g_state[key] = StateEntry{st, false};
    }
    return st;
}

// ---- parked plans
typedef std::tuple<int, void *, int, int, int, int, int, int, int, int, int, const void *, uint32_t, const void *, uint32_t,
                   const void *, uint32_t> PlanKey;
struct Parked {
    PlanKey key;
    at::Tensor plan;
    std::vector<at::Tensor> keep;      // the tensors the key names: held, so that their addresses stay theirs
};
std::deque<Parked> g_parked;
constexpr size_t kParkCap = 32;

PlanKey plan_key(const Call &c)
{
    // (the storage type is part of the key: at 16 / 64 channels per head a bfloat16 plan bins contiguous query ranges,
    // a float32 one interleaved ones)
    return PlanKey(c.value.get_device(), c.stream, c.B, c.S, c.H, c.C, c.L, c.Lq, c.P, boxattn_options_epoch(),
                   (int)c.value.scalar_type(), c.loc.data_ptr(), version_of(c.loc), c.w0.data_ptr(), version_of(c.w0),
                   c.w1 ? c.w1->data_ptr() : nullptr, c.w1 ? version_of(*c.w1) : 0u);
}
void park(PlanKey key, at::Tensor plan, std::vector<at::Tensor> keep)
{
    if (capturing()) return;       // (the plan tensor belongs to the graph's pool; the backward plans for itself)
    std::lock_guard<std::mutex> g(g_mu);
    for (auto it = g_parked.begin(); it != g_parked.end();)
        it = it->key == key ? g_parked.erase(it) : it + 1;
    while (g_parked.size() >= kParkCap) g_parked.pop_front();
    g_parked.push_back(Parked{key, std::move(plan), std::move(keep)});
}
at::Tensor take_parked(const PlanKey &key)
{
    std::lock_guard<std::mutex> g(g_mu);
    for (auto it = g_parked.begin(); it != g_parked.end(); ++it)
        if (it->key == key) {
            at::Tensor plan = it->plan;
            g_parked.erase(it);
            return plan;
        }
    return at::Tensor();
}

// ---- the storage type of `value`: e() / g() type the pointers of value-typed tensors (value, outputs, upstream
// gradients, grad_value) and of geometry-typed ones (locations, weights, their gradients); then that type's entry
// points.  float64 has the plain entries only -- no host tables, workspace, plan or state.
template <class E, class G> struct Storage {
    static constexpr bool plain_only = std::is_same<E, double>::value;
    static E *e(const at::Tensor &t) { return static_cast<E *>(t.data_ptr()); }
    static G *g(const at::Tensor &t) { return static_cast<G *>(t.data_ptr()); }
};
struct F64 : Storage<double, double> {
    static constexpr auto box_fwd = boxattn_fwd_f64, box_bwd = boxattn_bwd_f64;
    static constexpr auto inst_fwd = instattn_fwd_f64, inst_bwd = instattn_bwd_f64;
};
struct F32 : Storage<float, float> {
    static constexpr auto box_fwd_hl = boxattn_fwd_hl_f32, box_fwd_train = boxattn_fwd_train_f32;
    static constexpr auto inst_fwd = instattn_fwd_f32, inst_fwd_train = instattn_fwd_train_f32;
    static constexpr auto box_bwd_ws = boxattn_bwd_ws_f32, inst_bwd_ws = instattn_bwd_ws_f32;
};
struct BF16 : Storage<uint16_t, float> {
    static constexpr auto box_fwd_hl = boxattn_fwd_hl_bf16, box_fwd_train = boxattn_fwd_train_bf16;
    static constexpr auto inst_fwd = instattn_fwd_bf16, inst_fwd_train = instattn_fwd_train_bf16;
    static constexpr auto box_bwd_ws = boxattn_bwd_ws_bf16, inst_bwd_ws = instattn_bwd_ws_bf16;
};
struct F16 : Storage<uint16_t, float> {
    static constexpr auto box_fwd_hl = boxattn_fwd_hl_f16, box_fwd_train = boxattn_fwd_train_f16;
    static constexpr auto inst_fwd = instattn_fwd_f16, inst_fwd_train = instattn_fwd_train_f16;
    static constexpr auto box_bwd_ws = boxattn_bwd_ws_f16, inst_bwd_ws = instattn_bwd_ws_f16;
};
// call(one of the four structs above): the one place that looks at value's dtype (prepare admits no fifth)
template <class F> int with_storage(const at::Tensor &value, F call)
{
    switch (value.scalar_type()) {
    case at::kDouble: return call(F64());
    case at::kFloat: return call(F32());
    case at::kHalf: return call(F16());
    default: return call(BF16());
    }
}

// the arguments that *_fwd_train_* and *_bwd_ws_* take between the outputs and the stream, under the header's names
struct Extra {
    const int64_t *shapes_host, *lsi_host;
    void *workspace; size_t workspace_bytes;           // (backward)
    void *plan; size_t plan_bytes;
    void *state; size_t state_bytes;
    int hints, plan_built;                             // (plan_built: forward)
};

// The forward of both flavours but for float64.  If an input requires a gradient and the library plans for these
// dimensions: `train`, a *_fwd_train_* call with the plan buffer and the state buffer, whose plan is parked if one was
// built.  Else `plain`.  h: the caller's host tables, or NULL: fetched here, and only for the training forward.
template <class Train, class Plain> int forward(const Call &c, const HostTables *h, Train train, Plain plain)
{
    if (!c.value.requires_grad() && !c.loc.requires_grad() && !c.w0.requires_grad() && !(c.w1 && c.w1->requires_grad()))
        return plain();
    std::optional<HostTables> fetched;
    if (!h) h = &fetched.emplace(c);
    const size_t bytes = boxattn_plan_bytes(is_h16(c.value), c.B, c.S, c.H, c.C, c.L, c.Lq, c.P, h->sh(), h->ls());
    if (!bytes) return plain();
    at::Tensor plan = at::empty({(int64_t)bytes}, c.value.options().dtype(at::kByte));
    Extra x = {h->sh(), h->ls(), nullptr, 0, plan.data_ptr(), bytes};
    const at::Tensor state_buf = state(c, *h, &x.hints);
    x.state = state_buf.data_ptr(); x.state_bytes = (size_t)state_buf.numel();
    const int rc = train(x);          // a backward will follow: the forward's launch prepares its plan
    if (rc == 0 && x.plan_built)
        park(plan_key(c), plan, c.w1 ? std::vector<at::Tensor>{c.loc, c.w0, *c.w1} : std::vector<at::Tensor>{c.loc, c.w0});
    return rc;
}

// The backward of both flavours but for float64: `ws`, a *_bwd_ws_* call with the stream's workspace, the geometry's
// state buffer and the plan the forward parked, if it parked one.
template <class Ws> int backward_ws(const Call &c, Ws ws)
{
    const HostTables h(c);
    const at::Tensor scratch = workspace(c, h);
    Extra x = {h.sh(), h.ls(), scratch.data_ptr(), (size_t)scratch.numel()};
    const at::Tensor state_buf = state(c, h, &x.hints);
    x.state = state_buf.data_ptr(); x.state_bytes = (size_t)state_buf.numel();
    const at::Tensor plan = take_parked(plan_key(c));
    if (plan.defined()) { x.plan = plan.data_ptr(); x.plan_bytes = (size_t)plan.numel(); }
    return ws(x);
}

}  // namespace

// box_attn.h:29-54 -> output (B, Lq, H*C)
at::Tensor box_attn_forward(const at::Tensor &value, const at::Tensor &spatial_shapes,
                            const at::Tensor &level_start_index, const at::Tensor &sampling_loc,
                            const at::Tensor &attn_weight, const int im2col_step)
{
    Call c = prepare(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, nullptr, im2col_step);
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(value.device());
    at::Tensor out = at::empty({c.B, c.Lq, (int64_t)c.H * c.C}, value.options());
    c.stream = current_stream(value);
    check_rc(with_storage(value, [&](auto t) {
        if constexpr (decltype(t)::plain_only) {
            return t.box_fwd(t.e(value), c.sh, c.ls, t.g(sampling_loc), t.g(attn_weight), c.B, c.S, c.H, c.C, c.L, c.Lq,
                             c.P, t.e(out), c.stream);
        } else {
            const HostTables h(c);         // on every call: the _hl entry takes them too
            return forward(c, &h, [&](Extra &x) {
                return t.box_fwd_train(t.e(value), c.sh, c.ls, t.g(sampling_loc), t.g(attn_weight), c.B, c.S, c.H, c.C,
                                       c.L, c.Lq, c.P, t.e(out), x.shapes_host, x.lsi_host, x.plan, x.plan_bytes, x.state,
                                       x.state_bytes, x.hints, &x.plan_built, c.stream);
            }, [&]() {
                return t.box_fwd_hl(t.e(value), c.sh, c.ls, t.g(sampling_loc), t.g(attn_weight), c.B, c.S, c.H, c.C,
                                    c.L, c.Lq, c.P, t.e(out), h.sh(), h.ls(), c.stream);
            });
        }
    }), "boxattn_fwd");
    return out;
}

// box_attn.h:56-83 -> {grad_value, grad_sampling_loc, grad_attn_weight}
std::vector<at::Tensor> box_attn_backward(const at::Tensor &value, const at::Tensor &spatial_shapes,
                                          const at::Tensor &level_start_index, const at::Tensor &sampling_loc,
                                          const at::Tensor &attn_weight, const at::Tensor &grad_output,
                                          const int im2col_step)
{
    Call c = prepare(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, nullptr, im2col_step);
    check_input(grad_output, "grad_output");
    TORCH_CHECK(grad_output.scalar_type() == value.scalar_type(), "grad_output must have the dtype of value");
    TORCH_CHECK(grad_output.numel() == (int64_t)c.B * c.Lq * c.H * c.C, "grad_output must have B*Lq*H*C elements");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(value.device());
    // the library defines every output element: no zero-fill
    at::Tensor grad_value = at::empty_like(value);
    at::Tensor grad_loc = at::empty_like(sampling_loc);
    at::Tensor grad_attn = at::empty_like(attn_weight);
    c.stream = current_stream(value);
    check_rc(with_storage(value, [&](auto t) {
        if constexpr (decltype(t)::plain_only) {
            return t.box_bwd(t.e(value), c.sh, c.ls, t.g(sampling_loc), t.g(attn_weight), t.e(grad_output), c.B, c.S,
                             c.H, c.C, c.L, c.Lq, c.P, t.e(grad_value), t.g(grad_loc), t.g(grad_attn), c.stream);
        } else {
            return backward_ws(c, [&](const Extra &x) {
                return t.box_bwd_ws(t.e(value), c.sh, c.ls, t.g(sampling_loc), t.g(attn_weight), t.e(grad_output), c.B,
                                    c.S, c.H, c.C, c.L, c.Lq, c.P, t.e(grad_value), t.g(grad_loc), t.g(grad_attn),
                                    x.shapes_host, x.lsi_host, x.workspace, x.workspace_bytes, x.plan, x.plan_bytes,
                                    x.state, x.state_bytes, x.hints, c.stream);
            });
        }
    }), "boxattn_bwd");
    return {grad_value, grad_loc, grad_attn};
}

// instance_attn.h:32-59 -> {output (B,Lq,H*C), mask_output (B,Lq,P,H*C)}
std::vector<at::Tensor> instance_attn_forward(const at::Tensor &value, const at::Tensor &spatial_shapes,
                                              const at::Tensor &level_start_index, const at::Tensor &sampling_loc,
                                              const at::Tensor &spatial_attn_weight,
                                              const at::Tensor &level_attn_weight, const int im2col_step)
{
    Call c = prepare(value, spatial_shapes, level_start_index, sampling_loc, spatial_attn_weight, &level_attn_weight,
                     im2col_step);
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(value.device());
    at::Tensor out = at::empty({c.B, c.Lq, (int64_t)c.H * c.C}, value.options());
    at::Tensor mask = at::empty({c.B, c.Lq, c.P, (int64_t)c.H * c.C}, value.options());
    c.stream = current_stream(value);
    check_rc(with_storage(value, [&](auto t) {
        const auto plain = [&]() {         // (all four types; it takes no host tables)
            return t.inst_fwd(t.e(value), c.sh, c.ls, t.g(sampling_loc), t.g(spatial_attn_weight),
                              t.g(level_attn_weight), c.B, c.S, c.H, c.C, c.L, c.Lq, c.P, t.e(out), t.e(mask), c.stream);
        };
        if constexpr (decltype(t)::plain_only) {
            return plain();
        } else {
            return forward(c, nullptr, [&](Extra &x) {
                return t.inst_fwd_train(t.e(value), c.sh, c.ls, t.g(sampling_loc), t.g(spatial_attn_weight),
                                        t.g(level_attn_weight), c.B, c.S, c.H, c.C, c.L, c.Lq, c.P, t.e(out), t.e(mask),
                                        x.shapes_host, x.lsi_host, x.plan, x.plan_bytes, x.state, x.state_bytes, x.hints,
                                        &x.plan_built, c.stream);
            }, plain);
        }
    }), "instattn_fwd");
    return {out, mask};
}

// instance_attn.h:61-92 -> {grad_value, grad_sampling_loc, grad_spatial_attn_weight, grad_level_attn_weight}
std::vector<at::Tensor> instance_attn_backward(
    const at::Tensor &value, const at::Tensor &spatial_shapes, const at::Tensor &level_start_index,
    const at::Tensor &sampling_loc, const at::Tensor &spatial_attn_weight, const at::Tensor &level_attn_weight,
    const at::Tensor &grad_output, const at::Tensor &grad_mask_output, const int im2col_step)
{
    Call c = prepare(value, spatial_shapes, level_start_index, sampling_loc, spatial_attn_weight, &level_attn_weight,
                     im2col_step);
    check_input(grad_output, "grad_output");
    check_input(grad_mask_output, "grad_mask_output");
    TORCH_CHECK(grad_output.scalar_type() == value.scalar_type() && grad_mask_output.scalar_type() == value.scalar_type(),
                "grad_output / grad_mask_output must have the dtype of value");
    TORCH_CHECK(grad_output.numel() == (int64_t)c.B * c.Lq * c.H * c.C &&
                    grad_mask_output.numel() == (int64_t)c.B * c.Lq * c.P * c.H * c.C,
                "grad_output / grad_mask_output have the wrong number of elements");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(value.device());
    at::Tensor grad_value = at::empty_like(value);
    at::Tensor grad_loc = at::empty_like(sampling_loc);
    at::Tensor grad_sw = at::empty_like(spatial_attn_weight);
    at::Tensor grad_lw = at::empty_like(level_attn_weight);
    c.stream = current_stream(value);
    check_rc(with_storage(value, [&](auto t) {
        if constexpr (decltype(t)::plain_only) {
            return t.inst_bwd(t.e(value), c.sh, c.ls, t.g(sampling_loc), t.g(spatial_attn_weight), t.g(level_attn_weight),
                              t.e(grad_output), t.e(grad_mask_output), c.B, c.S, c.H, c.C, c.L, c.Lq, c.P,
                              t.e(grad_value), t.g(grad_loc), t.g(grad_sw), t.g(grad_lw), c.stream);
        } else {
            return backward_ws(c, [&](const Extra &x) {
                return t.inst_bwd_ws(t.e(value), c.sh, c.ls, t.g(sampling_loc), t.g(spatial_attn_weight),
                                     t.g(level_attn_weight), t.e(grad_output), t.e(grad_mask_output), c.B, c.S, c.H, c.C,
                                     c.L, c.Lq, c.P, t.e(grad_value), t.g(grad_loc), t.g(grad_sw), t.g(grad_lw),
                                     x.shapes_host, x.lsi_host, x.workspace, x.workspace_bytes, x.plan, x.plan_bytes,
                                     x.state, x.state_bytes, x.hints, c.stream);
            });
        }
    }), "instattn_bwd");
    return {grad_value, grad_loc, grad_sw, grad_lw};
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    m.def("box_attn_forward", &box_attn_forward, "box_attn_forward");
    m.def("box_attn_backward", &box_attn_backward, "box_attn_backward");
    m.def("instance_attn_forward", &instance_attn_forward, "instance_attn_forward");
    m.def("instance_attn_backward", &instance_attn_backward, "instance_attn_backward");
    m.def("abi_version", &boxattn_abi_version, "ABI version of the linked libboxattn_hip.so");
    m.def("parked_plans", []() { std::lock_guard<std::mutex> g(g_mu); return (int)g_parked.size(); },
          "plans parked by training forwards whose backward has not run yet");
    m.def("release_buffers", []() {
        std::lock_guard<std::mutex> g(g_mu);
        g_parked.clear(); g_workspace.clear(); g_state.clear(); g_tables.clear();
    }, "drop the cached scratch / state tensors, host tables and parked plans");
    m.attr("compiled_abi_version") = BOXATTN_ABI_VERSION;      // of the header this module was compiled against
}

}  // namespace e2edet
