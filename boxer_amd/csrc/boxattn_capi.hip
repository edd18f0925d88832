// C ABI of the box-attention operator (declared in include/boxattn.h): argument checks,
// kernel choice and launches.  No torch / ATen types anywhere in this library.
//
// Replaces the reference host code e2edet/module/ops/src/box_attn/box_attn.cu:15-135 and
// e2edet/module/ops/src/instance_attn/instance_attn.cu:15-157 (checks, output zero-fill,
// launch) and the launchers box_attn_kernel.cuh:1078-1123, 1126-1505.
#include "../../include/boxattn.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

#include "boxattn_binned.h"
#include "boxattn_boxes.h"
#include "boxattn_boxes_bwd.h"
#include "boxattn_gather2_boxes.h"
#include "boxattn_gather2_boxes_bwd.h"
#include "boxattn_fast.h"
#include "boxattn_gather2.h"
#include "boxattn_dense_plan.h"
#include "boxattn_generic.h"

using namespace boxattn;

namespace {

// 0 auto | 1 generic kernels only | 2 fast atomic kernels (error if the shape does not qualify,
// never the binned backward) | 3 binned backward required (error if not eligible)
std::atomic<int> g_variant{0};

// Tuning options (boxattn_set_option): process-wide knobs for A/B runs, relaxed atomics.  (The key numbers
// of rounds 1-3 are kept; the keys of the kernels that lost their A/B and were removed are gone.)
enum { kOptBinChunk = 10,     // records per work item of the accumulate kernels (0: from the number of sample points)
       kOptDense = 11,        // window-staged encoder kernels (forward + point gradients, bf16 and float32): 0 default (on),
                              // 1 off (row-gather kernels: the parity cross-check of the two kernel families), 2 on
       kOptRiders = 15,       // binning passes inside the point-gradient / accumulate (/ forward) launches: 0 default (on; one-pass
                              // fill where the map allows it, boxattn_spec.h; the combine inside the accumulate launch only
                              // for small problems), 1 off (launches of their own), 2 on except the combine (its own
                              // launch), 3 on, combine inside, 4 on with the two-pass binning of round 4 (count riders in the
                              // training forward, fill riders against the exact scan) instead of the one-pass fill
       kOptAccF32 = 19,       // float32 box attention, C = 32, accumulate: 0 default (bf16 matrix cores on exact three-term
                              // splits), 1 VALU list walk (4-byte records), 2 v_mfma_f32_32x32x2_f32
       kOptRideShift = 20,    // where the riders sit: (s_count + 1) | (s_fill + 1) << 4, a rider group every 2^s groups
                              // of 8 workgroups (s = 0: all in front); | v << 8: 64 v bin workgroups (riders) in all;
                              // 0: defaults
       kOptWideBox = 22,      // box attention with few (query, head) pairs and many points a pair (the mask model at
                              // inference): 0 default (the wave-per-pair kernel where it measured faster, wide_box_ok),
                              // 1 off (row-gather kernel: the parity cross-check of the two families), 2 on wherever
                              // the instance flavour takes the family
       kOptInstAcc16 = 23,    // 16-bit instance attention, C = 16 / 32 / 64, accumulate: 0 default (the matrix cores from
                              // kInstTrMinPoints points a slice), 1 VALU list walk (4-byte records: the parity cross-check),
                              // 2 the matrix cores (binned_accumulate_tr_kernel<ST, C, true>) wherever the shape is eligible
       kOptGroupRecords = 24, // 16-bit box attention, P == 4, matrix-core accumulate: the records of the binned backward.  0 default
                              // (group_default: the encoder shapes that passed the step rule),
                              // 1 point records {id, x, y, weight}, 2 group records (one int per (query, level, block))
                              // wherever the shape is eligible (record_kind)
       kNumOpts = 25 };
// (round 6 removed the keys whose non-default values had lost their A/B: 12 / 13 window margins, 17 staged forward off,
// 21 staged float32 kernels off -- 11 = 1 switches every window-staged kernel off)
std::atomic<int> g_opt[kNumOpts];      // 0 = default
inline int opt(int k) { return g_opt[k].load(std::memory_order_relaxed); }
inline bool opt_live(int k)
{
    return k == kOptBinChunk || k == kOptDense || k == kOptRiders || k == kOptAccF32 || k == kOptRideShift ||
           k == kOptWideBox || k == kOptInstAcc16 || k == kOptGroupRecords;
}
// (The riders' default place: count riders all in front of the forward kernel's grid -- measured: interleaving them with
// the tiles only stretches the count pass, riders and tiles want the same wave slots, profiles/r04_rider_sweep.log -- and
// fill riders in front of the point-gradient kernel's grid: shift 0 for both, ride_shift.)
constexpr int kBinWgTarget = 256;      // bin workgroups (= riders) in all, of 256 threads' worth: one per CU.  FEW, FAT riders
                                       // with the next step's locations always in flight cost a quarter of the chip's
                                       // wave slots; 1024 thin ones cost all of them for as long (C2 bf16 step
                                       // 146 / 139 / 135 / 154 us with 1024 / 512 / 256 / 128 riders)
constexpr int kSpecQPerRider = 600;    // ... of the one-pass fill (boxattn_spec.h) at encoder-sized problems: one rider per ~600
                                       // (query, slice) pairs, 256 ... 768 of them.  Its riders are bound by latency (two
                                       // barriers and an atomic round trip a step), not by instruction issue, so somewhat more,
                                       // shorter riders than the two-pass fill wants.  C2 bf16 (213 k pairs), one box, resident /
                                       // cache-cold inputs, us a step: 256 riders 126.3 / 140.2, 384: 122.5 / 132.9, 512: 119.8 /
                                       // 135.0, 768: 119.3 / 135.0, 1024: 122.8 / 136.2 (two-pass, 256: 124.0 / 133.2); C2' (354 k):
                                       // 512: 209.8 / 219.4, 1024: 218.5 / 225.1 (two-pass: 211.3 / 221.5) -- profiles/r06_onepass_ab.log
// one_pass: the shape's box-attention backward fills its bins in one pass (a property of the map, plan_layout)
inline long long bin_wg_target(bool one_pass, long long queries)
{
    const int v = (opt(kOptRideShift) >> 8) & 31;       // 64 v riders
    if (v > 0) return 64ll * v;
    if (!one_pass || queries < 65536) return kBinWgTarget;
    const long long r = (queries / kSpecQPerRider + 32) / 64 * 64;
    return std::min(768ll, std::max(256ll, r));
}
inline unsigned ride_shift(bool fill)
{
    const int o = opt(kOptRideShift), v = fill ? (o >> 4) & 15 : o & 15;
    return v > 0 ? (unsigned)(v - 1) : 0u;
}

inline int ceil_div_sz(size_t a, size_t b) { return (int)((a + b - 1) / b); }

// zero-fill on the stream (zero_fill_kernel, see there why not hipMemsetAsync)
inline hipError_t zero_async(void *p, size_t bytes, hipStream_t st)
{
    if (!bytes) return hipSuccess;
    const int blocks = (int)std::min<size_t>((bytes / 16 + 255) / 256 + 1, 2048);
    hipLaunchKernelGGL(zero_fill_kernel, dim3(blocks), dim3(256), 0, st, (unsigned char *)p, bytes,
                       (int)(bytes >= ((size_t)8 << 20)));
    return hipGetLastError();
}

inline bool aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

struct Dims {
    int B, S, H, C, L, Lq, P;
    bool valid() const
    {
        return B >= 0 && S >= 0 && H > 0 && C > 0 && L > 0 && Lq >= 0 && P > 0;
    }
    size_t n_qh() const { return (size_t)B * Lq * H; }
    size_t n_value() const { return (size_t)B * S * H * C; }
    bool empty() const { return n_qh() == 0; }
};

// Which G (lanes per (query, head)) the fast kernels are instantiated for, VEC = 4.
inline int fast_group(const Dims &d)
{
    if (d.C % 4 != 0 || d.L > kMaxLevels) return 0;
    const int g = d.C / 4;
    return (g == 4 || g == 8 || g == 16) ? g : 0;
}

// Calls f(std::integral_constant<int, G>{}) for the group size g the fast kernels are instantiated for (4, 8 or
// 16: what fast_group returns when it does not return 0); any other g: nothing is called.
template <typename F> inline void for_group(int g, F &&f)
{
    switch (g) {
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    }
}

template <typename ST>
bool fast_ok(const Dims &d, const void *value, const void *loc, const void *a, const void *b,
             const void *c)
{
    if (g_variant == 1) return false;
    if (fast_group(d) == 0) return false;
    const size_t va = 4 * sizeof(ST);
    return aligned(value, va) && aligned(loc, 8) && aligned(a, va) && aligned(b, va) &&
           aligned(c, va);
}
// What the forward's choice of kernel sees of its tensors' addresses.  fast: fast_ok's alignments (value and the
// outputs to 4 elements, loc to 8 bytes); rows16: value and the outputs to 16 bytes (8 channels a lane); staged:
// what the window-staged kernels ask (value, out to 16 bytes, loc to 8)
struct FwdAlign { bool fast, rows16, staged; };

// Lanes per (query, head) pair and channels per lane of the gather kernels (boxattn_gather2.h):
// 8 channels per lane when C allows and the rows can be fetched 16 bytes at a time.
constexpr int kGatherVecF32 = 4;    // measured: 128-byte fp32 rows gain nothing from 8 channels per lane
constexpr int kGatherVecBf16 = 8;
constexpr int kGatherU8F32 = 2, kGatherU8Bf16 = 4;      // points in flight of the 8-channel kernels
constexpr int kGatherU4F32 = 4, kGatherU4Bf16 = 4;      // ... of the 4-channel kernels
struct GatherCfg { int G, VEC; };
inline GatherCfg gather_cfg(int elem_bytes, const Dims &d, bool rows_16b_aligned)
{
    const int want = elem_bytes == 2 ? kGatherVecBf16 : kGatherVecF32;
    if (want == 8 && rows_16b_aligned && (d.C == 32 || d.C == 64)) return {d.C / 8, 8};
    return {fast_group(d), 4};
}
template <typename ST> inline GatherCfg gather_cfg(const Dims &d, bool rows_16b_aligned)
{
    return gather_cfg((int)sizeof(ST), d, rows_16b_aligned);
}
// points of a pair in flight per lane (loads issued before the first use)
template <typename ST, int G, int VEC> struct GatherUnroll {
    static constexpr int u8 = sizeof(ST) == 2 ? kGatherU8Bf16 : kGatherU8F32;
    static constexpr int u4 = sizeof(ST) == 2 ? kGatherU4Bf16 : kGatherU4F32;
    static constexpr int want = VEC == 8 ? u8 : u4;
    static constexpr int value = want > G ? G : want;
};
inline unsigned div_magic(unsigned d) { return d <= 1 ? 0xFFFFFFFFu : (unsigned)((1ull << 32) / d); }
// index constants of the gather kernels; false if the problem is outside their 32-bit arithmetic
inline bool gather_idx(const Dims &d, GatherIdx &ix, size_t elem_bytes)
{
    const size_t n_qh = d.n_qh();
    if (n_qh >= (1ull << 31) || (size_t)d.B * d.S >= (1ull << 31)) return false;
    ix.n_qh = (unsigned)n_qh;
    ix.magic_h = div_magic((unsigned)d.H);
    ix.magic_lq = div_magic((unsigned)d.Lq);
    ix.rcp_p = 1.0f / (float)d.P;
    // Head-per-XCD placement (pair_of_lane): measured +3..20 % when the queries sample far apart
    // (decoder queries with big boxes, random locations) and -2..7 % for the encoder's local
    // windows, where the contiguous query chunks already keep an XCD's rows together.  So: only
    // for decoder-like shapes (few queries against the map) whose per-head rows fit an XCD's L2.
    ix.head_xcd = (d.H == 8 && (long long)d.Lq * 4 <= d.S &&
                   (size_t)d.B * d.S * d.C * elem_bytes <= (3u << 20))
                      ? 1u : 0u;
    return true;
}
// workgroups (4 waves of `pairs` pairs) of a gather kernel
inline int gather_blocks(const Dims &d, const GatherIdx &ix, int pairs)
{
    if (ix.head_xcd) return 8 * ceil_div_sz((size_t)d.B * d.Lq, (size_t)pairs * 4);
    return ceil_div_sz(d.n_qh(), (size_t)pairs * 4);
}
// the launch geometry as explicit kernel arguments (GatherIdx: grid_x, grid_y, tps)
inline GatherIdx with_grid(GatherIdx ix, int grid_x, int grid_y, int tiles)
{
    ix.grid_x = (unsigned)grid_x;
    ix.grid_y = (unsigned)std::max(1, grid_y);
    ix.tps = (unsigned)((tiles + (int)ix.grid_y - 1) / (int)ix.grid_y);
    return ix;
}
// (the 8-channel kernels are only instantiated for the storage types that select them)
template <typename ST> struct GatherVec8 {
    static constexpr bool value = (sizeof(ST) == 2 ? kGatherVecBf16 : kGatherVecF32) == 8;
};
#define BOXATTN_GATHER_DISPATCH(cfg, X)                                                       \
    do {                                                                                      \
        if ((cfg).VEC == 8) {                                                                 \
            if constexpr (GatherVec8<ST>::value) {                                            \
                if ((cfg).G == 4) { X(4, 8) } else { X(8, 8) }                                \
            }                                                                                 \
        } else if ((cfg).G == 4) { X(4, 4) } else if ((cfg).G == 8) { X(8, 4) } else { X(16, 4) } \
    } while (0)

// Over how many workgroup rows (grid.y) the point tiles of a (query, head) pair are spread in the
// point-gradient kernel: aim at ~4096 workgroups when the query dimension alone gives fewer than 1024.
inline int point_split(int blocks, int tiles)
{
    if (blocks >= 1024 || tiles < 2) return 1;
    return std::max(1, std::min(tiles, (4096 + blocks - 1) / blocks));
}

inline int finish()
{
    return (int)hipGetLastError();
}

// ---- optional kernel timing (boxattn_profile_begin/_end) -------------------------------
struct EventPair { hipEvent_t a, b; };
enum { kSlotFwd = 0, kSlotBwdPoints = 1, kSlotBwdAccum = 2, kSlotBwdBin = 3, kSlotBwdCombine = 4,
       kSlotBwdPrep = 5, kNumSlots = BOXATTN_PROFILE_SLOTS };
struct Profile {
    std::atomic<bool> on{false};
    std::mutex mu;                          // forward and backward run on different host threads
    std::vector<EventPair> ev[kNumSlots];
} g_prof;
constexpr size_t kMaxProfiled = 4096;

struct ScopedKernelTimer {            // brackets one kernel launch when profiling is on
    hipStream_t st;
    EventPair ev{};
    std::vector<EventPair> *dst = nullptr;
    ScopedKernelTimer(std::vector<EventPair> &v, hipStream_t s) : st(s)
    {
        if (!g_prof.on.load(std::memory_order_relaxed)) return;
        if (hipEventCreate(&ev.a) != hipSuccess) return;
        if (hipEventCreate(&ev.b) != hipSuccess) { (void)hipEventDestroy(ev.a); return; }
        dst = &v;
        (void)hipEventRecord(ev.a, st);
    }
    ~ScopedKernelTimer()
    {
        if (!dst) return;
        (void)hipEventRecord(ev.b, st);
        std::lock_guard<std::mutex> g(g_prof.mu);
        if (dst->size() < kMaxProfiled) dst->push_back(ev);
        else { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
    }
};

inline void drain(std::vector<EventPair> &v, double *ms_sum, int *n)
{
    double sum = 0;
    int cnt = 0;
    for (auto &e : v) {
        float ms = 0;
        if (hipEventSynchronize(e.b) == hipSuccess &&
            hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
            sum += ms;
            ++cnt;
        }
        (void)hipEventDestroy(e.a);
        (void)hipEventDestroy(e.b);
    }
    v.clear();
    if (ms_sum) *ms_sum = sum;
    if (n) *n = cnt;
}


// rider workgroups of a launch: the caller sets ride.grid.n_riders / .shift, the rest follows from the grid
inline BinRide place_riders(const BinRide *ride_in, unsigned own_blocks, unsigned *total)
{
    BinRide ride = ride_in ? *ride_in : BinRide{};
    ride.grid = ride_grid(ride.grid.n_riders, own_blocks, ride.grid.shift, total);
    return ride;
}

// ------------------------------------------------------------------------------ forward
inline bool make_dense_plan(const Dims &d, const int64_t *sh, const int64_t *ls, DensePlan &p, int elem);

// A forward call's operands and its outputs, filled by the extern "C" wrappers (T: float; double for float64 storage).
// w_lv / mask: instance attention only; shapes_host / lsi_host: the host copies of the level tables (NULL in the entry
// points that take none).
template <typename ST> struct FwdIn {
    typedef typename Storage<ST>::compute T;
    const ST *value;
    const int64_t *shapes, *lsi;
    const T *loc, *w_sp, *w_lv;
    Dims d;
    const int64_t *shapes_host, *lsi_host;
    hipStream_t st;
};
template <typename ST> struct FwdOut { ST *out, *mask; };
// What only the training forward passes.  count_ride: the backward's count pass + scans to run as rider workgroups
// of the forward kernel; *ride_taken says whether the kernel that was launched carried them
struct FwdExtras {
    const BinRide *count_ride = nullptr;
    bool *ride_taken = nullptr;
    bool allow_dense = true;
    unsigned long long *stats = nullptr;
};
// The forward's kernel families (BOXATTN_FWD_*), and the ONE function that chooses among them: launch_fwd launches
// what it answers, boxattn_fwd_route reports it.
enum { kFwdGeneric = BOXATTN_FWD_GENERIC, kFwdFast = BOXATTN_FWD_FAST, kFwdGather = BOXATTN_FWD_GATHER,
       kFwdWide = BOXATTN_FWD_WIDE, kFwdStaged = BOXATTN_FWD_STAGED };
struct FwdRoute {
    GatherCfg cfg{0, 4};
    GatherIdx ix{};
    int blocks = 0;              // first generation / row gather: workgroups of 4 waves of 64 / G pairs
    int wblocks = 0;             // wave per pair: workgroups, of 4 / ws pairs
    unsigned ws = 1;             //                waves that share a pair
};
// Box attention on the wave-per-pair kernel (the instance flavour takes it from 64 / G points up): by default where
// it measured faster than the row-gather kernel's walk of one lane group over the pair's points at every query count
// and batch of the table (profiles/inference_forward_step.log) -- 16-bit storage from 64 points a level,
// float32 from 196.  Below that it wins at few pairs and ties or loses at 14 400 of them.
inline bool wide_box_ok(int elem_bytes, const Dims &d)
{
    const int o = opt(kOptWideBox);
    if (o == 1 || o == 2) return o == 2;
    return d.P >= (elem_bytes == 2 ? 64 : 196);
}
// -> family, or < 0: no kernel for these dimensions under the current switches (variant 2 and not eligible).
// r: the launch geometry of the gather families; dp: the plan of the window-staged one
inline int fwd_route(int elem_bytes, bool inst, const Dims &d, const FwdAlign &al, const int64_t *shapes_host,
                     const int64_t *lsi_host, bool allow_dense, FwdRoute &r, DensePlan &dp)
{
    r = FwdRoute{};
    if (elem_bytes == 8) return kFwdGeneric;                    // float64: the generic kernels, whatever the variant
    if (g_variant == 1 || fast_group(d) == 0 || !al.fast) return g_variant == 2 ? -1 : kFwdGeneric;
    // encoder case: window-staged forward
    if (!inst && allow_dense && shapes_host && lsi_host && al.staged &&
        make_dense_plan(d, shapes_host, lsi_host, dp, elem_bytes))
        return kFwdStaged;
    const size_t n_qh = d.n_qh(), vbytes = d.n_value() * (size_t)elem_bytes;
    const bool gen2 = g_variant != 2 && vbytes < kOobOffset && gather_idx(d, r.ix, (size_t)elem_bytes);   // buffer-load kernels
    r.cfg = gen2 ? gather_cfg(elem_bytes, d, al.rows16) : GatherCfg{fast_group(d), 4};
    const int pairs = kWave / r.cfg.G;
    r.blocks = gen2 ? gather_blocks(d, r.ix, pairs) : ceil_div_sz(n_qh, (size_t)pairs * 4);
    if (!gen2) return kFwdFast;
    // few (query, head) pairs and many points (the mask decoder): one wave per pair
    if (r.blocks < 1024 && d.P >= pairs) {
        // 8 or more point steps a pair: its points over the four waves of a workgroup
        const int steps = ceil_div_sz((size_t)d.P, (size_t)pairs);
        if (inst || wide_box_ok(elem_bytes, d)) {
            r.ws = steps >= 8 ? 4 : steps >= 4 ? 2 : 1;
            const size_t ppw = 4 / r.ws;
            r.wblocks = r.ix.head_xcd ? 8 * ceil_div_sz((size_t)d.B * d.Lq, ppw) : ceil_div_sz(n_qh, ppw);
            return kFwdWide;
        }
    }
    return kFwdGather;
}

template <typename ST, bool INST>
int launch_fwd(const FwdIn<ST> &in, const FwdOut<ST> &o, const FwdExtras &x)
{
    const Dims &d = in.d;
    const hipStream_t st = in.st;
    const BinRide *const count_ride = x.count_ride;
    bool *const ride_taken = x.ride_taken;
    if (ride_taken) *ride_taken = false;
    if (!d.valid()) return (int)hipErrorInvalidValue;
    if (d.empty()) return 0;                                   // no queries: nothing to write
    if (!in.shapes || !in.lsi || !in.loc || !in.w_sp || !o.out || (INST && (!in.w_lv || !o.mask)))
        return (int)hipErrorInvalidValue;
    const size_t n_qh = d.n_qh();
    if (d.n_value() == 0) {                                    // no pixels: every sample is 0
        hipError_t e = zero_async(o.out, n_qh * d.C * sizeof(ST), st);
        if (e == hipSuccess && INST)
            e = zero_async(o.mask, n_qh * d.C * d.P * sizeof(ST), st);
        return (int)e;
    }
    if (!in.value) return (int)hipErrorInvalidValue;
    const size_t va = 4 * sizeof(ST);
    FwdAlign al;
    al.fast = aligned(in.value, va) && aligned(in.loc, 8) && aligned(o.out, va) && (!INST || aligned(o.mask, va));
    al.rows16 = aligned(in.value, 16) && aligned(o.out, 16) && (!INST || aligned(o.mask, 16));
    al.staged = aligned(in.value, 16) && aligned(o.out, 16) && aligned(in.loc, 8);
    FwdRoute r;
    DensePlan dp;
    const int family = fwd_route((int)sizeof(ST), INST, d, al, in.shapes_host, in.lsi_host, x.allow_dense, r, dp);
    if (family < 0) return (int)hipErrorInvalidValue;
    if constexpr (!std::is_same<ST, double>::value) {
        if (family != kFwdGeneric) {
            ScopedKernelTimer timer(g_prof.ev[kSlotFwd], st);
            const size_t vbytes = d.n_value() * sizeof(ST);
            const GatherCfg cfg = r.cfg;
            const GatherIdx &ix = r.ix;
            if constexpr (!INST) {     // encoder case: window-staged forward (16-bit: matrix cores; float32: VALU)
                if (family == kFwdStaged) {
                    const BinRide ride = count_ride ? *count_ride : BinRide{};
                    if constexpr (IsHalf16<ST>::value)
                        launch_fwd_dense<ST>(in.value, in.loc, in.w_sp, o.out, dp, (unsigned)vbytes, ride, x.stats, st);
                    else launch_fwd_dense_f32(in.value, in.loc, in.w_sp, o.out, dp, (unsigned)vbytes, ride, x.stats, st);
                    if (count_ride && ride_taken) *ride_taken = true;
                    return finish();
                }
            }
            if (family == kFwdWide) {
                // few (query, head) pairs and many points (the mask decoder): one wave per pair, the points spread
                // over the lane groups (any storage type, no atomics); `ws` waves of a workgroup share a pair
                unsigned total = 0;
                const BinRide ride = place_riders(count_ride, (unsigned)r.wblocks, &total);
                const unsigned ws = r.ws;
                if constexpr (INST) {
#define BOXATTN_LAUNCH_WIDE(GG, VV)                                                           \
    hipLaunchKernelGGL((fwd_wide_kernel<ST, GG, VV, true>), dim3(total), dim3(256), 0, st,    \
                       in.value, in.shapes, in.lsi, in.loc, in.w_sp, in.w_lv, d.S, d.H, d.L,  \
                       d.Lq, d.P, o.out, o.mask, with_grid(ix, r.wblocks, 1, 1),              \
                       (unsigned)vbytes, ride, ws);
                    BOXATTN_GATHER_DISPATCH(cfg, BOXATTN_LAUNCH_WIDE);
#undef BOXATTN_LAUNCH_WIDE
                } else {
#define BOXATTN_LAUNCH_WIDE(GG, VV)                                                           \
    hipLaunchKernelGGL((fwd_wide_kernel<ST, GG, VV, false>), dim3(total), dim3(256), 0, st,   \
                       in.value, in.shapes, in.lsi, in.loc, in.w_sp, NoArg{}, d.S, d.H, d.L,  \
                       d.Lq, d.P, o.out, NoArg{}, with_grid(ix, r.wblocks, 1, 1),             \
                       (unsigned)vbytes, ride, ws);
                    BOXATTN_GATHER_DISPATCH(cfg, BOXATTN_LAUNCH_WIDE);
#undef BOXATTN_LAUNCH_WIDE
                }
                if (count_ride && ride_taken) *ride_taken = true;
                return finish();
            }
            const int blocks = r.blocks;
            if (family == kFwdGather) {
                unsigned total = 0;
                const BinRide ride = place_riders(count_ride, (unsigned)blocks, &total);
#define BOXATTN_FWD2(GG, VV)                                                                  \
    hipLaunchKernelGGL((fwd2_kernel<ST, GG, INST, GatherUnroll<ST, GG, VV>::value, VV>),      \
                       dim3(total, 1), dim3(256), 0, st, in.value, in.shapes, in.lsi, in.loc, \
                       in.w_sp, in.w_lv, d.S, d.H, d.L, d.Lq, d.P, o.out, o.mask,             \
                       with_grid(ix, blocks, 1, (d.P + GG - 1) / GG), (unsigned)vbytes, ride);
                BOXATTN_GATHER_DISPATCH(cfg, BOXATTN_FWD2);
#undef BOXATTN_FWD2
                if (count_ride && ride_taken) *ride_taken = true;
            } else {
                for_group(cfg.G, [&](auto g) {
                    hipLaunchKernelGGL((fwd_fast_kernel<ST, 4, decltype(g)::value, INST>), dim3(blocks), dim3(256), 0, st,
                                       in.value, in.shapes, in.lsi, in.loc, in.w_sp, in.w_lv, d.S, d.H, d.L, d.Lq, d.P,
                                       o.out, o.mask, n_qh);
                });
            }
            return finish();
        }
    }
    const size_t n = n_qh * d.C;
    const int blocks = (int)std::min<size_t>((n + 255) / 256, (size_t)1 << 20);
    ScopedKernelTimer timer(g_prof.ev[kSlotFwd], st);
    hipLaunchKernelGGL((fwd_generic_kernel<ST, INST>), dim3(blocks), dim3(256), 0, st, in.value,
                       in.shapes, in.lsi, in.loc, in.w_sp, in.w_lv, d.S, d.H, d.C, d.L, d.Lq, d.P, o.out, o.mask,
                       n);
    return finish();
}

// ---- attention from boxes and logits: the four routes and the host path they share --------------------------
// instance flavour (k x k points a level, 2x2 logits): fwd_wide_boxes_kernel (boxattn_boxes.h) and
// pointgrad_boxes_kernel (boxattn_boxes_bwd.h); box flavour (P points a level, L P logits): fwd2_boxes_kernel
// (boxattn_gather2_boxes.h) and bwd2_boxes_kernel (boxattn_gather2_boxes_bwd.h); the box flavour's window-staged
// forward with the host tables: fwd_dense_boxes_kernel / fwd_dense_f32_boxes_kernel (boxattn_dense_fwd.h,
// boxattn_dense_f32.h).  No other kernel behind these entries.

// What the eligibility queries know of the tensors' addresses.  aligned: 0 nothing beyond the elements' own alignment,
// 8 every tensor to 8 bytes, else to 16 bytes (staged: left false, boxattn_fwd_route sets it)
inline FwdAlign align_from_bytes(int elem_bytes, int aligned)
{
    const int bytes = aligned == 0 ? elem_bytes : aligned == 8 ? 8 : 16;
    return FwdAlign{bytes >= 4 * elem_bytes && bytes >= 8, bytes >= 16, false};
}

// Whether the instance kernels run these dimensions (P = k * k points a level): where the instance flavour of
// fwd_route takes the wave-per-pair family, for the k and L of the weight kernels (k even, 2 ... 32; L <= 16: the
// 4 L cells of a pair fit the lanes of a wave).  The ONE function behind instattn_{fwd,bwd}_boxes_ok and the entry
// points; r: the launch geometry.  Option key 22 is not read (the instance flavour does not read it).
inline bool boxes_route(int elem_bytes, const Dims &d, int k, const FwdAlign &al, FwdRoute &r)
{
    if ((elem_bytes != 2 && elem_bytes != 4) || !d.valid()) return false;
    if (k < 2 || k > 32 || k % 2 != 0 || d.P != k * k || d.L > 16) return false;
    DensePlan dp;
    return fwd_route(elem_bytes, true, d, al, nullptr, nullptr, false, r, dp) == kFwdWide;
}

// Whether the box kernels run these dimensions: where the box flavour of fwd_route, without host tables, takes the
// row gather, for the L of the level table and the L P of the softmax kernels (the pair's logits fit 64 / G rounds of
// a lane group).  The ONE function behind boxattn_{fwd,bwd}_boxes_ok and the entry points; r: the launch geometry.
inline bool box_boxes_route(int elem_bytes, const Dims &d, const FwdAlign &al, FwdRoute &r)
{
    if ((elem_bytes != 2 && elem_bytes != 4) || !d.valid()) return false;
    if (d.L > 16 || (long long)d.L * d.P > kBoxesMaxLP) return false;
    DensePlan dp;
    return fwd_route(elem_bytes, false, d, al, nullptr, nullptr, false, r, dp) == kFwdGather;
}

// Whether the window-staged forward from boxes runs these dimensions: where the box flavour of fwd_route WITH these
// host tables takes the window-staged family (make_dense_plan's conditions and switches; the tensors' alignment to 16
// bytes).  The ONE function behind boxattn_fwd_boxes_hl_ok and the boxattn_fwd_boxes_hl_* entry points; dp: the plan.
inline bool box_boxes_staged_route(int elem_bytes, const Dims &d, FwdAlign al, const int64_t *shapes_host,
                                   const int64_t *lsi_host, DensePlan &dp)
{
    if ((elem_bytes != 2 && elem_bytes != 4) || !d.valid()) return false;
    al.staged = al.rows16;
    FwdRoute r;
    return fwd_route(elem_bytes, false, d, al, shapes_host, lsi_host, true, r, dp) == kFwdStaged;
}

// A from-boxes call's operands, filled by the extern "C" wrappers.  Instance flavour: k x k points a level (d.P is
// not read: boxes_prepare sets it), V 4, angle_mode 0; box flavour: d.P points a level (k is not read).
template <typename ST> struct BoxesIn {
    const ST *value;
    const int64_t *shapes, *lsi;
    const float *ref;
    int ref_dim, ref_per_head;
    const float *offsets;
    int V, angle_mode;
    const float *kernel_idx, *valid_ratios, *logits;
    Dims d;
    int k;
    hipStream_t st;
    const int64_t *shapes_host = nullptr, *lsi_host = nullptr;     // the window-staged forward only
};
// An output of a from-boxes call (p NULL: an optional one that is absent) and its bytes a (query, head) pair
struct BoxesOutput { void *p; size_t pair_bytes; };
// What boxes_prepare hands a launcher: the dimensions (with P), the route's launch geometry and the kernels' arguments
struct BoxesLaunch {
    Dims d;
    FwdRoute r;
    GridDims gd;
    BoxesDims bd;           // instance flavour
    unsigned vbytes;
    DensePlan dp;           // window-staged forward (STAGED)
};

// Everything a from-boxes launcher does before its launch; false: the call ends here with rc.  The order shows in
// the return codes: the dimensions and the flavour's limit, no queries -> 0 before any pointer is looked at, the
// required pointers (have_required: those of the launcher's own), no pixels -> the outputs zero-filled, value, the
// route (rows / rows_opt: the row-sized tensors next to value, out / mask_out or grad_out / grad_mask; NULL: aligned).
// STAGED: the box flavour's window-staged forward -- the route is box_boxes_staged_route with in's host tables.
template <typename ST, bool INST, bool STAGED = false>
bool boxes_prepare(const BoxesIn<ST> &in, const ST *rows, const ST *rows_opt, bool have_required,
                   std::initializer_list<BoxesOutput> outputs, BoxesLaunch &l, int &rc)
{
    rc = (int)hipErrorInvalidValue;
    Dims &d = l.d = in.d;
    if constexpr (INST) {
        if (in.k < 2 || in.k > 32 || in.k % 2 != 0 || in.ref_dim < 4) return false;
        d.P = in.k * in.k;
    }
    if (!d.valid() || d.L > 16) return false;
    if constexpr (!INST) {
        if ((long long)d.L * d.P > kBoxesMaxLP) return false;
        if (in.angle_mode < 0 || in.angle_mode > 2 || in.V != (in.angle_mode == 1 ? 5 : 4) ||
            in.ref_dim < (in.angle_mode ? 5 : 4))
            return false;
    }
    if (d.empty()) {                                           // no queries: nothing to write
        rc = 0;
        return false;
    }
    if (!in.shapes || !in.lsi || !in.ref || !in.offsets || !in.kernel_idx || !in.logits || !have_required) return false;
    if (d.n_value() == 0) {                                    // no pixels: every sample and every gradient is 0
        hipError_t e = hipSuccess;
        for (const BoxesOutput &o : outputs)
            if (e == hipSuccess && o.p) e = zero_async(o.p, d.n_qh() * o.pair_bytes, in.st);
        rc = (int)e;
        return false;
    }
    if (!in.value) return false;
    const size_t va = 4 * sizeof(ST);
    const FwdAlign al{aligned(in.value, va) && aligned(rows, va) && aligned(rows_opt, va),
                      aligned(in.value, 16) && aligned(rows, 16) && aligned(rows_opt, 16), false};
    if constexpr (STAGED) {
        static_assert(!INST, "box flavour");
        if (!box_boxes_staged_route((int)sizeof(ST), d, al, in.shapes_host, in.lsi_host, l.dp)) return false;
    } else if (!(INST ? boxes_route((int)sizeof(ST), d, in.k, al, l.r) : box_boxes_route((int)sizeof(ST), d, al, l.r))) {
        return false;
    }
    l.gd = GridDims{d.Lq, d.H, d.L, d.P, in.V, in.ref_dim, in.ref_per_head ? 1 : 0, in.angle_mode};
    if constexpr (INST) {
        const float m = (float)(in.k / 2);
        l.bd = BoxesDims{in.k, in.k / 2, 1.f / (float)in.k, 1.f / (m * m)};
    }
    l.vbytes = (unsigned)(d.n_value() * sizeof(ST));
    return true;
}

// The gradients of a from-boxes backward: per (query, head, level) row V offsets, 5 window terms (optional) and the
// row's logits (instance flavour: 2x2; box flavour: P)
struct BoxesGrads { float *offsets, *ref_rows, *logits; };
template <typename ST, bool INST, bool STAGED = false>
bool boxes_prepare_bwd(const BoxesIn<ST> &in, const ST *grad_out, const ST *grad_mask, const BoxesGrads &g,
                       BoxesLaunch &l, int &rc)
{
    const size_t row = (size_t)in.d.L * sizeof(float);
    return boxes_prepare<ST, INST, STAGED>(
        in, grad_out, grad_mask, grad_out && g.offsets && g.logits,
        {{g.offsets, row * in.V}, {g.ref_rows, row * 5}, {g.logits, row * (INST ? 4 : in.d.P)}}, l, rc);
}

// mask NULL: the flavour without the mask output
template <typename ST> int launch_fwd_boxes(const BoxesIn<ST> &in, ST *out, ST *mask)
{
    // (pair_bytes are read after the dimensions and k have passed)
    const size_t row = (size_t)in.d.C * sizeof(ST);
    BoxesLaunch l;
    int rc;
    if (!boxes_prepare<ST, true>(in, out, mask, out != nullptr, {{out, row}, {mask, row * in.k * in.k}}, l, rc))
        return rc;
    const Dims &d = l.d;
    const GatherIdx ix = with_grid(l.r.ix, l.r.wblocks, 1, 1);
    ScopedKernelTimer timer(g_prof.ev[kSlotFwd], in.st);
    const auto launch = [&](auto inst, auto mask_arg) {
#define BOXATTN_LAUNCH_BOXES(GG, VV)                                                                             \
    hipLaunchKernelGGL((fwd_wide_boxes_kernel<ST, GG, VV, decltype(inst)::value>), dim3(l.r.wblocks), dim3(256), \
                       0, in.st, in.value, in.shapes, in.lsi, in.ref, in.offsets, in.kernel_idx,                 \
                       in.valid_ratios, in.logits, d.S, d.H, d.L, d.Lq, d.P, out, mask_arg, l.gd, l.bd, ix,      \
                       l.vbytes, (unsigned)l.r.ws);
        BOXATTN_GATHER_DISPATCH(l.r.cfg, BOXATTN_LAUNCH_BOXES);
#undef BOXATTN_LAUNCH_BOXES
    };
    if (mask) launch(std::true_type{}, mask);
    else launch(std::false_type{}, NoArg{});
    return finish();
}

template <typename ST> int launch_fwd_box_boxes(const BoxesIn<ST> &in, ST *out)
{
    BoxesLaunch l;
    int rc;
    if (!boxes_prepare<ST, false>(in, out, nullptr, out != nullptr, {{out, (size_t)in.d.C * sizeof(ST)}}, l, rc))
        return rc;
    const Dims &d = l.d;
    const unsigned stride = fwd2_boxes_pair_stride(d.L, d.L * d.P);
    ScopedKernelTimer timer(g_prof.ev[kSlotFwd], in.st);
#define BOXATTN_FWD2_BOXES(GG, VV)                                                                          \
    hipLaunchKernelGGL((fwd2_boxes_kernel<ST, GG, GatherUnroll<ST, GG, VV>::value, VV>), dim3(l.r.blocks),  \
                       dim3(256), (size_t)kGatherWaves * (kWave / GG) * stride * sizeof(u32x4_t), in.st,    \
                       in.value, in.shapes, in.lsi, in.ref, in.offsets, in.kernel_idx, in.valid_ratios,     \
                       in.logits, d.S, d.H, d.L, d.Lq, d.P, out, l.gd,                                      \
                       with_grid(l.r.ix, l.r.blocks, 1, (d.L * d.P + GG - 1) / GG), l.vbytes, stride);
    BOXATTN_GATHER_DISPATCH(l.r.cfg, BOXATTN_FWD2_BOXES);
#undef BOXATTN_FWD2_BOXES
    return finish();
}

// ... on the window-staged forward (in.shapes_host / in.lsi_host: the host copies of the level tables)
template <typename ST> int launch_fwd_box_boxes_staged(const BoxesIn<ST> &in, ST *out)
{
    BoxesLaunch l;
    int rc;
    if (!boxes_prepare<ST, false, true>(in, out, nullptr, out != nullptr, {{out, (size_t)in.d.C * sizeof(ST)}}, l, rc))
        return rc;
    ScopedKernelTimer timer(g_prof.ev[kSlotFwd], in.st);
    const DenseBoxes bx{in.ref, in.offsets, in.kernel_idx, in.valid_ratios, in.logits,
                        l.gd.ref_dim, l.gd.ref_per_head, l.gd.V, l.gd.angle_mode};
    launch_fwd_dense_boxes<ST>(in.value, bx, out, l.dp, l.vbytes, in.st);
    return finish();
}

// grad_mask NULL: the flavour without the level term
template <typename ST>
int launch_bwd_boxes(const BoxesIn<ST> &in, const ST *grad_out, const ST *grad_mask, const BoxesGrads &g)
{
    BoxesLaunch l;
    int rc;
    if (!boxes_prepare_bwd<ST, true>(in, grad_out, grad_mask, g, l, rc)) return rc;
    const Dims &d = l.d;
    const GatherIdx ix = with_grid(l.r.ix, l.r.wblocks, 1, 1);
    ScopedKernelTimer timer(g_prof.ev[kSlotBwdPoints], in.st);
    const auto launch = [&](auto inst, auto grad_mask_arg) {
#define BOXATTN_LAUNCH_BOXES(GG, VV)                                                                              \
    hipLaunchKernelGGL((pointgrad_boxes_kernel<ST, GG, VV, decltype(inst)::value>), dim3(l.r.wblocks), dim3(256), \
                       0, in.st, in.value, in.shapes, in.lsi, in.ref, in.offsets, in.kernel_idx,                  \
                       in.valid_ratios, in.logits, grad_out, grad_mask_arg, d.S, d.H, d.L, d.Lq, d.P, g.offsets,  \
                       g.ref_rows, g.logits, l.gd, l.bd, ix, l.vbytes, (unsigned)l.r.ws);
        BOXATTN_GATHER_DISPATCH(l.r.cfg, BOXATTN_LAUNCH_BOXES);
#undef BOXATTN_LAUNCH_BOXES
    };
    if (grad_mask) launch(std::true_type{}, grad_mask);
    else launch(std::false_type{}, NoArg{});
    return finish();
}

// The two gradient groups of a backward (BOXATTN_WANT_*): VALUE = grad_value, POINTS = grad_loc + the weight gradients
// (from boxes: the box and logit gradients).
enum { kWantValue = BOXATTN_WANT_VALUE, kWantPoints = BOXATTN_WANT_POINTS, kWantAll = kWantValue | kWantPoints };

// One launch of bwd2_boxes_kernel for a prepared call.  SCATTER / POINTS: the kernel's flavour; acc: the float32
// accumulator of grad_value (SCATTER), zero-filled by the caller
template <typename ST, bool SCATTER, bool POINTS>
void launch_bwd2_boxes(const BoxesIn<ST> &in, const BoxesLaunch &l, const ST *grad_out, const BoxesGrads &g, float *acc)
{
    const Dims &d = l.d;
    const unsigned stride = bwd2_boxes_pair_stride(d.L * d.P);
#define BOXATTN_BWD2_BOXES(GG, VV)                                                                          \
    hipLaunchKernelGGL((bwd2_boxes_kernel<ST, GG, GatherUnroll<ST, GG, VV>::value, VV, SCATTER, POINTS>),   \
                       dim3(l.r.blocks), dim3(256),                                                         \
                       (size_t)kGatherWaves * (kWave / GG) * stride * sizeof(float), in.st,                 \
                       in.value, in.shapes, in.lsi, in.ref, in.offsets, in.kernel_idx, in.valid_ratios,     \
                       in.logits, grad_out, d.S, d.H, d.L, d.Lq, d.P, g.offsets, g.ref_rows, g.logits,      \
                       l.gd, with_grid(l.r.ix, l.r.blocks, 1, (d.L * d.P + GG - 1) / GG), l.vbytes, stride, \
                       acc);
    BOXATTN_GATHER_DISPATCH(l.r.cfg, BOXATTN_BWD2_BOXES);
#undef BOXATTN_BWD2_BOXES
}

template <typename ST> int launch_bwd_box_boxes(const BoxesIn<ST> &in, const ST *grad_out, const BoxesGrads &g)
{
    BoxesLaunch l;
    int rc;
    if (!boxes_prepare_bwd<ST, false>(in, grad_out, nullptr, g, l, rc)) return rc;
    ScopedKernelTimer timer(g_prof.ev[kSlotBwdPoints], in.st);
    launch_bwd2_boxes<ST, false, true>(in, l, grad_out, g, nullptr);
    return finish();
}

// ... on the window-staged point-gradient kernels from boxes (in.shapes_host / in.lsi_host: the host copies of the
// level tables; the route of launch_fwd_box_boxes_staged, the alignment now value's and grad_out's).  A pair's 4 L
// logit gradients leave as 16-byte stores: grad_logits aligned to 16 bytes, checked last.
template <typename ST> int launch_bwd_box_boxes_staged(const BoxesIn<ST> &in, const ST *grad_out, const BoxesGrads &g)
{
    BoxesLaunch l;
    int rc;
    if (!boxes_prepare_bwd<ST, false, true>(in, grad_out, nullptr, g, l, rc)) return rc;
    if (!aligned(g.logits, 16)) return (int)hipErrorInvalidValue;
    ScopedKernelTimer timer(g_prof.ev[kSlotBwdPoints], in.st);
    const DenseBoxes bx{in.ref, in.offsets, in.kernel_idx, in.valid_ratios, in.logits,
                        l.gd.ref_dim, l.gd.ref_per_head, l.gd.V, l.gd.angle_mode};
    launch_pointgrad_dense_boxes<ST>(in.value, bx, grad_out, DenseBoxesGrads{g.offsets, g.ref_rows, g.logits}, l.dp,
                                     l.vbytes, in.st);
    return finish();
}

// Bytes of the float32 accumulator a 16-bit boxattn_bwd_boxes_value_* call takes as its workspace
inline size_t bwd_boxes_value_ws_bytes(int elem_bytes, const Dims &d)
{
    return elem_bytes == 2 ? d.n_value() * sizeof(float) : 0;
}

// The same step with grad_value in the launch (want: BOXATTN_WANT_*; POINTS alone is launch_bwd_box_boxes).  float32
// accumulates into grad_value itself, the 16-bit types into `ws` (float32, 16-byte aligned), cast by launch_bwd's pass.
// Every refusal comes before the first launch; no queries: grad_value is zero-filled, no pixels: the other gradients.
template <typename ST>
int launch_bwd_box_boxes_value(const BoxesIn<ST> &in, const ST *grad_out, const BoxesGrads &g, int want,
                               ST *grad_value, float *ws, size_t ws_bytes)
{
    if (want == kWantPoints) return launch_bwd_box_boxes<ST>(in, grad_out, g);
    if ((want != kWantValue && want != kWantAll) || !in.d.valid()) return (int)hipErrorInvalidValue;
    const bool wp = want == kWantAll;
    const size_t nv = in.d.n_value();
    float *acc = nullptr;
    if (nv) {
        if (!grad_value) return (int)hipErrorInvalidValue;
        if constexpr (IsHalf16<ST>::value) {
            if (!ws || !aligned(ws, 16) || ws_bytes < bwd_boxes_value_ws_bytes(2, in.d) ||
                !aligned(grad_value, 4 * sizeof(ST)))
                return (int)hipErrorInvalidValue;
            acc = ws;
        } else {
            acc = grad_value;
        }
    }
    BoxesLaunch l;
    int rc;
    const BoxesGrads none{nullptr, nullptr, nullptr};
    const bool ready = wp ? boxes_prepare_bwd<ST, false>(in, grad_out, nullptr, g, l, rc)
                          : boxes_prepare<ST, false>(in, grad_out, nullptr, grad_out != nullptr, {}, l, rc);
    if (!ready) {
        if (rc == 0 && nv) rc = (int)zero_async(grad_value, nv * sizeof(ST), in.st);   // no queries
        return rc;
    }
    ScopedKernelTimer timer(g_prof.ev[kSlotBwdPoints], in.st);
    hipError_t e = zero_async(acc, nv * sizeof(float), in.st);
    if (e != hipSuccess) return (int)e;
    if (wp) launch_bwd2_boxes<ST, true, true>(in, l, grad_out, g, acc);
    else launch_bwd2_boxes<ST, true, false>(in, l, grad_out, none, acc);
    if constexpr (IsHalf16<ST>::value) {
        rc = finish();
        if (rc) return rc;
        const int blocks = (int)std::min<size_t>((nv / 4 + 255) / 256 + 1, 256 * 16);
        if constexpr (std::is_same<ST, bf16_t>::value)
            hipLaunchKernelGGL(cvt_f32_to_bf16_kernel, dim3(blocks), dim3(256), 0, in.st, acc, grad_value, nv);
        else
            hipLaunchKernelGGL(cvt_f32_to_f16_kernel, dim3(blocks), dim3(256), 0, in.st, acc, grad_value, nv);
    }
    return finish();
}

// ----------------------------------------------------------------------------- backward

// A backward call's operands and its outputs, filled by the extern "C" wrappers (T: float; double for float64 storage).
// shapes_host / lsi_host: the host copies of the level tables (NULL in the entry points that take none).
template <typename ST> struct BwdIn {
    typedef typename Storage<ST>::compute T;
    const ST *value;
    const int64_t *shapes, *lsi;
    const T *loc, *w_sp, *w_lv;
    const ST *grad_out, *grad_mask;
    Dims d;
    const int64_t *shapes_host, *lsi_host;
    hipStream_t st;
};
template <typename ST> struct BwdOut {
    typedef typename Storage<ST>::compute T;
    ST *grad_value;
    T *grad_loc, *grad_sp, *grad_lv;
};

// The atomic kernels.  grad_value_acc = accumulation buffer for grad_value (the output itself for f32/f64, scratch for
// bf16 / f16).  want: the groups to compute -- the pointers of the other group are neither checked nor used, and the
// kernel is the flavour that leaves its work out (bwd_fast_kernel / bwd_generic_kernel: SCATTER, POINTS)
template <typename ST, bool INST>
int launch_bwd(const BwdIn<ST> &in, const BwdOut<ST> &out, typename Storage<ST>::compute *grad_value_acc, int want)
{
    typedef typename Storage<ST>::compute T;
    const Dims &d = in.d;
    const hipStream_t st = in.st;
    if (!d.valid()) return (int)hipErrorInvalidValue;
    const bool wv = (want & kWantValue) != 0, wp = (want & kWantPoints) != 0;
    const size_t nv = d.n_value();
    const size_t n_qh = d.n_qh();
    if (nv && wv) {
        if (!out.grad_value || !grad_value_acc) return (int)hipErrorInvalidValue;
    }
    if (n_qh) {
        if (!in.shapes || !in.lsi || !in.loc || !in.w_sp || !in.grad_out || (wp && (!out.grad_loc || !out.grad_sp)) ||
            (INST && (!in.w_lv || !in.grad_mask || (wp && !out.grad_lv))))
            return (int)hipErrorInvalidValue;
        if (nv && !in.value) return (int)hipErrorInvalidValue;
    }
    if (nv && wv) {
        hipError_t e = zero_async(grad_value_acc, nv * sizeof(T), st);
        if (e != hipSuccess) return (int)e;
    }
    if (n_qh && !nv) {                                         // no pixels: all gradients 0
        if (!wp) return 0;
        const size_t np = n_qh * d.L * d.P;
        hipError_t e = zero_async(out.grad_loc, 2 * np * sizeof(T), st);
        if (e == hipSuccess) e = zero_async(out.grad_sp, np * sizeof(T), st);
        if (e == hipSuccess && INST) e = zero_async(out.grad_lv, np * sizeof(T), st);
        return (int)e;
    }
    if (n_qh && nv) {
        // (the value-only kernel is the accumulate step of its call: it is timed as one)
        ScopedKernelTimer timer(g_prof.ev[wp ? kSlotBwdPoints : kSlotBwdAccum], st);
        bool done = false;
        if constexpr (!std::is_same<ST, double>::value) {
            // (grad_loc takes part in the choice only where it is an output of the call)
            if (fast_ok<ST>(d, in.value, in.loc, in.grad_out,
                            INST ? (const void *)in.grad_mask : (const void *)in.grad_out,
                            wp ? (const void *)out.grad_loc : (const void *)in.grad_out)) {
                const int G = fast_group(d);
                const int blocks = ceil_div_sz(n_qh, (size_t)(kWave / G) * 4);
                const auto launch = [&](auto kernel) {
                    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, st, in.value, in.shapes, in.lsi, in.loc,
                                       in.w_sp, in.w_lv, in.grad_out, in.grad_mask, d.S, d.H, d.L, d.Lq, d.P,
                                       grad_value_acc, out.grad_loc, out.grad_sp, out.grad_lv, n_qh);
                };
                for_group(G, [&](auto g) {
                    constexpr int GG = decltype(g)::value;
                    if (want == kWantAll) launch(bwd_fast_kernel<ST, 4, GG, INST>);
                    else if (wp) launch(bwd_fast_kernel<ST, 4, GG, INST, false>);
                    else launch(bwd_fast_kernel<ST, 4, GG, INST, true, false>);
                });
                done = true;
            } else if (g_variant == 2) {
                return (int)hipErrorInvalidValue;
            }
        }
        if (!done) {
            const int blocks = (int)std::min<size_t>((n_qh + 3) / 4, (size_t)1 << 20);
            const auto launch = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, st, in.value, in.shapes, in.lsi, in.loc, in.w_sp,
                                   in.w_lv, in.grad_out, in.grad_mask, d.S, d.H, d.C, d.L, d.Lq, d.P, grad_value_acc,
                                   out.grad_loc, out.grad_sp, out.grad_lv, n_qh);
            };
            if (want == kWantAll) launch(bwd_generic_kernel<ST, INST>);
            else if (wp) launch(bwd_generic_kernel<ST, INST, false>);
            else launch(bwd_generic_kernel<ST, INST, true, false>);
        }
        int rc = finish();
        if (rc) return rc;
    }
    if constexpr (IsHalf16<ST>::value) {
        if (nv && wv) {
            const int blocks = (int)std::min<size_t>((nv / 4 + 255) / 256 + 1, 256 * 16);
            if constexpr (std::is_same<ST, bf16_t>::value)
                hipLaunchKernelGGL(cvt_f32_to_bf16_kernel, dim3(blocks), dim3(256), 0, st,
                                   grad_value_acc, out.grad_value, nv);
            else
                hipLaunchKernelGGL(cvt_f32_to_f16_kernel, dim3(blocks), dim3(256), 0, st,
                                   grad_value_acc, out.grad_value, nv);
            return finish();
        }
    }
    return 0;
}


#include "boxattn_host_plan.h"       // make_plan / make_dense_plan, plan_layout / scratch_layout, acc_kind, riders_ok

// record format / query order / points per thread of the bin passes of a call
// The accumulate kernel of a CALL: acc_kind of its dimensions, and for 16-bit instance attention the operands only that
// route reads 16 bytes at a time -- a grad_mask view that is not 16-byte aligned (fast_ok asks 8) takes the VALU route
template <typename ST, bool INST>
inline AccKind acc_kind_at(const Dims &d, const void *grad_mask, const void *w_lv)
{
    const AccKind acc = acc_kind<ST, INST>(d);
    if constexpr (INST && IsHalf16<ST>::value) {
        if (acc == kAccTr && !(aligned(grad_mask, 16) && aligned(w_lv, 4))) return kAccValu;
    }
    return acc;
}
inline int bin_flavour(AccKind acc, const Dims &d, const float *loc, const float *w_sp, RecKind rec = kRecPoint)
{
    const bool wide = acc != kAccValu;
    // four points per thread where the layout allows 16-byte loads of a (query, level)'s points
    const bool pt4 = d.P % 4 == 0 && aligned(loc, 16) && (!wide || aligned(w_sp, 16));
    if (rec == kRecGroup) return kRideGroup | kRidePt4;       // (record_kind_at asked for the alignment)
    return (wide ? kRideWide : kRideInterleave) | (pt4 ? kRidePt4 : 0);
}
// The record format of a CALL: record_kind of its dimensions where its locations and weights allow the 16-byte loads of
// a whole group (the kRidePt4 condition); else point records
template <typename ST, bool INST>
inline RecKind record_kind_at(AccKind acc, const Dims &d, const float *loc, const float *w_sp)
{
    return acc == kAccTr && record_kind<ST, INST>(d) == kRecGroup && aligned(loc, 16) && aligned(w_sp, 16) ? kRecGroup
                                                                                                           : kRecPoint;
}
inline BinRide make_ride(const float *loc, const float *w_sp, const Dims &d, const BinPlan &plan,
                         const PlanLayout &pl, char *pbuf, const ScratchLayout *sl, char *sbuf, int flavour,
                         bool fill)
{
    BinRide r{};
    r.loc = loc; r.w_sp = w_sp;
    r.part = (int *)(pbuf + pl.part); r.subtot = (int *)(pbuf + pl.subtot); r.offsets = (int *)(pbuf + pl.offsets);
    r.items = (int4 *)(pbuf + pl.items); r.combos = (int4 *)(pbuf + pl.combos);
    r.n_items = (int *)(pbuf + pl.n_items); r.tickets = (int *)(pbuf + pl.tickets);
    r.records = sl ? (int *)(sbuf + sl->records) : nullptr;
    r.ctickets = fill && sl ? (int *)(sbuf + sl->ctickets) : nullptr;
    r.plan = plan;
    r.H = d.H; r.Lq = d.Lq; r.P = d.P; r.q_per_wg = pl.q_per_wg; r.n_wg = pl.n_wg;
    r.nwg_magic = div_magic((unsigned)pl.n_wg);
    r.flavour = flavour;
    r.grid.n_riders = (unsigned)(pl.n_wg * d.B * d.H);
    r.grid.shift = ride_shift(fill);
    return r;
}

// The bin passes as launches of their own (a backward that plans for itself; maps too big for the riders;
// host kernels that carry none): stages kBinCount | kBinScan | kBinFill.
enum { kBinCount = 1, kBinScan = 2, kBinFill = 4 };
inline void launch_binning(int flavour, const float *loc, const float *w_sp, const Dims &d, const BinPlan &plan,
                           const PlanLayout &w, char *pbuf, int *records, hipStream_t st, int stages,
                           int *ctickets)
{
    constexpr int BW = 8, BH = 4;
    const int ns = d.B * d.H;
    int *part = (int *)(pbuf + w.part), *subtot = (int *)(pbuf + w.subtot);
    int *n_items = (int *)(pbuf + w.n_items), *offsets = (int *)(pbuf + w.offsets);
    int4 *items = (int4 *)(pbuf + w.items), *combos = (int4 *)(pbuf + w.combos);
    const dim3 bgrid(w.n_wg, ns);
    const size_t bsh = ((size_t)plan.nblk + 1) * sizeof(int);
    const int inter = (flavour & kRideInterleave) ? 1 : 0;
    const bool wide = (flavour & kRideWide) != 0, pt4 = (flavour & kRidePt4) != 0, grp = (flavour & kRideGroup) != 0;
    ScopedKernelTimer timer(g_prof.ev[kSlotBwdBin], st);
#define BOXATTN_BIN(FILL_, WIDE_, PT_, ...)                                                         \
    hipLaunchKernelGGL((bin_kernel<BW, BH, FILL_, WIDE_, PT_, ##__VA_ARGS__>), bgrid, dim3(kBinThreads), bsh, st, loc, w_sp, \
                       plan, d.H, d.Lq, d.P, w.q_per_wg, w.n_wg, inter, part, subtot, offsets, records, ctickets)
    if (stages & kBinCount) {
        if (grp) BOXATTN_BIN(false, false, 4, true);
        else if (pt4) BOXATTN_BIN(false, false, 4); else BOXATTN_BIN(false, false, 1);
        if (plan.zero_workers > 0)         // sparse map: the zero workers' geometry table is part of the plan
            hipLaunchKernelGGL(zero_geo_kernel, dim3((plan.nblk + 255) / 256), dim3(256), 0, st, plan,
                               (int2 *)(pbuf + w.zgeo));
    }
    constexpr int kScanFuseWg = 48;        // up to this many bin workgroups per slice the block scan does kernel A's work too
                                           // (38 workgroups, the 300-query decoders: C3'' fp32 68 -> 61 us; 64, C2: binning 49 -> 61 us)
    // (big maps, multi-workgroup block scan: fused up to 8 bin workgroups per slice -- the 1 000-query BEV decoder has 1)
    const bool fuse_a = plan.nblk <= kScanThreads ? w.n_wg <= kScanFuseWg : w.n_wg <= 8;
    if (stages & kBinScan) {
        if (!fuse_a)
            hipLaunchKernelGGL(bin_scan_a_kernel,
                               dim3(kScanSub, ns, std::min(64, (plan.nblk + 255) / 256)), dim3(256), 0, st,
                               part, w.n_wg, subtot, plan);
        if (plan.nblk > kScanThreads) {           // big maps: the block scan over several CUs
            const int nseg = (plan.nblk + kScanThreads - 1) / kScanThreads;
            int4 *tmp = (int4 *)(pbuf + w.scan_tmp), *segtot = tmp + (size_t)ns * plan.nblk;
            hipLaunchKernelGGL(bin_scan_seg_kernel, dim3(nseg, ns), dim3(kScanThreads), 0, st, subtot,
                               offsets, tmp, segtot, plan, part, fuse_a ? w.n_wg : 0);
            hipLaunchKernelGGL(bin_scan_emit_kernel, dim3(nseg, ns), dim3(kScanThreads), 0, st, offsets,
                               tmp, segtot, items, combos, n_items, plan);
        } else {
            hipLaunchKernelGGL(bin_scan_kernel, dim3(ns), dim3(kScanThreads), 0, st, subtot, offsets,
                               items, combos, n_items, plan, part, fuse_a ? w.n_wg : 0);
        }
    }
    if (stages & kBinFill) {
        // (4-byte records: one point per thread -- neighbouring lanes then hold neighbouring slots and their
        // stores coalesce: 18.9 us against 23.0 with four)
        if (grp) BOXATTN_BIN(true, false, 4, true);
        else if (wide && pt4) BOXATTN_BIN(true, true, 4);
        else if (wide) BOXATTN_BIN(true, true, 1);
        else BOXATTN_BIN(true, false, 1);
    }
#undef BOXATTN_BIN
}

inline bool dense_pointgrad_ok(const DensePlan *dp, const void *value, const void *loc, const void *attn,
                               const void *grad_out, const void *grad_loc, const void *grad_attn)
{
    return dp && aligned(value, 16) && aligned(grad_out, 16) && aligned(loc, 8) &&
           aligned(attn, 4) && aligned(grad_loc, 16) && aligned(grad_attn, 16);
}

// Point gradients (grad_loc / grad_weight): query-major, independent of how grad_value is accumulated;
// `fill_ride`: the backward's fill pass as rider workgroups of this launch (*ride_taken: carried).
template <typename ST, int G, bool INST>
void launch_pointgrad(const BwdIn<ST> &in, const BwdOut<ST> &out, const BinRide *fill_ride, bool *ride_taken,
                      const DensePlan *dp)
{
    const Dims &d = in.d;
    const hipStream_t st = in.st;
    if (ride_taken) *ride_taken = false;
    ScopedKernelTimer timer(g_prof.ev[kSlotBwdPoints], st);
    if constexpr (!INST) {      // encoder case: the window-staged kernels (16-bit: matrix cores; float32: VALU)
        if (dense_pointgrad_ok(dp, in.value, in.loc, in.w_sp, in.grad_out, out.grad_loc, out.grad_sp)) {
            const unsigned vbytes = (unsigned)(d.n_value() * sizeof(ST));
            const BinRide ride = fill_ride ? *fill_ride : BinRide{};
            if constexpr (IsHalf16<ST>::value)
                launch_pointgrad_dense<ST>(in.value, in.loc, in.w_sp, in.grad_out, *dp, out.grad_loc, out.grad_sp, vbytes, st, ride);
            else
                launch_pointgrad_dense_f32(in.value, in.loc, in.w_sp, in.grad_out, *dp, out.grad_loc, out.grad_sp, vbytes, st, ride);
            if (fill_ride && ride_taken) *ride_taken = true;
            return;
        }
    }
    const size_t n_qh = d.n_qh();
    const size_t vbytes = d.n_value() * sizeof(ST);
    GatherIdx ix{};
    if (vbytes < kOobOffset && gather_idx(d, ix, sizeof(ST))) {
        const GatherCfg cfg = gather_cfg<ST>(d, aligned(in.value, 16) && aligned(in.grad_out, 16) &&
                                                (!INST || aligned(in.grad_mask, 16)));
        const int blocks = gather_blocks(d, ix, kWave / cfg.G);
        // few pairs x many points (instance attention on the mask-decoder grid): one wave
        // per pair, its lane groups over the point tiles; else one lane group per pair
        const int tiles = (d.L * d.P + cfg.G - 1) / cfg.G;
        const bool wpp = INST && blocks < 1024 && tiles >= kWave / cfg.G;
        unsigned total = 0;
        if (wpp) {
            const int wblocks = ix.head_xcd ? 8 * ceil_div_sz((size_t)d.B * d.Lq, 4)
                                            : ceil_div_sz(n_qh, 4);
            const int split = point_split(wblocks, tiles / (kWave / cfg.G));
            const BinRide ride = place_riders(fill_ride, (unsigned)wblocks, &total);
#define BOXATTN_PG2W(GG, VV)                                                                         \
hipLaunchKernelGGL((pointgrad2_kernel<ST, GG, INST, GatherUnroll<ST, GG, VV>::value, VV, true>), \
                   dim3(total, split), dim3(256), 0, st, in.value, in.shapes, in.lsi, in.loc, in.w_sp, in.w_lv, \
                   in.grad_out, in.grad_mask, d.S, d.H, d.L, d.Lq, d.P, out.grad_loc, out.grad_sp, out.grad_lv, \
                   with_grid(ix, wblocks, split, tiles), (unsigned)vbytes, ride);
            BOXATTN_GATHER_DISPATCH(cfg, BOXATTN_PG2W);
#undef BOXATTN_PG2W
        } else {
            const int split = point_split(blocks, tiles);
            const BinRide ride = place_riders(fill_ride, (unsigned)blocks, &total);
#define BOXATTN_PG2(GG, VV)                                                                   \
hipLaunchKernelGGL((pointgrad2_kernel<ST, GG, INST, GatherUnroll<ST, GG, VV>::value, VV>), \
                   dim3(total, split), dim3(256), 0, st, in.value, in.shapes, in.lsi, in.loc, in.w_sp, \
                   in.w_lv, in.grad_out, in.grad_mask, d.S, d.H, d.L, d.Lq, d.P, out.grad_loc, out.grad_sp, \
                   out.grad_lv, with_grid(ix, blocks, split, tiles), (unsigned)vbytes, ride);
            BOXATTN_GATHER_DISPATCH(cfg, BOXATTN_PG2);
#undef BOXATTN_PG2
        }
        if (fill_ride && ride_taken) *ride_taken = true;
    } else {
        const int blocks = ceil_div_sz(n_qh, (size_t)(kWave / G) * 4);
        hipLaunchKernelGGL((bwd_fast_kernel<ST, 4, G, INST, false>), dim3(blocks), dim3(256),
                           0, st, in.value, in.shapes, in.lsi, in.loc, in.w_sp, in.w_lv, in.grad_out, in.grad_mask,
                           d.S, d.H, d.L, d.Lq, d.P, (float *)nullptr, out.grad_loc, out.grad_sp, out.grad_lv,
                           n_qh);
    }
}

// The accumulate launch of a binned backward: one single-wave workgroup per potential work item (item_cap is
// the host-side bound; the real count lives on the device, surplus workgroups exit at once); the hardware
// dispatcher hands them out as waves retire -- dynamic load balancing without a work-queue atomic (a
// persistent-waves version with a software queue was 15 % slower).  The kernels map workgroups to (slice,
// worker) themselves (XCD affinity), hence the 8-aligned grid.
constexpr int kAccWgCap = 1024;   // accumulate workgroups per slice; beyond that a workgroup takes several items (its next one in
                                  // flight); 256 / 512 / 1024 / 3072 / 6144: C5 99 / 85 / 83 / 93 / 111 us, C2 67 / 54 / 54 / 55 / 54
                                  // (the same bound for the group-record flavour; sweep: DESIGN.md 4.2.3)
template <typename ST, int G, bool INST>
int launch_accumulate(AccKind acc, const ST *grad_out, const ST *grad_mask, const float *loc, const float *w_sp,
                      const float *w_lv, const Dims &d, const BinPlan &plan, const int *offsets, const int4 *items,
                      const int *n_items, const int *records, ST *grad_value, float *partials,
                      const ChunkCombine &cc, const ZeroRole &zr, hipStream_t st, RecKind rec = kRecPoint)
{
    constexpr int C = 4 * G;
    const int ns = d.B * d.H, ns8 = (ns + 7) / 8 * 8;
    const int wg_per_slice = std::min(kAccWgCap, std::max(1, plan.item_cap));
    ScopedKernelTimer timer(g_prof.ev[kSlotBwdAccum], st);
    if constexpr (IsHalf16<ST>::value && !INST) {
        if (acc == kAccTr && rec == kRecGroup) {
            launch_accumulate_tr_group<ST>(C, grad_out, (size_t)d.B * d.Lq * d.H * C * sizeof(ST), plan, d.S, d.H, d.Lq, items,
                                           n_items, records, grad_value, partials, wg_per_slice, ns8, cc, zr, st, loc, w_sp,
                                           d.n_qh() * (size_t)d.L * 4 * 8);
            return finish();
        }
        if (acc == kAccTr) {
            launch_accumulate_tr<ST>(C, grad_out, (size_t)d.B * d.Lq * d.H * C * sizeof(ST), plan, d.S, d.H, d.Lq, items,
                                 n_items, records, grad_value, partials, wg_per_slice, ns8, cc, zr, st);
            return finish();
        }
    }
    if constexpr (IsHalf16<ST>::value && INST) {
        if (acc == kAccTr) {
            launch_accumulate_tr_inst<ST>(C, grad_out, (size_t)d.B * d.Lq * d.H * C * sizeof(ST), plan, d.S, d.H, d.Lq, items,
                                          n_items, records, grad_value, partials, wg_per_slice, ns8, cc, zr, st, grad_mask,
                                          (size_t)d.B * d.Lq * d.P * d.H * C * sizeof(ST), w_lv, d.P);
            return finish();
        }
    }
    if constexpr (std::is_same<ST, float>::value && !INST && C == 32) {
        if (acc == kAccSplit) {
            launch_accumulate_split(grad_out, (size_t)d.B * d.Lq * d.H * C * sizeof(float), plan, d.S, d.H, d.Lq, items,
                                    n_items, records, grad_value, partials, wg_per_slice, ns8, cc, zr, st);
            return finish();
        }
        if (acc == kAccF32) {
            launch_accumulate_f32(grad_out, (size_t)d.B * d.Lq * d.H * C * sizeof(float), plan, d.S, d.H, d.Lq, items,
                                  n_items, records, grad_value, partials, wg_per_slice, ns8, cc, zr, st);
            return finish();
        }
    }
    if constexpr (std::is_same<ST, float>::value && INST && C == 32) {
        if (acc == kAccSplit) {
            launch_accumulate_split(grad_out, (size_t)d.B * d.Lq * d.H * C * sizeof(float), plan, d.S, d.H, d.Lq, items,
                                    n_items, records, grad_value, partials, wg_per_slice, ns8, cc, zr, st, grad_mask,
                                    (size_t)d.B * d.Lq * d.P * d.H * C * sizeof(float), w_lv, d.P);
            return finish();
        }
    }
    if (acc != kAccValu) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL((binned_accumulate_kernel<ST, C, INST, 1, false>), dim3(wg_per_slice + plan.zero_workers, ns8), dim3(64), 0, st,
                       grad_out, grad_mask, loc, w_sp, w_lv, plan, d.S, d.H, d.Lq, d.P, offsets, items, n_items,
                       records, grad_value, partials, cc, zr);
    return finish();
}

// A binned backward: [count -> scans, unless the training forward left a plan] -> point gradients with the
// fill pass riding in their launch -> accumulate (chunked blocks summed by their last chunk).
// points = false: the grad_value half alone (out.grad_loc / grad_sp / grad_lv and dp are not used; spec is null).
// spec: the caller's state of the one-pass fill (boxattn_spec.h) -- nullptr: two-pass binning; spec_warm: its ranges were
// planned by an earlier call (else this call runs the two-pass passes and spec_layout_kernel plans them from its scan)
template <typename ST, int G, bool INST>
int run_binned(const BwdIn<ST> &in, const BwdOut<ST> &out, const BinPlan &plan, const PlanLayout &pl, char *pbuf,
               const ScratchLayout &sl, char *sbuf, bool plan_ready, const DensePlan *dp, const SpecRide *spec,
               bool spec_warm, int *spec_tickets, bool points, AccKind acc, RecKind rkind)
{
    const Dims &d = in.d;
    const hipStream_t st = in.st;
    const float *loc = in.loc, *w_sp = in.w_sp;
    const int ns = d.B * d.H;
    const int flavour = bin_flavour(acc, d, loc, w_sp, rkind);
    int *records = (int *)(sbuf + sl.records);
    float *partials = (float *)(sbuf + sl.partials);
    const int *n_items = (const int *)(pbuf + pl.n_items), *offsets = (const int *)(pbuf + pl.offsets);
    const int4 *items = (const int4 *)(pbuf + pl.items), *combos = (const int4 *)(pbuf + pl.combos);
    const bool one_pass = spec && spec_warm;
    if (!plan_ready && !one_pass)
        launch_binning(flavour, loc, w_sp, d, plan, pl, pbuf, records, st, kBinCount | kBinScan, nullptr);
    bool filled = false;
    if (!points) {
        // grad_value only (*_bwd_part_*, BOXATTN_WANT_VALUE): no point-gradient launch, so nothing the fill pass could
        // ride in -- it runs as a launch of its own, below
    } else if (one_pass) {
        // point gradients + the fill riders' ONE pass over the locations into the ranges the state holds; the slice's
        // last rider writes the work items (and the next call's ranges)
        BinRide ride = make_ride(loc, w_sp, d, plan, pl, pbuf, &sl, sbuf, flavour | kRideSpec, true);
        ride.spec = *spec;
        ride.tickets = spec_tickets;
        launch_pointgrad<ST, G, INST>(in, out, &ride, &filled, dp);
        if (!filled)        // (the launched kernel carries no riders: the two-pass passes as launches, below)
            launch_binning(flavour, loc, w_sp, d, plan, pl, pbuf, records, st, kBinCount | kBinScan, nullptr);
    } else if (riders_ok(plan, pl)) {
        const BinRide ride = make_ride(loc, w_sp, d, plan, pl, pbuf, &sl, sbuf, flavour, true);
        launch_pointgrad<ST, G, INST>(in, out, &ride, &filled, dp);
    } else {
        launch_pointgrad<ST, G, INST>(in, out, nullptr, nullptr, dp);
    }
    // Chunked blocks: summed by their last chunk inside the accumulate launch (chunk_finish; the fill pass -- riding
    // or not -- clears the blocks' tickets) wherever the riders run: one launch less, C2 bf16 125.7 -> 122.9 us, C2 fp32
    // 245 -> 240, C2' fp32 420 -> 411 (profiles/r04_combine_sweep.log; with 1 024-record chunks and a spilling store
    // path it had been the other way round at encoder sizes) and for the short launch chains of few sample points.
    // Encoder-sized maps too big for the riders (the BEV encoder) keep combine_partials_kernel behind the
    // accumulate launch (C5' bf16 464 against 478 us).
    const bool small = (long long)d.Lq * d.L * d.P < 65536;
    const bool own_combine = opt(kOptRiders) == 1 || opt(kOptRiders) == 2 ||
                             (opt(kOptRiders) == 0 && !riders_ok(plan, pl) && !small);
    if (!filled)
        launch_binning(flavour, loc, w_sp, d, plan, pl, pbuf, records, st, kBinFill,
                       own_combine ? nullptr : (int *)(sbuf + sl.ctickets));
    ChunkCombine cc{};
    if (!own_combine) cc = ChunkCombine{(int *)(sbuf + sl.ctickets), combos, plan.nblk, plan.pslot_cap};
    // (sparse maps: zero workers in front of the accumulate grid store the zeros of the blocks without records)
    ZeroRole zr{offsets, (const int2 *)(pbuf + pl.zgeo)};
    BinPlan plan_acc = plan;
    if (one_pass && filled) {       // the front rows of the grid: redo workers for the blocks that outgrew their range
        zr = ZeroRole{nullptr, nullptr, spec->redo, loc, w_sp, d.P};
        plan_acc.zero_workers = kSpecRedoWorkers;
    }
    int rc = launch_accumulate<ST, G, INST>(acc, in.grad_out, in.grad_mask, loc, w_sp, in.w_lv, d, plan_acc, offsets, items,
                                            n_items, records, out.grad_value, partials, cc, zr, st, rkind);
    if (rc) return rc;
    if (spec && !(one_pass && filled))      // a cold state: the next call's ranges from this call's exact scan
        hipLaunchKernelGGL(spec_layout_kernel<256>, dim3(ns), dim3(256), 0, st, plan, offsets, spec->cursor, spec->cbase,
                           spec->redo);
    if (own_combine) {
        ScopedKernelTimer timer(g_prof.ev[kSlotBwdCombine], st);
        hipLaunchKernelGGL((combine_partials_kernel<ST, 4 * G>), dim3(64, ns), dim3(64), 0, st, combos,
                           n_items, partials, combine_plan(plan), d.S, d.H, out.grad_value);
    }
    return finish();
}

// The backward behind *_bwd_ws_* (want = kWantAll) and *_bwd_part_*: the one place where a call's route is decided.
// wv / wp: grad_value (VALUE) / the point gradients (POINTS) are wanted; the pointers of a group that is not wanted
// are dropped on entry and never looked at.
//
//   binned   variant 0 or 3, pixels and queries, make_plan, fast_ok (grad_loc takes part only with wp)
//            + with wv: a 256-aligned workspace that holds the scratch (and the plan, unless the caller's
//              plan_buf is usable: plan_ready) and a 16-aligned grad_value
//   not binned: variant 3 refuses; else the atomic kernels (launch_bwd) -- with wv and 16-bit storage the workspace is
//            their float32 accumulation buffer and must hold B S H C floats
//   binned, POINTS only: launch_pointgrad without a fill ride.  No workspace, plan or state
//   binned, VALUE only:  run_binned without its point-gradient launch: two-pass binning (count and scans unless
//            plan_ready, the fill as a launch of its own); the state is neither read nor written
//   binned, all: run_binned; the fill rides in the point-gradient launch, and where the shape allows (spec_ok) and no
//            plan came with the call it is the one-pass fill on the ranges the caller's state holds
template <typename ST, bool INST>
int launch_bwd_routed(const BwdIn<ST> &in, BwdOut<ST> out, void *workspace, size_t workspace_bytes,
                      const void *plan_buf, size_t plan_bytes, void *state, size_t state_bytes, int hints, int want)
{
    constexpr bool kH16 = IsHalf16<ST>::value;           // 16-bit storage (bf16 / f16): float32 scratch for the atomics
    const Dims &d = in.d;
    if ((want != kWantValue && want != kWantPoints && want != kWantAll) || !d.valid()) return (int)hipErrorInvalidValue;
    const bool wv = (want & kWantValue) != 0, wp = (want & kWantPoints) != 0;
    if (!wv) out.grad_value = nullptr;
    if (!wp) out.grad_loc = out.grad_sp = out.grad_lv = nullptr;
    BinPlan plan;
    const size_t nv = d.n_value();
    const AccKind acc = acc_kind_at<ST, INST>(d, in.grad_mask, in.w_lv);
    const RecKind rkind = record_kind_at<ST, INST>(acc, d, in.loc, in.w_sp);
    bool binned = (g_variant == 0 || g_variant == 3) && nv && d.n_qh() &&
                  make_plan(d, in.shapes_host, in.lsi_host, plan, rkind) &&
                  fast_ok<ST>(d, in.value, in.loc, in.grad_out,
                              INST ? (const void *)in.grad_mask : (const void *)in.grad_out,
                              wp ? (const void *)out.grad_loc : (const void *)in.grad_out);
    PlanLayout pl{};
    ScratchLayout sl{};
    bool plan_ready = false;
    if (binned && wv) {
        pl = plan_layout(d, plan);
        // (the layout the workspace query sized: where the shape's box attention takes group records the query answered
        // for those, and every other call of that shape -- instance attention -- is laid out for the records it writes)
        sl = scratch_layout(d, plan, rkind == kRecGroup ? 4
                                     : kH16 && record_kind<bf16_t, false>(d) == kRecGroup ? (acc != kAccValu ? 16 : 4)
                                     : workspace_record_bytes(kH16, d));
        // (a training forward plans for acc_kind's record order: a call that leaves that route for its operands'
        // alignment plans for itself; it builds no plan for a shape that may take group records)
        plan_ready = plan_buf && plan_bytes >= pl.total && aligned(plan_buf, 256) && acc == acc_kind<ST, INST>(d) &&
                     record_kind<ST, INST>(d) == kRecPoint;
        binned = workspace && aligned(workspace, 256) && aligned(out.grad_value, 16) &&
                 workspace_bytes >= (plan_ready ? sl.total : pl.total + sl.total);
    }
    if (!binned) {
        // (a plan the forward built is simply not used when the backward's own checks -- e.g. an
        // unaligned grad_out view -- rule the binned path out: the atomic path needs no plan)
        if (g_variant == 3) return (int)hipErrorInvalidValue;
        float *acc = nullptr;
        if (wv) {
            if constexpr (kH16) {
                if (!workspace || workspace_bytes < nv * sizeof(float)) return (int)hipErrorInvalidValue;
                acc = (float *)workspace;
            } else {
                acc = out.grad_value;
            }
        }
        return launch_bwd<ST, INST>(in, out, acc, want);
    }
    if (!in.shapes || !in.lsi || !in.loc || !in.w_sp || !in.grad_out || !in.value || (INST && (!in.w_lv || !in.grad_mask)) ||
        (wv && !out.grad_value) || (wp && (!out.grad_loc || !out.grad_sp || (INST && !out.grad_lv))))
        return (int)hipErrorInvalidValue;
    DensePlan dense;
    const DensePlan *dp = wp && !INST && !(hints & BOXATTN_HINT_NOT_LOCAL) &&
                                  make_dense_plan(d, in.shapes_host, in.lsi_host, dense, (int)sizeof(ST)) ? &dense : nullptr;
    if (!wv) {
        for_group(fast_group(d), [&](auto g) {
            launch_pointgrad<ST, decltype(g)::value, INST>(in, out, nullptr, nullptr, dp);
        });
        return finish();
    }
    char *ws = (char *)workspace;
    char *pbuf = plan_ready ? const_cast<char *>((const char *)plan_buf) : ws;
    char *sbuf = plan_ready ? ws : ws + pl.total;
    // the one-pass fill (boxattn_spec.h): the caller's state holds the bins' ranges
    SpecRide spec{};
    const SpecRide *sp = nullptr;
    bool spec_warm = false;
    int *spec_tickets = nullptr;
    if (wp && !plan_ready && spec_ok<ST, INST>(d, plan, pl)) {
        const StateLayout sy = state_layout(d, &plan);
        const int chk = state_check(state, state_bytes, sy, d, in.shapes_host, in.st, (hints & BOXATTN_HINT_FRESH_STATE) != 0,
                                    (int)rkind);
        if (chk < 0) return (int)hipErrorInvalidValue;
        if (chk > 0) {
            char *sb = (char *)state;
            spec = SpecRide{(int *)(sb + sy.cursor), (int *)(sb + sy.cbase), (int2 *)(sb + sy.redo),
                            (unsigned long long *)(sb + sy.spec_stats)};
            sp = &spec;
            spec_warm = chk == 2;
            spec_tickets = (int *)(sb + sy.tickets);
            state_learned(state);        // (whichever way this call goes, it leaves the next call's ranges behind)
        }
    }
    int rc = 0;
    for_group(fast_group(d), [&](auto g) {
        rc = run_binned<ST, decltype(g)::value, INST>(in, out, plan, pl, pbuf, sl, sbuf, plan_ready, dp, sp, spec_warm,
                                                      spec_tickets, wp, acc, rkind);
    });
    return rc;
}

// Training forward: the forward kernel with the backward's count pass and scans riding in its launch (they only
// depend on the sampling locations); `plan_buf` then carries the plan to the *_bwd_ws_* call.
template <typename ST, bool INST>
int launch_fwd_train(const FwdIn<ST> &in, const FwdOut<ST> &o, void *plan_buf, size_t plan_bytes, void *state,
                     size_t state_bytes, int hints, int *plan_built)
{
    const Dims &d = in.d;
    const hipStream_t st = in.st;
    if (plan_built) *plan_built = 0;
    // the locality counters of the window-staged forward, then the riders' tickets, then the one-pass fill's ranges
    const size_t tbytes = (size_t)std::max(0, d.B) * (size_t)std::max(0, d.H) * kRideTickets * sizeof(int);
    BinPlan plan;
    const bool planned = d.valid() && make_plan(d, in.shapes_host, in.lsi_host, plan);
    const StateLayout sy = state_layout(d, planned ? &plan : nullptr);
    // (a state buffer that is too small or misaligned is an error, not "no state": the caller would silently lose the
    // locality counters and pay a zero-fill launch in front of every forward)
    if (state_check(state, state_bytes, sy, d, in.shapes_host, st, (hints & BOXATTN_HINT_FRESH_STATE) != 0) < 0)
        return (int)hipErrorInvalidValue;
    const bool have_state = state != nullptr;
    FwdExtras x;                  // of every launch_fwd below; the one that carries the count riders adds them
    x.allow_dense = !(hints & BOXATTN_HINT_NOT_LOCAL);
    x.stats = have_state ? (unsigned long long *)state : nullptr;
    // what the backward will check and the forward can already see (its other operands, grad_out / grad_value, are
    // re-checked there; an ineligible backward ignores the plan)
    const auto bwd_fast_ok = [&] {
        return fast_ok<ST>(d, in.value, in.loc, o.out, INST ? (const void *)o.mask : (const void *)o.out, o.out);
    };
    // The backward of this shape fills its bins in one pass, from ranges it keeps in the state buffer: nothing of the
    // backward rides in the forward, and there is no plan to hand over (*plan_built stays 0)
    if (have_state && planned && d.n_value() && d.n_qh() && (g_variant == 0 || g_variant == 3) && bwd_fast_ok() &&
        spec_ok<ST, INST>(d, plan, plan_layout(d, plan)))
        return launch_fwd<ST, INST>(in, o, x);
    bool ok = (g_variant == 0 || g_variant == 3) && plan_buf && planned && d.n_value() && d.n_qh() &&
              aligned(plan_buf, 256) && bwd_fast_ok();
    PlanLayout pl{};
    if (ok) {
        pl = plan_layout(d, plan);
        ok = plan_bytes >= pl.total;
    }
    // (a shape that may take group records: its backward counts groups, and plans for itself)
    if (!ok || record_kind<ST, INST>(d) == kRecGroup) return launch_fwd<ST, INST>(in, o, x);
    char *pbuf = (char *)plan_buf;
    const float *loc = in.loc, *w_sp = in.w_sp;
    const int flavour = bin_flavour(acc_kind<ST, INST>(d), d, loc, w_sp);
    bool taken = false;
    BinRide ride;
    if (riders_ok(plan, pl)) {
        // The riders' tickets start at zero and are left zero by the call.  `state`: the caller's zeroed,
        // persistent ticket buffer (one per stream: calls on a stream never overlap); without it the tickets live
        // in the -- possibly fresh -- plan buffer and are cleared by a launch of their own (~5 us in front of
        // the forward kernel).
        ride = make_ride(loc, w_sp, d, plan, pl, pbuf, nullptr, nullptr, flavour, false);
        if (have_state) {
            ride.tickets = (int *)((char *)state + sy.tickets);
        } else {
            hipError_t e = zero_async(pbuf + pl.tickets, tbytes, st);
            if (e != hipSuccess) return (int)e;
        }
        x.count_ride = &ride;
        x.ride_taken = &taken;
    }
    int rc = launch_fwd<ST, INST>(in, o, x);
    if (rc) return rc;
    if (!taken)
        launch_binning(flavour, loc, w_sp, d, plan, pl, pbuf, nullptr, st, kBinCount | kBinScan, nullptr);
    rc = finish();
    if (rc == 0 && plan_built) *plan_built = 1;
    return rc;
}

// the C ABI passes 16-bit storage as uint16_t; f16 storage is f16_t inside
inline const f16_t *as_f16(const uint16_t *p) { return reinterpret_cast<const f16_t *>(p); }
inline f16_t *as_f16(uint16_t *p) { return reinterpret_cast<f16_t *>(p); }

}  // namespace

extern "C" {

#define DIMS Dims{B, S, H, C, L, Lq, P}
#define ST_ (hipStream_t) stream

// The storage types of the entry points: X(suffix, element type of the C ABI, storage type inside, cast, geometry
// type: double for float64, [FL]).  A family of entry points is one macro X, expanded over the three types
// (STORAGE_TYPES), the four with float64 in the header's order (STORAGE_TYPES_F64) or a part of them.  FL is what the
// expansion passes on to X: the flavour, BOX or INST, of the families that have both (the from-boxes ones take none)
#define STORAGE_F32(X, ...) X(f32, float, float, , float, __VA_ARGS__)
#define STORAGE_F64(X, ...) X(f64, double, double, , double, __VA_ARGS__)
#define STORAGE_H16(X, ...) \
    X(bf16, uint16_t, bf16_t, , float, __VA_ARGS__) X(f16, uint16_t, f16_t, as_f16, float, __VA_ARGS__)
#define STORAGE_TYPES(X, ...) STORAGE_F32(X, __VA_ARGS__) STORAGE_H16(X, __VA_ARGS__)
#define STORAGE_TYPES_F64(X, ...) STORAGE_F32(X, __VA_ARGS__) STORAGE_F64(X, __VA_ARGS__) STORAGE_H16(X, __VA_ARGS__)

// The two flavours FL of a family, BOX and INST: the prefix of the name, launch_*'s INST, a forward's / a backward's
// parameters up to its last output (include/boxattn.h documents them), and the FwdIn / FwdOut / BwdIn / BwdOut of the
// call, from those parameters by their names (the field order of the structs; SH, LH: the host tables or nullptr)
#define HEAD_PARAMS(CT, GT) const CT *value, const int64_t *shapes, const int64_t *lsi, const GT *loc
#define DIMS_PARAMS int B, int S, int H, int C, int L, int Lq, int P
#define HOST_TABLES const int64_t *shapes_host, const int64_t *lsi_host
#define BOX_NAME(fn) boxattn_##fn
#define BOX_INST false
#define BOX_FWD_PARAMS(CT, GT) HEAD_PARAMS(CT, GT), const GT *attn, DIMS_PARAMS, CT *out
#define BOX_FWD_IN(ST, CAST, SH, LH) FwdIn<ST>{CAST(value), shapes, lsi, loc, attn, nullptr, DIMS, SH, LH, ST_}
#define BOX_FWD_OUT(ST, CAST) FwdOut<ST>{CAST(out), nullptr}
#define BOX_BWD_PARAMS(CT, GT)                                                                                 \
    HEAD_PARAMS(CT, GT), const GT *attn, const CT *grad_out, DIMS_PARAMS, CT *grad_value, GT *grad_loc, GT *grad_attn
#define BOX_BWD_IN(ST, CAST, SH, LH) \
    BwdIn<ST>{CAST(value), shapes, lsi, loc, attn, nullptr, CAST(grad_out), nullptr, DIMS, SH, LH, ST_}
#define BOX_BWD_OUT(ST, CAST) BwdOut<ST>{CAST(grad_value), grad_loc, grad_attn, nullptr}
#define INST_NAME(fn) instattn_##fn
#define INST_INST true
#define INST_FWD_PARAMS(CT, GT) \
    HEAD_PARAMS(CT, GT), const GT *spatial_w, const GT *level_w, DIMS_PARAMS, CT *out, CT *mask_out
#define INST_FWD_IN(ST, CAST, SH, LH) \
    FwdIn<ST>{CAST(value), shapes, lsi, loc, spatial_w, level_w, DIMS, SH, LH, ST_}
#define INST_FWD_OUT(ST, CAST) FwdOut<ST>{CAST(out), CAST(mask_out)}
#define INST_BWD_PARAMS(CT, GT)                                                                                \
    HEAD_PARAMS(CT, GT), const GT *spatial_w, const GT *level_w, const CT *grad_out, const CT *grad_mask,      \
        DIMS_PARAMS, CT *grad_value, GT *grad_loc, GT *grad_spatial_w, GT *grad_level_w
#define INST_BWD_IN(ST, CAST, SH, LH)                                                                          \
    BwdIn<ST>{CAST(value), shapes, lsi, loc, spatial_w, level_w, CAST(grad_out), CAST(grad_mask), DIMS, SH, LH, ST_}
#define INST_BWD_OUT(ST, CAST) BwdOut<ST>{CAST(grad_value), grad_loc, grad_spatial_w, grad_level_w}

// *_fwd_train_*: the forward with the host tables, the plan and state buffers, hints and *plan_built
#define FWD_TRAIN(SUF, CT, ST, CAST, GT, FL)                                                                   \
    int FL##_NAME(fwd_train_##SUF)(FL##_FWD_PARAMS(CT, GT), HOST_TABLES, void *plan, size_t plan_bytes,        \
                                   void *state, size_t state_bytes, int hints, int *plan_built, void *stream)  \
    {                                                                                                          \
        return launch_fwd_train<ST, FL##_INST>(FL##_FWD_IN(ST, CAST, shapes_host, lsi_host),                   \
                                               FL##_FWD_OUT(ST, CAST), plan, plan_bytes, state, state_bytes,   \
                                               hints, plan_built);                                             \
    }
STORAGE_TYPES(FWD_TRAIN, BOX)
STORAGE_TYPES(FWD_TRAIN, INST)
#undef FWD_TRAIN

size_t boxattn_plan_bytes(int is_16bit, int B, int S, int H, int C, int L, int Lq, int P,
                          const int64_t *shapes_host, const int64_t *lsi_host)
{
    const Dims d = DIMS;
    BinPlan plan;
    if (!d.valid() || !make_plan(d, shapes_host, lsi_host, plan)) return 0;
    size_t need = plan_layout(d, plan).total;
    BinPlan gplan;        // (group records cut more work items: boxattn_bwd_workspace_bytes)
    if (is_16bit && record_kind<bf16_t, false>(d) == kRecGroup && make_plan(d, shapes_host, lsi_host, gplan, kRecGroup))
        need = std::max(need, plan_layout(d, gplan).total);
    return need;
}

size_t boxattn_state_bytes(int B, int S, int H, int C, int L, int Lq, int P, const int64_t *shapes_host,
                           const int64_t *lsi_host)
{
    const Dims d = DIMS;
    BinPlan plan;
    const bool planned = d.valid() && make_plan(d, shapes_host, lsi_host, plan);
    return state_layout(d, planned ? &plan : nullptr).total;
}

size_t boxattn_bwd_workspace_bytes(int is_16bit, int B, int S, int H, int C, int L, int Lq, int P,
                                   const int64_t *shapes_host, const int64_t *lsi_host)
{
    const Dims d = DIMS;
    if (!d.valid()) return 0;
    const size_t fallback = is_16bit ? align_up(d.n_value() * sizeof(float)) : 0;
    BinPlan plan;
    if (!make_plan(d, shapes_host, lsi_host, plan)) return fallback;
    size_t need = plan_layout(d, plan).total + scratch_layout(d, plan, workspace_record_bytes(is_16bit != 0, d)).total;
    // (a shape whose box attention takes group records: their plan -- smaller chunks, more partial tiles -- and 4-byte
    // records; instance attention keeps the point flavour's sizes where those are larger.  A box-attention call whose
    // locations are not 16-byte aligned would write 16-byte point records, which this area does not hold: it takes the
    // atomic kernels, like any call the binned route's checks rule out)
    BinPlan gplan;
    if (is_16bit && record_kind<bf16_t, false>(d) == kRecGroup && make_plan(d, shapes_host, lsi_host, gplan, kRecGroup)) {
        const size_t gneed = plan_layout(d, gplan).total + scratch_layout(d, gplan, 4).total;
        const bool inst_wide = inst_tr_ok(d);
        need = inst_wide ? std::max(need, gneed)
                         : std::max(gneed, plan_layout(d, plan).total + scratch_layout(d, plan, 4).total);
    }
    return std::max(fallback, need);
}

// *_bwd_ws_* and the partial backward *_bwd_part_* (BOXATTN_WANT_*): one body, the first with kWantAll
#define WS_PARAMS                                                                                              \
    void *workspace, size_t workspace_bytes, const void *plan, size_t plan_bytes, void *state, size_t state_bytes, \
        int hints
#define BWD_ROUTED(ST, CAST, FL, WANT)                                                                         \
    launch_bwd_routed<ST, FL##_INST>(FL##_BWD_IN(ST, CAST, shapes_host, lsi_host), FL##_BWD_OUT(ST, CAST),     \
                                     workspace, workspace_bytes, plan, plan_bytes, state, state_bytes, hints, WANT)
#define BWD_WS_PART(SUF, CT, ST, CAST, GT, FL)                                                                 \
    int FL##_NAME(bwd_ws_##SUF)(FL##_BWD_PARAMS(CT, GT), HOST_TABLES, WS_PARAMS, void *stream)                 \
    {                                                                                                          \
        return BWD_ROUTED(ST, CAST, FL, kWantAll);                                                             \
    }                                                                                                          \
    int FL##_NAME(bwd_part_##SUF)(FL##_BWD_PARAMS(CT, GT), HOST_TABLES, WS_PARAMS, void *stream, int want)     \
    {                                                                                                          \
        return BWD_ROUTED(ST, CAST, FL, want);                                                                 \
    }
STORAGE_TYPES(BWD_WS_PART, BOX)
STORAGE_TYPES(BWD_WS_PART, INST)
#undef BWD_WS_PART
#undef BWD_ROUTED
#undef WS_PARAMS

// The atomic kernels behind *_bwd_* (ACC: where grad_value is accumulated) and *_bwd_part_f64
#define BWD_ATOMIC(ST, CAST, FL, ACC, WANT)                                                                    \
    launch_bwd<ST, FL##_INST>(FL##_BWD_IN(ST, CAST, nullptr, nullptr), FL##_BWD_OUT(ST, CAST), ACC, WANT)
// float64: the arguments of *_bwd_f64 + want
#define BWD_PART_F64(SUF, CT, ST, CAST, GT, FL)                                                                \
    int FL##_NAME(bwd_part_##SUF)(FL##_BWD_PARAMS(CT, GT), void *stream, int want)                             \
    {                                                                                                          \
        if (want != kWantValue && want != kWantPoints && want != kWantAll) return (int)hipErrorInvalidValue;   \
        return BWD_ATOMIC(ST, CAST, FL, grad_value, want);                                                     \
    }
STORAGE_F64(BWD_PART_F64, BOX)
STORAGE_F64(BWD_PART_F64, INST)
#undef BWD_PART_F64

int boxattn_abi_version(void) { return BOXATTN_ABI_VERSION; }

#define STR_(x) #x
#define STR(x) STR_(x)
const char *boxattn_build_info(void)
{
    return "boxattn gfx950 (CDNA4, wave64) | hipcc " __VERSION__
           " | kernels: generic{f32,f64,bf16,f16}, gather{f32 4ch/lane, bf16/f16 8ch/lane} C={16,32,64}, "
           "window-staged encoder forward + point gradients{bf16/f16 on MFMA 4x4x4, f32 on VALU}, "
           "binned-bwd{bf16/f16 on MFMA 32x32x16, f32 on the bf16 MFMA over exact three-term bf16 splits} "
           "with fill / combine riding in the point-gradient and accumulate launches, "
           "one-pass fill into guessed bin ranges (caller-owned state), box-grid{f32} | abi " STR(BOXATTN_ABI_VERSION);
}
#undef STR
#undef STR_

int boxattn_profile_begin(void)
{
    std::lock_guard<std::mutex> g(g_prof.mu);
    for (auto &v : g_prof.ev) drain(v, nullptr, nullptr);
    g_prof.on = true;
    return 0;
}

int boxattn_profile_end(double *ms_sum, int *launches)
{
    g_prof.on = false;
    std::lock_guard<std::mutex> g(g_prof.mu);
    for (int i = 0; i < kNumSlots; ++i)
        drain(g_prof.ev[i], ms_sum ? ms_sum + i : nullptr, launches ? launches + i : nullptr);
    return 0;
}

std::atomic<int> g_epoch{0};
int boxattn_options_epoch(void) { return g_epoch.load(std::memory_order_relaxed); }

int boxattn_set_variant(int variant)
{
    g_epoch.fetch_add(1, std::memory_order_relaxed);
    return g_variant.exchange(variant);
}

// no effect: the time-stamp builds that read the buffer are gone; kept exported for ABI 8
void boxattn_set_debug_buffer(float *) {}

int boxattn_set_option(int key, int value)
{
    if (key < 0 || key >= kNumOpts || !opt_live(key)) return -1;
    g_epoch.fetch_add(1, std::memory_order_relaxed);
    return g_opt[key].exchange(value);
}


int boxattn_bwd_accumulate_kind(int elem_bytes, int instance, int B, int S, int H, int C, int L, int Lq, int P)
{
    const Dims d = DIMS;
    if (!d.valid()) return -1;
    // (bf16 and f16 storage route alike: one answer for elem_bytes == 2)
    if (elem_bytes == 2) return (int)(instance ? acc_kind<bf16_t, true>(d) : acc_kind<bf16_t, false>(d));
    if (elem_bytes == 4) return (int)(instance ? acc_kind<float, true>(d) : acc_kind<float, false>(d));
    return -1;          // float64 has no binned backward
}

int boxattn_bwd_record_kind(int elem_bytes, int instance, int B, int S, int H, int C, int L, int Lq, int P)
{
    const Dims d = DIMS;
    if (!d.valid()) return -1;
    if (elem_bytes == 2) return (int)(instance ? record_kind<bf16_t, true>(d) : record_kind<bf16_t, false>(d));
    if (elem_bytes == 4) return (int)(instance ? record_kind<float, true>(d) : record_kind<float, false>(d));
    return -1;          // float64 has no binned backward
}

int boxattn_fwd_route(int elem_bytes, int instance, int aligned, int B, int S, int H, int C, int L, int Lq, int P,
                      const int64_t *shapes_host, const int64_t *lsi_host)
{
    const Dims d = DIMS;
    if (!d.valid() || (elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8)) return -1;
    FwdAlign al = align_from_bytes(elem_bytes, aligned);
    al.staged = al.rows16;
    FwdRoute r;
    DensePlan dp;
    return fwd_route(elem_bytes, instance != 0, d, al, shapes_host, lsi_host, true, r, dp);
}

// ---- attention from boxes and logits: two eligibility queries a flavour (one answer) and an entry point per route
// and storage type
int instattn_fwd_boxes_ok(int elem_bytes, int aligned, int B, int S, int H, int C, int L, int Lq, int k)
{
    const Dims d{B, S, H, C, L, Lq, (int)((unsigned)k * (unsigned)k)};     // (any k: boxes_route tests it)
    FwdRoute r;
    return boxes_route(elem_bytes, d, k, align_from_bytes(elem_bytes, aligned), r) ? 1 : 0;
}
int instattn_bwd_boxes_ok(int elem_bytes, int aligned, int B, int S, int H, int C, int L, int Lq, int k)
{
    return instattn_fwd_boxes_ok(elem_bytes, aligned, B, S, H, C, L, Lq, k);   // boxes_route: one eligibility
}
int boxattn_fwd_boxes_ok(int elem_bytes, int aligned, int B, int S, int H, int C, int L, int Lq, int P)
{
    FwdRoute r;
    return box_boxes_route(elem_bytes, DIMS, align_from_bytes(elem_bytes, aligned), r) ? 1 : 0;
}
int boxattn_fwd_boxes_hl_ok(int elem_bytes, int aligned, int B, int S, int H, int C, int L, int Lq, int P,
                            const int64_t *shapes_host, const int64_t *lsi_host)
{
    DensePlan dp;
    const FwdAlign al = align_from_bytes(elem_bytes, aligned);
    return box_boxes_staged_route(elem_bytes, DIMS, al, shapes_host, lsi_host, dp) ? 1 : 0;
}
int boxattn_bwd_boxes_ok(int elem_bytes, int aligned, int B, int S, int H, int C, int L, int Lq, int P)
{
    return boxattn_fwd_boxes_ok(elem_bytes, aligned, B, S, H, C, L, Lq, P);   // box_boxes_route: one eligibility
}
int boxattn_bwd_boxes_hl_ok(int elem_bytes, int aligned, int B, int S, int H, int C, int L, int Lq, int P,
                            const int64_t *shapes_host, const int64_t *lsi_host)
{
    // box_boxes_staged_route: one eligibility
    return boxattn_fwd_boxes_hl_ok(elem_bytes, aligned, B, S, H, C, L, Lq, P, shapes_host, lsi_host);
}
int boxattn_bwd_boxes_value_ok(int elem_bytes, int aligned, int B, int S, int H, int C, int L, int Lq, int P)
{
    return boxattn_bwd_boxes_ok(elem_bytes, aligned, B, S, H, C, L, Lq, P);   // the same kernel family
}
size_t boxattn_bwd_boxes_value_workspace_bytes(int elem_bytes, int B, int S, int H, int C)
{
    if (B < 0 || S < 0 || H < 0 || C < 0) return 0;
    return bwd_boxes_value_ws_bytes(elem_bytes, Dims{B, S, H, C, 1, 0, 1});
}

// A wrapper's BoxesIn<ST>, from its parameters by their names (the field order of the struct); the instance flavour
// passes V 4, angle_mode 0 and no P, the box flavour no k
#define BOXES_IN(ST, CAST, V_, ANGLE_, P_, K_)                                                                 \
    BoxesIn<ST>{CAST(value), shapes, lsi, ref, ref_dim, ref_per_head, offsets, V_, ANGLE_, kernel_idx,         \
                valid_ratios, logits, Dims{B, S, H, C, L, Lq, P_}, K_, ST_}
#define BOXES_GRADS BoxesGrads{grad_offsets, grad_ref_rows, grad_logits}

#define INSTATTN_FWD_BOXES(SUF, CT, ST, CAST, ...)                                                             \
    int instattn_fwd_boxes_##SUF(const CT *value, const int64_t *shapes, const int64_t *lsi, const float *ref, \
                                 int ref_dim, int ref_per_head, const float *offsets, const float *kernel_idx, \
                                 const float *valid_ratios, const float *logits, int B, int S, int H, int C,   \
                                 int L, int Lq, int k, CT *out, CT *mask_out, void *stream)                    \
    {                                                                                                          \
        return launch_fwd_boxes<ST>(BOXES_IN(ST, CAST, 4, 0, 0, k), CAST(out), CAST(mask_out));                \
    }
STORAGE_TYPES(INSTATTN_FWD_BOXES)
#undef INSTATTN_FWD_BOXES

#define BOXATTN_FWD_BOXES(SUF, CT, ST, CAST, ...)                                                              \
    int boxattn_fwd_boxes_##SUF(const CT *value, const int64_t *shapes, const int64_t *lsi, const float *ref,  \
                                int ref_dim, int ref_per_head, const float *offsets, int V, int angle_mode,    \
                                const float *kernel_idx, const float *valid_ratios, const float *logits,       \
                                int B, int S, int H, int C, int L, int Lq, int P, CT *out, void *stream)       \
    {                                                                                                          \
        return launch_fwd_box_boxes<ST>(BOXES_IN(ST, CAST, V, angle_mode, P, 0), CAST(out));                   \
    }
STORAGE_TYPES(BOXATTN_FWD_BOXES)
#undef BOXATTN_FWD_BOXES

#define BOXATTN_FWD_BOXES_HL(SUF, CT, ST, CAST, ...)                                                           \
    int boxattn_fwd_boxes_hl_##SUF(const CT *value, const int64_t *shapes, const int64_t *lsi, const float *ref, \
                                   int ref_dim, int ref_per_head, const float *offsets, int V, int angle_mode, \
                                   const float *kernel_idx, const float *valid_ratios, const float *logits,    \
                                   int B, int S, int H, int C, int L, int Lq, int P, CT *out, HOST_TABLES,     \
                                   void *stream)                                                               \
    {                                                                                                          \
        BoxesIn<ST> in = BOXES_IN(ST, CAST, V, angle_mode, P, 0);                                              \
        in.shapes_host = shapes_host;                                                                          \
        in.lsi_host = lsi_host;                                                                                \
        return launch_fwd_box_boxes_staged<ST>(in, CAST(out));                                                 \
    }
STORAGE_TYPES(BOXATTN_FWD_BOXES_HL)
#undef BOXATTN_FWD_BOXES_HL

#define INSTATTN_BWD_BOXES(SUF, CT, ST, CAST, ...)                                                             \
    int instattn_bwd_boxes_##SUF(const CT *value, const int64_t *shapes, const int64_t *lsi, const float *ref, \
                                 int ref_dim, int ref_per_head, const float *offsets, const float *kernel_idx, \
                                 const float *valid_ratios, const float *logits, const CT *grad_out,           \
                                 const CT *grad_mask, int B, int S, int H, int C, int L, int Lq, int k,        \
                                 float *grad_offsets, float *grad_ref_rows, float *grad_logits, void *stream)  \
    {                                                                                                          \
        return launch_bwd_boxes<ST>(BOXES_IN(ST, CAST, 4, 0, 0, k), CAST(grad_out), CAST(grad_mask),           \
                                    BOXES_GRADS);                                                              \
    }
STORAGE_TYPES(INSTATTN_BWD_BOXES)
#undef INSTATTN_BWD_BOXES

#define BOXATTN_BWD_BOXES(SUF, CT, ST, CAST, ...)                                                              \
    int boxattn_bwd_boxes_##SUF(const CT *value, const int64_t *shapes, const int64_t *lsi, const float *ref,  \
                                int ref_dim, int ref_per_head, const float *offsets, int V, int angle_mode,    \
                                const float *kernel_idx, const float *valid_ratios, const float *logits,       \
                                const CT *grad_out, int B, int S, int H, int C, int L, int Lq, int P,          \
                                float *grad_offsets, float *grad_ref_rows, float *grad_logits, void *stream)   \
    {                                                                                                          \
        return launch_bwd_box_boxes<ST>(BOXES_IN(ST, CAST, V, angle_mode, P, 0), CAST(grad_out), BOXES_GRADS); \
    }
STORAGE_TYPES(BOXATTN_BWD_BOXES)
#undef BOXATTN_BWD_BOXES

#define BOXATTN_BWD_BOXES_HL(SUF, CT, ST, CAST, ...)                                                           \
    int boxattn_bwd_boxes_hl_##SUF(const CT *value, const int64_t *shapes, const int64_t *lsi, const float *ref, \
                                   int ref_dim, int ref_per_head, const float *offsets, int V, int angle_mode, \
                                   const float *kernel_idx, const float *valid_ratios, const float *logits,    \
                                   const CT *grad_out, int B, int S, int H, int C, int L, int Lq, int P,       \
                                   float *grad_offsets, float *grad_ref_rows, float *grad_logits, HOST_TABLES, \
                                   void *stream)                                                               \
    {                                                                                                          \
        BoxesIn<ST> in = BOXES_IN(ST, CAST, V, angle_mode, P, 0);                                              \
        in.shapes_host = shapes_host;                                                                          \
        in.lsi_host = lsi_host;                                                                                \
        return launch_bwd_box_boxes_staged<ST>(in, CAST(grad_out), BOXES_GRADS);                               \
    }
STORAGE_TYPES(BOXATTN_BWD_BOXES_HL)
#undef BOXATTN_BWD_BOXES_HL

#define BOXATTN_BWD_BOXES_VALUE(SUF, CT, ST, CAST, ...)                                                           \
    int boxattn_bwd_boxes_value_##SUF(const CT *value, const int64_t *shapes, const int64_t *lsi, const float *ref, \
                                      int ref_dim, int ref_per_head, const float *offsets, int V, int angle_mode, \
                                      const float *kernel_idx, const float *valid_ratios, const float *logits,    \
                                      const CT *grad_out, int B, int S, int H, int C, int L, int Lq, int P,       \
                                      int want, CT *grad_value, void *workspace, size_t workspace_bytes,          \
                                      float *grad_offsets, float *grad_ref_rows, float *grad_logits,              \
                                      void *stream)                                                               \
    {                                                                                                             \
        return launch_bwd_box_boxes_value<ST>(BOXES_IN(ST, CAST, V, angle_mode, P, 0), CAST(grad_out),            \
                                              BOXES_GRADS, want, CAST(grad_value), (float *)workspace,            \
                                              workspace_bytes);                                                   \
    }
STORAGE_TYPES(BOXATTN_BWD_BOXES_VALUE)
#undef BOXATTN_BWD_BOXES_VALUE
#undef BOXES_GRADS
#undef BOXES_IN

// *_fwd_*, and boxattn_fwd_hl_* with the host copies of the level tables (the window-staged kernels' plan)
#define FWD(SUF, CT, ST, CAST, GT, FL)                                                                         \
    int FL##_NAME(fwd_##SUF)(FL##_FWD_PARAMS(CT, GT), void *stream)                                            \
    {                                                                                                          \
        return launch_fwd<ST, FL##_INST>(FL##_FWD_IN(ST, CAST, nullptr, nullptr), FL##_FWD_OUT(ST, CAST), {}); \
    }
#define FWD_HL(SUF, CT, ST, CAST, GT, FL)                                                                      \
    int FL##_NAME(fwd_hl_##SUF)(FL##_FWD_PARAMS(CT, GT), HOST_TABLES, void *stream)                            \
    {                                                                                                          \
        return launch_fwd<ST, FL##_INST>(FL##_FWD_IN(ST, CAST, shapes_host, lsi_host), FL##_FWD_OUT(ST, CAST), \
                                         {});                                                                  \
    }
// *_bwd_*: float32 and float64 accumulate into grad_value itself, the 16-bit types into the float32 grad_value_ws
#define BWD(SUF, CT, ST, CAST, GT, FL)                                                                         \
    int FL##_NAME(bwd_##SUF)(FL##_BWD_PARAMS(CT, GT), void *stream)                                            \
    {                                                                                                          \
        return BWD_ATOMIC(ST, CAST, FL, grad_value, kWantAll);                                                 \
    }
#define BWD_H16(SUF, CT, ST, CAST, GT, FL)                                                                     \
    int FL##_NAME(bwd_##SUF)(FL##_BWD_PARAMS(CT, GT), float *grad_value_ws, void *stream)                      \
    {                                                                                                          \
        return BWD_ATOMIC(ST, CAST, FL, grad_value_ws, kWantAll);                                              \
    }
STORAGE_TYPES_F64(FWD, BOX)
STORAGE_TYPES(FWD_HL, BOX)
STORAGE_F32(BWD, BOX) STORAGE_F64(BWD, BOX) STORAGE_H16(BWD_H16, BOX)
STORAGE_TYPES_F64(FWD, INST)
STORAGE_F32(BWD, INST) STORAGE_F64(BWD, INST) STORAGE_H16(BWD_H16, INST)
#undef BWD_H16
#undef BWD
#undef FWD_HL
#undef FWD
#undef BWD_ATOMIC

#undef INST_BWD_OUT
#undef INST_BWD_IN
#undef INST_BWD_PARAMS
#undef INST_FWD_OUT
#undef INST_FWD_IN
#undef INST_FWD_PARAMS
#undef INST_INST
#undef INST_NAME
#undef BOX_BWD_OUT
#undef BOX_BWD_IN
#undef BOX_BWD_PARAMS
#undef BOX_FWD_OUT
#undef BOX_FWD_IN
#undef BOX_FWD_PARAMS
#undef BOX_INST
#undef BOX_NAME
#undef HOST_TABLES
#undef DIMS_PARAMS
#undef HEAD_PARAMS
#undef STORAGE_TYPES_F64
#undef STORAGE_TYPES
#undef STORAGE_H16
#undef STORAGE_F64
#undef STORAGE_F32
#undef ST_
#undef DIMS

}  // extern "C"
