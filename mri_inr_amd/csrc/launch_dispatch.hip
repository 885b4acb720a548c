// libmsiren.so, host side: the launches of what dispatch.h picks for a model and a call, the *_dev tiling steps and
// the slice pipeline.
//     [tiling] -> encoder -> modulator -> fused SIREN trunk -> [weighted fold]
// Nothing here falls back to the CPU: every function launches HIP kernels on the call's stream or fails.
#include <algorithm>
#include <cstdio>

#include "host_ctx.h"
#include "encoder_modulator.hip.h"
#include "encoder_modulator_f16x3.hip.h"
#include "siren_trunk_f16x3n.hip.h"
#include "siren_trunk_f16x3n_ragged.hip.h"
#include "siren_trunk_f16x3h.hip.h"
#include "siren_trunk_f16x3w.hip.h"
#include "siren_trunk_f32.hip.h"
#include "siren_trunk_f32_jet.hip.h"
#include "siren_trunk_f32_ragged.hip.h"
#include "siren_trunk_x1n.hip.h"
#include "siren_trunk_x1w.hip.h"
#include "tiling.hip.h"
#include "launch_dispatch.h"

namespace msiren {  // the trunk / prologue kernels are compiled in their own translation units (k_*.hip)
MSIREN_TRUNK_INSTANCES(MSIREN_EXTERN_TRUNK)
MSIREN_F32_JET_INSTANCES(MSIREN_EXTERN_TRUNK)
MSIREN_F32_RAGGED_INSTANCES(MSIREN_EXTERN_TRUNK)
MSIREN_F32_JET_RAGGED_INSTANCES(MSIREN_EXTERN_TRUNK)
MSIREN_F16X3N_RAGGED_INSTANCES(MSIREN_EXTERN_TRUNK)
MSIREN_F32_RAGGED_COND_INSTANCES(MSIREN_EXTERN_TRUNK)
MSIREN_PROLOGUE_INSTANCES(MSIREN_EXTERN_PROLOGUE)
}  // namespace msiren

namespace mh {

using msiren::Guard;
using msiren::Kernel;

// the kernel of each row of msiren::kInstances
const void* const kKernels[] = {
#define MSIREN_TRUNK_PTR(fam, ...) (const void*)msiren::siren_trunk_##fam##_kernel<__VA_ARGS__>,
#define MSIREN_PROLOGUE_PTR(fam, ...) (const void*)msiren::fam##_f16x3_kernel<__VA_ARGS__>,
    MSIREN_TRUNK_INSTANCES(MSIREN_TRUNK_PTR) MSIREN_PROLOGUE_INSTANCES(MSIREN_PROLOGUE_PTR)
#undef MSIREN_TRUNK_PTR
#undef MSIREN_PROLOGUE_PTR
};
static_assert(sizeof kKernels / sizeof kKernels[0] == msiren::kNumInstances, "one kernel per instance");

void describe_for_dispatch(msiren_ctx* h) {
    auto& d = h->dh;
    d.precision = h->cfg.precision;
    d.H = h->H, d.HP = h->HP, d.L = h->L, d.Z = h->Z, d.P = h->P;
    d.act = h->cfg.activation, d.res = h->cfg.residual, d.num_cus = h->num_cus;
    d.f16x3_ready = h->f16x3_ready, d.x1_ready = h->x1_ready, d.em_enc = h->em_enc, d.em_mod = h->em_mod;
    static_assert(msiren::WsLds<4>::total(msiren::WS_MAX_L) <= 160 * 1024, "unit images + tables of the deepest supported model must fit the LDS");
    // the depths at which each ring stops fitting (tests/test_dispatch.py and tests/trunk_cases.py model the two flags below by them)
    static_assert(msiren::F16Lds<4>::total(5) <= 160 * 1024 && msiren::F16Lds<4>::total(6) > 160 * 1024, "ring of 4: num_layers <= 5");
    static_assert(msiren::F16Lds<3>::total(11) <= 160 * 1024 && msiren::F16Lds<3>::total(12) > 160 * 1024, "ring of 3: num_layers <= 11");
    d.f16_ring3_fits = msiren::F16Lds<3>::total(h->L) <= 160 * 1024;
    d.f16_ring4_fits = msiren::F16Lds<4>::total(h->L) <= 160 * 1024;
    d.ws_depth_ok = h->L >= msiren::WS_MIN_L && h->L <= msiren::WS_MAX_L;
}

// The exact-fp32 jet trunk's instances (trunk_instances.h: a list of its own, outside msiren::kInstances), in the list's order
struct JetInstance { const void* k; const char* name; int HP, act; };
const JetInstance kJetInstances[] = {
#define MSIREN_JET_ROW(fam, hp, act) {(const void*)msiren::siren_trunk_##fam##_kernel<hp, act>, "siren_trunk_" #fam "_kernel<" #hp "," #act ">", hp, act},
    MSIREN_F32_JET_INSTANCES(MSIREN_JET_ROW)
#undef MSIREN_JET_ROW
};

// The ragged exact-fp32 trunks' instances (lists of their own as well): res = -1 marks the jet form
struct RaggedInstance { const void* k; const char* name; int HP, act, res; };
const RaggedInstance kRaggedInstances[] = {
#define MSIREN_RAGGED_ROW(fam, hp, act, res) {(const void*)msiren::siren_trunk_##fam##_kernel<hp, act, res>, "siren_trunk_" #fam "_kernel<" #hp "," #act "," #res ">", hp, act, res},
#define MSIREN_JET_RAGGED_ROW(fam, hp, act) {(const void*)msiren::siren_trunk_##fam##_kernel<hp, act>, "siren_trunk_" #fam "_kernel<" #hp "," #act ">", hp, act, -1},
    MSIREN_F32_RAGGED_INSTANCES(MSIREN_RAGGED_ROW) MSIREN_F32_JET_RAGGED_INSTANCES(MSIREN_JET_RAGGED_ROW)
#undef MSIREN_RAGGED_ROW
#undef MSIREN_JET_RAGGED_ROW
};

// The split-fp16 ragged trunk's instances and the conditional exact-fp32 ragged trunk behind them (lists of their own, too)
struct F16RaggedInstance { const void* k; const char* name; int act, ring, lfix; };
const F16RaggedInstance kF16RaggedInstances[] = {
#define MSIREN_F16_RAGGED_ROW(fam, act, ring, lfix) {(const void*)msiren::siren_trunk_##fam##_kernel<act, ring, lfix>, "siren_trunk_" #fam "_kernel<" #act "," #ring "," #lfix ">", act, ring, lfix},
    MSIREN_F16X3N_RAGGED_INSTANCES(MSIREN_F16_RAGGED_ROW)
#undef MSIREN_F16_RAGGED_ROW
};
struct RaggedCondInstance { const void* k; const char* name; };
const RaggedCondInstance kRaggedCondInstances[] = {  // [ACT]
#define MSIREN_RAGGED_COND_ROW(fam, act) {(const void*)msiren::siren_trunk_##fam##_kernel<act>, "siren_trunk_" #fam "_kernel<" #act ">"},
    MSIREN_F32_RAGGED_COND_INSTANCES(MSIREN_RAGGED_COND_ROW)
#undef MSIREN_RAGGED_COND_ROW
};

// Launch of kernel `k` with `lds` bytes of dynamic LDS on stream `s` of the handle.  The kernel's LDS limit is raised once per handle.
template <typename P>
int launch_kernel(msiren_ctx* h, int s, const void* k, int64_t grid, int lds, P p) {
    if (lds > 64 * 1024) {
        auto* e = std::begin(h->lds_set);
        while (e != std::end(h->lds_set) && e->k && e->k != k) ++e;
        if (e == std::end(h->lds_set) || e->bytes < lds) {
            HIPCHK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            if (e != std::end(h->lds_set)) *e = {k, lds};
        }
    }
    void* args[] = {&p};
    (void)hipLaunchKernel(k, dim3((unsigned)grid), dim3(256), args, (size_t)lds, h->sc[s].s);  // (as hipLaunchKernelGGL: errors below)
    HIPCHK(hipGetLastError());
    return 0;
}

// Launch of instance `inst` (a row of msiren::kInstances); `named`: the launch is the trunk msiren_last_trunk_kernel and the profile report.
template <typename P>
int launch(msiren_ctx* h, int s, int inst, int64_t grid, int lds, P p, bool named = false) {
    const int rc = launch_kernel(h, s, kKernels[inst], grid, lds, p);
    if (!rc && named) h->last_trunk = msiren::kInstances[inst].name;
    return rc;
}

msiren::TrunkParams make_trunk_params(msiren_ctx* h, const Call& c, const float* mods, int stride, int64_t B, float* out_dev) {
    msiren::TrunkParams p{};
    p.grid = c.cs.Q ? c.cs.coords : h->d_grid;
    p.l0 = h->d_l0;
    p.wp = h->d_wp;
    p.bias = h->d_bias;
    p.wout = h->d_wout;
    p.mods = mods;
    p.out = out_dev;
    p.bout = h->bout;
    p.cg0 = h->cg0;
    p.cg = h->cg;
    p.B = (int)B;
    p.P = c.P(h);
    p.L = h->L;
    p.mod_stride = stride;
    p.chunks = (p.P + 63) / 64;
    p.stamps = nullptr;
    p.plan = c.plan;
    return p;
}

// Pass queue of the persistent trunks.  Workgroup g starts with pass g; every executed pass performs exactly
// one atomicAdd on the counter, so a launch of n passes advances it by n: the counter is never reset, the
// host hands each launch the value it will find (no memset node per call).  The host value moves only once
// the launch has been accepted (queue_launched); a failure in between leaves it where the device counter is.
static int ensure_queue(msiren_ctx* h, int s) {
    auto& c = h->sc[s];
    if (c.queue.p) return 0;
    int rc = ensure(h, c.queue, 256);
    if (rc) return rc;
    // test knob: start the never-reset counter just below 2^32 (or 2^31) to exercise its wrap-around
    const unsigned start = h->queue_start;
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)c.queue.p, (int)start, 16, c.s));          // [0..15]: the pass counter's line
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)((int*)c.queue.p + 16), 0, 48, c.s));     // [16]: the domain guard's flag word; [32]: the slice pipeline's ticket counter
    c.pq.reset(start);
    return 0;
}

static int queue_for_launch(msiren_ctx* h, int s, int64_t npasses, int** counter, unsigned* base) {
    int rc = ensure_queue(h, s);
    if (rc) return rc;
    *counter = (int*)h->sc[s].queue.p;
    *base = h->sc[s].pq.begin(npasses);
    return 0;
}

static int queue_launched(msiren_ctx* h, int s, int rc) {
    if (rc == 0) h->sc[s].pq.commit();
    else h->sc[s].pq.abort();
    return rc;
}

// After a launch whose number of passes only the device knows (black patches skipped): reset the counter.
static int queue_reset_after_plan_launch(msiren_ctx* h, int s, bool by_the_next_kernel) {
    auto& c = h->sc[s];
    if (!c.queue.p) return 0;
    if (!by_the_next_kernel) HIPCHK(hipMemsetAsync(c.queue.p, 0, 4, c.s));  // (else: weighted_fold_kernel's reset_word)
    c.pq.reset(0);
    return 0;
}

// msiren_profile_enable: a HIP event pair around every trunk launch, on the stream it is launched on
int profile_begin(msiren_ctx* h, int s, hipEvent_t* end_event) {
    *end_event = nullptr;
    if (!h->profile) return 0;
    if (h->prof_used == h->prof_events.size()) {
        hipEvent_t a, b;
        HIPCHK(hipEventCreate(&a));
        HIPCHK(hipEventCreate(&b));
        h->prof_events.push_back({a, b, -1, 0});
    }
    HIPCHK(hipEventRecord(h->prof_events[h->prof_used].a, h->sc[s].s));
    *end_event = h->prof_events[h->prof_used].b;
    h->prof_used++;
    return 0;
}

// closes the pair profile_begin opened: the launch in between was h->last_trunk (or `name`: not a trunk) over `coords` coordinates
int profile_end(msiren_ctx* h, int s, hipEvent_t end_event, int64_t coords, const char* name) {
    if (!end_event) return 0;
    HIPCHK(hipEventRecord(end_event, h->sc[s].s));
    const bool trunk = !name;
    if (trunk) name = h->last_trunk;
    auto& r = h->prof_events[h->prof_used - 1];
    int k = 0;
    for (; k < (int)h->prof_kernels.size(); ++k)
        if (h->prof_kernels[k].name == name) break;
    if (k == (int)h->prof_kernels.size()) {
        h->prof_kernels.emplace_back();
        h->prof_kernels.back().name = name;
        h->prof_kernels.back().trunk = trunk;
    }
    r.kernel = k;
    r.coords = coords;
    return 0;
}

// the flag word a 16-bit trunk launch writes its number to: behind the stream's pass counter line, or the host's (Guard::host)
static int* guard_word(msiren_ctx* h, const msiren::TrunkPick& t, int* pass_counter) {
    return t.guard == Guard::host ? h->status_dev + 8 : pass_counter + 16;
}

// weight-stationary trunk (siren_trunk_f16x3w.hip.h): passes of 2..4 units, laid out by ws_schedule
static int launch_trunk_f16x3w(msiren_ctx* h, const Call& c, const msiren::TrunkPick& t, const float* mods_dev, int64_t B, float* out_dev) {
    msiren::TrunkWsParams p{};
    if (!h->d_dump) HIPCHK(hipMalloc((void**)&h->d_dump, 256 * sizeof(float)));
    p.dump = h->d_dump;
    p.s0t = c.cs.Q ? c.cs.table : h->d_s0t;
    p.wp = (const _Float16*)h->d_wp16n;
    p.bias = h->d_bias16;
    p.wout = h->d_wout16;
    p.mods = mods_dev;
    p.out = out_dev;
    for (int i = 0; i < 16; ++i) p.mscale[i] = h->mscale16[i];
    p.bout = h->bout;
    p.cg0 = h->cg0;
    p.cg = h->cg;
    p.B = (int)B;
    p.P = c.P(h);
    p.L = h->L;
    p.plan = c.plan;
    const int upp = (p.P + 31) / 32;
    const int64_t units = B * upp;
    if (units > 0x3fffffffLL) return fail(MSIREN_E_INVALID, "batch too large for one launch: B=%lld", (long long)B);
    p.units_per_patch = upp;
    p.unit_base = 0;
    p.total_units = (int)units;
    {   // unit / upp as a multiply-high: k = 30 + ceil(log2 upp), m = ceil(2^k / upp) (exact for units < 2^30)
        int lg = 0;
        while ((1 << lg) < upp) ++lg;
        p.div_k = 30 + lg;
        p.div_m = (unsigned)(((1ULL << p.div_k) + (unsigned)upp - 1) / (unsigned)upp);
    }
    // small batches: one pass of 2 units per workgroup (latency); otherwise one workgroup per CU
    const int grid = (int)std::min<int64_t>(h->num_cus, (units + 1) / 2);
    const msiren::WsSchedule sch = msiren::ws_schedule(units, grid);
    int rc = queue_for_launch(h, c.stream, sch.npasses(), &p.pass_counter, &p.pass_base);
    if (rc) return rc;
    p.status = guard_word(h, t, p.pass_counter);
    p.status_val = (int)h->range_epoch;
    return queue_launched(h, c.stream, launch(h, c.stream, t.inst, grid, msiren::WsLds<4>::total(h->L), p, true));
}

// register-resident trunk (siren_trunk_f16x3n.hip.h), or its half-unit form (siren_trunk_f16x3h.hip.h: 16 coordinates per wave).
// Measured and dropped, twice: running the ragged last round of a big launch (one 320x320 slice = 7.03 rounds of 256 x 4 waves) as
// half-units so that the main launch's workgroups finish together -- (1) as a second launch behind the main one on the same stream:
// 0.306 vs 0.295 ms per slice; (2) queued beside it on the handle's idle second stream (event fork / join, no launch gap): 0.315 vs
// 0.289 ms.  A half-unit pass on an otherwise idle chip is not half a round (its weight-fragment reads are those of a full unit;
// prologue and layer 0 do not shrink), and the cross-stream dependency costs more than the tail it removes.
static int launch_trunk_f16x3n(msiren_ctx* h, const Call& c, const msiren::TrunkPick& t, const float* mods_dev, int64_t B, float* out_dev) {
    msiren::TrunkF16Params p{};
    p.grid = c.cs.Q ? c.cs.coords : h->d_grid;
    p.l0 = h->d_l0;
    p.s0t = c.cs.Q ? c.cs.table : h->d_s0t;
    p.wp = (const _Float16*)h->d_wp16n;
    p.bias = h->d_bias16;
    p.wout = h->d_wout16;
    p.mods = mods_dev;
    p.out = out_dev;
    for (int i = 0; i < 16; ++i) p.winv[i] = h->mscale16[i];
    p.bout = h->bout;
    p.cg0 = h->cg0;
    p.cg = h->cg;
    p.B = (int)B;
    p.P = c.P(h);
    p.L = h->L;
    p.plan = c.plan;
    if (B * ((p.P + 31) / 32) > 0x3fffffffLL) return fail(MSIREN_E_INVALID, "batch too large for one launch: B=%lld", (long long)B);
    p.units_per_patch = t.half ? (p.P + 15) / 16 : (p.P + 31) / 32;
    p.unit_base = 0;
    p.total_units = (int)(B * p.units_per_patch);
    // the pass queue: workgroup g starts with pass g of 4 units, further passes come from the counter
    const int64_t passes = ((int64_t)p.total_units + 3) / 4;
    const int grid = (int)std::min<int64_t>(h->num_cus, passes);
    int rc = queue_for_launch(h, c.stream, passes, &p.pass_counter, &p.pass_base);
    if (rc) return rc;
    p.status = guard_word(h, t, p.pass_counter);
    p.status_val = (int)h->range_epoch;
    const int lds = t.ring == 4 ? msiren::F16Lds<4>::total(h->L) : msiren::F16Lds<3>::total(h->L);
    return queue_launched(h, c.stream, launch(h, c.stream, t.inst, grid, lds, p, true));
}

// single-product 16-bit trunk, H = 512: weight-stationary (siren_trunk_x1w.hip.h; it lays its passes out itself: x1w_schedule,
// 4-unit passes and a last round of 2-unit ones) or register-resident (siren_trunk_x1n.hip.h)
static int launch_trunk_x1(msiren_ctx* h, const Call& c, const msiren::TrunkPick& t, const float* mods_dev, int64_t B, float* out_dev) {
    const bool ws = msiren::kInstances[t.inst].family == Kernel::x1w;
    msiren::TrunkX1Params p{};
    p.s0t = c.cs.Q ? c.cs.table : h->d_s0t512;
    p.wp = (const unsigned short*)(ws ? h->d_wpx1w : h->d_wpx1n);
    p.bias32 = h->d_bias32x1;
    p.wout = (const _Float16*)h->d_woutx1;
    p.mods = mods_dev;
    p.out = out_dev;
    for (int i = 0; i < 64; ++i) p.winv[i] = h->winvx1[i];
    p.bout = h->bout;
    p.cg0 = h->cg0;
    p.cg = h->cg;
    p.B = (int)B;
    p.P = c.P(h);
    p.L = h->L;
    p.units_per_patch = (p.P + 31) / 32;
    const int64_t units = B * p.units_per_patch;
    if (units > 0x7fffffffLL) return fail(MSIREN_E_INVALID, "batch too large for one launch: B=%lld", (long long)B);
    p.total_units = (int)units;
    p.plan = c.plan;
    const int grid = t.balanced ? msiren::x1w_balanced_grid(units, h->num_cus) : (int)std::min<int64_t>(h->num_cus, (units + 3) / 4);
    int64_t npasses = (units + 3) / 4;
    if (ws) {
        const msiren::X1wSchedule sch = msiren::x1w_schedule(units, grid);
        npasses = (int64_t)sch.n4 + sch.n2;
    }
    int rc = queue_for_launch(h, c.stream, npasses, &p.pass_counter, &p.pass_base);
    if (rc) return rc;
    p.status = p.pass_counter + 16;  // the stream's flag word, behind the pass counter's line (the domain guard of the fp16 modulation table)
    p.status_val = (int)h->range_epoch;
    const int lds = ws ? msiren::X1wLds::total(h->L) : msiren::X1nLds<3>::total(h->L);
    return queue_launched(h, c.stream, launch(h, c.stream, t.inst, grid, lds, p, true));
}

// the fp32 trunks read modulation rows as float4: where dim_hidden is not its padded width, zero-padded copies in the stream's scratch
static int pad_mods(msiren_ctx* h, const Call& c, int64_t B, const float** mods, int* stride) {
    if (h->HP == h->H) return 0;
    auto& sc = h->sc[c.stream];
    int rc = ensure(h, sc.modpad, (size_t)h->L * B * h->HP * sizeof(float));
    if (rc) return rc;
    const int64_t n = (int64_t)h->L * B * h->HP;
    hipLaunchKernelGGL(msiren::pad_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sc.s,
                       *mods, (float*)sc.modpad.p, (int64_t)h->L * B, h->H, h->HP);
    HIPCHK(hipGetLastError());
    *mods = (const float*)sc.modpad.p;
    *stride = h->HP;
    return 0;
}

// exact-fp32 trunk: one workgroup per 64 coordinates of a patch
static int launch_trunk_f32(msiren_ctx* h, const Call& c, int inst, const float* mods_dev, int64_t B, float* out_dev) {
    const int chunks = (c.P(h) + 63) / 64;
    if (B * (int64_t)chunks > 0x7fffffffLL) return fail(MSIREN_E_INVALID, "batch too large for one launch: B=%lld", (long long)B);
    const float* mods = mods_dev;
    int stride = h->H, rc;
    if ((rc = pad_mods(h, c, B, &mods, &stride))) return rc;
    const msiren::TrunkParams p = make_trunk_params(h, c, mods, stride, B, out_dev);
    const int lds = h->HP * 256 + h->HP * 16;  // X image + layer-0 rows
    hipEvent_t e1 = nullptr;
    if ((rc = profile_begin(h, c.stream, &e1)) || (rc = launch(h, c.stream, inst, B * chunks, lds, p, true))) return rc;
    return profile_end(h, c.stream, e1, B * c.P(h));
}

int jet_supported(msiren_ctx* h) {
    if (h->HP > 256)
        return fail(MSIREN_E_INVALID, "the gradient calls need dim_hidden <= 256 (value and two tangents of 32 coordinates fill the LDS at 256), got %d", h->H);
    if (h->cfg.residual) return fail(MSIREN_E_INVALID, "the gradient calls do not support residual=1");
    return 0;
}

// Exact-fp32 trunk with its spatial gradient (siren_trunk_f32_jet.hip.h): one workgroup per 32 coordinates of a patch, on handles of
// every precision (the packed fp32 weights are on the device for every H <= 256).  Not msiren_last_trunk_kernel's trunk; the profile
// report names it like layer0_table_kernel, outside the trunk totals.
int launch_trunk_f32_jet(msiren_ctx* h, const Call& c, const float* mods_dev, int64_t B, float* out_dev, float* grad_dev, float gscale) {
    int rc = jet_supported(h);
    if (rc || B == 0) return rc;
    const int chunks = (c.P(h) + 31) / 32;
    if (B * (int64_t)chunks > 0x7fffffffLL) return fail(MSIREN_E_INVALID, "batch too large for one launch: B=%lld", (long long)B);
    const int act = h->cfg.activation == MSIREN_ACT_MORLET ? 1 : 0;
    const JetInstance* ji = std::begin(kJetInstances);
    while (ji != std::end(kJetInstances) && (ji->HP != h->HP || ji->act != act)) ++ji;
    if (ji == std::end(kJetInstances)) return fail(MSIREN_E_INVALID, "dim_hidden=%d (padded %d) is not supported by the gradient trunk", h->H, h->HP);
    const float* mods = mods_dev;
    int stride = h->H;
    if ((rc = pad_mods(h, c, B, &mods, &stride))) return rc;
    msiren::TrunkJetParams p{make_trunk_params(h, c, mods, stride, B, out_dev), grad_dev, gscale};
    p.t.chunks = chunks;
    hipEvent_t e1 = nullptr;
    if ((rc = profile_begin(h, c.stream, &e1)) || (rc = launch_kernel(h, c.stream, ji->k, B * chunks, msiren::jet_lds_bytes(h->HP), p))) return rc;
    return profile_end(h, c.stream, e1, B * c.P(h), ji->name);
}

// ---- one coordinate set per patch (siren_trunk_f32_ragged.hip.h) ----
// Every index of the launch in 32 bits: coordinates and patches below 2^30 (the unit checks above are the model), the grid of
// reps * (ceil(T / chunk) + NP) workgroups and the reps * T outputs below 2^31.
int ragged_check(const RaggedSet& r, int chunk) {
    if (r.T < 0 || r.NP < 0 || r.reps < 1 || r.T > 0x3fffffffLL || r.NP > 0x3fffffffLL)
        return fail(MSIREN_E_INVALID, "per-patch coordinate sets: %lld coordinates over %lld patches are too many for one call (2^30 - 1 each)", (long long)r.T, (long long)r.NP);
    const int64_t bound = (r.T + chunk - 1) / chunk + r.NP;
    if (r.reps * bound > 0x7fffffffLL || r.reps * r.T > 0x7fffffffLL || r.reps * r.NP > 0x7fffffffLL)
        return fail(MSIREN_E_INVALID, "per-patch coordinate sets: %lld x (%lld coordinates, %lld patches) are too many for one call", (long long)r.reps, (long long)r.T, (long long)r.NP);
    return 0;
}

// item table, then the trunk over the upper bound of items (the device-side total sends the surplus workgroups home).  grad_dev null: values
// only (siren_trunk_f32_ragged_kernel, what the fp32 trunk takes); else the jet (jet_supported).  The profile report names the kernels like
// the jet's, outside the trunk totals; msiren_last_trunk_kernel does not.
static int launch_ragged(msiren_ctx* h, const Call& c, const RaggedSet& r, const float* mods_dev, float* out_dev, float* grad_dev, float gscale) {
    const int chunk = grad_dev ? 32 : 64;
    int rc = grad_dev ? jet_supported(h) : 0;
    if (rc || (rc = ragged_check(r, chunk))) return rc;
    if (r.T == 0 || r.NP == 0) return 0;
    if (!grad_dev && !out_dev) return fail(MSIREN_E_INVALID, "null output");
    const int act = h->cfg.activation == MSIREN_ACT_MORLET ? 1 : 0, res = grad_dev ? -1 : h->cfg.residual ? 1 : 0;
    const RaggedInstance* ri = std::begin(kRaggedInstances);
    while (ri != std::end(kRaggedInstances) && (ri->HP != h->HP || ri->act != act || ri->res != res)) ++ri;
    if (ri == std::end(kRaggedInstances)) return fail(MSIREN_E_INVALID, "dim_hidden=%d (padded %d) is not supported by the exact-fp32 trunks", h->H, h->HP);
    const float* mods = mods_dev;
    int stride = h->H;
    if ((rc = pad_mods(h, c, r.rows, &mods, &stride))) return rc;
    msiren::TrunkRaggedParams p{};
    Call plain = c;  // (the coordinates and the plan reach the kernel through the ragged fields)
    plain.cs = CoordSet{};
    plain.plan = nullptr;
    p.t = make_trunk_params(h, plain, mods, stride, r.rows, out_dev);
    p.t.grid = r.coords;
    p.offsets = r.offsets, p.first = r.items, p.pos = r.pos, p.grad = grad_dev, p.gscale = gscale;
    p.NP = (int)r.NP, p.T = (int)r.T, p.reps = (int)r.reps;
    p.bound = (int)((r.T + chunk - 1) / chunk + r.NP);
    hipStream_t st = h->sc[c.stream].s;
    if (grad_dev) hipLaunchKernelGGL(msiren::ragged_items_kernel<32>, dim3(1), dim3(256), 0, st, r.offsets, p.NP, p.T, r.items);
    else hipLaunchKernelGGL(msiren::ragged_items_kernel<64>, dim3(1), dim3(256), 0, st, r.offsets, p.NP, p.T, r.items);
    HIPCHK(hipGetLastError());
    const int lds = grad_dev ? msiren::jet_lds_bytes(h->HP) : h->HP * 256 + h->HP * 16;
    hipEvent_t e1 = nullptr;
    if ((rc = profile_begin(h, c.stream, &e1)) || (rc = launch_kernel(h, c.stream, ri->k, r.reps * p.bound, lds, p))) return rc;
    return profile_end(h, c.stream, e1, r.reps * r.T, ri->name);
}

int launch_trunk_f32_ragged(msiren_ctx* h, const Call& c, const RaggedSet& r, const float* mods_dev, float* out_dev) {
    return launch_ragged(h, c, r, mods_dev, out_dev, nullptr, 1.f);
}

int launch_trunk_f32_jet_ragged(msiren_ctx* h, const Call& c, const RaggedSet& r, const float* mods_dev, float* out_dev, float* grad_dev, float gscale) {
    if (!grad_dev) return fail(MSIREN_E_INVALID, "null gradient output");
    return launch_ragged(h, c, r, mods_dev, out_dev, grad_dev, gscale);
}

// The handle's own trunk arithmetic over per-patch sets (siren_trunk_f16x3n_ragged.hip.h), beside launch_ragged: the item table in chunks of
// 32, the trunk over the bound reps * (ceil(T / 32) + NP) of units with the stream's pass counter -- how many of them are passes only the
// device knows (first[NP]), so the counter is reset behind the launch as behind a plan launch -- then the exact-fp32 ragged trunk as the
// conditional launch of the domain guard, with the flag word and number launch_trunk_f32_cond uses: a flagged call holds the exact path's
// bits, on the synchronous and the _dev forms alike.  Named in the profile report like the other ragged kernels; not msiren_last_trunk_kernel.
int launch_trunk_ragged_native(msiren_ctx* h, const Call& c, const RaggedSet& r, const float* mods_dev, float* out_dev) {
    const msiren::RaggedNativePick pk = msiren::ragged_native_pick(h->dh);
    if (!pk.native) return launch_trunk_f32_ragged(h, c, r, mods_dev, out_dev);
    int rc = ragged_check(r, 32);
    if (rc) return rc;
    if (r.T == 0 || r.NP == 0) return 0;
    if (!out_dev) return fail(MSIREN_E_INVALID, "null output");
    if (r.rows < 1 || r.rows > 0x7fffffffLL) return fail(MSIREN_E_INVALID, "per-patch coordinate sets: %lld modulation rows", (long long)r.rows);
    const int act = h->cfg.activation == MSIREN_ACT_MORLET ? 1 : 0;
    const F16RaggedInstance* fi = std::begin(kF16RaggedInstances);
    while (fi != std::end(kF16RaggedInstances) && (fi->act != act || fi->ring != pk.ring || fi->lfix != pk.lfix)) ++fi;
    if (fi == std::end(kF16RaggedInstances)) return fail(MSIREN_E_INVALID, "no split-fp16 ragged trunk for num_layers=%d", h->L);
    msiren::TrunkF16RaggedParams p{};
    p.t.l0 = h->d_l0;
    p.t.wp = (const _Float16*)h->d_wp16n;
    p.t.bias = h->d_bias16;
    p.t.wout = h->d_wout16;
    p.t.mods = mods_dev;
    p.t.out = out_dev;
    for (int i = 0; i < 16; ++i) p.t.winv[i] = h->mscale16[i];
    p.t.bout = h->bout;
    p.t.cg0 = h->cg0;
    p.t.cg = h->cg;
    p.t.B = (int)r.rows;
    p.t.L = h->L;
    p.r = {r.coords, r.offsets, r.items, r.pos, (int)r.NP, (int)r.T, (int)r.reps};
    const int64_t bound = r.reps * ((r.T + 31) / 32 + r.NP), passes = (bound + 3) / 4;  // (< 2^31: ragged_check)
    hipStream_t st = h->sc[c.stream].s;
    hipLaunchKernelGGL(msiren::ragged_items_kernel<32>, dim3(1), dim3(256), 0, st, r.offsets, (int)r.NP, (int)r.T, r.items);
    HIPCHK(hipGetLastError());
    if (++h->range_epoch == 0) h->range_epoch = 1;  // this launch's number (never 0: the flag word's rest state)
    hipEvent_t e1 = nullptr;
    if ((rc = profile_begin(h, c.stream, &e1)) || (rc = queue_for_launch(h, c.stream, passes, &p.t.pass_counter, &p.t.pass_base))) return rc;
    p.t.status = p.t.pass_counter + 16;
    p.t.status_val = (int)h->range_epoch;
    const int lds = pk.ring == 4 ? msiren::F16Lds<4>::total(h->L) : msiren::F16Lds<3>::total(h->L);
    const int grid = (int)std::min<int64_t>(h->num_cus, passes);
    if ((rc = queue_launched(h, c.stream, launch_kernel(h, c.stream, fi->k, grid, lds, p)))) return rc;
    if ((rc = queue_reset_after_plan_launch(h, c.stream, false)) || (rc = profile_end(h, c.stream, e1, r.reps * r.T, fi->name))) return rc;
    // the conditional launch: the exact-fp32 value kernel over the same sets (items of 64: its own prefix, behind the native trunk on the stream)
    msiren::TrunkRaggedParams q{};
    Call plain = c;
    plain.cs = CoordSet{};
    plain.plan = nullptr;
    q.t = make_trunk_params(h, plain, mods_dev, h->H, r.rows, out_dev);  // (H = 256 = HP: no padding of the rows)
    q.t.grid = r.coords;
    q.t.cond = p.t.status;
    q.t.cond_val = p.t.status_val;
    q.t.host_flag = h->status_dev;
    q.offsets = r.offsets, q.first = r.items, q.pos = r.pos, q.gscale = 1.f;
    q.NP = (int)r.NP, q.T = (int)r.T, q.reps = (int)r.reps;
    q.bound = (int)((r.T + 63) / 64 + r.NP);
    hipLaunchKernelGGL(msiren::ragged_items_kernel<64>, dim3(1), dim3(256), 0, st, r.offsets, q.NP, q.T, r.items);
    HIPCHK(hipGetLastError());
    if ((rc = profile_begin(h, c.stream, &e1)) || (rc = launch_kernel(h, c.stream, kRaggedCondInstances[act].k, r.reps * q.bound, 256 * 256 + 256 * 16, q))) return rc;
    return profile_end(h, c.stream, e1, 0, kRaggedCondInstances[act].name);
}

// Behind every split-fp16 trunk launch, on the same stream: the exact-fp32 trunk over the same batch as a conditional launch
// (siren_trunk_f32_cond_kernel: 32 KB of LDS, <= 96 registers, so that it fits beside a register-resident trunk of the other
// stream) -- its <= 2 workgroups per CU read the stream's flag word and leave unless the f16x3 launch
// wrote its number there (a scaled modulation beyond fp16, a NaN / inf).  So the output buffer always holds what the
// reference's fp32 arithmetic computes (modulated_siren.py:215-233), on the asynchronous API as well; the flag in host memory is
// informational (msiren_range_events).
int launch_trunk_f32_cond(msiren_ctx* h, const Call& c, const float* mods_dev, int64_t B, float* out_dev, const int* flag_word, unsigned flag_val) {
    const int cpp = (c.P(h) + 31) / 32;
    if (B * (int64_t)cpp > 0x7fffffffLL) return fail(MSIREN_E_INVALID, "batch too large for one launch: B=%lld", (long long)B);
    msiren::TrunkParams p = make_trunk_params(h, c, mods_dev, h->H, B, out_dev);  // (f16x3 needs H = 256 = HP: no padding of the rows)
    p.cond = flag_word ? flag_word : (const int*)h->sc[c.stream].queue.p + 16;
    p.cond_val = (int)(flag_word ? flag_val : h->range_epoch);
    p.items = (int)(B * cpp);
    p.host_flag = h->status_dev;
    const int act = h->cfg.activation == MSIREN_ACT_MORLET ? 1 : 0;
    return launch(h, c.stream, msiren::instance(Kernel::f32_cond, act), std::min<int64_t>(p.items, (int64_t)h->num_cus), 0, p);
}

int launch_trunk(msiren_ctx* h, const Call& c, const float* mods_dev, int64_t B, float* out_dev) {
    if (B == 0) return 0;
    if (c.trunk_wait) HIPCHK(hipStreamWaitEvent(h->sc[c.stream].s, c.trunk_wait, 0));
    const msiren::TrunkPick t = msiren::pick_trunk(h->dh, c.mode, B);
    if (t.inst < 0) return fail(MSIREN_E_INVALID, "dim_hidden=%d (padded %d) is not supported by the trunks", h->H, h->HP);
    const Kernel family = msiren::kInstances[t.inst].family;
    if (family == Kernel::f32) return launch_trunk_f32(h, c, t.inst, mods_dev, B, out_dev);
    hipEvent_t e1 = nullptr;
    int rc = profile_begin(h, c.stream, &e1);
    if (rc) return rc;
    if (t.guard != Guard::none && ++h->range_epoch == 0) h->range_epoch = 1;  // this launch's number (never 0: the flag word's rest state; unsigned: wraps)
    if (family == Kernel::f16x3w) rc = launch_trunk_f16x3w(h, c, t, mods_dev, B, out_dev);
    else if (family == Kernel::x1w || family == Kernel::x1n) rc = launch_trunk_x1(h, c, t, mods_dev, B, out_dev);
    else rc = launch_trunk_f16x3n(h, c, t, mods_dev, B, out_dev);
    if (rc || (rc = profile_end(h, c.stream, e1, B * c.P(h)))) return rc;
    if (t.guard == Guard::host) {  // (the caller looks at the flag in host memory behind its wait for the stream)
        *c.hc = {mods_dev, B, out_dev, h->range_epoch, true};
        return 0;
    }
    if (t.guard == Guard::f32_512) {  // H = 512: the 64-coordinate exact-fp32 trunk as the conditional launch (its workgroups read the flag word and leave)
        const int chunks = (c.P(h) + 63) / 64;
        if (B * (int64_t)chunks > 0x7fffffffLL) return fail(MSIREN_E_INVALID, "batch too large for one launch: B=%lld", (long long)B);
        msiren::TrunkParams p = make_trunk_params(h, c, mods_dev, h->H, B, out_dev);
        p.cond = (const int*)h->sc[c.stream].queue.p + 16;
        p.cond_val = (int)h->range_epoch;
        p.host_flag = h->status_dev;
        const int act = h->cfg.activation == MSIREN_ACT_MORLET ? 1 : 0, res = h->cfg.residual ? 1 : 0;
        return launch(h, c.stream, msiren::instance(Kernel::f32, 512, act, res), B * chunks, 512 * 256 + 512 * 16, p);  // (not named: the profile names the 16-bit trunk, not its stand-in)
    }
    return t.guard == Guard::f32_cond ? launch_trunk_f32_cond(h, c, mods_dev, B, out_dev) : 0;
}

// One Linear layer over the batch on the matrix cores: 16 x 16 output tiles (latency sizes) or 32 x 32 (throughput sizes; dispatch.h)
static int launch_linear(msiren_ctx* h, const Call& c, const msiren::ModulatorMfmaParams& mp) {
    hipStream_t s = h->sc[c.stream].s;
    if (msiren::linear_tiled(mp.B, mp.H, mp.Z, mp.Kh)) {
        dim3 grid((unsigned)((mp.B + 31) / 32), (unsigned)((mp.H + 31) / 32));
        hipLaunchKernelGGL((msiren::linear_mfma_tile_kernel<2, 2>), grid, dim3(256), 0, s, mp);
    } else {
        dim3 grid((unsigned)((mp.B + 15) / 16), (unsigned)(mp.H / 16));
        hipLaunchKernelGGL(msiren::modulator_layer_mfma_kernel, grid, dim3(256), 0, s, mp);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// encoder tail + Modulator in ONE launch (plus the conv kernel in front when tiles are given): split-fp16 arithmetic,
// a row block of 16 patches per workgroup through every layer (encoder_modulator_f16x3.hip.h).
//   tiles -> [z_out] -> [mods]     (tiles_dev given)        z_in -> mods     (tiles_dev null)
static int launch_prologue_f16x3(msiren_ctx* h, const Call& c, const float* tiles_dev, const float* z_in, int64_t B, float* z_out, float* mods_dev) {
    if (B == 0) return 0;
    auto& sc = h->sc[c.stream];
    const int64_t nblk = (B + msiren::EM_ROWS - 1) / msiren::EM_ROWS, rows16 = nblk * msiren::EM_ROWS;
    if (nblk > 0x7fffffffLL) return fail(MSIREN_E_INVALID, "batch too large for one launch: B=%lld", (long long)B);
    const int nph = h->H == 256 ? 2 : 4;
    int rc;
    msiren::EmTailParams p{};
    if (tiles_dev) {
        if ((rc = ensure(h, sc.feat, (size_t)rows16 * 2048 * 4 + (size_t)rows16 * 4 + msiren::EM_MAX_DEPTH * 2048))) return rc;  // (+ padding: conv3's B ring prefetches past the end)
        p.feat = (const msiren::em_u4*)sc.feat.p;
        p.feat_inv = (const float*)((const char*)sc.feat.p + (size_t)rows16 * 2048 * 4 + msiren::EM_MAX_DEPTH * 2048);
        msiren::EncoderParams enc = h->enc;
        enc.plan = c.plan;
        float* const finv = (float*)((char*)sc.feat.p + (size_t)rows16 * 2048 * 4 + msiren::EM_MAX_DEPTH * 2048);
        hipLaunchKernelGGL(msiren::encoder_conv_f16x3_kernel<1>, dim3((unsigned)B), dim3(256), 0, sc.s, enc, tiles_dev, (msiren::em_u4*)sc.feat.p, finv);
        HIPCHK(hipGetLastError());
    }
    if (mods_dev) {
        if ((rc = ensure(h, sc.cscratch, (size_t)nblk * std::max(1, h->L - 1) * nph * 512 * 16))) return rc;
        p.cscratch = (msiren::em_f4*)sc.cscratch.p;
    }
    p.wstream = (const msiren::em_u4*)h->d_emw;
    p.bias = h->d_embias;
    p.z_in = z_in;
    p.z_out = z_out;
    p.mods = mods_dev;
    p.winv_c3 = h->em_winv_c3;
    p.winv_fc = h->em_winv_fc;
    for (int l = 0; l < 64; ++l) {
        p.winv_z[l] = h->em_winv_z[l];
        p.winv_h[l] = h->em_winv_h[l];
    }
    p.B = (int)B;
    p.L = h->L;
    p.wave_stride = h->em_wave_stride;
    p.zp_start = h->em_zp_start;
    p.count = c.plan;
    p.row_blocks = (int)nblk;
    const msiren::ProloguePick pk = msiren::pick_prologue(h->dh, c.mode, tiles_dev ? (mods_dev ? 3 : 1) : 2, nblk);
    if (pk.pf_blocks) {
        p.pf_blocks = pk.pf_blocks;
        p.pf_lines = (unsigned)(((size_t)h->em_wave_stride * 4 * 16 / 8 + 1023) / 1024);
    }
    const int lds = nph == 2 ? msiren::em_tail_lds_bytes<2, 2>() : msiren::em_tail_lds_bytes<4, 1>();
    if ((rc = launch(h, c.stream, pk.inst, nblk + p.pf_blocks, lds, p))) return rc;
    h->last_prologue = msiren::kInstances[pk.inst].name;
    return 0;
}

int launch_modulator(msiren_ctx* h, const Call& c, const float* z_dev, int64_t B, float* mods_dev) {
    if (B == 0) return 0;
    if (!h->have_modulator) return fail(MSIREN_E_STATE, "modulator.* weights were not loaded");
    if (h->em_mod) return launch_prologue_f16x3(h, c, nullptr, z_dev, B, nullptr, mods_dev);
    h->last_prologue = "";  // (the per-layer exact-fp32 launches)
    size_t off = 0;
    static_assert(msiren::kModRows == msiren::MOD_ROWS, "dispatch.h sizes the VALU Modulator's LDS from the kernel's rows per workgroup");
    const bool mfma_ok = msiren::modulator_mfma(h->H, h->Z);
    for (int l = 0; l < h->L && mfma_ok; ++l) {
        const int Kh = (l == 0 ? 0 : h->H);
        msiren::ModulatorMfmaParams mp{};
        mp.w = h->d_modw_rm + off;
        mp.bias = h->d_modb + (size_t)l * h->H;
        mp.hprev = l == 0 ? nullptr : mods_dev + (size_t)(l - 1) * B * h->H;
        mp.z = z_dev;
        mp.out = mods_dev + (size_t)l * B * h->H;
        mp.B = (int)B;
        mp.H = h->H;
        mp.Z = h->Z;
        mp.Kh = Kh;
        mp.act = msiren::LIN_ACT_RELU;
        mp.count = c.plan;
        int rc = launch_linear(h, c, mp);
        if (rc) return rc;
        off += (size_t)(Kh + h->Z) * h->H;
    }
    if (mfma_ok) return 0;
    off = 0;  // (plain launches: at most 64 KB of LDS, static + dynamic -- msiren_create refuses the shapes past it, dispatch.h)
    for (int l = 0; l < h->L; ++l) {
        const int Kh = (l == 0 ? 0 : h->H);
        msiren::ModulatorLayerParams mp{};
        mp.wt = h->d_modw + off;
        mp.bias = h->d_modb + (size_t)l * h->H;
        mp.hprev = l == 0 ? nullptr : mods_dev + (size_t)(l - 1) * B * h->H;
        mp.z = z_dev;
        mp.out = mods_dev + (size_t)l * B * h->H;
        mp.B = (int)B;
        mp.H = h->H;
        mp.Z = h->Z;
        mp.Kh = Kh;
        mp.count = c.plan;
        dim3 grid((unsigned)((B + msiren::MOD_ROWS - 1) / msiren::MOD_ROWS), (unsigned)((h->H + 63) / 64));
        const size_t lds = (size_t)msiren::MOD_ROWS * (Kh + h->Z) * sizeof(float);
        hipLaunchKernelGGL(msiren::modulator_layer_kernel, grid, dim3(256), lds, h->sc[c.stream].s, mp);
        HIPCHK(hipGetLastError());
        off += (size_t)(Kh + h->Z) * h->H;
    }
    return 0;
}

int launch_encoder(msiren_ctx* h, const Call& c, const float* tiles_dev, int64_t B, float* z_dev) {
    if (B == 0) return 0;
    if (!h->have_encoder) return fail(MSIREN_E_STATE, "encoder.* weights were not loaded");
    if (h->em_enc) return launch_prologue_f16x3(h, c, tiles_dev, nullptr, B, z_dev, nullptr);
    h->last_prologue = "";  // (the per-layer exact-fp32 launches)
    auto& sc = h->sc[c.stream];
    msiren::EncoderParams enc = h->enc;
    enc.plan = c.plan;
    // Shapes the MFMA Linear kernels do not take (latent_dim not a multiple of 16): one fused per-tile kernel.  (Until round 6 batches
    // below 48 tiles took it as well, for two launches less -- but its VALU sums run in another order than the MFMA kernels', so an
    // fp32 handle's latent depended in the last bits on the size of the batch a tile came in; the split-fp16 prologue never had that seam.)
    if (msiren::encoder_fused_valu(h->Z)) {
        hipLaunchKernelGGL(msiren::encoder_kernel, dim3((unsigned)B), dim3(256), 0, sc.s, enc, tiles_dev, z_dev);
        HIPCHK(hipGetLastError());
        return 0;
    }
    // conv1+conv2 per tile, then conv3 == Linear(2048, 64) and Linear(64, Z) as GEMMs over the batch
    int rc = ensure(h, sc.feat, (size_t)B * (2048 + 64) * sizeof(float));
    if (rc) return rc;
    float* feat = (float*)sc.feat.p;
    float* a3 = feat + (size_t)B * 2048;
    hipLaunchKernelGGL(msiren::encoder_conv_kernel, dim3((unsigned)B), dim3(256), 0, sc.s, enc, tiles_dev, feat);
    HIPCHK(hipGetLastError());
    msiren::ModulatorMfmaParams mp{};
    mp.w = h->d_c3w_rm;
    mp.bias = h->enc.c3b;
    mp.z = feat;
    mp.out = a3;
    mp.B = (int)B;
    mp.H = 64;
    mp.Z = 2048;
    mp.act = msiren::LIN_ACT_LEAKY02;
    mp.count = c.plan;
    if ((rc = launch_linear(h, c, mp))) return rc;
    mp.w = h->d_fcw_rm;
    mp.bias = h->enc.fcb;
    mp.z = a3;
    mp.out = z_dev;
    mp.H = h->Z;
    mp.Z = 64;
    mp.act = msiren::LIN_ACT_NONE;
    return launch_linear(h, c, mp);
}

// encoder + modulator: tiles -> latent -> modulations; z_out: where the one-launch prologue stores the latent as well (null: nowhere)
static int launch_encoder_modulator(msiren_ctx* h, const Call& c, const float* tiles_dev, int64_t B, float* z_dev, float* mods_dev, float* z_out = nullptr) {
    if (B == 0) return 0;
    if (h->em_enc && h->em_mod) return launch_prologue_f16x3(h, c, tiles_dev, nullptr, B, z_out, mods_dev);  // (the latent stays in the workgroup)
    int rc = launch_encoder(h, c, tiles_dev, B, z_dev);
    if (rc) return rc;
    return launch_modulator(h, c, z_dev, B, mods_dev);
}

// msiren_encode_modulate_tiles(_dev): what forward_tiles_dev runs in front of its trunk, and nothing else
int encode_modulate_dev(msiren_ctx* h, const Call& c, const float* tiles_dev, int64_t B, float* z_dev, float* mods_dev) {
    if (!h->have_encoder || !h->have_modulator) return fail(MSIREN_E_STATE, "encoder.* / modulator.* weights were not loaded");
    float* z = z_dev;
    if (!z && !(h->em_enc && h->em_mod)) {  // (the per-layer launches pass the latent through HBM)
        int rc = ensure(h, h->sc[c.stream].latent, (size_t)B * h->Z * sizeof(float));
        if (rc) return rc;
        z = (float*)h->sc[c.stream].latent.p;
    }
    return launch_encoder_modulator(h, c, tiles_dev, B, z, mods_dev, z_dev);
}

int forward_latent_dev(msiren_ctx* h, const Call& c, const float* z_dev, int64_t B, float* out_dev, float* mods_out_dev) {
    auto& sc = h->sc[c.stream];
    float* mods = mods_out_dev;
    if (!mods) {
        int rc = ensure(h, sc.mods, (size_t)h->L * B * h->H * sizeof(float));
        if (rc) return rc;
        mods = (float*)sc.mods.p;
    }
    int rc = launch_modulator(h, c, z_dev, B, mods);
    if (rc) return rc;
    return launch_trunk(h, c, mods, B, out_dev);
}

int forward_tiles_dev(msiren_ctx* h, const Call& c, const float* tiles_dev, int64_t B, float* out_dev) {
    auto& sc = h->sc[c.stream];
    int rc = ensure(h, sc.latent, (size_t)B * h->Z * sizeof(float));
    if (rc) return rc;
    rc = ensure(h, sc.mods, (size_t)h->L * B * h->H * sizeof(float));
    if (rc) return rc;
    float* mods = (float*)sc.mods.p;
    rc = launch_encoder_modulator(h, c, tiles_dev, B, (float*)sc.latent.p, mods);
    if (rc) return rc;
    return launch_trunk(h, c, mods, B, out_dev);
}

// reflect padding + cut into O x O tiles at a stride of I (the caller has checked the shape: msiren_image_to_patches_dev)
static int launch_image_to_patches(msiren_ctx* h, int s, const float* images_dev, int64_t n, int32_t height, int32_t width, float* patches_dev) {
    const int pad = (h->O - h->I) / 2;
    const int vpad = (h->I - height % h->I) % h->I, hpad = (h->I - width % h->I) % h->I;
    const int nV = (height + vpad) / h->I, nH = (width + hpad) / h->I;
    const int64_t total = n * nV * nH * h->O * h->O;
    hipLaunchKernelGGL(msiren::image_to_patches_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->sc[s].s,
                       images_dev, patches_dev, n, height, width, nV, nH, h->O, h->I, pad);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace mh

using namespace mh;

// ---- tiling steps and the device-resident slice pipeline (include/msiren.h) -------------------------------------------------
extern "C" {

int msiren_recon_shape(msiren_handle h, int32_t height, int32_t width, int32_t* nv, int32_t* nh) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    if (height < 1 || width < 1) return fail(MSIREN_E_INVALID, "bad image size %dx%d", height, width);
    if (nv) *nv = (height + h->I - 1) / h->I;
    if (nh) *nh = (width + h->I - 1) / h->I;
    return 0;
}

int msiren_image_to_patches_dev(msiren_handle h, const float* images_dev, int64_t n, int32_t height, int32_t width, float* patches_dev) {
    int rc = check(h, false);
    if (rc) return rc;
    if (n < 0 || height < 1 || width < 1) return fail(MSIREN_E_INVALID, "bad arguments");
    if (n == 0) return 0;
    if ((rc = check_reflect_padding(h, height, width))) return rc;
    return launch_image_to_patches(h, h->cur, images_dev, n, height, width, patches_dev);
}

int msiren_weighted_fold_dev(msiren_handle h, const float* tiles_dev, int64_t n, int32_t nV, int32_t nH, float* recon_dev) {
    int rc = check(h);
    if (rc) return rc;
    if (n < 0 || nV < 1 || nH < 1) return fail(MSIREN_E_INVALID, "bad arguments");
    if (n == 0) return 0;
    const int64_t total = n * nV * h->I * (int64_t)nH * h->I;
    hipLaunchKernelGGL(msiren::weighted_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->sc[h->cur].s,
                       tiles_dev, h->d_foldw, recon_dev, nullptr, nullptr, n, nV, nH, h->S, h->I, (h->S - h->I) / 2, (int*)nullptr);
    HIPCHK(hipGetLastError());
    return 0;
}

int msiren_black_patch_flags_dev(msiren_handle h, const float* tiles_dev, int64_t n_tiles, int64_t tile_elems, int32_t* flags_dev) {
    int rc = check(h, false);
    if (rc) return rc;
    if (n_tiles < 0 || tile_elems < 1 || tile_elems > (1 << 24) || (n_tiles > 0 && (!tiles_dev || !flags_dev))) return fail(MSIREN_E_INVALID, "bad arguments");
    if (n_tiles == 0) return 0;
    if (n_tiles > 0x7fffffffLL) return fail(MSIREN_E_INVALID, "too many tiles for one call: %lld", (long long)n_tiles);
    hipLaunchKernelGGL(msiren::black_flags_kernel, dim3((unsigned)n_tiles), dim3(256), 0, h->sc[h->cur].s, tiles_dev, flags_dev, (int)tile_elems);
    HIPCHK(hipGetLastError());
    return 0;
}

static int copy_rows(msiren_handle h, const float* src, const int32_t* idx, int64_t n_idx, int64_t row_elems, float* dst, int scatter) {
    if (n_idx == 0) return 0;
    if (n_idx > 0x7fffffffLL) return fail(MSIREN_E_INVALID, "too many rows for one call: %lld", (long long)n_idx);
    hipLaunchKernelGGL(msiren::copy_rows_kernel, dim3((unsigned)n_idx), dim3(256), 0, h->sc[h->cur].s, src, dst, idx, (int)row_elems, scatter);
    HIPCHK(hipGetLastError());
    return 0;
}

int msiren_gather_rows_dev(msiren_handle h, const float* src_dev, const int32_t* idx_dev, int64_t n_idx, int64_t row_elems, float* dst_dev) {
    int rc = check(h, false);
    if (rc) return rc;
    if (n_idx < 0 || row_elems < 1 || row_elems > (1 << 24) || (n_idx > 0 && (!src_dev || !idx_dev || !dst_dev))) return fail(MSIREN_E_INVALID, "bad arguments");
    return copy_rows(h, src_dev, idx_dev, n_idx, row_elems, dst_dev, 0);
}

int msiren_scatter_rows_dev(msiren_handle h, const float* src_dev, const int32_t* idx_dev, int64_t n_idx, int64_t n_rows, int64_t row_elems, float* dst_dev) {
    int rc = check(h, false);
    if (rc) return rc;
    if (n_idx < 0 || n_rows < n_idx || row_elems < 1 || row_elems > (1 << 24) || (n_rows > 0 && !dst_dev) || (n_idx > 0 && (!src_dev || !idx_dev)))
        return fail(MSIREN_E_INVALID, "bad arguments");
    if (n_rows == 0) return 0;
    HIPCHK(hipMemsetAsync(dst_dev, 0, (size_t)n_rows * row_elems * sizeof(float), h->sc[h->cur].s));  // rows no index names stay zeros
    return copy_rows(h, src_dev, idx_dev, n_idx, row_elems, dst_dev, 1);
}

int msiren_patches_to_image_dev(msiren_handle h, const float* tiles_dev, int64_t n, int32_t nV, int32_t nH, float* image_dev) {
    int rc = check(h, false);
    if (rc) return rc;
    if (n < 0 || nV < 1 || nH < 1 || (n > 0 && (!tiles_dev || !image_dev))) return fail(MSIREN_E_INVALID, "bad arguments");
    if (n == 0) return 0;
    const int64_t total = n * nV * h->I * (int64_t)nH * h->I;
    hipLaunchKernelGGL(msiren::weighted_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->sc[h->cur].s,
                       tiles_dev, nullptr, image_dev, nullptr, nullptr, n, nV, nH, h->O, h->I, (h->O - h->I) / 2, (int*)nullptr);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"

namespace mh {

// What every slice call runs in front of its trunk: tiling -> black flags -> device-side plan -> the handle's prologue over the kept tiles.
// Leaves the black flags in sc.keep, the plan in sc.plan, the kept tiles' modulations in sc.mods; *pc: the call with the plan attached.
// `images_dev` given: `patches_rw` is scratch that image_to_patches fills; null: `patches_ro` are the caller's tiles
int slice_prologue(msiren_handle h, const Call& c, const float* images_dev, int32_t height, int32_t width, float* patches_rw, const float* patches_ro,
                   int64_t n, int32_t nV, int32_t nH, Call* pc, bool* fused_out) {
    int rc;
    auto& sc = h->sc[c.stream];
    const int64_t NP = n * nV * nH;
    const int upp = (c.P(h) + 31) / 32;
    if (NP > 0x7fffffffLL) return fail(MSIREN_E_INVALID, "too many patches for one call: %lld", (long long)NP);
    if ((rc = ensure(h, sc.keep, (size_t)(NP + 64) * sizeof(int)))) return rc;
    if ((rc = ensure(h, sc.latent, (size_t)NP * h->Z * sizeof(float)))) return rc;
    if ((rc = ensure(h, sc.mods, (size_t)h->L * NP * h->H * sizeof(float)))) return rc;
    int* black = (int*)sc.keep.p;
    // The reference compacts the non-black tiles, runs the model on those only, and scatters zeros back
    // (tiling.py:244-303).  Same here, on the device: black flags -> list of kept patches (the "plan") ->
    // encoder / modulator / trunk over the kept patches only (their count stays on the device) -> the fold
    // looks each patch up through the plan and lets black ones contribute zeros.
    if ((rc = ensure(h, sc.plan, (size_t)(2 + 2 * NP) * sizeof(int)))) return rc;
    int* plan = (int*)sc.plan.p;
    hipStream_t st = sc.s;
    const float* patches = images_dev ? patches_rw : patches_ro;
    const int pad = (h->O - h->I) / 2;
    // (round 5: 10 stream operations per slice -> 7 where fused; the flag is summed in the same order either way)
    const bool fused = msiren::fused_slice_tiling(c.mode, images_dev != nullptr);
    if (fused) {
        if ((rc = ensure_queue(h, c.stream))) return rc;
        msiren::TilingPlanParams tp{images_dev, patches_rw, black, plan, (unsigned*)sc.queue.p + 32, (int)n, height, width, nV, nH, h->O, h->I, pad, (int)NP, upp};
        hipLaunchKernelGGL(msiren::patches_flags_plan_kernel, dim3((unsigned)NP), dim3(256), 0, st, tp);
        HIPCHK(hipGetLastError());
    } else {
        if (images_dev && (rc = launch_image_to_patches(h, c.stream, images_dev, n, height, width, patches_rw))) return rc;
        hipLaunchKernelGGL(msiren::black_flags_kernel, dim3((unsigned)NP), dim3(256), 0, st, patches, black, h->O * h->O);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(msiren::compact_flags_kernel, dim3(1), dim3(256), 0, st, black, (int)NP, upp, plan);
        HIPCHK(hipGetLastError());
    }
    *pc = c;  // the model runs over the kept patches only: their count stays on the device
    pc->plan = plan;
    pc->mode.plan = true;
    *fused_out = fused;
    return launch_encoder_modulator(h, *pc, patches, NP, (float*)sc.latent.p, (float*)sc.mods.p);
}

// filter -> model -> reintegrate -> weighted fold on tiles that are already on the device (the call's stream)
// `images_dev` given: `patches` is scratch that image_to_patches fills; null: `patches` are the caller's tiles
// `og` (with c.cs): the output side at another stride (msiren_*_scaled); null: the model's own S, I and fold weights
static int reconstruct_tiles(msiren_handle h, const Call& c, const float* images_dev, int32_t height, int32_t width, float* patches_rw,
                             const float* patches_ro, int64_t n, int32_t nV, int32_t nH, float* recon_dev, const OutGeom* og,
                             const GradOut* go = nullptr) {
    int rc;
    auto& sc = h->sc[c.stream];
    const int64_t NP = n * nV * nH;
    const int P = c.P(h);
    const int oS = og ? og->tile : h->S, oI = og ? og->stride : h->I, opad = og ? og->pad : (h->S - h->I) / 2;
    const float* foldw = og ? og->foldw : h->d_foldw;
    if (NP > 0x7fffffffLL) return fail(MSIREN_E_INVALID, "too many patches for one call: %lld", (long long)NP);
    if ((rc = ensure(h, sc.rec, (size_t)NP * P * sizeof(float) * (go ? 3 : 1)))) return rc;  // (go: [value][d/d row][d/d column])
    Call pc;
    bool fused;
    if ((rc = slice_prologue(h, c, images_dev, height, width, patches_rw, patches_ro, n, nV, nH, &pc, &fused))) return rc;
    int* black = (int*)sc.keep.p;
    int* plan = (int*)sc.plan.p;
    float* rec = (float*)sc.rec.p;
    hipStream_t st = sc.s;
    if (go) rc = launch_trunk_f32_jet(h, pc, (const float*)sc.mods.p, NP, recon_dev ? rec : nullptr, rec + (size_t)NP * P, go->gscale);
    else rc = launch_trunk(h, pc, (const float*)sc.mods.p, NP, rec);
    if (rc) return rc;
    if ((rc = queue_reset_after_plan_launch(h, c.stream, fused))) return rc;
    const int64_t total = n * nV * oI * (int64_t)nH * oI;
    if ((total + 255) / 256 > 0x7fffffffLL) return fail(MSIREN_E_INVALID, "reconstruction too large for one call: %lld pixels", (long long)total);
    int* reset_word = fused && sc.queue.p ? (int*)sc.queue.p : nullptr;
    // value, then (go) the two gradient planes: the same weighted fold, black tiles contributing zeros with their weight
    for (int k = 0; k < (go ? 3 : 1); ++k) {
        float* dst = k == 0 ? recon_dev : go->grad + (size_t)(k - 1) * total;
        if (!dst) continue;
        hipLaunchKernelGGL(msiren::weighted_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                           rec + (size_t)k * NP * P, foldw, dst, black, plan + 2 + NP, n, nV, nH, oS, oI, opad, reset_word);
        HIPCHK(hipGetLastError());
        reset_word = nullptr;
    }
    return 0;
}

// slice pipeline on the call's stream (the host-pointer entry point enqueues its copies around it)
int reconstruct_slices(msiren_handle h, const Call& c, const float* images_dev, int64_t n, int32_t height, int32_t width, float* recon_dev, const OutGeom* og,
                       const GradOut* go) {
    int rc;
    if (n < 0 || (n > 0 && (!images_dev || (go ? !go->grad : !recon_dev)))) return fail(MSIREN_E_INVALID, "bad arguments");
    if (go && (rc = jet_supported(h))) return rc;
    if ((rc = check_tile_size(h, false))) return rc;
    if (n == 0) return 0;
    int32_t nV, nH;
    if ((rc = msiren_recon_shape(h, height, width, &nV, &nH))) return rc;
    const int64_t NP = n * nV * nH;
    if ((rc = check_reflect_padding(h, height, width))) return rc;
    auto& sc = h->sc[c.stream];
    if ((rc = ensure(h, sc.patches, (size_t)NP * h->O * h->O * sizeof(float)))) return rc;
    return reconstruct_tiles(h, c, images_dev, height, width, (float*)sc.patches.p, nullptr, n, nV, nH, recon_dev, og, go);
}

// msiren_weighted_fold_dev with the output side of another stride (kernel S', stride I', padding pad'): complete tiles, no black flags
int weighted_fold_dev(msiren_handle h, const Call& c, const float* tiles_dev, int64_t n, int32_t nV, int32_t nH, float* recon_dev, const OutGeom& og) {
    const int64_t total = n * nV * og.stride * (int64_t)nH * og.stride;
    if ((total + 255) / 256 > 0x7fffffffLL) return fail(MSIREN_E_INVALID, "reconstruction too large for one call: %lld pixels", (long long)total);
    hipLaunchKernelGGL(msiren::weighted_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->sc[c.stream].s,
                       tiles_dev, og.foldw, recon_dev, nullptr, nullptr, n, nV, nH, og.tile, og.stride, og.pad, (int*)nullptr);
    HIPCHK(hipGetLastError());
    return 0;
}

int reconstruct_tiles_dev(msiren_handle h, const Call& c, const float* tiles_dev, int64_t n, int32_t nV, int32_t nH, float* recon_dev, const OutGeom* og) {
    if (n < 0 || nV < 1 || nH < 1 || (n > 0 && (!tiles_dev || !recon_dev))) return fail(MSIREN_E_INVALID, "bad arguments");
    if (int rc = check_tile_size(h, false)) return rc;
    if (n == 0) return 0;
    return reconstruct_tiles(h, c, nullptr, 0, 0, nullptr, tiles_dev, n, nV, nH, recon_dev, og);
}

}  // namespace mh

extern "C" {

int msiren_reconstruct_tiles_dev(msiren_handle h, const float* tiles_dev, int64_t n, int32_t nV, int32_t nH, float* recon_dev) {
    int rc = check(h);
    if (rc) return rc;
    return reconstruct_tiles_dev(h, dev_call(h), tiles_dev, n, nV, nH, recon_dev);
}

int msiren_reconstruct_slices_dev(msiren_handle h, const float* images_dev, int64_t n, int32_t height, int32_t width, float* recon_dev) {
    int rc = check(h);
    if (rc) return rc;
    return reconstruct_slices(h, dev_call(h), images_dev, n, height, width, recon_dev);
}

}  // extern "C"

