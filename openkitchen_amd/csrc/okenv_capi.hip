// okenv_capi.hip -- implementation of the C ABI declared in include/okenv.h.
//
// Host side of the batched Environment step: owns the device-resident struct-of-arrays state, builds and
// uploads the uniform grid, chooses the launch geometry and enqueues the kernels of okenv_kernels.h on the
// handle's HIP stream.  There is no CPU fallback anywhere in this file: without a usable GPU
// okenv_create fails with OKENV_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/okenv.h"
#include "Environment/RaceTrack.h"
#include "ok_grid.h"
#include "ok_render.h"
#include "okenv_kernels.h"
#include "ok_actor.h"
#include "ok_batch.h"
#include "ok_learn.h"
#include "ok_dqn.h"
#include "ok_ddpg.h"
#include "ok_reinforce.h"
#include "ok_gauss.h"
#include "ok_gcl.h"
#include "ok_lidar.h"
#include "ok_flow.h"
#include "ok_bev.h"
#include "ok_cnn.h"
#include "ok_world.h"
#include "ok_memory.h"
#include "ok_memtrain.h"
#include "ok_qcnn.h"
#include "ok_vit.h"
#include "ok_vithead.h"
#include "ok_expert.h"

namespace
{
thread_local std::string g_create_error = "";

constexpr size_t kLdsBudget = 160U * 1024U; // one workgroup may take the whole CU's LDS on gfx950
// LDS kept free behind the track image for the Q-learning kernel's copy of the centre line (8 B per point)
constexpr size_t kLdsReserve = 16U * 1024U;

struct EventPair
{
    hipEvent_t start, stop;
};

// spin-wait hint of the host loops that watch a word in mapped memory
inline void okCpuRelax()
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield" ::: "memory");
#else
    std::atomic_signal_fence(std::memory_order_seq_cst);
#endif
}
} // namespace

// ---- launch policy -------------------------------------------------------------------------------------------------------
// Which step kernel a call runs (enum okenv_step_form) and with what grid, workgroup, LDS and lane-group width.  Everything from
// here to the end of this namespace is plain arithmetic on the structs below -- no HIP call, no environment, no handle -- so that
// okenv_debug_plan_step can run it on a machine without a device for any shape, knob and compute-unit count
// (tests/test_step_form_table.py).  okenv_create fills the shape once, launchStep asks for a plan per launch.
namespace
{
constexpr size_t kCoopLdsExtra      = 16U; // LDS every cooperative launch needs behind the image (the per-SIMD progress words)
constexpr int    kResidentMaxAgents = 64;

// The OKENV_* tuning / ablation variables that bear on launches, as parsed (readKnobs).  The default of each is its "unset" state;
// a value outside the stated range is ignored like an unset one.
struct OkKnobs
{
    int   lanes_per_agent{0};   // a power of two up to 64: fold the fan over fewer lanes (ray r, r+G, ... share one) or spread it over more
    long  block_threads{0};     // a multiple of 64 and of G up to 1024: smaller workgroups (two per CU when the LDS image allows)
    int   coop{1};              // 0: every lane walks its own ray to the end
    int   agents_per_block{-1}; // >= 0 and within the workgroup; 0 = dense
    int   tail_max_agents{-1};  // 0: never use the tail kernel; > 0: caps the rule
    float phase1_range{-1.F};   // >= 0 [px]; 0: no phase 1.  Overrides the 16-ray and spare-lane rules
    int   resident{-1};         // 0: never keep the packed-step kernel resident, 1: from the first eligible step on
    int   front_back{1};        // 0: every launch stays on the combined image (same results)
};

// What okenv_create decides once for a handle.
struct OkLaunchShape
{
    int    N{0}, R{0}, cus{256}; // agents, rays, compute units of the device (an MI355X in CPX / DPX partition mode shows 32 / 128 of its 256)
    int    G{1}, natural_g{1}, rays_per_lane{1};
    float  phase1_range{48.F};   // T1 of the cooperative kernel [px]
    float  cell_default{OKGRID_DEFAULT_CELL};
    int    grid_mode{kGridLds};
    bool   front_back{false};    // the front / back split of the segment set is to be built (ok_grid.h)
    int    block_threads{1024}, grid_blocks{1};
    bool   coop{false};          // cooperative two-phase kernel (LDS form, one ray per lane)
    int    agents_per_block{0};  // coop, tiny populations: agents per workgroup (the other lanes only stage); 0 = dense
    int    tail_max_agents{-1};  // episode lists up to this long are stepped by okStepTailKernel: -1 = what one round of workgroups holds, 0 = never
    int    resident_mode{-1};    // 0 never, 1 from the first eligible step on, default: after a run of quick steps
    // known once the grid is built and uploaded: the combined image, the [front | back] blob; fb_ok: launches may use the latter
    size_t image_bytes{0}, fb_bytes{0};
    bool   fb_ok{false};
};

int pow2ceil(int v)
{
    int p = 1;
    while (p < v)
        p <<= 1;
    return p;
}

// Widest lane group (up to 64) with which `agents` agents still take at most half of the machine's lanes (compute units x 1024),
// so that the waves of a CU do not start competing for issue.
int okWidenLanes(int G, const long agents, const int cus)
{
    while (G < 64 && agents * (2L * G) <= 512L * cus)
        G *= 2;
    return G;
}

// Workgroup size and count for `lanes` lanes: spread over the CUs (a workgroup on every CU before they grow to 1024 lanes), but at
// least four waves each: with a handful of agents the launch is dominated by staging the ~70-90 KB track image into LDS, which a
// single wave does four times slower (waves without an agent leave right after it).
void okSpread(const long lanes, const int cus, long *per_block, long *blocks)
{
    const long per = ((((lanes + cus - 1) / cus) + 63) / 64) * 64;
    *per_block     = per < 256 ? 256 : (per > 1024 ? 1024 : per);
    *blocks        = (lanes + *per_block - 1) / *per_block;
}

// First stage, before the grid exists: lanes per agent, phase 1 and the cell edge the grid is built with by default.
OkLaunchShape okPlanLanes(const int N, const int R, const int cus, const OkKnobs &k)
{
    OkLaunchShape s;
    s.N   = N;
    s.R   = R;
    s.cus = cus;
    // lanes per agent: the fan's width rounded up to a power of two -- and more when the population is far too small to fill the
    // machine: the spare lanes of an agent's group take intervals of its rays in phase 2, which shortens the dependent chain of a
    // step (11.5-13 us instead of 15.6 us per step for RL-sized populations).
    s.natural_g = pow2ceil(R) > 64 ? 64 : pow2ceil(R);
    s.G         = okWidenLanes(s.natural_g, N, cus);
    if (k.lanes_per_agent >= 1 && k.lanes_per_agent <= 64 && (k.lanes_per_agent & (k.lanes_per_agent - 1)) == 0)
        s.G = k.lanes_per_agent;
    // with spare lanes there is no phase 1: phase 2 cuts every ray into intervals from its origin on (a 4 px phase 1 in
    // front of it cost a second walk set-up per step: 6.5 -> 5.2 us for one five-ray agent, 8.4 -> 7.0 us at 4096 x 5)
    if (s.G > s.natural_g)
        s.phase1_range = 0.F;
    s.rays_per_lane = (R + s.G - 1) / s.G;
    // cell edge: 24 px when a wave holds one agent (all 64 rays leave one origin), 20 px when it holds several (measured:
    // Silverstone / Spa x 64 rays 4 % faster at 24, Monza x 32 rays 6 % faster at 20)
    // (round 3: 16-ray fans four to a wave -- BASELINE config 5 -- 24 px cells with a 32 px phase 1: 15.6 against 16.4 us per step)
    const bool narrow16 = s.G == 16 && s.rays_per_lane == 1;
    // (wide fans, one agent per wave: 28 px since the front / back split halved the points per cell -- 9.5-10.0 us per C2 step at
    // 28-30 px against 10.4 at 24 and 10.7 at 20, profiles/r4/front_back_ab.txt; 16-ray fans stay at 24, 32-ray fans at 20)
    const bool wide64 = s.G == 64 && s.rays_per_lane == 1 && R > 32;
    s.cell_default    = wide64 ? 28.F : (narrow16 ? 24.F : OKGRID_DEFAULT_CELL);
    if (narrow16)
        s.phase1_range = 32.F;
    if (k.phase1_range >= 0.F)
        s.phase1_range = k.phase1_range;
    return s;
}

// Second stage, once the grid builder has said whether the track image fits the LDS: the grid form and the launch geometry.
void okPlanGeometry(OkLaunchShape &s, const uint32_t flags, const bool image_fits_lds, const OkKnobs &k)
{
    if (flags & OKENV_FLAG_BRUTE_FORCE)
        s.grid_mode = kGridBrute;
    else if (!image_fits_lds || (flags & OKENV_FLAG_FORCE_GLOBAL_GRID))
        s.grid_mode = kGridGlobal;
    else
        s.grid_mode = kGridLds;
    s.front_back = s.grid_mode == kGridLds && k.front_back != 0;
    const long total_lanes = static_cast<long>(s.N) * s.G;
    long       per_block, blocks;
    okSpread(total_lanes, s.cus, &per_block, &blocks);
    if (k.block_threads >= 64 && k.block_threads <= 1024 && k.block_threads % 64 == 0 && k.block_threads % s.G == 0)
        per_block = k.block_threads;
    s.block_threads = static_cast<int>(per_block);
    s.grid_blocks   = static_cast<int>((total_lanes + per_block - 1) / per_block);
    s.coop          = s.grid_mode == kGridLds && s.rays_per_lane == 1 && k.coop != 0;
    // up to one agent per CU with a wave each (the populations of the reference's applications: 1, 15, 30, 50): one agent per
    // workgroup, i.e. per CU -- four such waves on one CU take 7.8 us for a step, one alone 6.0 us -- and three more waves
    // that only help with the staging
    s.agents_per_block = 0;
    if (s.coop && s.G == 64 && s.N <= s.cus && per_block == 256)
        s.agents_per_block = 1;
    if (s.coop && k.agents_per_block >= 0 && static_cast<long>(k.agents_per_block) * s.G <= per_block)
        s.agents_per_block = k.agents_per_block;
    if (s.agents_per_block > 0)
        s.grid_blocks = (s.N + s.agents_per_block - 1) / s.agents_per_block;
    s.resident_mode   = k.resident;
    s.tail_max_agents = k.tail_max_agents;
}

// okenv_step_packed may keep its kernel resident on handles of this shape (the call and the handle's state decide the rest)
bool okResidentShape(const OkLaunchShape &s)
{
    return s.resident_mode != 0 && s.agents_per_block == 1 && s.N <= kResidentMaxAgents;
}

size_t okCoopLdsBytes(const size_t image_bytes)
{
    return image_bytes + kCoopLdsExtra;
}

// The tail kernel's workgroup (okStepTailKernel: one agent, every ray cut into kTailSplit intervals): lanes that walk, and LDS
// behind an image of `image_bytes`.  Q-learning: the centre line and its buckets (q_bytes) and the agent's table in LDS too.
unsigned okTailLanes(const OkLaunchShape &s)
{
    return static_cast<unsigned>(((s.R * kTailSplit + 63) / 64) * 64);
}

size_t okTailLdsBytes(const size_t image_bytes, const bool q_launch, const size_t q_bytes)
{
    return image_bytes + 16U + sizeof(float) * kTailLdsFloats + (q_launch ? q_bytes + sizeof(float) * kTailQFloats : 0U);
}

// Longest episode list the tail kernel takes on this shape: one round of workgroups -- as many per CU as the LDS holds, times the
// device's compute units (256 on an MI355X in SPX mode; measured there, 32-ray MLP agents: 8.1 us per step up to 256 agents, 9.2 at
// 512 with two per CU, against 11.2-11.8 for the cooperative kernel; a second round loses: 17 us) -- or OKENV_TAIL_MAX_AGENTS;
// 0: the tail kernel does not apply.
long okTailLimit(const OkLaunchShape &s, const bool q_launch, const size_t q_bytes)
{
    if (s.grid_mode != kGridLds || !s.coop || s.tail_max_agents == 0)
        return 0;
    const size_t lds = okTailLdsBytes(s.image_bytes, q_launch, q_bytes);
    if (okTailLanes(s) > 512U || lds > kLdsBudget)
        return 0;
    const long fit = static_cast<long>(kLdsBudget / lds) * s.cus;
    return s.tail_max_agents > 0 ? std::min<long>(s.tail_max_agents, fit) : fit;
}

// The first rollout of an episode lists the whole population when it fits the tail kernel (prelistEpisode).  The controller
// rollout has no tail form.
bool okPrelist(const OkLaunchShape &s, const int action_source, const size_t q_bytes)
{
    return action_source != kActionsController && static_cast<long>(s.N) <= okTailLimit(s, action_source == kActionsQLearning, q_bytes);
}

// What differs from one step launch to the next.
struct OkStepRequest
{
    int      action_source{kActionsStored};
    int      n_listed{-1};       // agents on the episode's list; -1: no list, the whole population
    bool     packed{false};      // okenv_step_packed's exchange records
    bool     resident{false};    // ... served by the kernel that stays (startResident)
    int      do_move{1};
    uint32_t reset_flags{0};
    int      ctrl_num_params{0};
    size_t   q_bytes{0};         // LDS of the centre line and its cell buckets (qLdsBytes; it changes with okenv_set_centerline)
};

struct OkStepPlan
{
    int      form{OKENV_FORM_COOP};
    unsigned grid{1}, block{64};
    size_t   lds{0};            // dynamic LDS bytes
    uint32_t image_off{0};      // where the image ends in LDS (tail and cooperative kernels)
    float    phase1{0.F};
    int      G{1};              // lane-group width of this launch
    bool     front_back{false}; // the launch walks the [front | back] images
    uint32_t ctrl_lds_off{0};   // controller parameters staged in LDS from here; 0: read from global memory
    size_t   waves() const { return static_cast<size_t>(grid) * (block / 64U); }
};

OkStepPlan okPlanStep(const OkLaunchShape &s, const OkStepRequest &q)
{
    OkStepPlan pl;
    pl.grid         = static_cast<unsigned>(s.grid_blocks);
    pl.block        = static_cast<unsigned>(s.block_threads);
    pl.G            = s.G;
    pl.phase1       = s.phase1_range;
    const bool mlp  = q.action_source == kActionsMlpPolicy;
    const bool qlrn = q.action_source == kActionsQLearning;
    if (q.n_listed >= 0)
    { // an episode's list: the grid covers the listed agents, spread over the CUs like a population of that size
        if (qlrn)
        { // ... and a list that has become short gets what a population that small gets from okPlanLanes: wider lane groups
          // whose spare lanes take intervals of the agent's rays, no phase 1 (16 rays, 64 listed agents: 9.3 against 11.8 us
          // per step; the fused MLP's steps gain nothing from it and keep their width)
            pl.G = okWidenLanes(s.G, q.n_listed, s.cus);
            if (pl.G > s.G)
                pl.phase1 = 0.F;
        }
        long per, blocks;
        okSpread(static_cast<long>(q.n_listed) * pl.G, s.cus, &per, &blocks);
        pl.block = static_cast<unsigned>(per);
        pl.grid  = static_cast<unsigned>(blocks);
    }
    // The tail of an episode: a short list is stepped one agent per workgroup, every ray cut into eight intervals
    // (okStepTailKernel).  Two such workgroups fit a CU's LDS; beyond about two rounds of them the cooperative kernel's shared
    // waves win again.
    if (q.n_listed > 0 && (mlp || qlrn) && q.n_listed <= okTailLimit(s, qlrn, q.q_bytes))
    {
        pl.G      = s.G; // (unused by the tail kernel; undoes the widening above)
        pl.grid   = static_cast<unsigned>(q.n_listed);
        // (Q-learning: one more wave, without rays -- it looks up the nearest centre-line index while the others walk)
        pl.block  = okTailLanes(s) + (qlrn ? 64U : 0U);
        pl.lds    = okTailLdsBytes(s.image_bytes, qlrn, q.q_bytes);
        // the front / back split while the list fits one round of workgroups with the larger image (fewer of them share a CU);
        // longer lists keep the combined image and their two workgroups per CU
        const size_t lds_fb = okTailLdsBytes(s.fb_bytes, qlrn, q.q_bytes);
        pl.front_back       = s.fb_ok && lds_fb <= kLdsBudget && static_cast<long>(q.n_listed) <= static_cast<long>(kLdsBudget / lds_fb) * s.cus;
        if (pl.front_back)
            pl.lds = lds_fb;
        pl.image_off = static_cast<uint32_t>(pl.front_back ? s.fb_bytes : s.image_bytes);
        // (15 rays: the reference's own fan -- Agent.cpp:13-17; EvolutionaryRacer's 17-30-6 network --, weights in registers as well)
        pl.form = qlrn ? OKENV_FORM_TAIL_Q : (s.R == 32 ? OKENV_FORM_TAIL_MLP32 : (s.R == 15 ? OKENV_FORM_TAIL_MLP15 : OKENV_FORM_TAIL_MLP));
        return pl;
    }
    if (s.grid_mode != kGridLds)
    {
        const bool global = s.grid_mode == kGridGlobal;
        pl.form = mlp ? (global ? OKENV_FORM_GLOBAL_MLP : OKENV_FORM_BRUTE_MLP) : (global ? OKENV_FORM_GLOBAL : OKENV_FORM_BRUTE);
        return pl;
    }
    if (!s.coop)
    {
        pl.lds  = s.image_bytes;
        pl.form = mlp ? OKENV_FORM_LDS_MLP : OKENV_FORM_LDS;
        return pl;
    }
    // the front / back split, when everything else the launch stages still fits behind it
    const bool ctrl  = q.action_source == kActionsController;
    pl.front_back    = s.fb_ok && okCoopLdsBytes(s.fb_bytes) + (qlrn || ctrl ? q.q_bytes : 0U) <= kLdsBudget;
    const size_t img = pl.front_back ? s.fb_bytes : s.image_bytes;
    pl.image_off     = static_cast<uint32_t>(img);
    pl.lds           = okCoopLdsBytes(img);
    // policy-free launches of a population with spare lanes and no phase 1 use the kernel's direct dealing of intervals to lanes
    // (okStepCoopKernel's kDirect)
    const bool direct = s.phase1_range <= 0.F && s.G >= 2 * s.R;
    if (qlrn)
    {
        pl.lds += q.q_bytes;
        pl.form = OKENV_FORM_COOP_Q;
    }
    else if (ctrl)
    { // the controllers' parameters of a workgroup's agents go into its LDS when they fit behind the centre line
        pl.lds += q.q_bytes;
        const size_t base  = ((pl.lds + 15U) / 16U) * 16U;
        const size_t stage = static_cast<size_t>(pl.block / static_cast<unsigned>(pl.G)) * static_cast<size_t>(q.ctrl_num_params) * sizeof(float);
        if (base + stage <= kLdsBudget)
        {
            pl.ctrl_lds_off = static_cast<uint32_t>(base);
            pl.lds          = base + stage;
        }
        pl.form = OKENV_FORM_COOP_CTRL;
    }
    else if (mlp) // (32 rays in 32-lane groups, C3 / C4's fan: group and fan width compile-time constants)
        pl.form = s.G == 32 && s.R == 32 ? OKENV_FORM_COOP_MLP32 : OKENV_FORM_COOP_MLP;
    else if (q.resident)
        pl.form = direct ? OKENV_FORM_RESIDENT_DIRECT : OKENV_FORM_RESIDENT;
    else if (q.packed)
        pl.form = direct ? OKENV_FORM_COOP_PACKED_DIRECT : OKENV_FORM_COOP_PACKED;
    else if (direct)
        pl.form = OKENV_FORM_COOP_DIRECT;
    else if (s.G == 64 && q.action_source == kActionsPhiloxReset && q.do_move != 0 && q.reset_flags == 0U)
        pl.form = OKENV_FORM_COOP_G64_RANDOM; // okenv_rollout_random without device-side resetAgent: its launch-time switches as constants (-1 %)
    else if (s.G == 64)
        pl.form = OKENV_FORM_COOP_G64; // one agent per wave, the group width a compile-time constant (-1 % on 20-step launches)
    else
        pl.form = OKENV_FORM_COOP;
    return pl;
}
} // namespace

// A replay ring as the handle keeps it, Deep-Q's or DDPG's (both may live on one handle): the fields on the device, the counter words
// and the push's count scratch.  The two differ in the action's row only.
struct OkRing
{
    size_t    action_bytes;        // of one slot's action: an int64 index, or two floats
    bool      ok{false};
    uint32_t  flags{0};
    int32_t   capacity{0};
    float    *state{nullptr}, *next_state{nullptr};
    uint8_t  *action{nullptr};
    float    *reward{nullptr}, *done{nullptr};
    uint64_t *d_words{nullptr};    // [0] pushed, [1] its value before the latest push
    uint32_t *d_counts{nullptr};   // [workgroups of the push]
    explicit OkRing(const size_t action_bytes_) : action_bytes(action_bytes_) {}
};

// The events around every kernel of an update's latest timed call (okenv_set_timing on): created on demand, kept for the next call
struct OkEventLog
{
    std::vector<hipEvent_t> events;
    size_t                  want{0}, at{0}, timed{0}; // events of the call under way, the last one recorded, events of the latest complete timed call
};

// The device scratch of an update or a batch (grown, never shrunk: growScratch) and the events of its latest timed call
struct OkUpdateScratch
{
    uint8_t   *part{nullptr};
    size_t     bytes{0};
    OkEventLog log;
};

// A device buffer of the handle that grows and never shrinks (growBuffers): the pointer and its room in floats
struct OkBuffer
{
    float *d{nullptr};
    size_t cap{0};
};

// What a family that attaches a network keeps in the handle beside its configuration ("The drivers' life cycle on the host"):
// the shared entries reach it through the family's DriverKind
struct OkDriver
{
    bool            ok{false};                   // okenv_*_create has run
    bool            set[3]{false, false, false}; // per parameter vector: okenv_*_set_params has filled it
    size_t          cap{0};                      // floats of one vector's room
    float          *d{nullptr}, *d2{nullptr};    // the vectors on the device, [vectors][cap] (d2: a second block, the actor's and DDPG's)
    const uint32_t *draw_offset{nullptr};        // okenv_*_set_draw_offset's device word
};

struct okenv
{
    int         device{0};
    hipStream_t stream{nullptr};
    bool        own_stream{true};
    OkLaunchShape shape; // population, fan and every launch decision taken once (okPlanLanes, okPlanGeometry)
    int         S{0};
    uint32_t    flags{0};
    OkGridHost  grid;
    OkPolyImage poly;
    void       *d_image{nullptr};
    OkSeg      *d_segs{nullptr};
    uint32_t   *d_refs32{nullptr}, *d_start{nullptr};
    float      *d_ray_deg{nullptr};
    float       sensor_offset{0.F};
    float      *d_cx{nullptr}, *d_cy{nullptr}, *d_chead{nullptr};
    int         P{0}, centerline_capacity{0};
    float      *d_lane_l{nullptr}, *d_lane_r{nullptr}; // left_bound_inner_ / right_bound_inner_, xy pairs
    int         lane_points{0}, lane_capacity{0};
    uint32_t    reset_flags{0}, reset_seed{0}, reset_agent_base{0}; // okenv_set_auto_reset
    // packed host exchange (okenv_step_packed): pinned host staging + device records, allocated on first use
    void       *h_stage{nullptr};
    void       *h_stage_device{nullptr}; // the same buffer as the device sees it (mapped host memory)
    void       *d_stage{nullptr};
    OkTracker   tracker{};
    int         tracker_kind{-1};
    // Environment steps taken by okenv_step / okenv_rollout_policy.  While auto-reset is on the device copy is the
    // authoritative one (it is the epoch of the reset draws and advances under graph replay); otherwise the host copy.
    uint32_t    step_count{0};
    uint32_t   *d_step_count{nullptr};
    OkDeviceState st{};
    std::vector<void *> allocations;
    // EvolutionaryRacer state
    int      mlp_hidden{0};
    // front / back split of the segment set (ok_grid.h): classification, the two images, and their copy on the device as one blob
    // [front | back] (shape.fb_bytes of it, usable when shape.fb_ok)
    OkFrontBack       fbc;
    OkFrontBackImages fbi;
    uint8_t          *d_image_fb{nullptr};
    size_t            fb_back_off{0};
    float   *d_mlp_w{nullptr}, *d_mlp_w_new{nullptr}, *d_score{nullptr}, *d_parent_score{nullptr};
    int32_t *d_nearest{nullptr}, *d_parents{nullptr}, *d_alive{nullptr};
    // Q-learning state
    float   *d_q_table{nullptr};
    int32_t *d_q_state{nullptr}, *d_q_action{nullptr}, *d_q_prev{nullptr}, *d_q_reset_nearest{nullptr};
    void    *d_scratch{nullptr};       // staging for calls that take host arrays (every user synchronises before it returns)
    size_t   scratch_bytes{0};
    float   *d_ctrl_params{nullptr};   // CMA-ES controllers: [N][ctrl_num_params]
    int      ctrl_hidden{0}, ctrl_num_params{0};
    float   *d_q_reset_query{nullptr}; // (x, y) of the episode's reset point, the query of its nearest-index kernel
    float    q_reset_query[2]{0.F, 0.F}; // host copy the upload reads: lives as long as the handle
    float   *d_q_sums{nullptr};
    uint16_t *d_cl_start{nullptr}, *d_cl_idx{nullptr}; // centre line bucketed by grid cell (Q-learning's nearest index)
    size_t    cl_capacity{0};
    bool      cl_dirty{true};
    int      q_ray[5]{0, 0, 0, 0, 0};
    float    q_epsilon{0.F};
    unsigned long long *d_stamps{nullptr}; // -DOKENV_STAMPS builds: per-wave stamps of the last launch
    size_t    stamp_waves{0}, stamp_waves_cap{0};
    // episodes (okenv_episode_begin / _compact / _end)
    bool      episode{false};
    int       n_active{-1};       // agents listed for the policy rollouts (-1: everybody, no list)
    int       ep_kind{0};         // policy of the episode's rollouts: 0 none yet, kPolicyMlp, kPolicyQ
    uint32_t  ep_steps{0};        // steps taken since okenv_episode_begin
    uint32_t  ep_q_seed{0}, ep_q_agent_base{0}, ep_q_step_base{0}; // Q-learning: the draws' key, global step of episode step 1
    float     ep_q_epsilon{0.F};
    int32_t  *d_active{nullptr}, *d_ep_counts{nullptr}, *d_q_next_state{nullptr};
    uint8_t  *d_settled{nullptr};
    uint32_t *d_crash_step{nullptr}, *d_ep_out{nullptr};
    float    *d_crash_thr{nullptr}, *d_crash_steer{nullptr};
    unsigned long long *d_live{nullptr};
    std::vector<float> host_cx, host_cy, host_chead, host_ray_deg;
    uint32_t    packed_seq{0};      // okenv_step_packed: sequence number of the last launch's completion word
    // resident step kernel (okenv_step_packed called in quick succession, see startResident)
    hipStream_t resident_stream{nullptr};
    bool        resident{false};
    int         resident_steps{0}, resident_fallbacks{0}; // statistics (okenv_get_info)
    int         resident_stall_us{0}; // OKENV_RESIDENT_STALL_US, fault injection for the tests: the host dawdles this long before
                                      // it hands a step to the resident kernel, which has left by then
    int         resident_need{16};  // quick steps in a row that start it: kResidentStreak, more after residencies that ended early
    int         resident_served_now{0}; // steps the current residency has served
    int         packed_streak{0};   // packed steps in a row that came within kResidentGapUs of the one before
    std::chrono::steady_clock::time_point packed_last_end{};
    size_t      stage_slots_off{0}; // where the agents' slots lie in h_stage
    bool        ep_prelist{false};  // okenv_episode_begin has run, the episode's first rollout has not: it decides the pre-listing
    // step-kernel launches by form and attribute (okenv_debug_step_forms)
    uint64_t    form_counts[OKENV_NUM_STEP_FORMS][1 + OKENV_NUM_STEP_FORM_ATTRS]{};
    std::string last_error;
    bool        timing{false};
    std::vector<EventPair> events;      // recorded pairs awaiting resolution
    double      timing_carry_ms{0.0};    // pairs resolved early (before a stream switch), not yet reported
    uint64_t    timing_carry_n{0};
    std::vector<EventPair> event_pool;  // reusable pairs
    // bird's-eye views (okenv_render_create): the validated descriptor, the draw list's grid on the device and its sizes
    bool            render_ok{false};
    okenv_view_desc render_desc{};
    OkRenderGeom    render_geom;        // scalars only: the CSR arrays are released after the upload
    size_t          render_refs{0};
    OkRenderTri    *d_render_tris{nullptr};
    uint32_t       *d_render_start{nullptr};
    // expert drivers (okenv_expert_create): parameters and the per-ray cos / sin table [cos R | sin R]
    bool                expert_ok{false};
    okenv_expert_params expert{};
    double             *d_expert_tab{nullptr};
    // shared-network actors (okenv_actor_create): parameters, the two networks' vectors (padded to four floats) and what has been set
    // (actor_drv: d the policy's vector, d2 the value's; set[0], set[1] likewise)
    OkDriver           actor_drv;
    okenv_actor_params actor{};
    // episode -> batch (okenv_batch_prepare): scratch for the planes, column partials, group counts, statistics and M; grown, never
    // shrunk; the events of the latest timed call
    OkUpdateScratch batch_scratch;
    int32_t        *d_batch_count{nullptr};
    // PPO's update (okenv_learner_create): Adam's moments beside the actor's parameters, the step number, the chunk partials (grown,
    // never shrunk) and the events of the latest timed okenv_ppo_update
    bool                    learner_ok{false};
    okenv_learner_params    learner{};
    int64_t                 learn_t{0};
    float                  *d_learn_moments{nullptr}; // [4][cap]: policy m, policy v, value m, value v
    size_t                  learn_cap{0};
    OkUpdateScratch         learn_scratch;
    // Deep-Q (okenv_replay_create, okenv_dqn_params): the ring, the update's constants, the target network's copy, the chunk partials
    // (grown, never shrunk) and the events of the latest timed update
    OkRing                  replay{sizeof(int64_t)};
    okenv_dqn_config        dqn{0.99F, 0U, 0, 0U};
    float                  *d_dqn_target{nullptr};
    bool                    dqn_target_set{false};
    OkUpdateScratch         dqn_scratch;
    // DDPG (okenv_ddpg_create, okenv_ddpg_replay_create): the four networks [actor | critic | actor target | critic target] and the four
    // moments [actor m | actor v | critic m | critic v], each ddpg_drv.cap floats (ddpg_drv: d the networks, d2 the moments; set[0] the
    // actor, set[1] the critic); the ring, the
    // update's chunk partials (grown, never shrunk) and timing events.  Nothing here is shared with the actor, the learner or the
    // Deep-Q ring above.
    OkDriver                ddpg_drv;
    okenv_ddpg_config       ddpg{};
    int64_t                 ddpg_t{0};
    OkRing                  ddpg_ring{2U * sizeof(float)};
    OkUpdateScratch         ddpg_scratch;
    // REINFORCE (okenv_actor_set_dropout, okenv_reinforce_update): the policy network's dropout, the update's scratch
    // [chunk partials | accumulator] (grown, never shrunk) and timing events.  The learner is the one above.
    float                   actor_dropout{0.F};
    uint32_t                actor_dropout_seed{0};
    OkUpdateScratch         reinforce_scratch;
    // Continuous REINFORCE (okenv_gauss_create, okenv_gauss_learner_create): the parameter vector and Adam's two moments
    // [params | m | v], each gauss_drv.cap floats, the update's scratch [chunk partials | accumulator] (grown, never shrunk) and timing
    // events.  Nothing here is shared with the actor, the learner or the DDPG object above.
    OkDriver                gauss_drv;
    bool                    gauss_learner_ok{false};
    okenv_gauss_config      gauss{};
    okenv_learner_params    gauss_learner{};
    int64_t                 gauss_t{0};
    OkUpdateScratch         gauss_scratch;
    // Guided cost learning (okenv_gcl_create, okenv_gcl_learner_create): the three networks [policy | value | cost], each
    // [params | m | v] of gcl_drv.cap floats (gcl_drv.set[which]: the network has its parameters); the expert bank (grown, never shrunk); per network the update's scratch [chunk partials |
    // accumulator] (the policy's also holds its chunks' clip counts) and timing; the advantages' scratch [adv | S, Q partials | mean, std]
    OkDriver                gcl_drv;
    bool                    gcl_learner_ok{false};
    okenv_gcl_config        gcl{};
    okenv_learner_params    gcl_learner{}, gcl_cost_learner{};
    int64_t                 gcl_t{0}, gcl_cost_t{0};
    OkBuffer                gcl_bank; // [state rows | action rows]
    int32_t                 gcl_bank_rows{0};
    OkUpdateScratch         gcl_scratch[3], gcl_adv_scratch;
    // Lidar transformer driver (okenv_lidar_create): the parameter vector in torch's order with the positional table behind it
    OkDriver                lidar_drv;
    okenv_lidar_config      lidar{};
    // Flow-matching driver (okenv_flow_create): the trunk's parameter vector in torch's order
    OkDriver                flow_drv;
    okenv_flow_config       flow{};
    // The flow driver's image encoder (okenv_bev_create): the parameter vector in torch's order; the conv kernels' copy of the weights
    // and the two layers' outputs that pass through global memory, all allocated at create
    OkDriver                bev_drv;
    okenv_bev_config        bev{};
    OkBuffer                bev_pack, bev_act1, bev_act2;
    // Behavioural-cloning image policy (okenv_cnn_create): the parameter vector in torch's order; the kernels' copy of the weights and
    // the features that pass from the conv kernel to the head, both allocated at create
    OkDriver                cnn_drv;
    okenv_cnn_config        cnn{};
    OkBuffer                cnn_pack, cnn_feat;
    // World-model racers (okenv_world_create): the encoder vector in torch's order in world_drv.d; one workspace for everything else
    // (okWorldPlaces: packed weights, controllers, activations, partial latents, fitness, list), allocated at create; the lane widths
    OkDriver                world_drv;
    okenv_world_config      world{};
    OkBuffer                world_ws;
    float                  *d_world_widths{nullptr};
    bool                    world_widths{false};
    // The racers' memory (okenv_memory_create): the network vector in torch's order in mem_drv.d; one workspace for everything else
    // (okMemoryPlaces: packed matrices, controllers, mu, x0 and the two hidden buffers), allocated at create
    OkDriver                mem_drv;
    okenv_memory_config     mem{};
    OkBuffer                mem_ws;
    // ... and its learner (okenv_memory_learner_create): Adam's moments, the step number and every buffer of a minibatch in one
    // workspace (okMemTrainPlaces), allocated at create
    bool                        mem_learn_ok{false};
    okenv_memory_learner_config mem_learn{};
    OkBuffer                    mem_learn_ws;
    // Deep-Q image racers (okenv_qcnn_create, okenv_qcnn_ring_create): the parameter vector in torch's order; the kernels' copy of the
    // weights and the features that pass from the conv kernel to the head, both allocated at create; the frame ring (its planes have
    // the network's image_size) and the push's slot of every agent
    OkDriver                qcnn_drv;
    okenv_qcnn_config       qcnn{};
    OkBuffer                qcnn_pack, qcnn_feat;
    OkRing                  qcnn_ring{sizeof(int64_t)};
    int32_t                 qcnn_ring_side{0};
    long long              *d_qcnn_slots{nullptr};
    // Image transformer driver (okenv_vit_create): the parameter vector in torch's order; the activations of the agents of one pass
    // (vit_pass of them), allocated at create
    OkDriver                vit_drv;
    okenv_vit_config        vit{};
    OkBuffer                vit_work;
    size_t                  vit_pass{0};
    // ... and its head's learner (okenv_vit_head_learner_create): Adam's moments [m | v] of the head's parameters, the step number, the
    // scratch of a minibatch's rows
    bool                    vit_head_ok{false};
    okenv_vit_head_params   vit_head{};
    int64_t                 vit_head_t{0};
    OkBuffer                vit_head_mv;
    OkUpdateScratch         vit_head_scratch;
};

struct okenv_track
{
    std::unique_ptr<RaceTrack> track;
    std::vector<Segment2d>     segments;
};

namespace
{
int fail(okenv *h, const int code, const std::string &msg)
{
    if (h)
        h->last_error = msg;
    else
        g_create_error = msg;
    return code;
}

#define OK_HIP(h, call)                                                                                                \
    do                                                                                                                 \
    {                                                                                                                  \
        const hipError_t e_ = (call);                                                                                  \
        if (e_ != hipSuccess)                                                                                          \
            return fail((h), OKENV_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));                        \
    } while (0)

template <class T>
int devAlloc(okenv *h, T **out, const size_t count)
{
    void *p = nullptr;
    OK_HIP(h, hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)));
    h->allocations.push_back(p); // (owned by the handle from here on, whatever happens next)
    OK_HIP(h, hipMemsetAsync(p, 0, std::max<size_t>(count, 1) * sizeof(T), h->stream));
    *out = static_cast<T *>(p);
    return OKENV_OK;
}

// Buffers that are created on first use, in groups: each one is allocated if it is not there yet, so that a call which ran out of
// memory half-way through its group can simply be repeated (the sizes depend on the handle's N and R only).
template <class T>
int devEnsure(okenv *h, T **out, const size_t count)
{
    return *out != nullptr ? OKENV_OK : devAlloc(h, out, count);
}

// Device staging space owned by the handle, grown on demand.  Each caller waits for the stream before it returns, so one
// buffer serves them all; the stream-ordered pool (hipMallocAsync) is not used anywhere: a tiny upload into pool memory
// that was freed again without a wait gave q_racer_sim's episodes two different outcomes from run to run.
int deviceScratch(okenv *h, const size_t bytes, void **out)
{
    if (bytes > h->scratch_bytes)
    {
        OK_HIP(h, hipStreamSynchronize(h->stream)); // nobody is still reading the old one
        uint8_t *p  = nullptr;
        const int rc = devAlloc(h, &p, bytes + bytes / 2U);
        if (rc != OKENV_OK)
            return rc;
        h->d_scratch     = p;
        h->scratch_bytes = bytes + bytes / 2U;
    }
    *out = h->d_scratch;
    return OKENV_OK;
}

struct FieldDesc
{
    void  *ptr;
    size_t bytes;
};

FieldDesc fieldOf(okenv *h, const int f)
{
    const size_t N = h->shape.N, NR = static_cast<size_t>(h->shape.N) * h->shape.R;
    auto        &s = h->st;
    switch (f)
    {
    case OKENV_F_POS_X: return {s.pos_x, 4 * N};
    case OKENV_F_POS_Y: return {s.pos_y, 4 * N};
    case OKENV_F_ROT: return {s.rot, 4 * N};
    case OKENV_F_SPEED: return {s.speed, 4 * N};
    case OKENV_F_ACC: return {s.acc, 4 * N};
    case OKENV_F_THROTTLE: return {s.thr, 4 * N};
    case OKENV_F_STEER: return {s.steer, 4 * N};
    case OKENV_F_MODE: return {s.mode, N};
    case OKENV_F_CRASHED: return {s.crashed, N};
    case OKENV_F_TIMED_OUT: return {s.timed_out, N};
    case OKENV_F_DISP_CTR: return {s.disp_ctr, 4 * N};
    case OKENV_F_DISP_X: return {s.disp_x, 4 * N};
    case OKENV_F_DISP_Y: return {s.disp_y, 4 * N};
    case OKENV_F_DISP_TO: return {s.disp_to, N};
    case OKENV_F_HIT_X: return {s.hit_x, 4 * NR};
    case OKENV_F_HIT_Y: return {s.hit_y, 4 * NR};
    case OKENV_F_REL_X: return {s.rel_x, 4 * NR};
    case OKENV_F_REL_Y: return {s.rel_y, 4 * NR};
    case OKENV_F_DIST: return {s.dist, 4 * NR};
    case OKENV_F_REWARD: return {h->tracker.reward, h->tracker.reward ? 4 * N : 0};
    case OKENV_F_FITNESS: return {h->tracker.fitness, h->tracker.fitness ? 4 * N : 0};
    case OKENV_F_TRACK_IDX: return {h->tracker.prev_idx, h->tracker.prev_idx ? 4 * N : 0};
    case OKENV_F_EPISODE_STEPS: return {h->tracker.ep_steps, h->tracker.ep_steps ? 4 * N : 0};
    case OKENV_F_EPISODE_RETURN: return {h->tracker.ep_return, h->tracker.ep_return ? 4 * N : 0};
    case OKENV_F_PREV_CRASHED: return {h->tracker.prev_crashed, h->tracker.prev_crashed ? N : 0};
    default: return {nullptr, 0};
    }
}

OkStepParams baseParams(okenv *h)
{
    OkStepParams p{};
    p.st            = h->st;
    p.N             = h->shape.N;
    p.R             = h->shape.R;
    p.G             = h->shape.G;
    p.rays_per_lane = h->shape.rays_per_lane;
    p.ray_deg       = h->d_ray_deg;
    p.sensor_offset = h->sensor_offset;
    p.image         = static_cast<const uint8_t *>(h->d_image);
    p.image_bytes   = static_cast<uint32_t>(h->shape.image_bytes);
    p.off_hdr       = static_cast<uint32_t>(h->poly.off_hdr);
    p.side_tol      = h->poly.side_tol;
    p.geom          = h->grid.g;
    p.g_segs        = h->d_segs;
    p.g_refs32      = h->d_refs32;
    p.g_start       = h->d_start;
    p.S             = h->S;
    p.n_steps       = 1;
    p.do_move       = 1;
    p.action_source = kActionsStored;
    p.cx            = h->d_cx;
    p.cy            = h->d_cy;
    p.chead         = h->d_chead;
    p.P             = h->P;
    p.reset_flags   = h->reset_flags;
    p.reset_seed    = h->reset_seed;
    p.agent_base    = h->reset_agent_base;
    p.step_counter  = h->d_step_count;
    p.agents_per_block = h->shape.coop ? h->shape.agents_per_block : 0;
    p.lane_l        = h->d_lane_l;
    p.lane_r        = h->d_lane_r;
    p.mlp_w         = h->d_mlp_w;
    p.q_table       = h->d_q_table;
    p.q_state       = h->d_q_state;
    p.q_action      = h->d_q_action;
    p.q_prev_idx    = h->d_q_prev;
    for (int i = 0; i < 5; ++i)
        p.q_ray[i] = h->q_ray[i];
    p.q_epsilon = h->q_epsilon;
    p.ctrl_params     = h->d_ctrl_params;
    p.ctrl_num_params = h->ctrl_num_params;
    p.ctrl_hidden     = h->ctrl_hidden;
    p.trk             = h->tracker;
    p.trk_kind        = h->tracker_kind;
    p.cl_start  = h->cl_dirty ? nullptr : h->d_cl_start;
    p.cl_idx    = h->cl_dirty ? nullptr : h->d_cl_idx;
    if (h->episode)
    { // read by the policy kernels only
        p.settled      = h->d_settled;
        p.crash_step   = h->d_crash_step;
        p.crash_thr    = h->d_crash_thr;
        p.crash_steer  = h->d_crash_steer;
        p.live         = h->d_live;
        p.q_next_state = h->d_q_next_state;
        p.ep_step0     = h->ep_steps;
        if (h->n_active >= 0)
        {
            p.active           = h->d_active;
            p.n_active         = h->n_active;
            p.agents_per_block = 0; // listed agents are packed densely
        }
    }
    return p;
}

// An episode ends without its end-of-episode corrections when agent state is changed from outside the policy rollouts.
void dropEpisode(okenv *h)
{
    h->episode    = false;
    h->n_active   = -1;
    h->ep_kind    = 0;
    h->ep_prelist = false;
}

// LDS the Q-learning kernel needs behind the track image: the centre line (8 B per point) and its cell buckets
size_t qLdsBytes(const okenv *h)
{
    const size_t cells = static_cast<size_t>(h->grid.g.nx) * h->grid.g.ny;
    return 8U * static_cast<size_t>(h->P) + 2U * (cells + 1U) + 2U * static_cast<size_t>(h->P) + 16U;
}

// The first rollout of an episode (action_source: kActionsMlpPolicy / kActionsQLearning / kActionsController): a population that fits the tail kernel (the
// reference's 50 agents, say) is listed from the start.  Nobody is settled yet, so the list is 0 ... N-1 and its length is known
// without asking the device -- the very first rollout then already runs one agent per workgroup, each leaving with its agent,
// instead of the cooperative kernel that okenv_episode_compact would only replace after the first launch.  Decided here and not in
// okenv_episode_begin because it depends on the rollout's policy (the Q-learning kernel's tail limit is lower; the controller
// rollout has no tail form), and a handle may have several policies attached.
int prelistEpisode(okenv *h, const int action_source)
{
    if (!h->ep_prelist)
        return OKENV_OK;
    h->ep_prelist = false;
    if (h->n_active >= 0 || !okPrelist(h->shape, action_source, qLdsBytes(h)))
        return OKENV_OK;
    hipLaunchKernelGGL(okEpisodeCompactKernel, dim3(1), dim3(1024), 0, h->stream, h->d_settled, h->st.crashed, h->shape.N, h->d_active, h->d_ep_counts);
    OK_HIP(h, hipGetLastError());
    h->n_active = h->shape.N;
    return OKENV_OK;
}

int beginTiming(okenv *h, EventPair *ev)
{
    if (!h->timing)
        return OKENV_OK;
    if (!h->event_pool.empty())
    {
        *ev = h->event_pool.back();
        h->event_pool.pop_back();
    }
    else
    {
        OK_HIP(h, hipEventCreate(&ev->start));
        OK_HIP(h, hipEventCreate(&ev->stop));
    }
    OK_HIP(h, hipEventRecord(ev->start, h->stream));
    return OKENV_OK;
}

int endTiming(okenv *h, const EventPair &ev)
{
    if (!h->timing)
        return OKENV_OK;
    OK_HIP(h, hipEventRecord(ev.stop, h->stream));
    h->events.push_back(ev);
    return OKENV_OK;
}

// Buckets the centre-line points by the cells of the raycast grid (CSR, indices ascending inside a cell) and uploads
// them; a centre line with more than 65535 points keeps the full scan.
int buildCenterlineBuckets(okenv *h)
{
    if (!h->cl_dirty)
        return OKENV_OK;
    const OkGridGeom &g     = h->grid.g;
    const size_t      cells = static_cast<size_t>(g.nx) * g.ny;
    if (h->P <= 0 || h->P > 65535)
        return OKENV_OK; // stays dirty: the kernel scans the whole line
    std::vector<uint16_t> start(cells + 1U, 0), idx(static_cast<size_t>(h->P));
    std::vector<int>      cell_of(static_cast<size_t>(h->P));
    std::vector<uint32_t> count(cells, 0U);
    for (int i = 0; i < h->P; ++i)
    {
        // same arithmetic as the kernel's lookup; points outside the grid go to the nearest border cell, which only
        // makes their bucket a superset
        int ci = static_cast<int>((h->host_cx[i] - g.x0) * g.inv_cell), cj = static_cast<int>((h->host_cy[i] - g.y0) * g.inv_cell);
        ci     = ci < 0 ? 0 : (ci >= g.nx ? g.nx - 1 : ci);
        cj     = cj < 0 ? 0 : (cj >= g.ny ? g.ny - 1 : cj);
        cell_of[i] = cj * g.nx + ci;
        ++count[static_cast<size_t>(cell_of[i])];
    }
    uint32_t run = 0;
    for (size_t c = 0; c < cells; ++c)
    {
        start[c] = static_cast<uint16_t>(run);
        run += count[c];
    }
    start[cells] = static_cast<uint16_t>(run);
    std::vector<uint32_t> fill(cells, 0U);
    for (int i = 0; i < h->P; ++i)
    {
        const size_t c                = static_cast<size_t>(cell_of[i]);
        idx[start[c] + fill[c]++] = static_cast<uint16_t>(i);
    }
    const size_t need = cells + 1U + static_cast<size_t>(h->P);
    if (need > h->cl_capacity)
    {
        int rc;
        if ((rc = devAlloc(h, &h->d_cl_start, cells + 1U)) || (rc = devAlloc(h, &h->d_cl_idx, static_cast<size_t>(h->P))))
            return rc;
        h->cl_capacity = need;
    }
    OK_HIP(h, hipMemcpyAsync(h->d_cl_start, start.data(), 2U * (cells + 1U), hipMemcpyHostToDevice, h->stream));
    OK_HIP(h, hipMemcpyAsync(h->d_cl_idx, idx.data(), 2U * static_cast<size_t>(h->P), hipMemcpyHostToDevice, h->stream));
    OK_HIP(h, hipStreamSynchronize(h->stream));
    h->cl_dirty = false;
    return OKENV_OK;
}

// ---- resident step kernel ------------------------------------------------------------------------------------------------
// The C++ facade's Environment::step() is one okenv_step_packed per step for 1-50 agents.  Launched one by one, such a
// step costs ~19-22 us of which only ~6 us are the step: 3 us to enqueue the launch, ~3 us until its first wave runs, ~2-3 us
// to stage the track image into LDS again, and the completion.  When the steps follow each other closely the kernel
// therefore stays: every workgroup (one agent each) keeps the image in its LDS and watches its agent's 64-byte slot in
// mapped host memory; the host puts the record there, the workgroup steps it and answers through the same record / hits /
// completion word as a one-shot launch.  The kernel leaves by itself after kResidentIdleTicks without work -- so it can
// never outlive its process by more than that -- or when the host says so; every other entry point of the C ABI stops it
// first (OK_QUIESCE), so nothing else ever runs against the handle's state while it is resident.
constexpr uint32_t kResidentIdleTicks = 30000U; // 100 MHz ticks: 300 us
constexpr double   kResidentGapUs     = 100.0;  // the host treats the kernel as gone after this long without a step
constexpr int      kResidentStreak    = 16;     // quick steps in a row before the kernel is made resident
constexpr int      kResidentShort     = 32;     // a residency that served fewer steps than this quadruples that number
constexpr uint32_t kResidentExit      = 0xFFFFFFFFU;

int stopResident(okenv *h)
{
    if (!h->resident)
        return OKENV_OK;
    volatile uint32_t *slots = reinterpret_cast<volatile uint32_t *>(static_cast<uint8_t *>(h->h_stage) + h->stage_slots_off);
    for (int i = 0; i < h->shape.N; ++i)
        for (int q = 3; q < 16; q += 4)
            slots[16 * i + q] = kResidentExit;
    std::atomic_thread_fence(std::memory_order_seq_cst);
    h->resident      = false;
    h->packed_streak = 0;
    // A residency that ends after a few steps was not worth its start and stop -- and a caller that waits for the whole
    // device between its steps (hipDeviceSynchronize) sits out the kernel's idle time whenever one is resident: back off.
    h->resident_need       = h->resident_served_now < kResidentShort ? std::min(h->resident_need * 4, 1 << 20) : kResidentStreak;
    h->resident_served_now = 0;
    OK_HIP(h, hipStreamSynchronize(h->resident_stream));
    // a step the kernel left half done (it timed out between two workgroups) may have left the finish counter behind
    OK_HIP(h, hipMemsetAsync(h->d_step_count + 1, 0, sizeof(uint32_t), h->stream));
    OK_HIP(h, hipStreamSynchronize(h->stream));
    return OKENV_OK;
}

#define OK_QUIESCE(h)                                                                                                  \
    do                                                                                                                 \
    {                                                                                                                  \
        if ((h) != nullptr && (h)->resident)                                                                           \
        {                                                                                                              \
            const int qrc_ = stopResident(h);                                                                          \
            if (qrc_ != OKENV_OK)                                                                                      \
                return qrc_;                                                                                           \
        }                                                                                                              \
    } while (0)

// sequence numbers of packed steps: 0 is "nothing yet" and kResidentExit the resident kernel's order to leave
uint32_t nextPackedSeq(okenv *h)
{
    h->packed_seq = okNextPackedSeq(h->packed_seq);
    return h->packed_seq;
}

// Points a launch at the [front | back] images instead of the combined one (ok_grid.h: okClassifyFrontBack).
void useFrontBack(const okenv *h, OkStepParams &p)
{
    p.image            = h->d_image_fb;
    p.image_bytes      = static_cast<uint32_t>(h->shape.fb_bytes);
    p.off_hdr          = static_cast<uint32_t>(h->fbi.front.off_hdr);
    p.side_tol         = h->fbi.front.side_tol;
    p.fb               = 1U;
    p.fb_back_off      = static_cast<uint32_t>(h->fb_back_off);
    p.fb_back_off_hdr  = static_cast<uint32_t>(h->fb_back_off + h->fbi.back.off_hdr);
    p.fb_back_side_tol = h->fbi.back.side_tol;
    p.fb_e_s           = h->fbc.e_s;
    p.fb_e_t           = h->fbc.e_t;
    p.fb_t12           = h->fbc.t12;
    p.fb_t34           = h->fbc.t34;
}

// One step-kernel launch of form `form` (enum okenv_step_form) with parameters `p`: counted next to every hipLaunchKernelGGL of a
// step kernel, so that the tests can tell which instantiation a call ran (okenv_debug_step_forms).  Host-side only.
void countForm(okenv *h, const int form, const OkStepParams &p)
{
    uint64_t *c = h->form_counts[form];
    c[0] += 1U;
    c[1 + OKENV_FORM_ATTR_FRONT_BACK] += p.fb != 0U ? 1U : 0U;
    c[1 + OKENV_FORM_ATTR_LIST] += p.active != nullptr ? 1U : 0U;
    c[1 + OKENV_FORM_ATTR_WIDENED] += p.G > h->shape.G ? 1U : 0U;
    c[1 + OKENV_FORM_ATTR_CTRL_LDS] += p.ctrl_lds_off != 0U ? 1U : 0U;
    c[1 + OKENV_FORM_ATTR_AGENTS_PER_BLOCK] += p.agents_per_block > 0 ? 1U : 0U;
}

// Every step-kernel launch of the library: asks the launch policy (okPlanStep) for a plan, applies it to `p` and launches the
// plan's form -- the one hipLaunchKernelGGL under its case label below.
int launchStep(okenv *h, OkStepParams p) // (by value: the plan is applied to it)
{
    OK_HIP(h, hipSetDevice(h->device));
    EventPair ev{};
    int       rc = beginTiming(h, &ev);
    if (rc != OKENV_OK)
        return rc;
    OkStepRequest rq;
    rq.action_source   = p.action_source;
    rq.n_listed        = p.active != nullptr ? p.n_active : -1;
    rq.packed          = p.rec_in != nullptr;
    rq.resident        = p.slots != nullptr;
    rq.do_move         = p.do_move;
    rq.reset_flags     = p.reset_flags;
    rq.ctrl_num_params = h->ctrl_num_params;
    rq.q_bytes         = qLdsBytes(h);
    const OkStepPlan plan = okPlanStep(h->shape, rq);
    if (plan.front_back)
        useFrontBack(h, p);
    p.G            = plan.G;
    p.ctrl_lds_off = plan.ctrl_lds_off;
#if defined(OKENV_STAMPS)
    { // diagnostic build: stamp space for every wave of THIS launch (the grid differs between populations, lists and forms).  Tail
      // kernel: [0] policy, [1] pre-step, [3] interval walk + min, [5] epilogue, [6] barrier, [7] crash test + Q-learning; [2] / [4] start / end
        if (plan.waves() > h->stamp_waves_cap)
        {
            unsigned long long *d = nullptr;
            const int           src = devAlloc(h, &d, plan.waves() * kStampWords);
            if (src != OKENV_OK)
                return src;
            h->d_stamps        = d;
            h->stamp_waves_cap = plan.waves();
        }
        h->stamp_waves = plan.waves();
        p.stamps       = h->d_stamps;
    }
#endif
    countForm(h, plan.form, p);
    const dim3        grid(plan.grid), block(plan.block);
    const size_t      lds    = plan.lds;
    const uint32_t    off    = plan.image_off;
    const float       phase1 = plan.phase1;
    const hipStream_t stream = rq.resident ? h->resident_stream : h->stream;
    switch (plan.form)
    { // (the kernels lie in the code object in the order of these cases)
    case OKENV_FORM_RESIDENT_DIRECT: // (the image is staged once for the kernel's whole residency)
        hipLaunchKernelGGL((okStepCoopKernel<kPolicyNone, true, true, true>), grid, block, lds, stream, p, off, phase1);
        break;
    case OKENV_FORM_RESIDENT:
        hipLaunchKernelGGL((okStepCoopKernel<kPolicyNone, true, true>), grid, block, lds, stream, p, off, phase1);
        break;
    case OKENV_FORM_TAIL_Q:
        hipLaunchKernelGGL((okStepTailKernel<kPolicyQ, 0>), grid, block, lds, stream, p, off);
        break;
    case OKENV_FORM_TAIL_MLP32:
        hipLaunchKernelGGL((okStepTailKernel<kPolicyMlp, 32>), grid, block, lds, stream, p, off);
        break;
    case OKENV_FORM_TAIL_MLP15:
        hipLaunchKernelGGL((okStepTailKernel<kPolicyMlp, 15>), grid, block, lds, stream, p, off);
        break;
    case OKENV_FORM_TAIL_MLP:
        hipLaunchKernelGGL((okStepTailKernel<kPolicyMlp, 0>), grid, block, lds, stream, p, off);
        break;
    case OKENV_FORM_COOP_Q:
        hipLaunchKernelGGL(okStepCoopKernel<kPolicyQ>, grid, block, lds, stream, p, off, phase1);
        break;
    case OKENV_FORM_COOP_CTRL:
        hipLaunchKernelGGL(okStepCoopKernel<kPolicyCtrl>, grid, block, lds, stream, p, off, phase1);
        break;
    case OKENV_FORM_COOP_MLP32:
        hipLaunchKernelGGL((okStepCoopKernel<kPolicyMlp, false, false, false, 32>), grid, block, lds, stream, p, off, phase1);
        break;
    case OKENV_FORM_COOP_MLP:
        hipLaunchKernelGGL(okStepCoopKernel<kPolicyMlp>, grid, block, lds, stream, p, off, phase1);
        break;
    case OKENV_FORM_COOP_PACKED_DIRECT:
        hipLaunchKernelGGL((okStepCoopKernel<kPolicyNone, true, false, true>), grid, block, lds, stream, p, off, phase1);
        break;
    case OKENV_FORM_COOP_PACKED:
        hipLaunchKernelGGL((okStepCoopKernel<kPolicyNone, true>), grid, block, lds, stream, p, off, phase1);
        break;
    case OKENV_FORM_COOP_DIRECT:
        hipLaunchKernelGGL((okStepCoopKernel<kPolicyNone, false, false, true>), grid, block, lds, stream, p, off, phase1);
        break;
    case OKENV_FORM_COOP_G64_RANDOM:
        hipLaunchKernelGGL((okStepCoopKernel<kPolicyNone, false, false, false, 64, true>), grid, block, lds, stream, p, off, phase1);
        break;
    case OKENV_FORM_COOP_G64:
        hipLaunchKernelGGL((okStepCoopKernel<kPolicyNone, false, false, false, 64>), grid, block, lds, stream, p, off, phase1);
        break;
    case OKENV_FORM_COOP:
        hipLaunchKernelGGL(okStepCoopKernel<kPolicyNone>, grid, block, lds, stream, p, off, phase1);
        break;
    case OKENV_FORM_LDS_MLP:
        hipLaunchKernelGGL((okStepKernel<kGridLds, kPolicyMlp>), grid, block, lds, stream, p);
        break;
    case OKENV_FORM_LDS:
        hipLaunchKernelGGL((okStepKernel<kGridLds, kPolicyNone>), grid, block, lds, stream, p);
        break;
    case OKENV_FORM_GLOBAL_MLP:
        hipLaunchKernelGGL((okStepKernel<kGridGlobal, kPolicyMlp>), grid, block, lds, stream, p);
        break;
    case OKENV_FORM_GLOBAL:
        hipLaunchKernelGGL((okStepKernel<kGridGlobal, kPolicyNone>), grid, block, lds, stream, p);
        break;
    case OKENV_FORM_BRUTE_MLP:
        hipLaunchKernelGGL((okStepKernel<kGridBrute, kPolicyMlp>), grid, block, lds, stream, p);
        break;
    case OKENV_FORM_BRUTE:
        hipLaunchKernelGGL((okStepKernel<kGridBrute, kPolicyNone>), grid, block, lds, stream, p);
        break;
    }
    OK_HIP(h, hipGetLastError());
    return endTiming(h, ev);
}

// Starts the resident kernel on a stream of its own; `p` carries the exchange pointers of okenv_step_packed.
int startResident(okenv *h, OkStepParams p, volatile uint32_t *slots)
{
    OK_HIP(h, hipStreamSynchronize(h->stream)); // whatever was enqueued against the state comes first
    if (!h->resident_stream)
        OK_HIP(h, hipStreamCreateWithFlags(&h->resident_stream, hipStreamNonBlocking));
    for (int i = 0; i < 16 * h->shape.N; ++i)
        slots[i] = 0U;
    std::atomic_thread_fence(std::memory_order_seq_cst);
    p.done_seq = okNextPackedSeq(h->packed_seq); // the first number the kernel waits for
    const int rc = launchStep(h, p); // (p.slots makes it the resident form)
    if (rc != OKENV_OK)
        return rc;
    h->resident = true;
    return OKENV_OK;
}

// One step through the resident kernel: the records go into the agents' slots, the sequence number after them; then the
// host waits for the completion word.  *served is false when nobody answered (the kernel had left: idle for too long, e.g.
// because this thread was descheduled): the kernel is drained and the caller redoes the step with a launch of its own, which
// works from the same input records.
int stepResident(okenv *h, const okenv_agent_record *in, volatile uint32_t *slots, const volatile uint32_t *done_word, const bool just_started,
                 bool *served)
{
    if (h->resident_stall_us > 0 && h->resident_steps % 7 == 6)
    { // (tests only) every seventh resident step comes too late
        const auto until = std::chrono::steady_clock::now() + std::chrono::microseconds(h->resident_stall_us);
        while (std::chrono::steady_clock::now() < until)
        {
        }
    }
    const uint32_t seq = nextPackedSeq(h);
    const size_t   N   = static_cast<size_t>(h->shape.N);
    for (size_t i = 0; i < N; ++i)
    { // record word j goes to slot word j + j / 3: words 3, 7, 11, 15 of a slot carry the sequence number
        uint32_t w[sizeof(okenv_agent_record) / 4U];
        std::memcpy(w, &in[i], sizeof(okenv_agent_record));
        for (unsigned j = 0; j < sizeof(okenv_agent_record) / 4U; ++j)
            slots[16U * i + j + j / 3U] = w[j];
    }
    std::atomic_thread_fence(std::memory_order_release); // records before sequence numbers (and x86 keeps store order)
    for (size_t i = 0; i < N; ++i)
        for (unsigned q = 3; q < 16U; q += 4U)
            slots[16U * i + q] = seq;
    bool       answered = false;
    const auto t_asked  = std::chrono::steady_clock::now();
    while (!answered)
    {
        for (int spin = 0; spin < 1024 && !answered; ++spin)
        {
            answered = *done_word == seq;
            if (!answered)
                okCpuRelax();
        }
        if (answered)
            break;
        // (a kernel launched a moment ago may still be on its way -- the first launch of a process loads the code object -- and
        // its patience only starts when it does)
        const double waited_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_asked).count();
        // Giving up on a kernel that is merely slow is safe because a packed step is a pure function of the input records: the
        // resident instantiation (kPacked && kResident) takes ALL agent state from the slot, never advances step_counter[0]
        // (auto-reset makes a handle ineligible) and writes only the exchange buffers and the per-ray arrays, which the redo
        // overwrites with the same values.  Anything added to the resident form that accumulates device state breaks this.
        if (waited_us > (just_started ? 2.0e6 : 2.5 * kResidentGapUs))
        { // ... and only a kernel that has really left is given up on: one that is still on its stream is merely slow (it polls
          // its slot every few hundred nanoseconds, so it has the step) and will answer -- up to a bound, so that a hung device
          // ends in the launch path's error and not in an endless wait
            if (!just_started && waited_us < 20000.0 && hipStreamQuery(h->resident_stream) == hipErrorNotReady)
                continue;
            break;
        }
        if (just_started && waited_us > 1000.0 && hipStreamQuery(h->resident_stream) != hipErrorNotReady)
            break; // its stream has drained (or failed): nobody is going to answer
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    ++h->resident_steps;
    ++h->resident_served_now;
    *served = answered;
    if (!answered)
    {
        ++h->resident_fallbacks;
        return stopResident(h);
    }
    return OKENV_OK;
}

// okenv_step_packed: the step kernel's last workgroup stores the launch's sequence number into mapped host memory once all
// results are there.  Spinning on that word returns about 5 us earlier than hipStreamSynchronize (which waits for the
// queue's completion signal: 10.9 us against 6.0 us for an empty kernel on this machine).  The stream is asked now and
// then, so that a failed launch ends in an error and not in an endless wait.
constexpr size_t kDoneWordBytes = 128;

int waitPackedDone(okenv *h, const volatile uint32_t *word, const uint32_t seq)
{
    for (;;)
    {
        for (int spin = 0; spin < 4096; ++spin)
        {
            if (*word == seq)
            {
                std::atomic_thread_fence(std::memory_order_acquire);
                return OKENV_OK;
            }
            okCpuRelax();
        }
        const hipError_t q = hipStreamQuery(h->stream);
        if (q == hipErrorNotReady)
            continue;
        if (q != hipSuccess)
            return fail(h, OKENV_ERR_HIP, std::string("okenv_step_packed: ") + hipGetErrorString(q));
        // the stream has drained: the word is there by now, or the kernel never got to write it
        std::atomic_thread_fence(std::memory_order_acquire);
        if (*word == seq)
            return OKENV_OK;
        return fail(h, OKENV_ERR_HIP, "okenv_step_packed: the step kernel finished without announcing it");
    }
}

// The step counter also lives on the device (it is the epoch of the auto-reset draws and must advance when a captured
// graph of the step is replayed): okFinishLaunch at the end of the step kernels.
int advanceStepCount(okenv *h, const int n_steps)
{
    h->step_count += static_cast<uint32_t>(n_steps); // the device copy is advanced by the step kernel itself
    return OKENV_OK;
}

int copyAny(okenv *h, void *dst, const void *src, const size_t bytes)
{
    if (bytes == 0)
        return OKENV_OK;
    OK_HIP(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, h->stream));
    return OKENV_OK;
}

// Buffers of the handle replaced by fresh, zeroed ones (every buffer that is allocated anew on a live handle goes through here): waits
// for the stream, since an earlier call may still be working in the old ones; releases those from `allocations` and frees them; then
// allocates each anew.  After a failure the slots that were not reached are nullptr, and the caller's sizes and flags say so already.
struct OkFresh
{
    void **slot;
    size_t bytes;
};

template <class T>
OkFresh fresh(T *&slot, const size_t count)
{
    return OkFresh{reinterpret_cast<void **>(&slot), std::max<size_t>(count, 1) * sizeof(T)};
}

int regrow(okenv *h, const std::vector<OkFresh> &buffers)
{
    OK_HIP(h, hipStreamSynchronize(h->stream));
    for (const OkFresh &b : buffers)
        if (*b.slot != nullptr)
        {
            h->allocations.erase(std::remove(h->allocations.begin(), h->allocations.end(), *b.slot), h->allocations.end());
            (void)hipFree(*b.slot);
            *b.slot = nullptr;
        }
    for (const OkFresh &b : buffers)
    {
        uint8_t *p = nullptr;
        if (const int rc = devAlloc(h, &p, b.bytes))
            return rc;
        *b.slot = p;
    }
    return OKENV_OK;
}

// Buffers of the handle that grow and never shrink (OkBuffer; a driver's vector), brought to what a call needs.  Nothing happens when
// every need fits its room.  Otherwise all of them are replaced through regrow -- its wait for the stream, its zeroed memory -- each
// with the larger of its need and its room; the rooms are zero while the allocation is under way, so that a failed one leaves none.
struct OkGrow
{
    float **slot;
    size_t *cap;
    size_t  need; // floats
};

OkGrow grown(OkBuffer &b, const size_t need)
{
    return OkGrow{&b.d, &b.cap, need};
}

int growBuffers(okenv *h, const std::initializer_list<OkGrow> buffers)
{
    if (std::all_of(buffers.begin(), buffers.end(), [](const OkGrow &b) { return b.need <= *b.cap; }))
        return OKENV_OK;
    std::vector<OkGrow>  all(buffers);
    std::vector<OkFresh> anew;
    for (OkGrow &b : all)
    {
        b.need = std::max(b.need, *b.cap);
        *b.cap = 0;
        anew.push_back(fresh(*b.slot, b.need));
    }
    if (const int rc = regrow(h, anew))
        return rc;
    for (const OkGrow &b : all)
        *b.cap = b.need;
    return OKENV_OK;
}

// A scratch buffer of the handle that grows to 1.5 x what a call needs and never shrinks (the updates' chunk partials, the batch's
// planes)
int growScratch(okenv *h, OkUpdateScratch &u, const size_t bytes)
{
    if (bytes <= u.bytes)
        return OKENV_OK;
    u.bytes = 0;
    if (const int rc = regrow(h, {fresh(u.part, bytes + bytes / 2U)}))
        return rc;
    u.bytes = bytes + bytes / 2U;
    return OKENV_OK;
}

// The dynamic-LDS limit of each kernel raised, to the whole budget unless the site knows its need
template <class Kernel>
const void *kernelOf(Kernel *kernel)
{
    return reinterpret_cast<const void *>(kernel);
}

int raiseLdsLimit(okenv *h, const std::initializer_list<const void *> kernels, const size_t bytes = kLdsBudget)
{
    for (const void *k : kernels)
        OK_HIP(h, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes)));
    return OKENV_OK;
}

// ---- the event log of an update or a batch: eventsBegin before the first launch, eventsMark behind every launch, eventsSums afterwards ----------

// (With okenv_set_timing off the call runs untimed, and the log says so.)
int eventsBegin(okenv *h, OkEventLog &log, const size_t launches)
{
    log.timed = log.at = 0;
    log.want  = h->timing ? launches + 1U : 0U;
    if (log.want == 0U)
        return OKENV_OK;
    while (log.events.size() < log.want)
    {
        hipEvent_t e = nullptr;
        OK_HIP(h, hipEventCreate(&e));
        log.events.push_back(e);
    }
    OK_HIP(h, hipEventRecord(log.events[0], h->stream));
    return OKENV_OK;
}

// (The log is complete, and eventsSums has something to answer, only once the call's last launch has its event.)
int eventsMark(okenv *h, OkEventLog &log)
{
    if (log.want == 0U)
        return OKENV_OK;
    OK_HIP(h, hipEventRecord(log.events[++log.at], h->stream));
    if (log.at + 1U == log.want)
        log.timed = log.want;
    return OKENV_OK;
}

// out[k]: the device time, in milliseconds, of the launches number k mod period of the latest timed call
int eventsSums(okenv *h, OkEventLog &log, double *out, const size_t period)
{
    OK_HIP(h, hipEventSynchronize(log.events[log.timed - 1U]));
    for (size_t k = 0; k < period; ++k)
        out[k] = 0.0;
    for (size_t k = 0; k + 1U < log.timed; ++k)
    {
        float ms = 0.F;
        OK_HIP(h, hipEventElapsedTime(&ms, log.events[k], log.events[k + 1U]));
        out[k % period] += ms;
    }
    return OKENV_OK;
}

// The okenv_debug_*_timing entries, behind the exported functions' OK_QUIESCE: out[period] of the latest timed call of `update`
int updateTiming(okenv *h, OkUpdateScratch okenv::*scratch, const char *entry, const char *update, double *out, const size_t period)
{
    if (!h || !out)
        return fail(h, OKENV_ERR_INVALID, std::string(entry) + ": NULL argument");
    if ((h->*scratch).log.timed < period + 1U)
        return fail(h, OKENV_ERR_STATE, std::string(entry) + ": no " + update + " has run with okenv_set_timing on");
    return eventsSums(h, (h->*scratch).log, out, period);
}

// ---- the act kernels' frame and the whole-episode updates' loop, behind the exported functions' OK_QUIESCE ------------------------------------

// What okenv_actor_act, okenv_ddpg_act and okenv_gauss_act hand their kernels alike (ok_actor.h); draw_offset: the learner's own word
OkActFrame actFrame(const okenv *h)
{
    OkActFrame f{};
    f.st = h->st;
    f.N  = h->shape.N;
    f.R  = h->shape.R;
    return f;
}

OkActDrawWords actDrawWords(const okenv *h, const uint32_t *draw_offset)
{
    OkActDrawWords w{};
    w.step_word   = (h->reset_flags & kAutoResetOn) != 0U ? h->d_step_count : nullptr; // (the step kernels advance it only then)
    w.host_steps  = h->step_count;
    w.draw_offset = draw_offset;
    return w;
}

// okenv_reinforce_update's and okenv_gauss_update's slices: two launches each, the learner's gradient kernel and the join kernel
// (ok_reinforce.h).  j is okJoinOn's (the parameter vector, its moments, reduce and the gradient's output); t is the learner's step number,
// lp its Adam; loss takes one value per step, or is nullptr.  launch_grad(base, Bk, C) enqueues the gradient kernel of the slice of Bk
// positions from `base` on, C workgroups writing to u.part.
template <class LaunchGrad>
int sliceUpdate(okenv *h, OkUpdateScratch &u, const int32_t M, const int32_t B, const bool accumulate, OkJoinParams j, int64_t &t,
                const okenv_learner_params &lp, float *loss, const LaunchGrad &launch_grad)
{
    // the scratch: [chunk partials | accumulator], each piece 256-aligned
    const auto   up    = [](const size_t b) { return (b + 255U) & ~static_cast<size_t>(255U); };
    const size_t c_max = (static_cast<size_t>(std::min(B, M)) + OK_LEARN_CHUNK - 1U) / OK_LEARN_CHUNK;
    const size_t parts = up(sizeof(float) * c_max * static_cast<size_t>(j.cols)), acc_bytes = sizeof(float) * static_cast<size_t>(j.cols);
    if (const int rc = growScratch(h, u, parts + up(acc_bytes)))
        return rc;
    j.part = reinterpret_cast<float *>(u.part);
    if (accumulate)
    {
        j.acc = reinterpret_cast<float *>(u.part + parts);
        OK_HIP(h, hipMemsetAsync(j.acc, 0, acc_bytes, h->stream));
    }
    const int slices = okLearnMinibatches(M, B);
    if (const int rc = eventsBegin(h, u.log, 2U * static_cast<size_t>(slices)))
        return rc;
    const unsigned step_grid = static_cast<unsigned>((j.cols + kLearnStepCols - 1) / kLearnStepCols);
    int            slot      = 0;
    for (int k = 0; k < slices; ++k)
    {
        const long base = static_cast<long>(k) * B;
        const int  Bk   = static_cast<int>(std::min<long>(B, M - base));
        j.C             = (Bk + OK_LEARN_CHUNK - 1) / OK_LEARN_CHUNK;
        launch_grad(base, Bk, j.C);
        OK_HIP(h, hipGetLastError());
        if (const int rc = eventsMark(h, u.log))
            return rc;
        if (accumulate && k + 1 < slices)
        {
            hipLaunchKernelGGL(okReinforceStepKernel<false>, dim3(step_grid), dim3(kLearnStepCols * kLearnStepRows), 0, h->stream, j);
            OK_HIP(h, hipGetLastError());
        }
        else
        {
            j.count = static_cast<float>(accumulate ? M : Bk);
            j.adam  = okLearnAdamConsts(lp, t + 1);
            j.loss  = loss != nullptr ? loss + slot : nullptr;
            hipLaunchKernelGGL(okReinforceStepKernel<true>, dim3(step_grid), dim3(kLearnStepCols * kLearnStepRows), 0, h->stream, j);
            OK_HIP(h, hipGetLastError());
            // (the step number advances once the step's kernels are enqueued, as in okenv_ppo_update)
            t += 1;
            ++slot;
        }
        if (const int rc = eventsMark(h, u.log))
            return rc;
    }
    return OKENV_OK;
}

// Guided cost learning's vectors in gcl_drv.d: network `which` (OKENV_GCL_POLICY / _VALUE / _COST), vector k (0 params, 1 m, 2 v)
float *gclVector(const okenv *h, const int which, const int k)
{
    return h->gcl_drv.d + (static_cast<size_t>(which) * 3U + static_cast<size_t>(k)) * h->gcl_drv.cap;
}

// floats of the handle's networks as their configs stand
int actorPolicyParams(const okenv *h)
{
    return ok_actor_num_params(h->shape.R, h->actor.hidden, h->actor.num_actions);
}

int actorValueParams(const okenv *h)
{
    return h->actor.value_hidden > 0 ? ok_actor_num_params(h->shape.R, h->actor.value_hidden, 1) : 0;
}

int ddpgActorParams(const okenv *h)
{
    return ok_actor_num_params(h->shape.R, h->ddpg.hidden, 2);
}

int ddpgCriticParams(const okenv *h)
{
    return ok_ddpg_critic_params(h->shape.R, h->ddpg.critic_hidden);
}

int gaussNumParams(const okenv *h)
{
    return ok_gauss_num_params(h->shape.R, h->gauss.hidden1, h->gauss.hidden2, 2);
}

int gclNumParams(const okenv *h, const int which)
{
    const bool cost = which == OKENV_GCL_COST;
    return ok_gcl_num_params(which, h->shape.R, cost ? h->gcl.cost_hidden1 : h->gcl.hidden1, cost ? h->gcl.cost_hidden2 : h->gcl.hidden2);
}

// ---- the drivers' life cycle, behind the exported functions' OK_QUIESCE ("The drivers' life cycle on the host") ---------------

// Which family an exported entry works on: its record in the handle, the prefix of its entries' names (for the messages), who "needs its
// parameters" in act's refusal and in get's, and whether num_params and set_params look at their pointer before the state (the
// families that came after the first four do, and refuse a NULL out pointer of num_params; the others write nothing through one).
// The flat-vector families (one vector in torch's order that grows on demand: lidar, flow and the six image families) describe
// themselves further, and their shared entries below (flatNumParams, flatSetParams, flatGetParams, actBeginFrames) read nothing else.
struct DriverKind
{
    OkDriver okenv::*drv;
    const char      *prefix;
    const char      *act_needs, *get_needs;
    bool             argument_first;
    int (*total)(const okenv *h);      // the floats of vector 0 as the stored config stands
    int (*repack)(okenv *h);           // nullptr, or: enqueues the kernels that rebuild the conv / GRU kernels' copy of the weights behind an upload
    int (*image_size)(const okenv *h); // nullptr, or: the side of the frames the act takes
    // world and memory: vector 1, [N][controller] inside the workspace, with set flag 1
    int (*controller)(const okenv *h);     // nullptr, or: the floats of one agent's controller
    float *(*controllers)(const okenv *h); // ... where the agents' controllers begin
    const char *which;                     // ... and the two names of `which`, for the refusal
};

// The kernels' copy of a conv family's weights (cnn, qcnn, bev, world): one thread per float of the pack, behind the upload on the stream
template <class Params, class Shape>
int packLaunch(okenv *h, void (*kernel)(Params), const Shape &s, const float *params, float *pack, const int pack_total)
{
    Params p{};
    p.s      = s;
    p.params = params;
    p.pack   = pack;
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>((pack_total + 255) / 256)), dim3(256), 0, h->stream, p);
    OK_HIP(h, hipGetLastError());
    return OKENV_OK;
}

ok_memory_shape memoryShape(const okenv *h)
{
    return okMemoryShape(h->world, h->mem);
}

int memoryRepack(okenv *h); // (beside okenv_memory_act's launches)

static_assert(kBevThreads == 256 && OKENV_WORLD_ENCODER == 0 && OKENV_WORLD_CONTROLLERS == 1 && OKENV_MEMORY_NETWORK == 0 && OKENV_MEMORY_CONTROLLERS == 1,
              "packLaunch's block and the shared entries' `which`");

const DriverKind kActorDriver{&okenv::actor_drv, "okenv_actor_", "every attached network needs its parameters", nullptr, false},
    kDdpgDriver{&okenv::ddpg_drv, "okenv_ddpg_", "the actor needs its parameters", "both networks need their parameters", false},
    kGaussDriver{&okenv::gauss_drv, "okenv_gauss_", "the actor needs its parameters", "the actor needs its parameters", false},
    kGclDriver{&okenv::gcl_drv, "okenv_gcl_", "the policy needs its parameters", "the network needs its parameters", false},
    kLidarDriver{&okenv::lidar_drv, "okenv_lidar_", "the policy needs its parameters", "the policy needs its parameters", true,
                 [](const okenv *h) { return ok_lidar_offsets(okLidarShape(h->lidar)).total; }},
    kFlowDriver{&okenv::flow_drv, "okenv_flow_", "the policy needs its parameters", "the policy needs its parameters", true,
                [](const okenv *h) { return ok_flow_offsets(okFlowShape(h->flow)).total; }},
    kBevDriver{&okenv::bev_drv, "okenv_bev_", "the encoder needs its parameters", "the encoder needs its parameters", true,
               [](const okenv *h) { return ok_bev_offsets(okBevShape(h->bev)).total; },
               [](okenv *h) {
                   const ok_bev_shape s = okBevShape(h->bev);
                   return packLaunch(h, okBevPackKernel, s, h->bev_drv.d, h->bev_pack.d, okBevPlaces(s).pack_total);
               },
               nullptr}, // (okenv_bev_encode checks its frames itself, behind its output)
    kCnnDriver{&okenv::cnn_drv, "okenv_cnn_", "the policy needs its parameters", "the policy needs its parameters", true,
               [](const okenv *h) { return ok_cnn_offsets(okCnnShape(h->cnn)).total; },
               [](okenv *h) {
                   const ok_cnn_shape s = okCnnShape(h->cnn);
                   return packLaunch(h, okCnnPackKernel, s, h->cnn_drv.d, h->cnn_pack.d, okCnnPlaces(s).pack_total);
               },
               [](const okenv *h) { return h->cnn.image_size; }},
    kWorldDriver{&okenv::world_drv, "okenv_world_", "the encoder and the controllers need their parameters", "the vector needs its parameters", true,
                 [](const okenv *h) { return ok_world_offsets(okWorldShape(h->world)).total; },
                 [](okenv *h) {
                     const ok_world_shape s = okWorldShape(h->world);
                     return packLaunch(h, okWorldPackKernel, s, h->world_drv.d, h->world_ws.d, okWorldPlaces(s, static_cast<size_t>(h->shape.N)).pack_total);
                 },
                 [](const okenv *h) { return h->world.image_size; },
                 [](const okenv *h) { return ok_world_controller_params(okWorldShape(h->world)); },
                 [](const okenv *h) { return h->world_ws.d + okWorldPlaces(okWorldShape(h->world), static_cast<size_t>(h->shape.N)).ctrl; },
                 "OKENV_WORLD_ENCODER or OKENV_WORLD_CONTROLLERS"},
    kMemoryDriver{&okenv::mem_drv, "okenv_memory_", "the network and the controllers need their parameters", "the vector needs its parameters", true,
                  [](const okenv *h) { return ok_memory_offsets(memoryShape(h)).total; },
                  memoryRepack,
                  [](const okenv *h) { return h->world.image_size; }, // (the racers' frames)
                  [](const okenv *h) { return ok_memory_controller_params(memoryShape(h)); },
                  [](const okenv *h) { return h->mem_ws.d + okMemoryPlaces(memoryShape(h), static_cast<size_t>(h->shape.N)).ctrl; },
                  "OKENV_MEMORY_NETWORK or OKENV_MEMORY_CONTROLLERS"},
    kQcnnDriver{&okenv::qcnn_drv, "okenv_qcnn_", "the network needs its parameters", "the network needs its parameters", true,
                [](const okenv *h) { return ok_qcnn_offsets(okQcnnShape(h->qcnn)).total; },
                [](okenv *h) {
                    const ok_qcnn_shape s = okQcnnShape(h->qcnn);
                    return packLaunch(h, okQcnnPackKernel, s, h->qcnn_drv.d, h->qcnn_pack.d, okQcnnPlaces(s).pack_total);
                },
                [](const okenv *h) { return h->qcnn.image_size; }},
    kVitDriver{&okenv::vit_drv, "okenv_vit_", "the policy needs its parameters", "the policy needs its parameters", true,
               [](const okenv *h) { return ok_vit_offsets(okVitShape(h->vit)).total; }, nullptr, [](const okenv *h) { return h->vit.image_size; }};

int driverRefuses(okenv *h, const int code, const DriverKind &k, const char *entry, const std::string &why)
{
    return fail(h, code, std::string(k.prefix) + entry + ": " + why);
}

// The refusals an entry can have, in the order in which the gate looks at them
enum : unsigned
{
    kGateHandle   = 1U,  // a NULL handle is INVALID "NULL handle" (create, act)
    kGateArgFirst = 2U,  // a NULL handle or argument is INVALID "NULL argument", before the state
    kGateCreated  = 4U,  // STATE "call ..create first"; also for a NULL handle, which none of the above caught
    kGateStored   = 8U,  // get's: STATE "<who> needs its parameters first (..create, ..set_params)" unless created and set
    kGateSet      = 16U, // act's: STATE "call ..set_params first (<who> needs its parameters)" unless set
    kGateArgLast  = 32U, // a NULL argument is INVALID "NULL argument", behind the state
};

// need: the set flags (bit i for set[i]) that kGateStored / kGateSet ask for
int driverGate(okenv *h, const DriverKind &k, const char *entry, const unsigned checks, const bool argument = true, const unsigned need = 0U)
{
    const auto prefix = [&k] { return std::string(k.prefix); }; // (only a refusal builds a string)
    if ((checks & kGateHandle) != 0U && !h)
        return driverRefuses(h, OKENV_ERR_INVALID, k, entry, "NULL handle");
    if ((checks & kGateArgFirst) != 0U && (!h || !argument))
        return driverRefuses(h, OKENV_ERR_INVALID, k, entry, "NULL argument");
    const OkDriver *d = h != nullptr ? &(h->*k.drv) : nullptr;
    const bool created = d != nullptr && d->ok;
    bool       set     = created;
    for (unsigned i = 0; set && i < 3U; ++i)
        set = (need >> i & 1U) == 0U || d->set[i];
    if ((checks & kGateStored) != 0U && !set)
        return driverRefuses(h, OKENV_ERR_STATE, k, entry, std::string(k.get_needs) + " first (" + prefix() + "create, " + prefix() + "set_params)");
    if ((checks & kGateCreated) != 0U && !created)
        return driverRefuses(h, OKENV_ERR_STATE, k, entry, "call " + prefix() + "create first");
    if ((checks & kGateSet) != 0U && !set)
        return driverRefuses(h, OKENV_ERR_STATE, k, entry, "call " + prefix() + "set_params first (" + k.act_needs + ")");
    if ((checks & kGateArgLast) != 0U && !argument)
        return driverRefuses(h, OKENV_ERR_INVALID, k, entry, "NULL argument");
    return OKENV_OK;
}

// okenv_*_create of the families of fixed capacity, behind their gate and config check: room for the widest network once (`vectors` of
// `cap` floats in d, `vectors2` in d2), so that a later create with other widths allocates nothing; the kernels' LDS limit; the vectors
// zeroed on the stream where the family keeps Adam's moments among them.  The caller stores its config and resets its own dependants.
int driverCreateFixed(okenv *h, const DriverKind &k, const size_t cap, const size_t vectors, const size_t vectors2, const bool zero,
                      const std::initializer_list<const void *> kernels)
{
    OkDriver &d = h->*k.drv;
    d.cap       = cap;
    int rc      = devEnsure(h, &d.d, vectors * cap);
    if (rc != OKENV_OK || (vectors2 > 0U && (rc = devEnsure(h, &d.d2, vectors2 * cap)) != OKENV_OK) || (rc = raiseLdsLimit(h, kernels)) != OKENV_OK)
        return rc;
    if (zero)
    {
        OK_HIP(h, hipMemsetAsync(d.d, 0, vectors * cap * sizeof(float), h->stream));
        if (vectors2 > 0U)
            OK_HIP(h, hipMemsetAsync(d.d2, 0, vectors2 * cap * sizeof(float), h->stream));
    }
    d.ok = true;
    for (bool &set : d.set)
        set = false;
    return OKENV_OK;
}

// okenv_*_create of the flat-vector families, behind their gate, config check and own refusals: detached and the parameters forgotten
// before anything is allocated, so that a failure leaves the driver so; the vector's room is kept when it suffices; the kernels' LDS
// limits; then the family's other buffers (`buffers`: as one group, growBuffers).  The driver stays detached: the caller resets what
// depends on the network, stores its config and only then says that the driver is created.
int driverCreateFlat(okenv *h, const DriverKind &k, const size_t total, const std::initializer_list<const void *> kernels,
                     const std::initializer_list<OkGrow> buffers = {})
{
    OK_HIP(h, hipSetDevice(h->device));
    OkDriver &d = h->*k.drv;
    d.ok        = false;
    for (bool &set : d.set)
        set = false;
    if (const int rc = growBuffers(h, {OkGrow{&d.d, &d.cap, total}}))
        return rc;
    if (const int rc = raiseLdsLimit(h, kernels))
        return rc;
    return growBuffers(h, buffers);
}

// One parameter vector of a set or get: where it lies on the device, the caller's pointer (host or device; nullptr: not this one), its
// floats, and the set flag that a set raises
struct OkVector
{
    float *device;
    void  *other;
    size_t floats;
    int    flag;
};

OkVector vectorOf(float *device, const void *other, const int floats, const int flag = 0)
{
    return OkVector{device, const_cast<void *>(other), static_cast<size_t>(floats), flag};
}

// okenv_*_set_params behind the gate: copies on the stream, no synchronisation
int driverSet(okenv *h, const DriverKind &k, const std::initializer_list<OkVector> vectors)
{
    OK_HIP(h, hipSetDevice(h->device));
    for (const OkVector &v : vectors)
        if (v.other != nullptr)
        {
            if (const int rc = copyAny(h, v.device, v.other, sizeof(float) * v.floats))
                return rc;
            (h->*k.drv).set[v.flag] = true;
        }
    return OKENV_OK;
}

// okenv_*_get_params / _get_state behind the gate: copies on the stream and waits for it
int driverGet(okenv *h, const std::initializer_list<OkVector> vectors)
{
    OK_HIP(h, hipSetDevice(h->device));
    for (const OkVector &v : vectors)
        if (v.other != nullptr)
            if (const int rc = copyAny(h, v.other, v.device, sizeof(float) * v.floats))
                return rc;
    OK_HIP(h, hipStreamSynchronize(h->stream));
    return OKENV_OK;
}

// okenv_*_num_params / _set_params / _get_params of the flat-vector families behind their OK_QUIESCE, from the family's description.
// which: 0 for vector 0 (the only one of most families), 1 for the controllers of a family that has them; an entry without a `which`
// passes 0.  controller: the second out pointer of such a family's num_params.
int flatNumParams(okenv *h, const DriverKind &k, int32_t *vector0, int32_t *controller = nullptr)
{
    const bool argument = vector0 != nullptr && (k.controller == nullptr || controller != nullptr);
    if (const int rc = driverGate(h, k, "num_params", kGateArgFirst | kGateCreated, argument))
        return rc;
    *vector0 = k.total(h);
    if (k.controller != nullptr)
        *controller = k.controller(h);
    return OKENV_OK;
}

bool flatWhichBad(const DriverKind &k, const int32_t which)
{
    return which != 0 && (which != 1 || k.controller == nullptr);
}

int flatSetParams(okenv *h, const DriverKind &k, const int32_t which, const float *params)
{
    if (const int rc = driverGate(h, k, "set_params", kGateArgFirst | kGateCreated, params != nullptr))
        return rc;
    if (flatWhichBad(k, which))
        return driverRefuses(h, OKENV_ERR_INVALID, k, "set_params", std::string("which must be ") + k.which);
    if (which == 1)
        return driverSet(h, k, {vectorOf(k.controllers(h), params, h->shape.N * k.controller(h), 1)});
    if (const int rc = driverSet(h, k, {vectorOf((h->*k.drv).d, params, k.total(h))}))
        return rc;
    return k.repack != nullptr ? k.repack(h) : OKENV_OK;
}

// (the gate, which asks for the vector's own set flag, comes before a bad `which`, which asks for flag 0)
int flatGetParams(okenv *h, const DriverKind &k, const int32_t which, float *params)
{
    const bool controllers = which == 1 && k.controller != nullptr;
    if (const int rc = driverGate(h, k, "get_params", kGateArgFirst | kGateStored, params != nullptr, controllers ? 2U : 1U))
        return rc;
    if (flatWhichBad(k, which))
        return driverRefuses(h, OKENV_ERR_INVALID, k, "get_params", std::string("which must be ") + k.which);
    if (controllers)
        return driverGet(h, {vectorOf(k.controllers(h), params, h->shape.N * k.controller(h))});
    return driverGet(h, {vectorOf((h->*k.drv).d, params, k.total(h))});
}

int driverSetDrawOffset(okenv *h, const DriverKind &k, const uint32_t *device_word)
{
    if (const int rc = driverGate(h, k, "set_draw_offset", kGateCreated))
        return rc;
    (h->*k.drv).draw_offset = device_word;
    return OKENV_OK;
}

// greedy_of: the family's config member
template <class Config>
int driverSetGreedy(okenv *h, const DriverKind &k, Config okenv::*config, const int32_t greedy)
{
    if (const int rc = driverGate(h, k, "set_greedy", kGateCreated))
        return rc;
    if (greedy != 0 && greedy != 1)
        return driverRefuses(h, OKENV_ERR_INVALID, k, "set_greedy", "greedy must be 0 or 1");
    (h->*config).greedy = greedy;
    return OKENV_OK;
}

// How every okenv_*_act opens: the gate, then the entry's own last refusal (`missing`: nullptr or its text), the episode dropped, the device
int actBegin(okenv *h, const DriverKind &k, const unsigned need, const char *missing = nullptr)
{
    if (const int rc = driverGate(h, k, "act", kGateHandle | kGateCreated | kGateSet, true, need))
        return rc;
    if (missing != nullptr)
        return driverRefuses(h, OKENV_ERR_INVALID, k, "act", missing);
    dropEpisode(h);
    OK_HIP(h, hipSetDevice(h->device));
    return OKENV_OK;
}

// ... and how it closes: one workgroup of `threads` per `agents` agents, on the stream
template <class Params>
int actLaunch(okenv *h, void (*kernel)(Params), const int agents, const unsigned threads, const size_t lds, const Params &p)
{
    const unsigned blocks = static_cast<unsigned>((h->shape.N + agents - 1) / agents);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), lds, h->stream, p);
    OK_HIP(h, hipGetLastError());
    return OKENV_OK;
}

// What an entry refuses in its frames argument, `count` RGBA8 frames of image_size x image_size pixels: nullptr when they are as the
// kernels need them.  align: 4, or 16 for kernels that move a frame as 16-byte vectors wherever its pixels are a multiple of 4
const char *framesMissing(const void *frames, const int64_t frame_bytes, const int64_t count, const int image_size, const unsigned align)
{
    const int px = image_size * image_size;
    if (!frames)
        return "NULL argument";
    if (frame_bytes != count * px * 4)
        return "frame_bytes is not num_agents x image_size x image_size x 4";
    if (align == 4U)
        return reinterpret_cast<uintptr_t>(frames) % 4U != 0U ? "frames must be 4-byte aligned" : nullptr;
    if (reinterpret_cast<uintptr_t>(frames) % (px % 4 == 0 ? 16U : 4U) != 0U)
        return "frames must be 16-byte aligned (4-byte where image_size x image_size is no multiple of 4)";
    return nullptr;
}

// actBegin of the families that act on one frame per agent: what framesMissing says of them is the entry's last refusal, and they are looked
// at only once the driver is created (before that the state is all an act reports)
int actBeginFrames(okenv *h, const DriverKind &k, const unsigned need, const void *frames, const int64_t frame_bytes, const unsigned align = 4U)
{
    const bool created = h != nullptr && (h->*k.drv).ok;
    return actBegin(h, k, need, created ? framesMissing(frames, frame_bytes, h->shape.N, k.image_size(h), align) : nullptr);
}

// okenv_bev_encode behind its OK_QUIESCE: the kernels named in `stages` (OKENV_BEV_STAGE_*), in their order, on the stream
int bevEncode(okenv *h, const uint8_t *frames, const int64_t frame_bytes, float *out, const unsigned stages)
{
    if (const int rc = driverGate(h, kBevDriver, "encode", kGateHandle | kGateCreated | kGateSet, true, 1U))
        return rc;
    const ok_bev_shape s = okBevShape(h->bev);
    if (const char *why = !out ? "NULL argument" : framesMissing(frames, frame_bytes, h->shape.N, s.S, 4U))
        return driverRefuses(h, OKENV_ERR_INVALID, kBevDriver, "encode", why);
    OK_HIP(h, hipSetDevice(h->device));
    const OkBevPlaces pl = okBevPlaces(s);
    OkBevEncodeParams p{};
    p.N      = h->shape.N;
    p.s      = s;
    p.frames = frames;
    p.params = h->bev_drv.d;
    p.pack   = h->bev_pack.d;
    p.act1   = h->bev_act1.d;
    p.act2   = h->bev_act2.d;
    p.out    = out;
    const auto tiles = [](const int side, const int t) { return static_cast<unsigned>((side + t - 1) / t); };
    const unsigned N = static_cast<unsigned>(h->shape.N), ta = tiles(ok_bev_side(s, 1), pl.ta), tb = tiles(ok_bev_side(s, 2), pl.tb);
    const size_t   front = sizeof(float) * static_cast<size_t>(pl.front_end), back = sizeof(float) * static_cast<size_t>(pl.back_end);
    if ((stages & OKENV_BEV_STAGE_FRONT) != 0U)
        hipLaunchKernelGGL(pl.ta == 8 ? okBevFrontKernel<8> : okBevFrontKernel<4>, dim3(N * ta * ta), dim3(kBevThreads), front, h->stream, p);
    OK_HIP(h, hipGetLastError());
    if ((stages & OKENV_BEV_STAGE_BACK) != 0U)
        hipLaunchKernelGGL(pl.tb == 8 ? okBevBackKernel<8> : okBevBackKernel<4>, dim3(N * tb * tb), dim3(kBevThreads), back, h->stream, p);
    OK_HIP(h, hipGetLastError());
    if ((stages & OKENV_BEV_STAGE_HEAD) != 0U)
        hipLaunchKernelGGL(okBevHeadKernel, dim3(N), dim3(kBevThreads), 0, h->stream, p);
    OK_HIP(h, hipGetLastError());
    return OKENV_OK;
}

// okenv_cnn_act behind its OK_QUIESCE: the kernels named in `stages` (OKENV_CNN_STAGE_*), in their order, on the stream
int cnnAct(okenv *h, const uint8_t *frames, const int64_t frame_bytes, const okenv_cnn_record *rec, const unsigned stages)
{
    if (const int rc = actBeginFrames(h, kCnnDriver, 1U, frames, frame_bytes))
        return rc;
    const ok_cnn_shape s  = okCnnShape(h->cnn);
    const OkCnnPlaces  pl = okCnnPlaces(s);
    OkCnnActParams     p{};
    p.st          = h->st;
    p.N           = h->shape.N;
    p.s           = s;
    p.frames      = frames;
    p.params      = h->cnn_drv.d;
    p.pack        = h->cnn_pack.d;
    p.feat        = h->cnn_feat.d;
    p.throttle    = h->cnn.throttle;
    p.steer_scale = h->cnn.steer_scale;
    if (rec != nullptr)
        p.rec = *rec;
    if ((stages & OKENV_CNN_STAGE_CONV) != 0U)
        if (const int rc = actLaunch(h, okCnnConvKernel, 1, kConvThreads, sizeof(float) * static_cast<size_t>(pl.conv_end), p))
            return rc;
    if ((stages & OKENV_CNN_STAGE_HEAD) != 0U)
    {
        void (*const heads[kConvMaxColTiles])(OkCnnActParams) = {okCnnHeadKernel<1>, okCnnHeadKernel<2>, okCnnHeadKernel<3>, okCnnHeadKernel<4>};
        return actLaunch(h, heads[pl.ct - 1], kConvAgents, kConvThreads, sizeof(float) * static_cast<size_t>(pl.head_end), p);
    }
    return OKENV_OK;
}

// What okenv_qcnn_act and okenv_qcnn_push refuse in their frames: nullptr when they are as the kernels need them
const char *qcnnFramesMissing(const okenv *h, const void *frames, const int64_t frame_bytes)
{
    return framesMissing(frames, frame_bytes, h->shape.N, h->qcnn.image_size, 16U); // (OkQcnnPlaces' vec)
}

template <int RT>
int qcnnHead(okenv *h, const OkQcnnPlaces &pl, const OkQcnnActParams &p)
{
    void (*const heads[kConvMaxColTiles])(OkQcnnActParams) = {okQcnnHeadKernel<1, RT>, okQcnnHeadKernel<2, RT>, okQcnnHeadKernel<3, RT>, okQcnnHeadKernel<4, RT>};
    const size_t lds = sizeof(float) * static_cast<size_t>(kConvAgents * RT * (pl.ldt + pl.ldh));
    return actLaunch(h, heads[pl.ct - 1], kConvAgents * RT, kConvThreads, lds, p);
}

// okenv_qcnn_act behind its OK_QUIESCE: the kernels named in `stages` (OKENV_QCNN_STAGE_*), in their order, on the stream
int qcnnAct(okenv *h, const uint8_t *frames, const int64_t frame_bytes, const okenv_qcnn_record *rec, const unsigned stages)
{
    if (const int rc = actBeginFrames(h, kQcnnDriver, 1U, frames, frame_bytes, 16U)) // (as qcnnFramesMissing)
        return rc;
    const ok_qcnn_shape s  = okQcnnShape(h->qcnn);
    const OkQcnnPlaces  pl = okQcnnPlaces(s);
    OkQcnnActParams     p{};
    p.st     = h->st;
    p.N      = h->shape.N;
    p.s      = s;
    p.frames = frames;
    p.params = h->qcnn_drv.d;
    p.pack   = h->qcnn_pack.d;
    p.feat   = h->qcnn_feat.d;
    p.draw   = actDrawWords(h, h->qcnn_drv.draw_offset);
    p.cfg    = h->qcnn;
    if (rec != nullptr)
        p.rec = *rec;
    if ((stages & OKENV_QCNN_STAGE_CONV) != 0U)
        if (const int rc = actLaunch(h, okQcnnConvKernel, 1, kConvThreads, sizeof(float) * static_cast<size_t>(pl.conv_end), p))
            return rc;
    if ((stages & OKENV_QCNN_STAGE_HEAD) != 0U)
        if (const int rc = qcnnHead<1>(h, pl, p))
            return rc;
    if ((stages & OKENV_QCNN_STAGE_HEAD_32) != 0U)
        return qcnnHead<2>(h, pl, p);
    return OKENV_OK;
}

// One launch of the image transformer's linear kernel: the M x N outputs in tiles of 64 x 64
template <int kSrc, int kEpi>
void vitLinear(okenv *h, OkVitLinearParams p, const long M, const int K, const int N, const float *a, const long lda, const float *w, const float *bias,
               float *out, const long ldo)
{
    p.M = M, p.K = K, p.N = N, p.a = a, p.lda = lda, p.w = w, p.bias = bias, p.out = out, p.ldo = ldo;
    hipLaunchKernelGGL((okVitLinearKernel<kSrc, kEpi>), dim3(static_cast<unsigned>((M + kVitTile - 1) / kVitTile), static_cast<unsigned>((N + kVitTile - 1) / kVitTile)),
                       dim3(kVitThreads), 0, h->stream, p);
}

// The backbone of one pass: the frames of `count` sequences (at most vit_pass) through the patch embedding and the blocks, into the
// workspace's x [count][T][D]; 1 + 7 depth launches on the stream
int vitBackbone(okenv *h, const uint8_t *frames, const size_t count)
{
    const ok_vit_shape  s  = okVitShape(h->vit);
    const ok_vit_layout at = ok_vit_offsets(s);
    const OkVitPlaces   pl = okVitPlaces(s);
    const int           T = pl.T, D = s.D, F = s.ff;
    const float        *prm = h->vit_drv.d;
    OkVitLinearParams   lp{};
    lp.S = s.S, lp.P = s.P, lp.side = ok_vit_side(s), lp.T = T;
    for (int c = 0; c < 3; ++c)
        lp.mean[c] = h->vit.mean[c], lp.std[c] = h->vit.std[c];
    lp.pos = prm + at.pos, lp.cls = prm + at.cls;
    const long M = static_cast<long>(count) * T;
    float     *x = h->vit_work.d, *n = x + static_cast<size_t>(M) * D, *ctx = n + static_cast<size_t>(M) * D, *qkv = ctx + static_cast<size_t>(M) * D,
          *hid = qkv + static_cast<size_t>(M) * 3U * D;
    lp.frames = frames;
    vitLinear<kVitSrcPatch, kVitEpiPos>(h, lp, static_cast<long>(count) * (T - 1), ok_vit_patch_k(s), D, nullptr, 0, prm + at.pe_w, prm + at.pe_b, x, D);
    OK_HIP(h, hipGetLastError());
    const unsigned norm_blocks = static_cast<unsigned>((M + kVitNormRows - 1) / kVitNormRows);
    OkVitAttendParams ap{};
    ap.T = T, ap.D = D, ap.heads = s.heads, ap.dh = pl.dh, ap.qtiles = (T + kVitQueries - 1) / kVitQueries;
    ap.scale = ok_lidar_scale(pl.dh), ap.qkv = qkv, ap.ctx = ctx;
    for (int i = 0; i < s.depth; ++i)
    {
        const float *bp = prm + at.block0 + static_cast<size_t>(i) * at.block_stride;
        hipLaunchKernelGGL(okVitNormKernel, dim3(norm_blocks), dim3(kVitThreads), 0, h->stream, M, D, x, bp + at.n1_g, bp + at.n1_b, h->vit.ln_eps, n);
        vitLinear<kVitSrcPlain, kVitEpiNone>(h, lp, M, D, 3 * D, n, D, bp + at.qkv_w, bp + at.qkv_b, qkv, 3L * D);
        hipLaunchKernelGGL(okVitAttendKernel, dim3(static_cast<unsigned>(count * s.heads * ap.qtiles)), dim3(kVitThreads),
                           sizeof(float) * static_cast<size_t>(pl.attend), h->stream, ap);
        vitLinear<kVitSrcPlain, kVitEpiResidual>(h, lp, M, D, D, ctx, D, bp + at.proj_w, bp + at.proj_b, x, D);
        hipLaunchKernelGGL(okVitNormKernel, dim3(norm_blocks), dim3(kVitThreads), 0, h->stream, M, D, x, bp + at.n2_g, bp + at.n2_b, h->vit.ln_eps, n);
        vitLinear<kVitSrcPlain, kVitEpiGelu>(h, lp, M, D, F, n, D, bp + at.fc1_w, bp + at.fc1_b, hid, F);
        vitLinear<kVitSrcPlain, kVitEpiResidual>(h, lp, M, F, D, hid, F, bp + at.fc2_w, bp + at.fc2_b, x, D);
        OK_HIP(h, hipGetLastError());
    }
    return OKENV_OK;
}

// okenv_vit_embed behind its OK_QUIESCE: the backbone over m frames in passes of vit_pass, the class tokens' LayerNorm behind each
int vitEmbed(okenv *h, const uint8_t *frames, const int32_t m, const int64_t frame_bytes, float *embedding)
{
    if (const int rc = driverGate(h, kVitDriver, "embed", kGateHandle | kGateCreated | kGateSet, true, 1U))
        return rc;
    const ok_vit_shape s = okVitShape(h->vit);
    const size_t       frame = static_cast<size_t>(s.S) * static_cast<size_t>(s.S) * 4U;
    if (!frames || !embedding)
        return driverRefuses(h, OKENV_ERR_INVALID, kVitDriver, "embed", "NULL argument");
    if (m < 1 || frame_bytes != static_cast<int64_t>(m) * static_cast<int64_t>(frame)) // (its own text: the frames are m, not num_agents)
        return driverRefuses(h, OKENV_ERR_INVALID, kVitDriver, "embed", "m must be at least 1 and frame_bytes m x image_size x image_size x 4");
    if (const char *why = framesMissing(frames, frame_bytes, m, s.S, 4U))
        return driverRefuses(h, OKENV_ERR_INVALID, kVitDriver, "embed", why);
    OK_HIP(h, hipSetDevice(h->device));
    const ok_vit_layout at = ok_vit_offsets(s);
    const int           T = ok_vit_tokens(s), D = s.D;
    for (size_t a0 = 0; a0 < static_cast<size_t>(m); a0 += h->vit_pass)
    {
        const size_t count = std::min(h->vit_pass, static_cast<size_t>(m) - a0);
        if (const int rc = vitBackbone(h, frames + a0 * frame, count))
            return rc;
        hipLaunchKernelGGL(okVitEmbedKernel, dim3(static_cast<unsigned>((count + kVitNormRows - 1) / kVitNormRows)), dim3(kVitThreads), 0, h->stream,
                           static_cast<int>(count), D, static_cast<long>(T) * D, h->vit_work.d, h->vit_drv.d + at.norm_g, h->vit_drv.d + at.norm_b, h->vit.ln_eps,
                           embedding + a0 * D);
        OK_HIP(h, hipGetLastError());
    }
    return OKENV_OK;
}

// The head's slice of the handle's parameter vector, and Adam's moments k = 0 (m), 1 (v)
float *vitHeadParams(const okenv *h)
{
    return h->vit_drv.d + ok_vit_offsets(okVitShape(h->vit)).hw0;
}

int vitHeadTotal(const okenv *h)
{
    return ok_vithead_offsets(h->vit.dim, h->vit.head_hidden1, h->vit.head_hidden2).total;
}

float *vitHeadMoment(const okenv *h, const int k)
{
    return h->vit_head_mv.d + static_cast<size_t>(k) * (h->vit_head_mv.cap / 2U);
}

// okenv_vit_head_update (update == true: `epochs` passes in `order`, a step per minibatch) and okenv_vit_head_eval (one sequential pass, the
// losses only) behind their OK_QUIESCE: two launches per minibatch on the stream
int vitHeadRun(okenv *h, const char *entry, const bool update, const float *embedding, const float *steer, const int32_t M, const int32_t B, const int32_t epochs,
               const int32_t *order, float *loss, float *grad)
{
    if (!h)
        return fail(h, OKENV_ERR_INVALID, std::string(entry) + ": NULL handle");
    if (!h->vit_drv.ok || !h->vit_head_ok)
        return fail(h, OKENV_ERR_STATE, std::string(entry) + ": call okenv_vit_head_learner_create first");
    if (const char *why = okVitHeadCheckCall(embedding, steer, M, B, epochs))
        return fail(h, OKENV_ERR_INVALID, std::string(entry) + ": " + why);
    OK_HIP(h, hipSetDevice(h->device));
    const int    D = h->vit.dim, H1 = h->vit.head_hidden1, H2 = h->vit.head_hidden2, slices = okLearnMinibatches(M, B);
    const size_t qp_max = (static_cast<size_t>(std::min(B, M)) + OK_VITHEAD_CHUNK - 1U) / OK_VITHEAD_CHUNK * OK_VITHEAD_CHUNK;
    if (const int rc = growScratch(h, h->vit_head_scratch, sizeof(float) * okVitHeadScratchFloats(D, H1, H2, qp_max)))
        return rc;
    const okenv_learner_params lp = okVitHeadAdam(h->vit_head);
    OkVitHeadForwardParams     f{};
    f.D = D, f.H1 = H1, f.H2 = H2, f.M = M, f.head = vitHeadParams(h), f.embedding = embedding, f.steer = steer;
    f.steer_scale = h->vit.steer_scale, f.weight = h->vit_head.weight, f.threshold = h->vit_head.threshold;
    f.out = okVitHeadScratchAt(reinterpret_cast<float *>(h->vit_head_scratch.part), D, H1, H2, qp_max);
    OkVitHeadGradParams g{};
    g.D = D, g.H1 = H1, g.H2 = H2, g.in = f.out, g.head = vitHeadParams(h), g.m = vitHeadMoment(h, 0), g.v = vitHeadMoment(h, 1);
    const int    units = okVitHeadUnits(D, H1, H2);
    const size_t lds = okVitHeadLdsBytes(D, H1, H2);
    for (int e = 0; e < epochs; ++e)
        for (int k = 0; k < slices; ++k)
        {
            f.base  = static_cast<long>(k) * B;
            f.Bk    = static_cast<int>(std::min<long>(B, M - f.base));
            f.order = order != nullptr ? order + static_cast<size_t>(e) * M : nullptr;
            g.Bk    = f.Bk;
            g.chunks = (f.Bk + OK_VITHEAD_CHUNK - 1) / OK_VITHEAD_CHUNK;
            g.loss   = loss != nullptr ? loss + static_cast<size_t>(e) * slices + k : nullptr;
            hipLaunchKernelGGL(okVitHeadForwardKernel, dim3(static_cast<unsigned>(g.chunks * (OK_VITHEAD_CHUNK / kVitHeadRows))), dim3(kLidarThreads), lds, h->stream, f);
            OK_HIP(h, hipGetLastError());
            if (update)
            {
                g.first_unit = 0;
                g.adam       = okLearnAdamConsts(lp, h->vit_head_t + 1);
                g.grad       = (e + 1 == epochs && k + 1 == slices) ? grad : nullptr;
                hipLaunchKernelGGL(okVitHeadGradKernel<true>, dim3(static_cast<unsigned>((units + kLidarWaves - 1) / kLidarWaves)), dim3(kLidarThreads), 0, h->stream, g);
                OK_HIP(h, hipGetLastError());
                h->vit_head_t += 1; // (the step number advances once the step's kernels are enqueued, as in okenv_ppo_update)
            }
            else if (loss != nullptr)
            {
                g.first_unit = units - 1;
                hipLaunchKernelGGL(okVitHeadGradKernel<false>, dim3(1), dim3(64), 0, h->stream, g);
                OK_HIP(h, hipGetLastError());
            }
        }
    return OKENV_OK;
}

// okenv_vit_act behind its OK_QUIESCE: the fixed launch sequence (ok_vit.h), once per pass of vit_pass agents, on the stream
int vitAct(okenv *h, const uint8_t *frames, const int64_t frame_bytes, const okenv_vit_record *rec)
{
    if (const int rc = actBeginFrames(h, kVitDriver, 1U, frames, frame_bytes))
        return rc;
    const ok_vit_shape  s  = okVitShape(h->vit);
    const OkVitPlaces   pl = okVitPlaces(s);
    const float        *prm = h->vit_drv.d;
    const size_t        frame = static_cast<size_t>(s.S) * static_cast<size_t>(s.S) * 4U;
    for (size_t a0 = 0; a0 < static_cast<size_t>(h->shape.N); a0 += h->vit_pass)
    {
        const size_t count = std::min(h->vit_pass, static_cast<size_t>(h->shape.N) - a0);
        float       *x = h->vit_work.d;
        if (const int rc = vitBackbone(h, frames + a0 * frame, count))
            return rc;
        OkVitFinalParams fp{};
        fp.st = h->st, fp.a0 = static_cast<long>(a0), fp.count = static_cast<int>(count), fp.s = s, fp.params = prm, fp.x = x;
        fp.eps = h->vit.ln_eps, fp.throttle = h->vit.throttle, fp.steer_scale = h->vit.steer_scale;
        if (rec != nullptr)
            fp.rec = *rec;
        hipLaunchKernelGGL(okVitFinalKernel, dim3(static_cast<unsigned>((count + kVitAgents - 1) / kVitAgents)), dim3(kLidarThreads),
                           sizeof(float) * static_cast<size_t>(pl.final), h->stream, fp);
        OK_HIP(h, hipGetLastError());
    }
    return OKENV_OK;
}

// okenv_world_act behind its OK_QUIESCE: the kernels named in `stages` (OKENV_WORLD_STAGE_*), in their order, on the stream.  Every
// grid is sized for all N agents; workgroups past the list's end leave at once.
int worldKernels(okenv *h, const uint8_t *frames, const okenv_world_record *rec, unsigned stages);

int worldAct(okenv *h, const uint8_t *frames, const int64_t frame_bytes, const okenv_world_record *rec, const unsigned stages)
{
    if (const int rc = actBeginFrames(h, kWorldDriver, 3U, frames, frame_bytes))
        return rc;
    return worldKernels(h, frames, rec, stages);
}

// ... and its launches, which okenv_memory_act shares up to the head
int worldKernels(okenv *h, const uint8_t *frames, const okenv_world_record *rec, const unsigned stages)
{
    const ok_world_shape  s  = okWorldShape(h->world);
    const ok_world_layout at = ok_world_offsets(s);
    const size_t          N  = static_cast<size_t>(h->shape.N);
    const OkWorldPlaces   pl = okWorldPlaces(s, N);
    float                *ws = h->world_ws.d;
    int                  *list = reinterpret_cast<int *>(ws + pl.list), *count = reinterpret_cast<int *>(ws + pl.count);
    if ((stages & OKENV_WORLD_STAGE_LIST) != 0U)
    {
        hipLaunchKernelGGL(okWorldListKernel, dim3(1), dim3(256), 0, h->stream, h->st.crashed, h->shape.N, h->world.skip_crashed, list, count);
        OK_HIP(h, hipGetLastError());
    }
    for (int l = 0; l < 4; ++l)
    {
        if ((stages & (OKENV_WORLD_STAGE_CONV0 << l)) == 0U)
            continue;
        OkWorldConvJob j{};
        j.frames = frames;
        j.in     = l > 0 ? ws + pl.act[l - 1] : nullptr;
        j.out    = ws + pl.act[l];
        j.w      = ws + pl.pack[l];
        j.bias   = h->world_drv.d + at.b[l];
        j.list   = list;
        j.count  = count;
        j.S      = s.S >> l;
        j.side   = ok_world_side(s, l);
        j.Cin    = ok_world_cin(s, l);
        j.Cout   = s.c[l];
        const size_t rows = N * static_cast<size_t>(j.side) * j.side;
        const dim3   grid(static_cast<unsigned>((rows + kWorldRows - 1) / kWorldRows), static_cast<unsigned>((j.Cout + kWorldCols - 1) / kWorldCols));
        const size_t lds = sizeof(float) * kWorldRows * kWorldLda;
        if (l == 0)
            hipLaunchKernelGGL(okWorldConvKernel<true>, grid, dim3(kWorldThreads), lds, h->stream, j);
        else
            hipLaunchKernelGGL(okWorldConvKernel<false>, grid, dim3(kWorldThreads), lds, h->stream, j);
        OK_HIP(h, hipGetLastError());
    }
    const int P = ok_world_side(s, 3) * ok_world_side(s, 3);
    if ((stages & OKENV_WORLD_STAGE_LATENT) != 0U)
    {
        OkWorldLatentJob j{};
        j.act3  = ws + pl.act[3];
        j.w     = ws + pl.pack[4];
        j.part  = ws + pl.part;
        j.count = count;
        j.P     = P;
        j.C     = s.c[3];
        j.Z     = s.Z;
        const dim3 grid(static_cast<unsigned>((N + kWorldAgents - 1) / kWorldAgents), static_cast<unsigned>(P));
        hipLaunchKernelGGL(okWorldLatentKernel, grid, dim3(64 * (s.Z / 16)), sizeof(float) * kWorldAgents * (s.c[3] + 2), h->stream, j);
        OK_HIP(h, hipGetLastError());
    }
    if ((stages & OKENV_WORLD_STAGE_HEAD) != 0U)
    {
        OkWorldHeadParams p{};
        p.st          = h->st;
        p.s           = s;
        p.enc         = h->world_drv.d;
        p.ctrl        = ws + pl.ctrl;
        p.part        = ws + pl.part;
        p.list        = list;
        p.count       = count;
        p.throttle    = h->world.throttle;
        p.steer_scale = h->world.steer_scale;
        if (rec != nullptr)
            p.rec = *rec;
        return actLaunch(h, okWorldHeadKernel, kWorldHeadSlots, 64 * kWorldHeadSlots, 0, p);
    }
    return OKENV_OK;
}

// okenv_memory_act behind its OK_QUIESCE: the kernels named in `stages` (OKENV_MEMORY_STAGE_*), in their order, on the stream.  The
// encoder is okenv_world_act's own launches (worldAct without its head); every grid behind it is sized for all N agents as well.
int memoryAct(okenv *h, const uint8_t *frames, const int64_t frame_bytes, const okenv_memory_record *rec, const unsigned stages)
{
    if (h != nullptr && h->mem_drv.ok && (!h->world_drv.ok || !h->world_drv.set[0]))
        return driverRefuses(h, OKENV_ERR_STATE, kMemoryDriver, "act", "call okenv_world_set_params first (the encoder needs its parameters)");
    if (const int rc = actBeginFrames(h, kMemoryDriver, 3U, frames, frame_bytes))
        return rc;
    const ok_world_shape   w   = okWorldShape(h->world);
    const ok_memory_shape  s   = memoryShape(h);
    const ok_world_layout  wat = ok_world_offsets(w);
    const ok_memory_layout at  = ok_memory_offsets(s);
    const size_t           N   = static_cast<size_t>(h->shape.N);
    const OkWorldPlaces    wpl = okWorldPlaces(w, N);
    const OkMemoryPlaces   pl  = okMemoryPlaces(s, N);
    float                 *ws = h->mem_ws.d, *net = h->mem_drv.d;
    const int             *list = reinterpret_cast<const int *>(h->world_ws.d + wpl.list), *count = reinterpret_cast<const int *>(h->world_ws.d + wpl.count);
    if ((stages & OKENV_MEMORY_STAGE_ENCODER) != 0U)
    {
        // (the racers' own controllers are not read: only their encoder must be set)
        if (const int rc = worldKernels(h, frames, nullptr, ~static_cast<unsigned>(OKENV_WORLD_STAGE_HEAD)))
            return rc;
    }
    const int LH = s.L * s.H;
    if ((stages & OKENV_MEMORY_STAGE_INPUT) != 0U)
    {
        OkMemoryInputJob j{};
        j.st       = h->st;
        j.enc_bias = h->world_drv.d + wat.mb;
        j.part     = h->world_ws.d + wpl.part;
        j.z_mean   = net + at.z_mean;
        j.z_std    = net + at.z_std;
        j.a_mean   = net + at.a_mean;
        j.a_std    = net + at.a_std;
        j.mu       = ws + pl.mu;
        j.x0       = ws + pl.x0;
        j.list     = list;
        j.count    = count;
        j.Z        = s.Z;
        j.P        = ok_world_side(w, 3) * ok_world_side(w, 3);
        const size_t threads = N * static_cast<size_t>(s.Z + OK_MEMORY_ACTIONS);
        hipLaunchKernelGGL(okMemoryInputKernel, dim3(static_cast<unsigned>((threads + 255U) / 256U)), dim3(256), 0, h->stream, j);
        OK_HIP(h, hipGetLastError());
    }
    for (int l = 0; l < s.L; ++l)
    {
        if ((stages & (OKENV_MEMORY_STAGE_LAYER0 << l)) == 0U)
            continue;
        OkMemoryLayerJob j{};
        j.x       = l == 0 ? ws + pl.x0 : ws + pl.fresh + static_cast<size_t>(l - 1) * s.H;
        j.x_pitch = l == 0 ? okMemoryPitch(s) : LH;
        j.Kin     = okMemoryKin(s, l);
        j.hidden  = ws + pl.hidden + static_cast<size_t>(l) * s.H;
        j.fresh   = ws + pl.fresh + static_cast<size_t>(l) * s.H;
        j.wih     = ws + pl.ih[l];
        j.whh     = ws + pl.hh[l];
        j.tail    = l == 0 ? net + at.wih[0] : nullptr;
        j.bih     = net + at.bih[l];
        j.bhh     = net + at.bhh[l];
        j.list    = list;
        j.count   = count;
        j.H       = s.H;
        j.LH      = LH;
        j.carry   = s.carry;
        const dim3 grid(static_cast<unsigned>((N + kMemRows - 1) / kMemRows), static_cast<unsigned>((s.H + kMemCols - 1) / kMemCols));
        hipLaunchKernelGGL(okMemoryLayerKernel, grid, dim3(kMemThreads), okMemoryLdsBytes(s), h->stream, j);
        OK_HIP(h, hipGetLastError());
    }
    if ((stages & OKENV_MEMORY_STAGE_HEAD) != 0U)
    {
        OkMemoryHeadParams p{};
        p.st          = h->st;
        p.s           = s;
        p.net         = net;
        p.ctrl        = ws + pl.ctrl;
        p.mu          = ws + pl.mu;
        p.fresh       = ws + pl.fresh;
        p.hidden      = ws + pl.hidden;
        p.list        = list;
        p.count       = count;
        p.throttle    = h->mem.throttle;
        p.steer_scale = h->mem.steer_scale;
        if (rec != nullptr)
            p.rec = *rec;
        return actLaunch(h, okMemoryHeadKernel, kMemHeadSlots, 64 * kMemHeadSlots, 0, p);
    }
    return OKENV_OK;
}

// The layer kernel's copy of the GRU matrices behind an upload of the network: one launch per matrix on the stream
int memoryRepack(okenv *h)
{
    const ok_memory_shape  s  = memoryShape(h);
    const OkMemoryPlaces   pl = okMemoryPlaces(s, static_cast<size_t>(h->shape.N));
    const ok_memory_layout at = ok_memory_offsets(s);
    for (int m = 0; m < 2 * s.L; ++m)
    {
        const int       l = m / 2;
        OkMemoryPackJob j{};
        j.cols   = 3 * s.H;
        j.K      = m % 2 == 0 ? okMemoryKin(s, l) : s.H;
        j.stride = m % 2 == 0 ? ok_memory_in(s, l) : s.H;
        j.src    = h->mem_drv.d + (m % 2 == 0 ? at.wih[l] : at.whh[l]);
        j.dst    = h->mem_ws.d + (m % 2 == 0 ? pl.ih[l] : pl.hh[l]);
        hipLaunchKernelGGL(okMemoryPackKernel, dim3(static_cast<unsigned>((j.cols * j.K + 255) / 256)), dim3(256), 0, h->stream, j);
        OK_HIP(h, hipGetLastError());
    }
    return OKENV_OK;
}

// One job of the product kernel as a list of one
int memTrainProduct(okenv *h, const OkMemTrainGemm &job)
{
    OkMemTrainGemmJobs js{};
    js.count  = 1;
    js.job[0] = job;
    hipLaunchKernelGGL(okMemTrainGemmKernel, dim3(static_cast<unsigned>((okMemTrainTiles(job) + kMemTrainWaves - 1) / kMemTrainWaves), 1U), dim3(kMemTrainThreads), 0,
                       h->stream, js);
    OK_HIP(h, hipGetLastError());
    return OKENV_OK;
}

// okenv_memory_update (update == true: `epochs` passes in `order`, a step per minibatch) and okenv_memory_eval (one sequential pass, the
// losses only) behind their OK_QUIESCE: the launches of ok_memtrain.h on the stream
int memoryLearnRun(okenv *h, const char *entry, const bool update, const float *latent, const float *action, const int32_t rows, const int32_t *start,
                   const int32_t M, const int32_t stride, const int32_t B, const int32_t epochs, const int32_t *order, const float *lr_schedule, float *loss,
                   float *norm, float *grad_out)
{
    if (!h)
        return fail(h, OKENV_ERR_INVALID, std::string(entry) + ": NULL handle");
    if (!h->mem_drv.ok || !h->mem_learn_ok)
        return fail(h, OKENV_ERR_STATE, std::string(entry) + ": call okenv_memory_learner_create first");
    if (const char *why = okMemTrainCheckCall(latent, action, rows, start, M, B, epochs))
        return fail(h, OKENV_ERR_INVALID, std::string(entry) + ": " + why);
    const okenv_memory_learner_config &c = h->mem_learn;
    if (std::min(B, M) > c.max_batch)
        return fail(h, OKENV_ERR_INVALID, std::string(entry) + ": a minibatch of min(B, M) windows is beyond the learner's max_batch");
    OK_HIP(h, hipSetDevice(h->device));
    const ok_memory_shape  s  = memoryShape(h);
    const ok_memory_layout at = ok_memory_offsets(s);
    const int              Z = s.Z, H = s.H, H3 = 3 * s.H, S = c.seq_len, Bmax = c.max_batch, in0 = Z + OK_MEMORY_ACTIONS, T = ok_memtrain_trainable(s);
    const OkMemTrainPlaces pl = okMemTrainPlaces(s, S, Bmax);
    float                 *ws = h->mem_learn_ws.d, *net = h->mem_drv.d, *g = ws + pl.grad;
    long long             *t_dev = reinterpret_cast<long long *>(ws + pl.scalars + kMemTrainStepAt);
    ok_learn_adam_consts  *adam_dev = reinterpret_cast<ok_learn_adam_consts *>(ws + pl.scalars + kMemTrainConstsAt);
    const int              slices = okLearnMinibatches(M, B);
    const auto blocks = [](const long n) { return dim3(static_cast<unsigned>((n + 255) / 256)); };
    for (int e = 0; e < epochs; ++e)
        for (int k = 0; k < slices; ++k)
        {
            const long   base = static_cast<long>(k) * B;
            const int    Bk = static_cast<int>(std::min<long>(B, M - base)), P = Bk * S;
            const size_t at_step = static_cast<size_t>(e) * slices + k;
            const float  count = static_cast<float>(Bk * S * Z);
            // a layer's rows: h_prev of position p at hp + p H, its h' at hp + (Bk + p) H
            const auto hp = [&](const int l) { return ws + pl.h[l] + static_cast<size_t>(Bmax - Bk) * H; };
            OkMemTrainGatherJob gj{};
            gj.latent = latent, gj.action = action, gj.net = net, gj.start = start;
            gj.order = order != nullptr ? order + static_cast<size_t>(e) * M : nullptr;
            gj.x0 = ws + pl.x0, gj.y = ws + pl.y, gj.base = base, gj.rows = rows, gj.M = M, gj.stride = stride, gj.Bk = Bk, gj.S = S, gj.Z = Z, gj.at = at;
            hipLaunchKernelGGL(okMemTrainGatherKernel, blocks(static_cast<long>(P) * (2 * Z + OK_MEMORY_ACTIONS)), dim3(256), 0, h->stream, gj);
            OK_HIP(h, hipGetLastError());
            // ---- forward, layer by layer
            for (int l = 0; l < s.L; ++l)
            {
                const int      in = ok_memory_in(s, l);
                OkMemTrainGemm gi{};
                gi.a = l == 0 ? ws + pl.x0 : hp(l - 1) + static_cast<size_t>(Bk) * H, gi.a_rs = l == 0 ? in0 : H, gi.a_cs = 1;
                gi.b = net + at.wih[l], gi.b_rs = 1, gi.b_cs = in, gi.bias = net + at.bih[l];
                gi.c = ws + pl.gi, gi.c_rs = H3, gi.M = P, gi.N = H3, gi.K = okMemoryKin(s, l);
                if (const int rc = memTrainProduct(h, gi))
                    return rc;
                for (int st = 0; st < S; ++st)
                {
                    const size_t   row = static_cast<size_t>(st) * Bk;
                    OkMemTrainGemm gh{};
                    gh.a = hp(l) + row * H, gh.a_rs = H, gh.a_cs = 1;
                    gh.b = net + at.whh[l], gh.b_rs = 1, gh.b_cs = H, gh.bias = net + at.bhh[l];
                    gh.c = ws + pl.gh, gh.c_rs = H3, gh.M = Bk, gh.N = H3, gh.K = H;
                    if (const int rc = memTrainProduct(h, gh))
                        return rc;
                    OkMemTrainGateJob gt{};
                    gt.gi = ws + pl.gi + row * H3, gt.gh = ws + pl.gh;
                    gt.xa = l == 0 ? ws + pl.x0 + row * in0 : nullptr, gt.tail = l == 0 ? net + at.wih[0] : nullptr;
                    gt.h_prev = hp(l) + row * H, gt.h = hp(l) + (row + Bk) * H;
                    gt.r = ws + pl.r[l] + row * H, gt.u = ws + pl.u[l] + row * H, gt.n = ws + pl.n[l] + row * H, gt.ghn = ws + pl.ghn[l] + row * H;
                    gt.Bk = Bk, gt.H = H, gt.Z = Z;
                    hipLaunchKernelGGL(okMemTrainGateKernel, blocks(static_cast<long>(Bk) * H), dim3(256), 0, h->stream, gt);
                    OK_HIP(h, hipGetLastError());
                }
            }
            const float   *top = hp(s.L - 1) + static_cast<size_t>(Bk) * H;
            OkMemTrainGemm hd{};
            hd.a = top, hd.a_rs = H, hd.a_cs = 1, hd.b = net + at.hw, hd.b_rs = 1, hd.b_cs = H, hd.bias = net + at.hb;
            hd.c = ws + pl.zn, hd.c_rs = Z, hd.M = P, hd.N = Z, hd.K = H;
            if (const int rc = memTrainProduct(h, hd))
                return rc;
            hipLaunchKernelGGL(okMemTrainSeedKernel, blocks(static_cast<long>(P) * Z), dim3(256), 0, h->stream, ws + pl.zn, ws + pl.y, ws + pl.tt,
                               static_cast<long>(P) * Z);
            OK_HIP(h, hipGetLastError());
            OkMemTrainGemmJobs sums{};
            OkMemTrainGemm    &lj = sums.job[sums.count++]; // the loss column: the terms against 1.0f
            lj.a = ws + pl.tt, lj.a_rs = 1, lj.a_cs = Z, lj.b = ws + pl.tt, lj.c = ws + pl.lossj, lj.c_ones = ws + pl.lossj, lj.M = Z, lj.N = 0, lj.K = P;
            float *loss_at = loss != nullptr ? loss + at_step : ws + pl.scalars + kMemTrainLossAt;
            if (update)
            {
                // ---- backward, top layer first, in a layer from the last step down
                OkMemTrainGemm dn{};
                dn.a = ws + pl.zn, dn.a_rs = Z, dn.a_cs = 1, dn.b = net + at.hw, dn.b_rs = H, dn.b_cs = 1;
                dn.c = ws + pl.down, dn.c_rs = H, dn.M = P, dn.N = H, dn.K = Z;
                if (const int rc = memTrainProduct(h, dn))
                    return rc;
                for (int l = s.L - 1; l >= 0; --l)
                {
                    for (int st = S - 1; st >= 0; --st)
                    {
                        const size_t      row = static_cast<size_t>(st) * Bk;
                        OkMemTrainCellJob cj{};
                        cj.down = ws + pl.down + row * H, cj.back = ws + pl.back, cj.keep = ws + pl.keep;
                        cj.r = ws + pl.r[l] + row * H, cj.u = ws + pl.u[l] + row * H, cj.n = ws + pl.n[l] + row * H, cj.ghn = ws + pl.ghn[l] + row * H;
                        cj.h_prev = hp(l) + row * H, cj.dgi = ws + pl.dgi[l] + row * H3, cj.dgh = ws + pl.dgh[l] + row * H3;
                        cj.Bk = Bk, cj.H = H, cj.last = st == S - 1 ? 1 : 0;
                        hipLaunchKernelGGL(okMemTrainCellKernel, blocks(static_cast<long>(Bk) * H), dim3(256), 0, h->stream, cj);
                        OK_HIP(h, hipGetLastError());
                        if (st > 0)
                        {
                            OkMemTrainGemm bk{};
                            bk.a = cj.dgh, bk.a_rs = H3, bk.a_cs = 1, bk.b = net + at.whh[l], bk.b_rs = H, bk.b_cs = 1;
                            bk.c = ws + pl.back, bk.c_rs = H, bk.M = Bk, bk.N = H, bk.K = H3;
                            if (const int rc = memTrainProduct(h, bk))
                                return rc;
                        }
                    }
                    if (l > 0)
                    {
                        OkMemTrainGemm dx{};
                        dx.a = ws + pl.dgi[l], dx.a_rs = H3, dx.a_cs = 1, dx.b = net + at.wih[l], dx.b_rs = H, dx.b_cs = 1;
                        dx.c = ws + pl.down, dx.c_rs = H, dx.M = P, dx.N = H, dx.K = H3;
                        if (const int rc = memTrainProduct(h, dx))
                            return rc;
                    }
                }
                // ---- the parameter sums over the positions: one launch
                for (int l = 0; l < s.L; ++l)
                {
                    const int       in = ok_memory_in(s, l);
                    OkMemTrainGemm &wi = sums.job[sums.count++];
                    wi.a = ws + pl.dgi[l], wi.a_rs = 1, wi.a_cs = H3;
                    wi.b = l == 0 ? ws + pl.x0 : hp(l - 1) + static_cast<size_t>(Bk) * H, wi.b_rs = l == 0 ? in0 : H, wi.b_cs = 1;
                    wi.c = g + at.wih[l], wi.c_rs = in, wi.c_ones = g + at.bih[l], wi.M = H3, wi.N = in, wi.K = P, wi.div = count;
                    OkMemTrainGemm &wh = sums.job[sums.count++];
                    wh.a = ws + pl.dgh[l], wh.a_rs = 1, wh.a_cs = H3, wh.b = hp(l), wh.b_rs = H, wh.b_cs = 1;
                    wh.c = g + at.whh[l], wh.c_rs = H, wh.c_ones = g + at.bhh[l], wh.M = H3, wh.N = H, wh.K = P, wh.div = count;
                }
                OkMemTrainGemm &hw = sums.job[sums.count++];
                hw.a = ws + pl.zn, hw.a_rs = 1, hw.a_cs = Z, hw.b = top, hw.b_rs = H, hw.b_cs = 1;
                hw.c = g + at.hw, hw.c_rs = H, hw.c_ones = g + at.hb, hw.M = Z, hw.N = H, hw.K = P, hw.div = count;
            }
            int tiles = 0;
            for (int i = 0; i < sums.count; ++i)
                tiles = std::max(tiles, okMemTrainTiles(sums.job[i]));
            hipLaunchKernelGGL(okMemTrainGemmKernel, dim3(static_cast<unsigned>((tiles + kMemTrainWaves - 1) / kMemTrainWaves), static_cast<unsigned>(sums.count)),
                               dim3(kMemTrainThreads), 0, h->stream, sums);
            OK_HIP(h, hipGetLastError());
            hipLaunchKernelGGL(okMemTrainLossKernel, dim3(1), dim3(64), 0, h->stream, ws + pl.lossj, Z, count, loss_at);
            OK_HIP(h, hipGetLastError());
            if (!update)
                continue;
            // ---- the norm, level by level, then the step
            int    left = (T + OK_MEMTRAIN_BLOCK - 1) / OK_MEMTRAIN_BLOCK;
            float *from = ws + pl.sum_a, *to = ws + pl.sum_b;
            hipLaunchKernelGGL(okMemTrainSquareKernel, blocks(left), dim3(256), 0, h->stream, g, T, from);
            OK_HIP(h, hipGetLastError());
            while (left > 1)
            {
                const int next = (left + OK_MEMTRAIN_BLOCK - 1) / OK_MEMTRAIN_BLOCK;
                hipLaunchKernelGGL(okMemTrainSumKernel, blocks(next), dim3(256), 0, h->stream, from, left, to);
                OK_HIP(h, hipGetLastError());
                std::swap(from, to);
                left = next;
            }
            const float lr = lr_schedule != nullptr ? lr_schedule[at_step] : c.lr;
            hipLaunchKernelGGL(okMemTrainTickKernel, dim3(1), dim3(64), 0, h->stream, t_dev, adam_dev, okMemTrainConsts(c), lr);
            OK_HIP(h, hipGetLastError());
            OkMemTrainStepJob sj{};
            sj.params = net, sj.m = ws + pl.m, sj.v = ws + pl.v, sj.grad = g, sj.total = from, sj.adam = adam_dev;
            sj.norm_out = norm != nullptr ? norm + at_step : nullptr;
            sj.grad_out = (e + 1 == epochs && k + 1 == slices) ? grad_out : nullptr;
            sj.clip_grad = c.clip_grad, sj.decay = ok_memtrain_decay(lr, c.weight_decay), sj.T = T;
            hipLaunchKernelGGL(okMemTrainStepKernel, blocks(T), dim3(256), 0, h->stream, sj);
            OK_HIP(h, hipGetLastError());
        }
    return update ? memoryRepack(h) : OKENV_OK; // (the act's copy of the matrices follows the last step; the training reads the vector itself)
}

// ---- the replay rings' entries, behind the exported functions' OK_QUIESCE ---------------------------------------------------------

// Which ring an exported entry works on: its record in the handle, the prefix of its entries' names (for the messages) and the widest
// fan its learner takes
struct RingKind
{
    OkRing okenv::*ring;
    const char    *prefix;
    int            max_rays;
};
const RingKind kDqnRing{&okenv::replay, "okenv_replay_", OK_ACTOR_MAX_RAYS}, kDdpgRing{&okenv::ddpg_ring, "okenv_ddpg_replay_", OK_DDPG_MAX_RAYS};

// The record's fields as the public struct of its kind (okenv_replay_ring, okenv_ddpg_ring)
template <class Ring>
Ring ringFields(const OkRing &r)
{
    Ring o{};
    o.state      = r.state;
    o.next_state = r.next_state;
    o.action     = reinterpret_cast<decltype(o.action)>(r.action);
    o.reward     = r.reward;
    o.done       = r.done;
    return o;
}

int ringMissing(okenv *h, const RingKind &k, const char *entry)
{
    return fail(h, OKENV_ERR_STATE, std::string(k.prefix) + entry + ": call " + k.prefix + "create first");
}

// lds_kernel: the update's gradient kernel whose dynamic-LDS limit is raised with the ring, or nullptr
int ringCreate(okenv *h, const RingKind &k, const int32_t capacity, const uint32_t flags, const void *lds_kernel)
{
    const std::string name = std::string(k.prefix) + "create: ";
    if (!h)
        return fail(h, OKENV_ERR_INVALID, name + "NULL handle");
    if (const char *why = okReplayCheckCreate(capacity, flags))
        return fail(h, OKENV_ERR_INVALID, name + why);
    if (h->shape.R > k.max_rays)
        return fail(h, OKENV_ERR_INVALID, name + "the fan needs 1 .. " + std::to_string(k.max_rays) + " rays");
    OkRing &r = h->*k.ring;
    OK_HIP(h, hipSetDevice(h->device));
    r.ok = false;
    const size_t C = static_cast<size_t>(capacity), R = static_cast<size_t>(h->shape.R);
    const size_t blocks = (static_cast<size_t>(h->shape.N) + kReplayThreads - 1U) / kReplayThreads;
    // (the wait: nobody is still working in an earlier ring)
    int rc = regrow(h, {fresh(r.state, C * R), fresh(r.next_state, C * R), fresh(r.action, C * r.action_bytes), fresh(r.reward, C), fresh(r.done, C)});
    if (rc != OKENV_OK || (rc = devEnsure(h, &r.d_words, 2)) != OKENV_OK || (rc = devEnsure(h, &r.d_counts, blocks)) != OKENV_OK)
        return rc;
    OK_HIP(h, hipMemsetAsync(r.d_words, 0, 2U * sizeof(uint64_t), h->stream));
    if (lds_kernel != nullptr && (rc = raiseLdsLimit(h, {lds_kernel})) != OKENV_OK)
        return rc;
    OK_HIP(h, hipStreamSynchronize(h->stream));
    r.capacity = capacity;
    r.flags    = flags;
    r.ok       = true;
    return OKENV_OK;
}

int ringReset(okenv *h, const RingKind &k)
{
    if (!h || !(h->*k.ring).ok)
        return ringMissing(h, k, "reset");
    OK_HIP(h, hipSetDevice(h->device));
    OK_HIP(h, hipMemsetAsync((h->*k.ring).d_words, 0, 2U * sizeof(uint64_t), h->stream));
    return OKENV_OK;
}

// Params: the push kernels' parameter struct of the ring's kind (OkReplayParams, OkDdpgReplayParams); Rec: its record
template <class Params, class Rec>
int ringPush(okenv *h, const RingKind &k, const Rec *rec, const float *reward)
{
    const std::string name = std::string(k.prefix) + "push: ";
    if (!h)
        return fail(h, OKENV_ERR_INVALID, name + "NULL handle");
    const OkRing &r = h->*k.ring;
    if (!r.ok)
        return ringMissing(h, k, "push");
    if (!rec)
        return fail(h, OKENV_ERR_INVALID, name + "the record is NULL");
    if (!rec->state || !rec->action)
        return fail(h, OKENV_ERR_INVALID, name + "the record needs state and action");
    if (!rec->alive && (r.flags & OKENV_REPLAY_PUSH_ALL) == 0U)
        return fail(h, OKENV_ERR_INVALID, name + "the record needs alive (or create the ring with OKENV_REPLAY_PUSH_ALL)");
    OK_HIP(h, hipSetDevice(h->device));
    Params p{};
    p.N        = h->shape.N;
    p.R        = h->shape.R;
    p.flags    = r.flags;
    p.capacity = static_cast<uint64_t>(r.capacity);
    p.ring     = ringFields<decltype(p.ring)>(r);
    p.pushed   = r.d_words;
    p.snapshot = r.d_words + 1;
    p.counts   = r.d_counts;
    p.rec      = *rec;
    p.dist     = h->st.dist;
    p.crashed  = h->st.crashed;
    p.reward   = reward;
    const unsigned blocks = static_cast<unsigned>((h->shape.N + kReplayThreads - 1) / kReplayThreads);
    hipLaunchKernelGGL(okReplayCountKernel<Params>, dim3(blocks), dim3(kReplayThreads), 0, h->stream, p);
    OK_HIP(h, hipGetLastError());
    hipLaunchKernelGGL(okReplayScatterKernel<Params>, dim3(blocks), dim3(kReplayThreads), 0, h->stream, p);
    OK_HIP(h, hipGetLastError());
    return OKENV_OK;
}

int ringSize(okenv *h, const RingKind &k, int64_t *size, int64_t *pushed)
{
    if (!h || !(h->*k.ring).ok)
        return ringMissing(h, k, "size");
    const OkRing &r = h->*k.ring;
    OK_HIP(h, hipSetDevice(h->device));
    uint64_t word = 0;
    OK_HIP(h, hipMemcpyAsync(&word, r.d_words, sizeof(word), hipMemcpyDeviceToHost, h->stream));
    OK_HIP(h, hipStreamSynchronize(h->stream));
    if (size)
        *size = static_cast<int64_t>(ok_dqn_size(word, static_cast<uint64_t>(r.capacity)));
    if (pushed)
        *pushed = static_cast<int64_t>(word);
    return OKENV_OK;
}

template <class Ring>
int ringGet(okenv *h, const RingKind &k, const Ring *out)
{
    if (!h || !out)
        return fail(h, OKENV_ERR_INVALID, std::string(k.prefix) + "get: NULL argument");
    const OkRing &r = h->*k.ring;
    if (!r.ok)
        return ringMissing(h, k, "get");
    OK_HIP(h, hipSetDevice(h->device));
    const size_t C = static_cast<size_t>(r.capacity), R = static_cast<size_t>(h->shape.R);
    void *const       dst[5]   = {out->state, out->next_state, out->action, out->reward, out->done};
    const void *const src[5]   = {r.state, r.next_state, r.action, r.reward, r.done};
    const size_t      bytes[5] = {C * R * sizeof(float), C * R * sizeof(float), C * r.action_bytes, C * sizeof(float), C * sizeof(float)};
    for (int i = 0; i < 5; ++i)
        if (dst[i] != nullptr)
        {
            const int rc = copyAny(h, dst[i], src[i], bytes[i]);
            if (rc != OKENV_OK)
                return rc;
        }
    OK_HIP(h, hipStreamSynchronize(h->stream));
    return OKENV_OK;
}

// The launch knobs as the environment sets them: the one place that reads them.
OkKnobs readKnobs()
{
    OkKnobs k;
    if (const char *e = std::getenv("OKENV_LANES_PER_AGENT"))
        k.lanes_per_agent = std::atoi(e);
    if (const char *e = std::getenv("OKENV_BLOCK_THREADS"))
        k.block_threads = std::atol(e);
    if (const char *e = std::getenv("OKENV_COOP"))
        k.coop = std::atoi(e);
    if (const char *e = std::getenv("OKENV_AGENTS_PER_BLOCK"))
        k.agents_per_block = std::atoi(e);
    if (const char *e = std::getenv("OKENV_TAIL_MAX_AGENTS"))
        k.tail_max_agents = std::atoi(e);
    if (const char *e = std::getenv("OKENV_PHASE1_RANGE"))
        k.phase1_range = static_cast<float>(std::atof(e));
    if (const char *e = std::getenv("OKENV_RESIDENT"))
        k.resident = std::atoi(e);
    if (const char *e = std::getenv("OKENV_FRONT_BACK"))
        k.front_back = std::atoi(e);
    return k;
}

// ---- okenv_debug_math / okenv_debug_adam_device ----

// their device buffer: freed on every way out
struct DebugBuffer
{
    float *d = nullptr;
    ~DebugBuffer()
    {
        if (d != nullptr)
            (void)hipFree(d);
    }
};

int debugNeedsDevice(const char *who)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, OKENV_ERR_NO_DEVICE, std::string(who) + ": no HIP device");
    return OKENV_OK;
}

template <int kFn>
int debugMath(const int32_t device, const float *a, const float *b, float *out0, float *out1, const int32_t n)
{
    const size_t count = static_cast<size_t>(n);
    if (device == OKENV_DEBUG_ON_HOST)
    {
        // elements are independent: up to eight host threads share them (ok_sincosf's fmod and the normalisers' loops are slow)
        const size_t        workers = std::min<size_t>(8, count / 65536 + 1);
        std::vector<std::thread> pool;
        for (size_t w = 0; w < workers; ++w)
            pool.emplace_back([=] {
                for (size_t i = count * w / workers; i < count * (w + 1) / workers; ++i)
                    okDebugMathElement<kFn>(a, b, out0, out1, i);
            });
        for (std::thread &t : pool)
            t.join();
        return OKENV_OK;
    }
    if (const int rc = debugNeedsDevice("okenv_debug_math"))
        return rc;
    if (n == 0)
        return OKENV_OK;
    OK_HIP(nullptr, hipSetDevice(device));
    // four arrays: a, b (OKENV_FN_ATAN2 and OKENV_FN_SINCOS_PAIR only) of n floats, out0, out1 (OKENV_FN_SINCOS and
    // OKENV_FN_SINCOS_PAIR only) of n floats, 2 n for OKENV_FN_SINCOS_PAIR
    constexpr bool kPair = kFn == OKENV_FN_SINCOS_PAIR;
    const size_t   wide  = kPair ? 2U * count : count;
    DebugBuffer    buf;
    OK_HIP(nullptr, hipMalloc(reinterpret_cast<void **>(&buf.d), 4U * (2U * count + 2U * wide)));
    float *da = buf.d, *db = buf.d + count, *d0 = buf.d + 2U * count, *d1 = d0 + wide;
    OK_HIP(nullptr, hipMemcpy(da, a, 4U * count, hipMemcpyHostToDevice));
    if (kFn == OKENV_FN_ATAN2 || kPair)
        OK_HIP(nullptr, hipMemcpy(db, b, 4U * count, hipMemcpyHostToDevice));
    const unsigned un = static_cast<unsigned>(n);
    hipLaunchKernelGGL(okDebugMathKernel<kFn>, dim3((un + 255U) / 256U), dim3(256), 0, nullptr, da, db, d0, d1, un);
    OK_HIP(nullptr, hipGetLastError());
    OK_HIP(nullptr, hipMemcpy(out0, d0, 4U * wide, hipMemcpyDeviceToHost));
    if (kFn == OKENV_FN_SINCOS || kPair)
        OK_HIP(nullptr, hipMemcpy(out1, d1, 4U * wide, hipMemcpyDeviceToHost));
    return OKENV_OK;
}
} // namespace

extern "C"
{
    const char *okenv_last_error(okenv_t h)
    {
        return h ? h->last_error.c_str() : g_create_error.c_str();
    }

    int okenv_create(okenv_t     *out,
                     const float *segments_xyxy,
                     int32_t      num_segments,
                     int32_t      num_agents,
                     int32_t      num_rays,
                     const float *ray_angles_deg,
                     int32_t      device,
                     uint32_t     flags,
                     float        grid_cell)
    {
        if (!out)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_create: out is NULL");
        *out = nullptr;
        // TrackSegments asserts num_segments > 0 (TrackSegments.cu:72); CollisionChecker needs >= 1 agent with >= 1 ray
        if (!segments_xyxy || num_segments <= 0)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_create: need at least one segment");
        if (num_agents <= 0 || num_rays <= 0 || !ray_angles_deg)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_create: need at least one agent and one ray");
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
            return fail(nullptr, OKENV_ERR_NO_DEVICE, "okenv_create: no HIP device available (there is no CPU fallback)");
        if (device < 0 || device >= ndev)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_create: device ordinal out of range");

        // every early return below releases what has been allocated so far (stream, device buffers)
        struct Destroy
        {
            void operator()(okenv *e) const { okenv_destroy(e); }
        };
        std::unique_ptr<okenv, Destroy> hp(new okenv);
        okenv                          *h = hp.get();
        h->device                = device;
        h->S                     = num_segments;
        h->flags                 = flags;
        OK_HIP(nullptr, hipSetDevice(device));
        OK_HIP(nullptr, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));

        // lanes per agent, phase 1 and the default cell edge; the device is asked for its compute units (an MI355X in CPX / DPX
        // partition mode shows 32 / 128 of its 256 CUs)
        const OkKnobs knobs = readKnobs();
        int           cus   = 0;
        OK_HIP(nullptr, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
        h->shape = okPlanLanes(num_agents, num_rays, cus > 0 ? cus : 256, knobs);

        // ---- grid ------------------------------------------------------------------------------------
        const OkSeg *segs = reinterpret_cast<const OkSeg *>(segments_xyxy);
        bool         fits = false;
        h->grid = okBuildGridAuto(segs, static_cast<size_t>(num_segments), grid_cell > 0.F ? grid_cell : h->shape.cell_default,
                                  kLdsBudget - kLdsReserve, &fits, &h->poly);
        okPlanGeometry(h->shape, flags, fits, knobs);
        // The front / back split (ok_grid.h): the outer boundary polylines in an image of their own, walked only by the rays that
        // need it.  OKENV_FRONT_BACK=0 keeps every launch on the combined image (ablation; same results).
        if (h->shape.front_back)
        {
            auto classify = [&]() {
                h->fbc = okClassifyFrontBack(segs, static_cast<size_t>(num_segments), h->grid, h->poly.max_seg_len);
                h->fbi = okBuildFrontBackImages(segs, static_cast<size_t>(num_segments), h->grid, h->fbc);
            };
            classify();
            // 32-lane groups (the EvolutionaryRacer shape): most of a generation's steps are taken by the tail kernel, one agent per
            // workgroup, and the drivers hand a list over to it at up to two workgroups per CU -- which the two images allow only when
            // they fit the CU's LDS twice.  With a default cell edge the smallest of 20 / 24 / 28 / 32 px that manages it is taken
            // (larger cells, smaller images; the cooperative kernel's step time is flat over that range: profiles/r4/front_back_ab.txt).
            auto twice = [&]() { return 2U * okTailLdsBytes(h->fbi.front.bytes.size() + h->fbi.back.bytes.size(), false, 0U) <= kLdsBudget; };
            if (grid_cell <= 0.F && h->shape.G == 32 && h->fbi.ok && !twice())
            {
                const OkGridHost       grid0 = h->grid;
                const OkPolyImage      poly0 = h->poly;
                const OkFrontBack      fbc0  = h->fbc;
                const OkFrontBackImages fbi0 = h->fbi;
                bool                   found = false;
                for (const float c : {24.F, 28.F, 32.F})
                {
                    bool        fits2 = false;
                    OkPolyImage poly2;
                    OkGridHost  grid2 = okBuildGridAuto(segs, static_cast<size_t>(num_segments), c, kLdsBudget - kLdsReserve, &fits2, &poly2);
                    if (!fits2)
                        break;
                    h->grid = grid2;
                    h->poly = poly2;
                    classify();
                    if (h->fbi.ok && twice())
                    {
                        found = true;
                        break;
                    }
                }
                if (!found)
                {
                    h->grid = grid0;
                    h->poly = poly0;
                    h->fbc  = fbc0;
                    h->fbi  = fbi0;
                }
            }
        }

        int rc;
        if ((rc = devAlloc(h, &h->d_segs, static_cast<size_t>(num_segments))) != OKENV_OK)
            return fail(nullptr, rc, h->last_error);
        OK_HIP(nullptr, hipMemcpyAsync(h->d_segs, segs, sizeof(OkSeg) * num_segments, hipMemcpyHostToDevice, h->stream));
        if (h->shape.grid_mode == kGridLds)
        {
            h->shape.image_bytes            = h->poly.bytes.size();
            const std::vector<uint8_t> &img = h->poly.bytes;
            uint8_t *dimg = nullptr;
            if ((rc = devAlloc(h, &dimg, h->shape.image_bytes)) != OKENV_OK)
                return fail(nullptr, rc, h->last_error);
            h->d_image = dimg;
            OK_HIP(nullptr, hipMemcpyAsync(dimg, img.data(), h->shape.image_bytes, hipMemcpyHostToDevice, h->stream));
            // The front / back split (ok_grid.h; classified before the images were uploaded, above): its two images as one blob.
            if (h->fbi.ok && h->fbi.front.bytes.size() + h->fbi.back.bytes.size() <= kLdsBudget - kLdsReserve)
            {
                h->fb_back_off    = h->fbi.front.bytes.size(); // (a multiple of 16: both parts of an image are 16-byte aligned)
                h->shape.fb_bytes = h->fb_back_off + h->fbi.back.bytes.size();
                if ((rc = devAlloc(h, &h->d_image_fb, h->shape.fb_bytes)) != OKENV_OK)
                    return fail(nullptr, rc, h->last_error);
                OK_HIP(nullptr, hipMemcpyAsync(h->d_image_fb, h->fbi.front.bytes.data(), h->fb_back_off, hipMemcpyHostToDevice, h->stream));
                OK_HIP(nullptr, hipMemcpyAsync(h->d_image_fb + h->fb_back_off, h->fbi.back.bytes.data(), h->fbi.back.bytes.size(), hipMemcpyHostToDevice,
                                               h->stream));
                h->shape.fb_ok = true;
            }
            OK_HIP(nullptr, hipStreamSynchronize(h->stream));
            if ((rc = raiseLdsLimit(nullptr, {kernelOf(okStepKernel<kGridLds, kPolicyNone>), kernelOf(okStepKernel<kGridLds, kPolicyMlp>),
                                              kernelOf(okDebugCastKernel<kGridLds>)}, h->shape.image_bytes)) != OKENV_OK ||
                (rc = raiseLdsLimit(nullptr, {kernelOf(okStepCoopKernel<kPolicyNone>), kernelOf(okStepCoopKernel<kPolicyNone, true>),
                                              kernelOf(okStepCoopKernel<kPolicyNone, true, true>),
                                              kernelOf(okStepCoopKernel<kPolicyNone, false, false, false, 64, true>),
                                              kernelOf(okStepCoopKernel<kPolicyNone, false, false, false, 64>),
                                              kernelOf(okStepCoopKernel<kPolicyNone, false, false, true>),
                                              kernelOf(okStepCoopKernel<kPolicyNone, true, false, true>),
                                              kernelOf(okStepCoopKernel<kPolicyNone, true, true, true>), kernelOf(okStepCoopKernel<kPolicyMlp>),
                                              kernelOf(okStepCoopKernel<kPolicyQ>), kernelOf(okStepCoopKernel<kPolicyCtrl>),
                                              kernelOf(okStepCoopKernel<kPolicyMlp, false, false, false, 32>),
                                              kernelOf(okStepTailKernel<kPolicyMlp, 32>), kernelOf(okStepTailKernel<kPolicyMlp, 15>),
                                              kernelOf(okStepTailKernel<kPolicyMlp, 0>), kernelOf(okStepTailKernel<kPolicyQ, 0>)})) != OKENV_OK)
                return rc;
        }
        else if (h->shape.grid_mode == kGridGlobal)
        {
            if ((rc = devAlloc(h, &h->d_refs32, h->grid.refs.size())) != OKENV_OK ||
                (rc = devAlloc(h, &h->d_start, h->grid.start.size())) != OKENV_OK)
                return fail(nullptr, rc, h->last_error);
            OK_HIP(nullptr, hipMemcpyAsync(h->d_refs32, h->grid.refs.data(), 4U * h->grid.refs.size(), hipMemcpyHostToDevice, h->stream));
            OK_HIP(nullptr, hipMemcpyAsync(h->d_start, h->grid.start.data(), 4U * h->grid.start.size(), hipMemcpyHostToDevice, h->stream));
        }

        // ---- state -----------------------------------------------------------------------------------
        const size_t N = num_agents, NR = static_cast<size_t>(num_agents) * num_rays;
        auto        &s = h->st;
        if ((rc = devAlloc(h, &s.pos_x, N)) || (rc = devAlloc(h, &s.pos_y, N)) || (rc = devAlloc(h, &s.rot, N)) ||
            (rc = devAlloc(h, &s.speed, N)) || (rc = devAlloc(h, &s.acc, N)) || (rc = devAlloc(h, &s.thr, N)) ||
            (rc = devAlloc(h, &s.steer, N)) || (rc = devAlloc(h, &s.mode, N)) || (rc = devAlloc(h, &s.crashed, N)) ||
            (rc = devAlloc(h, &s.timed_out, N)) || (rc = devAlloc(h, &s.disp_to, N)) || (rc = devAlloc(h, &s.disp_ctr, N)) ||
            (rc = devAlloc(h, &s.disp_x, N)) || (rc = devAlloc(h, &s.disp_y, N)) || (rc = devAlloc(h, &s.hit_x, NR)) ||
            (rc = devAlloc(h, &s.hit_y, NR)) || (rc = devAlloc(h, &s.rel_x, NR)) || (rc = devAlloc(h, &s.rel_y, NR)) ||
            (rc = devAlloc(h, &s.dist, NR)) || (rc = devAlloc(h, &h->d_ray_deg, static_cast<size_t>(num_rays))) ||
            (rc = devAlloc(h, &h->d_step_count, 2))) // [0] steps, [1] finished workgroups of the running launch
            return fail(nullptr, rc, h->last_error);
        OK_HIP(nullptr, hipMemcpyAsync(h->d_ray_deg, ray_angles_deg, 4U * num_rays, hipMemcpyHostToDevice, h->stream));
        h->host_ray_deg.assign(ray_angles_deg, ray_angles_deg + num_rays);

        if (const char *env_stall = std::getenv("OKENV_RESIDENT_STALL_US"))
            h->resident_stall_us = std::atoi(env_stall);
        OK_HIP(nullptr, hipStreamSynchronize(h->stream));
        *out = hp.release();
        return OKENV_OK;
    }

    int okenv_destroy(okenv_t h)
    {
        if (!h)
            return OKENV_OK;
        (void)hipSetDevice(h->device);
        if (h->resident)
            (void)stopResident(h);
        if (h->resident_stream)
            (void)hipStreamDestroy(h->resident_stream);
        // a borrowed stream (okenv_set_stream) may already be gone, or be capturing: wait for the device instead of touching it
        if (h->own_stream)
            (void)hipStreamSynchronize(h->stream);
        else
            (void)hipDeviceSynchronize();
        for (void *p : h->allocations)
            (void)hipFree(p);
        if (h->h_stage)
            (void)hipHostFree(h->h_stage);
        for (auto &e : h->events)
        {
            (void)hipEventDestroy(e.start);
            (void)hipEventDestroy(e.stop);
        }
        for (auto &e : h->event_pool)
        {
            (void)hipEventDestroy(e.start);
            (void)hipEventDestroy(e.stop);
        }
        for (OkUpdateScratch *u : {&h->batch_scratch, &h->learn_scratch, &h->dqn_scratch, &h->ddpg_scratch, &h->reinforce_scratch, &h->gauss_scratch, &h->gcl_scratch[0],
                                   &h->gcl_scratch[1], &h->gcl_scratch[2], &h->gcl_adv_scratch, &h->vit_head_scratch})
            for (hipEvent_t e : u->log.events)
                (void)hipEventDestroy(e);
        if (h->own_stream && h->stream)
            (void)hipStreamDestroy(h->stream);
        delete h;
        return OKENV_OK;
    }

    int okenv_get_info(okenv_t h, okenv_info *out)
    {
        if (!h || !out)
            return fail(h, OKENV_ERR_INVALID, "okenv_get_info: NULL argument");
        out->num_agents      = h->shape.N;
        out->num_rays        = h->shape.R;
        out->num_segments    = h->S;
        out->compute_units   = h->shape.cus;
        out->front_back_bytes = h->shape.fb_ok ? static_cast<int32_t>(h->shape.fb_bytes) : 0;
        out->back_segments    = h->shape.fb_ok ? static_cast<int32_t>(h->fbc.n_back) : 0;
        out->grid_nx         = h->grid.g.nx;
        out->grid_ny         = h->grid.g.ny;
        out->grid_cell       = h->grid.g.cell;
        out->grid_refs       = static_cast<int32_t>(h->grid.refs.size());
        out->grid_in_lds     = h->shape.grid_mode == kGridLds ? 1 : 0;
        out->lds_bytes       = h->shape.grid_mode == kGridLds ? static_cast<int32_t>(h->shape.image_bytes) : 0;
        out->block_threads   = h->shape.block_threads;
        out->grid_blocks     = h->shape.grid_blocks;
        out->agents_per_block      = h->shape.coop ? h->shape.agents_per_block : 0;
        out->packed_resident       = h->resident ? 1 : 0;
        out->packed_resident_steps = h->resident_steps;
        out->packed_fallbacks      = h->resident_fallbacks;
        out->lanes_per_agent = h->shape.G;
        out->device          = h->device;
        return OKENV_OK;
    }

    int okenv_set_sensor_offset(okenv_t h, float offset)
    {
        if (!h)
            return OKENV_ERR_INVALID;
        if (offset == h->sensor_offset)
            return OKENV_OK; // the C++ facade says it before every step: not a reason to stop a resident step kernel
        OK_QUIESCE(h);
        h->sensor_offset = offset;
        return OKENV_OK;
    }

    int okenv_set_centerline(okenv_t h, const float *x, const float *y, const float *heading_deg, int32_t num_points)
    {
        OK_QUIESCE(h);
        if (!h || !x || !y || !heading_deg || num_points <= 0)
            return fail(h, OKENV_ERR_INVALID, "okenv_set_centerline: bad argument");
        OK_HIP(h, hipSetDevice(h->device));
        int rc;
        if (num_points > h->centerline_capacity)
        { // grow only: repeated calls with the same track reuse the buffers
            if ((rc = devAlloc(h, &h->d_cx, static_cast<size_t>(num_points))) || (rc = devAlloc(h, &h->d_cy, static_cast<size_t>(num_points))) ||
                (rc = devAlloc(h, &h->d_chead, static_cast<size_t>(num_points))))
                return rc;
            h->centerline_capacity = num_points;
        }
        h->P        = num_points;
        h->cl_dirty = true;
        h->host_cx.resize(num_points), h->host_cy.resize(num_points), h->host_chead.resize(num_points);
        OK_HIP(h, hipMemcpy(h->host_cx.data(), x, 4U * num_points, hipMemcpyDefault));
        OK_HIP(h, hipMemcpy(h->host_cy.data(), y, 4U * num_points, hipMemcpyDefault));
        OK_HIP(h, hipMemcpy(h->host_chead.data(), heading_deg, 4U * num_points, hipMemcpyDefault));
        OK_HIP(h, hipMemcpyAsync(h->d_cx, x, 4U * num_points, hipMemcpyDefault, h->stream));
        OK_HIP(h, hipMemcpyAsync(h->d_cy, y, 4U * num_points, hipMemcpyDefault, h->stream));
        OK_HIP(h, hipMemcpyAsync(h->d_chead, heading_deg, 4U * num_points, hipMemcpyDefault, h->stream));
        OK_HIP(h, hipStreamSynchronize(h->stream));
        return OKENV_OK;
    }

    int okenv_set_stream(okenv_t h, void *hip_stream)
    {
        OK_QUIESCE(h);
        if (!h)
            return OKENV_ERR_INVALID;
        // no synchronisation here: the call must be legal while the new stream is being captured into a graph; work
        // already queued on the old stream completes on its own (hipStreamDestroy defers), ordering is the caller's
        if (h->own_stream && h->stream)
        {
            // timing events recorded on the stream about to be destroyed are resolved first (nothing can be captured on a
            // stream this handle owns, so waiting for them is legal here) and carried into the next okenv_get_timing
            for (auto &e : h->events)
            {
                float ms = 0.F;
                if (hipEventSynchronize(e.stop) == hipSuccess && hipEventElapsedTime(&ms, e.start, e.stop) == hipSuccess)
                {
                    h->timing_carry_ms += ms;
                    ++h->timing_carry_n;
                }
                h->event_pool.push_back(e);
            }
            h->events.clear();
            (void)hipStreamDestroy(h->stream);
        }
        h->stream     = static_cast<hipStream_t>(hip_stream);
        h->own_stream = false;
        return OKENV_OK;
    }

    int okenv_sync(okenv_t h)
    {
        OK_QUIESCE(h);
        if (!h)
            return OKENV_ERR_INVALID;
        OK_HIP(h, hipStreamSynchronize(h->stream));
        return OKENV_OK;
    }

    int okenv_set_field(okenv_t h, int32_t field, const void *src)
    {
        OK_QUIESCE(h);
        if (h)
            dropEpisode(h);
        if (!h || !src)
            return fail(h, OKENV_ERR_INVALID, "okenv_set_field: NULL argument");
        const FieldDesc d = fieldOf(h, field);
        if (!d.ptr)
            return fail(h, OKENV_ERR_INVALID, "okenv_set_field: unknown field (tracker fields exist after okenv_tracker_create)");
        int rc = copyAny(h, d.ptr, src, d.bytes);
        if (rc != OKENV_OK)
            return rc;
        OK_HIP(h, hipStreamSynchronize(h->stream)); // the caller may reuse src immediately
        return OKENV_OK;
    }

    int okenv_get_field(okenv_t h, int32_t field, void *dst)
    {
        OK_QUIESCE(h);
        if (!h || !dst)
            return fail(h, OKENV_ERR_INVALID, "okenv_get_field: NULL argument");
        const FieldDesc d = fieldOf(h, field);
        if (!d.ptr)
            return fail(h, OKENV_ERR_INVALID, "okenv_get_field: unknown field (tracker fields exist after okenv_tracker_create)");
        int rc = copyAny(h, dst, d.ptr, d.bytes);
        if (rc != OKENV_OK)
            return rc;
        OK_HIP(h, hipStreamSynchronize(h->stream));
        return OKENV_OK;
    }

    static int moveState(okenv_t h, const okenv_state_view *v, const bool upload)
    {
        if (!h || !v)
            return fail(h, OKENV_ERR_INVALID, "state view is NULL");
        const size_t N = h->shape.N;
        auto        &s = h->st;
        struct Item
        {
            void  *dev;
            void  *host;
            size_t bytes;
        };
        const Item items[] = {{s.pos_x, v->pos_x, 4 * N},       {s.pos_y, v->pos_y, 4 * N},     {s.rot, v->rot, 4 * N},
                              {s.speed, v->speed, 4 * N},       {s.acc, v->acc, 4 * N},         {s.thr, v->throttle, 4 * N},
                              {s.steer, v->steer, 4 * N},       {s.mode, v->mode, N},           {s.crashed, v->crashed, N},
                              {s.timed_out, v->timed_out, N},   {s.disp_ctr, v->disp_ctr, 4 * N}, {s.disp_x, v->disp_x, 4 * N},
                              {s.disp_y, v->disp_y, 4 * N},     {s.disp_to, v->disp_timed_out, N}};
        for (const Item &it : items)
        {
            if (!it.host)
                continue;
            const int rc = upload ? copyAny(h, it.dev, it.host, it.bytes) : copyAny(h, it.host, it.dev, it.bytes);
            if (rc != OKENV_OK)
                return rc;
        }
        OK_HIP(h, hipStreamSynchronize(h->stream));
        return OKENV_OK;
    }

    int okenv_upload_state(okenv_t h, const okenv_state_view *host_view)
    {
        OK_QUIESCE(h);
        if (h)
            dropEpisode(h);
        return moveState(h, host_view, true);
    }

    int okenv_download_state(okenv_t h, const okenv_state_view *host_view)
    {
        OK_QUIESCE(h);
        return moveState(h, host_view, false);
    }

    int okenv_set_actions(okenv_t h, const float *throttle, const float *steer)
    {
        OK_QUIESCE(h);
        if (h)
            dropEpisode(h);
        if (!h || !throttle || !steer)
            return fail(h, OKENV_ERR_INVALID, "okenv_set_actions: NULL argument");
        int rc;
        if ((rc = copyAny(h, h->st.thr, throttle, 4U * h->shape.N)) || (rc = copyAny(h, h->st.steer, steer, 4U * h->shape.N)))
            return rc;
        OK_HIP(h, hipStreamSynchronize(h->stream));
        return OKENV_OK;
    }

    int okenv_reset_agents(okenv_t h, const int32_t *idx, const float *x, const float *y, const float *rot_deg, int32_t n)
    {
        OK_QUIESCE(h);
        if (h)
            dropEpisode(h);
        if (!h || n < 0 || (n > 0 && (!idx || !x || !y || !rot_deg)))
            return fail(h, OKENV_ERR_INVALID, "okenv_reset_agents: bad argument");
        if (n == 0)
            return OKENV_OK;
        OK_HIP(h, hipSetDevice(h->device));
        // one staging buffer: idx | x | y | rot
        const size_t bytes = static_cast<size_t>(n) * 16U;
        void        *stage = nullptr;
        const int    src   = deviceScratch(h, bytes, &stage);
        if (src != OKENV_OK)
            return src;
        char *b = static_cast<char *>(stage);
        OK_HIP(h, hipMemcpyAsync(b, idx, 4U * n, hipMemcpyHostToDevice, h->stream));
        OK_HIP(h, hipMemcpyAsync(b + 4U * n, x, 4U * n, hipMemcpyHostToDevice, h->stream));
        OK_HIP(h, hipMemcpyAsync(b + 8U * n, y, 4U * n, hipMemcpyHostToDevice, h->stream));
        OK_HIP(h, hipMemcpyAsync(b + 12U * n, rot_deg, 4U * n, hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(okResetKernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->st, reinterpret_cast<const int32_t *>(b),
                           reinterpret_cast<const float *>(b + 4U * n), reinterpret_cast<const float *>(b + 8U * n),
                           reinterpret_cast<const float *>(b + 12U * n), n, h->shape.N);
        OK_HIP(h, hipGetLastError());
        OK_HIP(h, hipStreamSynchronize(h->stream));
        return OKENV_OK;
    }

    int okenv_set_lane_bounds(okenv_t h, const float *left_inner_xy, const float *right_inner_xy, int32_t num_points)
    {
        OK_QUIESCE(h);
        if (!h || !left_inner_xy || !right_inner_xy || num_points <= 0)
            return fail(h, OKENV_ERR_INVALID, "okenv_set_lane_bounds: bad argument");
        OK_HIP(h, hipSetDevice(h->device));
        if (num_points > h->lane_capacity)
        {
            int rc;
            if ((rc = devAlloc(h, &h->d_lane_l, 2U * static_cast<size_t>(num_points))) ||
                (rc = devAlloc(h, &h->d_lane_r, 2U * static_cast<size_t>(num_points))))
                return rc;
            h->lane_capacity = num_points;
        }
        h->lane_points = num_points;
        OK_HIP(h, hipMemcpyAsync(h->d_lane_l, left_inner_xy, 8U * num_points, hipMemcpyDefault, h->stream));
        OK_HIP(h, hipMemcpyAsync(h->d_lane_r, right_inner_xy, 8U * num_points, hipMemcpyDefault, h->stream));
        OK_HIP(h, hipStreamSynchronize(h->stream));
        return OKENV_OK;
    }

    // shared precondition of the two resetAgent entry points
    static int checkResetInputs(okenv_t h, const uint32_t flags, const char *who)
    {
        if (h->P <= 0)
            return fail(h, OKENV_ERR_STATE, std::string(who) + ": call okenv_set_centerline first");
        if ((flags & OK_RESET_RANDOM_POINT) == 0U && h->P <= static_cast<int>(OK_RESET_START_IDX))
            return fail(h, OKENV_ERR_STATE, std::string(who) + ": the centre line is shorter than RaceTrack::kStartingIdx");
        if ((flags & OK_RESET_RANDOM_POINT) != 0U && (flags & OK_RESET_RANDOM_LANE) != 0U && h->lane_points != h->P)
            return fail(h, OKENV_ERR_STATE, std::string(who) + ": lane randomisation needs okenv_set_lane_bounds with as many points as the centre line");
        return OKENV_OK;
    }

    int okenv_reset_random(okenv_t h, const int32_t *idx, int32_t n, uint32_t flags, uint32_t seed, uint32_t epoch, uint32_t agent_base)
    {
        OK_QUIESCE(h);
        if (h)
            dropEpisode(h);
        if (!h || n < 0)
            return fail(h, OKENV_ERR_INVALID, "okenv_reset_random: bad argument");
        if (!idx)
            n = h->shape.N;
        if (n == 0)
            return OKENV_OK;
        int rc = checkResetInputs(h, flags, "okenv_reset_random");
        if (rc != OKENV_OK)
            return rc;
        OK_HIP(h, hipSetDevice(h->device));
        int32_t *didx = nullptr;
        if (idx)
        {
            void     *sp  = nullptr;
            const int src = deviceScratch(h, 4U * static_cast<size_t>(n), &sp);
            if (src != OKENV_OK)
                return src;
            didx = static_cast<int32_t *>(sp);
            OK_HIP(h, hipMemcpyAsync(didx, idx, 4U * static_cast<size_t>(n), hipMemcpyDefault, h->stream));
        }
        hipLaunchKernelGGL(okResetRandomKernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->st, didx, n, h->shape.N, flags, seed, epoch,
                           agent_base, h->d_cx, h->d_cy, h->d_chead, h->d_lane_l, h->d_lane_r, h->P);
        OK_HIP(h, hipGetLastError());
        if (didx)
            OK_HIP(h, hipStreamSynchronize(h->stream)); // the caller may reuse idx, the next call the staging space
        return OKENV_OK;
    }

    int okenv_set_auto_reset(okenv_t h, int32_t enabled, uint32_t flags, uint32_t seed, uint32_t agent_base)
    {
        OK_QUIESCE(h);
        if (h)
            dropEpisode(h);
        if (!h)
            return OKENV_ERR_INVALID;
        uint32_t count = 0;
        int      rc    = okenv_get_step_count(h, &count); // folds the device copy back while it is still authoritative
        if (rc != OKENV_OK)
            return rc;
        if (!enabled)
        {
            h->reset_flags = 0;
            return OKENV_OK;
        }
        if ((rc = checkResetInputs(h, flags, "okenv_set_auto_reset")) != OKENV_OK)
            return rc;
        if ((rc = okenv_set_step_count(h, count)) != OKENV_OK)
            return rc;
        h->reset_flags      = (flags & (OK_RESET_RANDOM_POINT | OK_RESET_RANDOM_LANE | OK_RESET_RANDOM_HEADING)) | kAutoResetOn;
        h->reset_seed       = seed;
        h->reset_agent_base = agent_base;
        return OKENV_OK;
    }

    int okenv_get_step_count(okenv_t h, uint32_t *out)
    {
        OK_QUIESCE(h);
        if (!h || !out)
            return fail(h, OKENV_ERR_INVALID, "okenv_get_step_count: NULL argument");
        if ((h->reset_flags & kAutoResetOn) != 0U)
        {
            OK_HIP(h, hipSetDevice(h->device));
            OK_HIP(h, hipMemcpyAsync(&h->step_count, h->d_step_count, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
            OK_HIP(h, hipStreamSynchronize(h->stream));
        }
        *out = h->step_count;
        return OKENV_OK;
    }

    int okenv_set_step_count(okenv_t h, uint32_t value)
    {
        OK_QUIESCE(h);
        if (h)
            dropEpisode(h);
        if (!h)
            return OKENV_ERR_INVALID;
        h->step_count = value;
        OK_HIP(h, hipSetDevice(h->device));
        OK_HIP(h, hipMemcpyAsync(h->d_step_count, &h->step_count, sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        OK_HIP(h, hipStreamSynchronize(h->stream));
        return OKENV_OK;
    }

    int okenv_field_device_ptr(okenv_t h, int32_t field, void **ptr, uint64_t *bytes)
    {
        OK_QUIESCE(h);
        if (!h || !ptr)
            return fail(h, OKENV_ERR_INVALID, "okenv_field_device_ptr: NULL argument");
        const FieldDesc d = fieldOf(h, field);
        if (!d.ptr)
            return fail(h, OKENV_ERR_INVALID, "okenv_field_device_ptr: unknown field (tracker fields exist after okenv_tracker_create)");
        *ptr = d.ptr;
        if (bytes)
            *bytes = d.bytes;
        return OKENV_OK;
    }

    int okenv_get_hits(okenv_t h, float *out_xy)
    {
        OK_QUIESCE(h);
        if (!h || !out_xy)
            return fail(h, OKENV_ERR_INVALID, "okenv_get_hits: NULL argument");
        const size_t       NR = static_cast<size_t>(h->shape.N) * h->shape.R;
        std::vector<float> rx(NR), ry(NR);
        int                rc;
        if ((rc = copyAny(h, rx.data(), h->st.rel_x, 4U * NR)) || (rc = copyAny(h, ry.data(), h->st.rel_y, 4U * NR)))
            return rc;
        OK_HIP(h, hipStreamSynchronize(h->stream));
        for (size_t k = 0; k < NR; ++k)
        {
            out_xy[2 * k]     = rx[k];
            out_xy[2 * k + 1] = ry[k];
        }
        return OKENV_OK;
    }

    int okenv_get_distances(okenv_t h, float *out)
    {
        OK_QUIESCE(h);
        return okenv_get_field(h, OKENV_F_DIST, out);
    }

    int okenv_get_flags(okenv_t h, uint8_t *out)
    {
        OK_QUIESCE(h);
        if (!h || !out)
            return fail(h, OKENV_ERR_INVALID, "okenv_get_flags: NULL argument");
        std::vector<uint8_t> c(h->shape.N), t(h->shape.N);
        int                  rc;
        if ((rc = copyAny(h, c.data(), h->st.crashed, h->shape.N)) || (rc = copyAny(h, t.data(), h->st.timed_out, h->shape.N)))
            return rc;
        OK_HIP(h, hipStreamSynchronize(h->stream));
        for (int i = 0; i < h->shape.N; ++i)
            out[i] = static_cast<uint8_t>((c[i] ? 1 : 0) | (t[i] ? 2 : 0));
        return OKENV_OK;
    }

    int okenv_step(okenv_t h, int32_t n_steps)
    {
        OK_QUIESCE(h);
        if (h)
            dropEpisode(h);
        if (!h || n_steps < 0)
            return fail(h, OKENV_ERR_INVALID, "okenv_step: bad argument");
        if (n_steps == 0)
            return OKENV_OK;
        OkStepParams p = baseParams(h);
        p.n_steps      = n_steps;
        const int rc   = launchStep(h, p);
        return rc == OKENV_OK ? advanceStepCount(h, n_steps) : rc;
    }

    int okenv_step_packed(okenv_t h, const okenv_agent_record *in, okenv_agent_record *out, float *sensor_hits_xy, uint32_t flags)
    {
        if (h)
            dropEpisode(h);
        if (!h || !in || !out || !sensor_hits_xy)
            return fail(h, OKENV_ERR_INVALID, "okenv_step_packed: NULL argument");
        OK_HIP(h, hipSetDevice(h->device));
        const size_t N = static_cast<size_t>(h->shape.N), NR = N * static_cast<size_t>(h->shape.R);
        const size_t rec_bytes = N * sizeof(okenv_agent_record), hit_bytes = NR * 2U * sizeof(float);
        // mapped host memory: [ in records | out records | hits | completion word | one 64-byte slot per agent (resident kernel) ]
        const size_t out_off   = (rec_bytes + 255U) & ~static_cast<size_t>(255U);
        const size_t hit_off   = 2U * out_off;
        const size_t done_off  = (hit_off + hit_bytes + 63U) & ~static_cast<size_t>(63U);
        const size_t slots_off = done_off + kDoneWordBytes;
        const size_t stage_all = slots_off + 64U * N;
        if (!h->h_stage)
        { // both buffers are committed together: a failed second allocation must not leave a half-initialised pair behind
            void *pinned = nullptr, *mapped = nullptr;
            // coherent (fine-grained): the device's stores go straight to the host's memory, in order with the completion word
            OK_HIP(h, hipHostMalloc(&pinned, stage_all, hipHostMallocMapped | hipHostMallocCoherent));
            std::memset(pinned, 0, stage_all);
            uint8_t *d = nullptr;
            if (hipHostGetDevicePointer(&mapped, pinned, 0) != hipSuccess || devAlloc(h, &d, hit_off + hit_bytes) != OKENV_OK)
            {
                (void)hipHostFree(pinned);
                return fail(h, OKENV_ERR_HIP, "okenv_step_packed: cannot allocate the exchange buffers");
            }
            h->h_stage         = pinned;
            h->h_stage_device  = mapped;
            h->d_stage         = d;
            h->stage_slots_off = slots_off;
        }
        uint8_t *hs = static_cast<uint8_t *>(h->h_stage), *ds = static_cast<uint8_t *>(h->d_stage);
        if (h->shape.grid_mode == kGridLds && h->shape.coop)
        { // ONE kernel: it reads the records from, and writes records and sensor_hits_ to, the mapped host buffer
            uint8_t     *hm = static_cast<uint8_t *>(h->h_stage_device);
            OkStepParams p  = baseParams(h);
            p.rec_in         = reinterpret_cast<const okenv_agent_record *>(hm);
            p.rec_out        = reinterpret_cast<okenv_agent_record *>(hm + out_off);
            p.hits_xy_out    = reinterpret_cast<float *>(hm + hit_off);
            p.rec_with_stats = (flags & OKENV_PACKED_WITH_STATS) ? 1 : 0;
            p.done_flag      = reinterpret_cast<uint32_t *>(hm + done_off); // behind the hits, on a cache line of its own
            const volatile uint32_t *done_word = reinterpret_cast<const volatile uint32_t *>(hs + done_off);

            // steps that follow each other closely are served by a resident kernel (see startResident)
            const auto   t_in  = std::chrono::steady_clock::now();
            const bool   quick = h->packed_seq != 0U && std::chrono::duration<double, std::micro>(t_in - h->packed_last_end).count() < kResidentGapUs;
            const bool eligible = okResidentShape(h->shape) && h->own_stream && !h->timing &&
                                  (h->reset_flags & kAutoResetOn) == 0U && flags == OKENV_PACKED_WITH_STATS;
            // (a run of quick steps counts only while every one of them is of the kind the resident kernel serves: a caller that
            // alternates step() and checkCollision() must not start and stop a kernel on every other call)
            h->packed_streak = (quick && eligible) ? h->packed_streak + 1 : 0;
            if (h->resident && (!eligible || !quick))
            { // too long since the last step (the kernel may have left by itself), or a kind of step it does not serve
                const int src = stopResident(h);
                if (src != OKENV_OK)
                    return src;
            }
            const bool was_resident = h->resident;
            if (!h->resident && eligible && (h->shape.resident_mode == 1 || h->packed_streak >= h->resident_need))
            {
                p.slots          = reinterpret_cast<const uint32_t *>(hm + slots_off);
                p.idle_ticks     = kResidentIdleTicks;
                const int src = startResident(h, p, reinterpret_cast<volatile uint32_t *>(hs + slots_off));
                if (src != OKENV_OK)
                    return src;
            }
            bool served = false;
            if (h->resident)
            {
                const int src = stepResident(h, in, reinterpret_cast<volatile uint32_t *>(hs + slots_off), done_word, !was_resident, &served);
                if (src != OKENV_OK)
                    return src;
            }
            if (!served)
            {
                std::memcpy(hs, in, rec_bytes);
                p.slots    = nullptr;
                p.done_seq = nextPackedSeq(h);
                if (flags & OKENV_PACKED_COLLIDE_ONLY)
                {
                    p.do_move     = 0;
                    p.reset_flags = 0;
                }
                const int rc = launchStep(h, p);
                if (rc != OKENV_OK)
                    return rc;
                const int wrc = waitPackedDone(h, done_word, p.done_seq);
                if (wrc != OKENV_OK)
                    return wrc;
            }
            if ((flags & OKENV_PACKED_COLLIDE_ONLY) == 0U)
                advanceStepCount(h, 1);
            const okenv_agent_record *src = reinterpret_cast<const okenv_agent_record *>(hs + out_off);
            for (size_t i = 0; i < N; ++i)
            {
                okenv_agent_record r = src[i];
                if ((flags & OKENV_PACKED_WITH_STATS) == 0U)
                { // the caller's DisplacementStats members stay as they were (`out` may alias `in`: read before writing)
                    r.disp_x         = in[i].disp_x;
                    r.disp_y         = in[i].disp_y;
                    r.disp_ctr       = in[i].disp_ctr;
                    r.disp_timed_out = in[i].disp_timed_out;
                }
                out[i] = r;
            }
            std::memcpy(sensor_hits_xy, hs + hit_off, hit_bytes);
            h->packed_last_end = std::chrono::steady_clock::now();
            return OKENV_OK;
        }
        std::memcpy(hs, in, rec_bytes);
        OK_HIP(h, hipMemcpyAsync(ds, hs, rec_bytes, hipMemcpyHostToDevice, h->stream));
        const unsigned blocks_n = static_cast<unsigned>((N + 255U) / 256U);
        hipLaunchKernelGGL(okUnpackRecordsKernel, dim3(blocks_n), dim3(256), 0, h->stream, h->st,
                           reinterpret_cast<const okenv_agent_record *>(ds), h->shape.N, (flags & OKENV_PACKED_WITH_STATS) ? 1 : 0);
        OkStepParams p = baseParams(h);
        if (flags & OKENV_PACKED_COLLIDE_ONLY)
        {
            p.do_move     = 0;
            p.reset_flags = 0;
        }
        int rc = launchStep(h, p);
        if (rc != OKENV_OK)
            return rc;
        if ((flags & OKENV_PACKED_COLLIDE_ONLY) == 0U)
            advanceStepCount(h, 1);
        const size_t threads = NR > N ? NR : N;
        hipLaunchKernelGGL(okPackRecordsKernel, dim3(static_cast<unsigned>((threads + 255U) / 256U)), dim3(256), 0, h->stream, h->st,
                           reinterpret_cast<okenv_agent_record *>(ds + out_off), reinterpret_cast<float *>(ds + hit_off), h->shape.N, h->shape.R);
        OK_HIP(h, hipGetLastError());
        OK_HIP(h, hipMemcpyAsync(hs + out_off, ds + out_off, (hit_off - out_off) + hit_bytes, hipMemcpyDeviceToHost, h->stream));
        OK_HIP(h, hipStreamSynchronize(h->stream));
        if ((flags & OKENV_PACKED_WITH_STATS) != 0U)
            std::memcpy(out, hs + out_off, rec_bytes);
        else
        { // the caller's DisplacementStats members stay as they were
            const okenv_agent_record *src = reinterpret_cast<const okenv_agent_record *>(hs + out_off);
            for (size_t i = 0; i < N; ++i)
            {
                okenv_agent_record r = src[i];
                r.disp_x             = in[i].disp_x;
                r.disp_y             = in[i].disp_y;
                r.disp_ctr           = in[i].disp_ctr;
                r.disp_timed_out     = in[i].disp_timed_out;
                out[i]               = r;
            }
        }
        std::memcpy(sensor_hits_xy, hs + hit_off, hit_bytes);
        return OKENV_OK;
    }

    int okenv_collide(okenv_t h)
    {
        OK_QUIESCE(h);
        if (h)
            dropEpisode(h);
        if (!h)
            return OKENV_ERR_INVALID;
        OkStepParams p = baseParams(h);
        p.do_move      = 0;
        p.reset_flags  = 0;
        return launchStep(h, p);
    }

    int okenv_rollout_random(okenv_t h, int32_t n_steps, uint32_t seed, uint32_t agent_base, uint32_t step_base)
    {
        OK_QUIESCE(h);
        if (h)
            dropEpisode(h);
        if (!h || n_steps < 0)
            return fail(h, OKENV_ERR_INVALID, "okenv_rollout_random: bad argument");
        if (h->P <= 0)
            return fail(h, OKENV_ERR_STATE, "okenv_rollout_random: call okenv_set_centerline first");
        if (n_steps == 0)
            return OKENV_OK;
        OkStepParams p  = baseParams(h);
        p.n_steps       = n_steps;
        p.action_source = kActionsPhiloxReset;
        p.reset_flags   = 0; // this driver re-places crashed agents itself
        p.seed          = seed;
        p.agent_base    = agent_base;
        p.step_base     = step_base;
        return launchStep(h, p);
    }

    int okenv_init_bench_state(okenv_t h, uint32_t agent_base, int32_t mode)
    {
        OK_QUIESCE(h);
        if (h)
            dropEpisode(h);
        if (!h)
            return OKENV_ERR_INVALID;
        if (h->P <= 0)
            return fail(h, OKENV_ERR_STATE, "okenv_init_bench_state: call okenv_set_centerline first");
        OK_HIP(h, hipSetDevice(h->device));
        hipLaunchKernelGGL(okInitBenchKernel, dim3((h->shape.N + 255) / 256), dim3(256), 0, h->stream, h->st, h->d_cx, h->d_cy, h->d_chead,
                           h->P, h->shape.N, h->shape.R, agent_base, mode);
        OK_HIP(h, hipGetLastError());
        return OKENV_OK;
    }

    int okenv_nearest_track_idx(okenv_t h, const float *qx, const float *qy, int32_t n, int32_t *out)
    {
        OK_QUIESCE(h);
        if (!h || !out)
            return fail(h, OKENV_ERR_INVALID, "okenv_nearest_track_idx: NULL argument");
        if (h->P <= 0)
            return fail(h, OKENV_ERR_STATE, "okenv_nearest_track_idx: call okenv_set_centerline first");
        OK_HIP(h, hipSetDevice(h->device));
        const bool agents = (qx == nullptr);
        if (!agents && !qy) // every argument is validated before anything is allocated
            return fail(h, OKENV_ERR_INVALID, "okenv_nearest_track_idx: qy is NULL");
        if (agents)
            n = h->shape.N;
        if (n <= 0)
            return OKENV_OK;
        void     *sp  = nullptr; // [ out: n x i32 | queries: 2n x f32 ]
        const int src = deviceScratch(h, 12U * static_cast<size_t>(n), &sp);
        if (src != OKENV_OK)
            return src;
        int32_t     *dout = static_cast<int32_t *>(sp);
        float       *dq   = reinterpret_cast<float *>(dout + n);
        const float *dqx = h->st.pos_x, *dqy = h->st.pos_y;
        if (!agents)
        {
            OK_HIP(h, hipMemcpyAsync(dq, qx, 4U * n, hipMemcpyDefault, h->stream));
            OK_HIP(h, hipMemcpyAsync(dq + n, qy, 4U * n, hipMemcpyDefault, h->stream));
            dqx = dq;
            dqy = dq + n;
        }
        hipLaunchKernelGGL(okNearestIdxKernel, dim3((n * kNearestLanes + 255) / 256), dim3(256), 0, h->stream, h->d_cx, h->d_cy, h->P, dqx, dqy, n,
                           dout);
        OK_HIP(h, hipGetLastError());
        OK_HIP(h, hipMemcpyAsync(out, dout, 4U * n, hipMemcpyDefault, h->stream));
        OK_HIP(h, hipStreamSynchronize(h->stream));
        return OKENV_OK;
    }

    // ---- rollout bookkeeping ---------------------------------------------------------------------------------------

    int okenv_tracker_create(okenv_t h, int32_t reward_kind)
    {
        OK_QUIESCE(h);
        if (!h || (reward_kind != OKENV_REWARD_STEP && reward_kind != OKENV_REWARD_PROGRESS))
            return fail(h, OKENV_ERR_INVALID, "okenv_tracker_create: unknown reward kind");
        if (h->P <= 0)
            return fail(h, OKENV_ERR_STATE, "okenv_tracker_create: call okenv_set_centerline first");
        OK_HIP(h, hipSetDevice(h->device));
        {
            const size_t N = static_cast<size_t>(h->shape.N);
            int          rc;
            if ((rc = devEnsure(h, &h->tracker.prev_idx, N)) || (rc = devEnsure(h, &h->tracker.fitness, N)) ||
                (rc = devEnsure(h, &h->tracker.reward, N)) || (rc = devEnsure(h, &h->tracker.ep_steps, N)) ||
                (rc = devEnsure(h, &h->tracker.ep_return, N)) || (rc = devEnsure(h, &h->tracker.prev_crashed, N)))
                return rc;
        }
        h->tracker_kind = reward_kind;
        return OKENV_OK;
    }

    static int launchTracker(okenv_t h, const int begin, const char *who)
    {
        if (!h)
            return OKENV_ERR_INVALID;
        if (h->tracker_kind < 0)
            return fail(h, OKENV_ERR_STATE, std::string(who) + ": call okenv_tracker_create first");
        OK_HIP(h, hipSetDevice(h->device));
        const long threads = static_cast<long>(h->shape.N) * (h->tracker_kind == kRewardProgress ? kNearestLanes : 1);
        hipLaunchKernelGGL(okTrackerKernel, dim3(static_cast<unsigned>((threads + 255) / 256)), dim3(256), 0, h->stream, h->st, h->d_cx, h->d_cy,
                           h->P, h->tracker, h->shape.N, h->tracker_kind, begin);
        OK_HIP(h, hipGetLastError());
        return OKENV_OK;
    }

    // Inside a controller episode the fused rollout carries the bookkeeping in registers and writes it back per launch: a tracker
    // call or new parameters from outside would be double counted, lost or half applied -- refused, loudly.
    static bool ctrlEpisodeRunning(okenv_t h)
    {
        return h != nullptr && h->episode && h->ep_kind == kPolicyCtrl;
    }

    int okenv_tracker_begin(okenv_t h)
    {
        OK_QUIESCE(h);
        if (ctrlEpisodeRunning(h))
            return fail(h, OKENV_ERR_STATE, "okenv_tracker_begin: a controller episode is running (okenv_rollout_controller does the bookkeeping); okenv_episode_end first");
        return launchTracker(h, 1, "okenv_tracker_begin");
    }

    int okenv_tracker_update(okenv_t h)
    {
        OK_QUIESCE(h);
        if (ctrlEpisodeRunning(h))
            return fail(h, OKENV_ERR_STATE, "okenv_tracker_update: a controller episode is running (okenv_rollout_controller does the bookkeeping); okenv_episode_end first");
        return launchTracker(h, 0, "okenv_tracker_update");
    }

    // ---- CMA-ES controller -----------------------------------------------------------------------------------------

    int okenv_controller_create(okenv_t h, int32_t hidden)
    {
        OK_QUIESCE(h);
        if (!h || hidden < 2 || hidden > OK_CTRL_MAX_HIDDEN || (hidden & 1) != 0)
            return fail(h, OKENV_ERR_INVALID, "okenv_controller_create: hidden width must be even and in [2, 64]");
        if (h->shape.R > 64)
            return fail(h, OKENV_ERR_INVALID, "okenv_controller_create: at most 64 rays");
        OK_HIP(h, hipSetDevice(h->device));
        const int np = ok_controller_num_params(h->shape.R, hidden, 2);
        if (!h->d_ctrl_params || np != h->ctrl_num_params)
        {
            const int rc = devAlloc(h, &h->d_ctrl_params, static_cast<size_t>(h->shape.N) * np);
            if (rc != OKENV_OK)
                return rc;
        }
        h->ctrl_hidden     = hidden;
        h->ctrl_num_params = np;
        return OKENV_OK;
    }

    int okenv_controller_num_params(okenv_t h, int32_t *out)
    {
        OK_QUIESCE(h);
        if (!h || !out || !h->d_ctrl_params)
            return fail(h, OKENV_ERR_STATE, "okenv_controller_num_params: call okenv_controller_create first");
        *out = h->ctrl_num_params;
        return OKENV_OK;
    }

    int okenv_controller_set_params(okenv_t h, const float *params)
    {
        OK_QUIESCE(h);
        if (!h || !params || !h->d_ctrl_params)
            return fail(h, OKENV_ERR_STATE, "okenv_controller_set_params: call okenv_controller_create first");
        if (ctrlEpisodeRunning(h))
            return fail(h, OKENV_ERR_STATE, "okenv_controller_set_params: a controller episode is running; okenv_episode_end first");
        OK_HIP(h, hipSetDevice(h->device));
        return copyAny(h, h->d_ctrl_params, params, sizeof(float) * static_cast<size_t>(h->shape.N) * h->ctrl_num_params);
    }

    int okenv_controller_act(okenv_t h, float throttle, float steering_scale)
    {
        OK_QUIESCE(h);
        if (h)
            dropEpisode(h);
        if (!h || !h->d_ctrl_params)
            return fail(h, OKENV_ERR_STATE, "okenv_controller_act: call okenv_controller_create first");
        OK_HIP(h, hipSetDevice(h->device));
        const int      lanes  = h->ctrl_hidden <= 16 ? 16 : (h->ctrl_hidden <= 32 ? 32 : 64);
        const unsigned blocks = static_cast<unsigned>((static_cast<long>(h->shape.N) * lanes + 255) / 256);
        if (lanes == 16)
            hipLaunchKernelGGL(okControllerKernel<16>, dim3(blocks), dim3(256), 0, h->stream, h->st, h->d_ctrl_params, h->ctrl_num_params, h->shape.N,
                               h->shape.R, h->ctrl_hidden, throttle, steering_scale);
        else if (lanes == 32)
            hipLaunchKernelGGL(okControllerKernel<32>, dim3(blocks), dim3(256), 0, h->stream, h->st, h->d_ctrl_params, h->ctrl_num_params, h->shape.N,
                               h->shape.R, h->ctrl_hidden, throttle, steering_scale);
        else
            hipLaunchKernelGGL(okControllerKernel<64>, dim3(blocks), dim3(256), 0, h->stream, h->st, h->d_ctrl_params, h->ctrl_num_params, h->shape.N,
                               h->shape.R, h->ctrl_hidden, throttle, steering_scale);
        OK_HIP(h, hipGetLastError());
        return OKENV_OK;
    }

    // ---- expert drivers (FieldNavigators/) ---------------------------------------------------------------------------------

    int okenv_expert_create(okenv_t h, const okenv_expert_params *params)
    {
        OK_QUIESCE(h);
        if (!h)
            return fail(h, OKENV_ERR_INVALID, "okenv_expert_create: NULL handle");
        if (const char *why = okExpertCheckParams(params, h->shape.R))
            return fail(h, OKENV_ERR_INVALID, std::string("okenv_expert_create: ") + why);
        if (h->P <= 0)
            return fail(h, OKENV_ERR_STATE, "okenv_expert_create: call okenv_set_centerline first");
        OK_HIP(h, hipSetDevice(h->device));
        int rc = devEnsure(h, &h->d_expert_tab, 2U * static_cast<size_t>(h->shape.R));
        if (rc != OKENV_OK || (rc = buildCenterlineBuckets(h)) != OKENV_OK)
            return rc;
        std::vector<double> c, s;
        okExpertRayTables(h->host_ray_deg.data(), h->shape.R, c, s);
        OK_HIP(h, hipMemcpyAsync(h->d_expert_tab, c.data(), 8U * static_cast<size_t>(h->shape.R), hipMemcpyHostToDevice, h->stream));
        OK_HIP(h, hipMemcpyAsync(h->d_expert_tab + h->shape.R, s.data(), 8U * static_cast<size_t>(h->shape.R), hipMemcpyHostToDevice, h->stream));
        OK_HIP(h, hipStreamSynchronize(h->stream)); // the tables are locals
        h->expert    = *params;
        h->expert_ok = true;
        return OKENV_OK;
    }

    int okenv_expert_act(okenv_t h, const okenv_expert_record *rec)
    {
        OK_QUIESCE(h);
        if (!h)
            return fail(h, OKENV_ERR_INVALID, "okenv_expert_act: NULL handle");
        if (!h->expert_ok)
            return fail(h, OKENV_ERR_STATE, "okenv_expert_act: call okenv_expert_create first");
        if (h->P <= 0)
            return fail(h, OKENV_ERR_STATE, "okenv_expert_act: call okenv_set_centerline first");
        dropEpisode(h);
        OK_HIP(h, hipSetDevice(h->device));
        OkExpertParams p{};
        p.st       = h->st;
        p.N        = h->shape.N;
        p.R        = h->shape.R;
        p.P        = h->P;
        p.cx       = h->d_cx;
        p.cy       = h->d_cy;
        p.cl_start = h->cl_dirty ? nullptr : h->d_cl_start;
        p.cl_idx   = h->cl_dirty ? nullptr : h->d_cl_idx;
        p.geom     = h->grid.g;
        p.ray_cos  = h->d_expert_tab;
        p.ray_sin  = h->d_expert_tab + h->shape.R;
        p.first    = h->host_ray_deg.front();
        p.last     = h->host_ray_deg.back();
        p.ep       = h->expert;
        if (rec != nullptr)
            p.rec = *rec;
        const unsigned blocks = static_cast<unsigned>((static_cast<long>(h->shape.N) * kExpertLanes + 255) / 256);
        hipLaunchKernelGGL(okExpertKernel, dim3(blocks), dim3(256), 0, h->stream, p);
        OK_HIP(h, hipGetLastError());
        return OKENV_OK;
    }

    int okenv_expert_act_host(const okenv_expert_params *params, const float *ray_angles_deg, int32_t num_rays, const float *cx, const float *cy,
                              int32_t num_points, int32_t n, const float *pos_x, const float *pos_y, const float *rot_deg, const float *dist,
                              const float *goal_x, const float *goal_y, float *throttle, float *steer)
    {
        if (!ray_angles_deg || num_rays <= 0 || n < 0 || !pos_x || !pos_y || !rot_deg || !dist || !throttle || !steer)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_expert_act_host: bad argument");
        if (const char *why = okExpertCheckParams(params, num_rays))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_expert_act_host: ") + why);
        const bool given = goal_x != nullptr || goal_y != nullptr;
        if (given ? (!goal_x || !goal_y) : (!cx || !cy || num_points <= 0))
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_expert_act_host: needs a centre line or both goal arrays");
        okExpertActHost(*params, ray_angles_deg, num_rays, cx, cy, num_points, n, pos_x, pos_y, rot_deg, dist, goal_x, goal_y, throttle, steer);
        return OKENV_OK;
    }

    int okenv_debug_atan2f(const float *y, const float *x, float *out, int32_t n)
    {
        if (!y || !x || !out || n < 0)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_debug_atan2f: bad argument");
        for (int32_t i = 0; i < n; ++i)
            out[i] = ok_atan2f(y[i], x[i]);
        return OKENV_OK;
    }

    int okenv_debug_expert_normalize_angle(const float *angle_deg, float *out, int32_t n)
    {
        if (!angle_deg || !out || n < 0)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_debug_expert_normalize_angle: bad argument");
        for (int32_t i = 0; i < n; ++i)
            out[i] = ok_expert_normalize_angle_deg(angle_deg[i]);
        return OKENV_OK;
    }

    // ---- shared-network actors (RLRacers/PPO, Reinforce, Deep_Q_Learning) --------------------------------------------------

    int okenv_actor_create(okenv_t h, const okenv_actor_params *params)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kActorDriver, "create", kGateHandle))
            return rc;
        if (const char *why = okActorCheckParams(params, h->shape.R))
            return driverRefuses(h, OKENV_ERR_INVALID, kActorDriver, "create", why);
        OK_HIP(h, hipSetDevice(h->device));
        // room for the widest networks of this fan, so that a later create with other widths allocates nothing
        const size_t cap = static_cast<size_t>(ok_actor_num_params(h->shape.R, OK_ACTOR_MAX_HIDDEN, OK_ACTOR_MAX_ACTIONS)) + 4U;
        if (const int rc = driverCreateFixed(h, kActorDriver, cap, 1, 1, false, {kernelOf(okActorKernel<false>), kernelOf(okActorKernel<true>)}))
            return rc;
        h->actor          = *params;
        h->actor_dropout  = 0.F;   // (okenv_actor_set_dropout is per actor)
        h->learner_ok     = false; // (Adam's moments belong to the networks that were just replaced)
        h->dqn_target_set = false; // (and so does the target network's copy)
        return OKENV_OK;
    }

    int okenv_actor_num_params(okenv_t h, int32_t *policy, int32_t *value)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kActorDriver, "num_params", kGateCreated))
            return rc;
        if (policy)
            *policy = actorPolicyParams(h);
        if (value)
            *value = actorValueParams(h);
        return OKENV_OK;
    }

    int okenv_actor_set_params(okenv_t h, const float *policy, const float *value)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kActorDriver, "set_params", kGateCreated))
            return rc;
        if (value != nullptr && h->actor.value_hidden == 0)
            return fail(h, OKENV_ERR_INVALID, "okenv_actor_set_params: the actor has no value network");
        return driverSet(h, kActorDriver, {vectorOf(h->actor_drv.d, policy, actorPolicyParams(h), 0), vectorOf(h->actor_drv.d2, value, actorValueParams(h), 1)});
    }

    int okenv_actor_set_epsilon(okenv_t h, float epsilon)
    {
        OK_QUIESCE(h);
        if (!h || !h->actor_drv.ok)
            return fail(h, OKENV_ERR_STATE, "okenv_actor_set_epsilon: call okenv_actor_create first");
        if (!(epsilon >= 0.F && epsilon <= 1.F))
            return fail(h, OKENV_ERR_INVALID, "okenv_actor_set_epsilon: epsilon outside [0, 1]");
        h->actor.epsilon = epsilon;
        return OKENV_OK;
    }

    int okenv_actor_set_draw_offset(okenv_t h, const uint32_t *device_word)
    {
        OK_QUIESCE(h);
        return driverSetDrawOffset(h, kActorDriver, device_word);
    }

    int okenv_actor_act(okenv_t h, const okenv_actor_record *rec)
    {
        OK_QUIESCE(h);
        if (const int rc = actBegin(h, kActorDriver, h != nullptr && h->actor.value_hidden > 0 ? 3U : 1U))
            return rc;
        OkActorParams p{};
        p.f      = actFrame(h);
        p.draw   = actDrawWords(h, h->actor_drv.draw_offset);
        p.policy = h->actor_drv.d;
        p.value  = h->actor_drv.d2;
        p.ap     = h->actor;
        if (rec != nullptr)
            p.rec = *rec;
        if (h->actor_dropout > 0.F)
            p.drop = ok_reinforce_mask{h->actor_dropout, ok_reinforce_scale(h->actor_dropout), h->actor_dropout_seed, 0U, 0U};
        return actLaunch(h, h->actor_dropout > 0.F ? okActorKernel<true> : okActorKernel<false>, kActorAgents, kActorThreads,
                         okActorLdsBytes(h->shape.R, h->actor), p);
    }

    int okenv_actor_act_host(const okenv_actor_params *params, const float *policy, const float *value, int32_t num_rays, int32_t n, const float *dist,
                             const uint8_t *crashed, uint32_t draw_index, float *throttle, float *steer, int64_t *action, float *prob,
                             float *value_out, float *state, uint8_t *alive)
    {
        if (const char *why = okActorCheckParams(params, num_rays))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_actor_act_host: ") + why);
        if (!policy || n < 0 || !dist || (params->value_hidden > 0 && !value))
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_actor_act_host: bad argument");
        okActorActHost(*params, policy, value, num_rays, n, dist, crashed, draw_index, throttle, steer, action, prob, value_out, state, alive);
        return OKENV_OK;
    }

    // ---- from a recorded episode to the learner's batch (ok_batch.h) ---------------------------------------------------------

    int okenv_batch_prepare(okenv_t h, const okenv_batch_params *params, const okenv_batch_input *in, const okenv_batch_output *out)
    {
        OK_QUIESCE(h);
        if (!h)
            return fail(h, OKENV_ERR_INVALID, "okenv_batch_prepare: NULL handle");
        if (const char *why = okBatchCheck(params, in, out))
            return fail(h, OKENV_ERR_INVALID, std::string("okenv_batch_prepare: ") + why);
        OK_HIP(h, hipSetDevice(h->device));
        OkBatchParams p{};
        p.T         = params->num_steps;
        p.N         = params->num_agents;
        p.R         = params->state_width;
        p.W         = (p.N + kBatchWave - 1) / kBatchWave;
        p.rs        = params->record_stride != 0 ? params->record_stride : p.N;
        p.fs        = params->field_stride != 0 ? params->field_stride : p.N;
        p.L         = static_cast<long>(p.T) * p.W;
        p.groups    = (p.L + kBatchGroupChunks - 1) / kBatchGroupChunks;
        p.gamma     = params->gamma;
        p.gl        = static_cast<float>(static_cast<double>(params->gamma) * static_cast<double>(params->lambda));
        p.normalize = params->normalize;
        p.in        = *in;
        p.out       = *out;
        // the scratch: [G plane | A plane | column partials | their counts | group counts | statistics | M], each piece 256-aligned
        const auto   up    = [](const size_t b) { return (b + 255U) & ~static_cast<size_t>(255U); };
        const size_t plane = up(sizeof(float) * static_cast<size_t>(p.T) * static_cast<size_t>(p.N));
        const size_t parts = up(4U * sizeof(double) * static_cast<size_t>(p.N)), part_m = up(sizeof(uint32_t) * static_cast<size_t>(p.N));
        const size_t group = up(sizeof(uint32_t) * static_cast<size_t>(p.groups));
        const size_t bytes = 2U * plane + parts + part_m + group + 256U + 256U;
        if (const int rc = growScratch(h, h->batch_scratch, bytes))
            return rc;
        uint8_t *at = h->batch_scratch.part;
        p.g_plane   = out->ret_plane != nullptr ? out->ret_plane : reinterpret_cast<float *>(at);
        p.a_plane   = out->adv_plane != nullptr ? out->adv_plane : reinterpret_cast<float *>(at + plane);
        at += 2U * plane;
        p.part = reinterpret_cast<double *>(at);
        at += parts;
        p.part_m = reinterpret_cast<uint32_t *>(at);
        at += part_m;
        p.group = reinterpret_cast<uint32_t *>(at);
        at += group;
        p.stats = reinterpret_cast<okenv_batch_stats *>(at);
        at += 256U;
        p.count          = reinterpret_cast<int32_t *>(at);
        h->d_batch_count = p.count;
        const unsigned bt   = static_cast<unsigned>(params->block_threads != 0 ? params->block_threads : kBatchWalkThreads);
        const unsigned wide = static_cast<unsigned>(p.groups);
        if (const int rc = eventsBegin(h, h->batch_scratch.log, 5))
            return rc;
        if (in->value != nullptr)
            hipLaunchKernelGGL(okBatchWalkKernel<true>, dim3((static_cast<unsigned>(p.N) + bt - 1U) / bt), dim3(bt), 0, h->stream, p);
        else
            hipLaunchKernelGGL(okBatchWalkKernel<false>, dim3((static_cast<unsigned>(p.N) + bt - 1U) / bt), dim3(bt), 0, h->stream, p);
        if (const int rc = eventsMark(h, h->batch_scratch.log))
            return rc;
        hipLaunchKernelGGL(okBatchTreeKernel, dim3(1), dim3(1024), 0, h->stream, p);
        if (const int rc = eventsMark(h, h->batch_scratch.log))
            return rc;
        hipLaunchKernelGGL(okBatchCountKernel, dim3(wide), dim3(kBatchWideThreads), 0, h->stream, p);
        if (const int rc = eventsMark(h, h->batch_scratch.log))
            return rc;
        hipLaunchKernelGGL(okBatchScanKernel, dim3(1), dim3(1024), 0, h->stream, p);
        if (const int rc = eventsMark(h, h->batch_scratch.log))
            return rc;
        hipLaunchKernelGGL(okBatchGatherKernel, dim3(wide), dim3(kBatchWideThreads), 0, h->stream, p);
        if (const int rc = eventsMark(h, h->batch_scratch.log))
            return rc;
        OK_HIP(h, hipGetLastError());
        return OKENV_OK;
    }

    int okenv_batch_count(okenv_t h, int32_t *count)
    {
        OK_QUIESCE(h);
        if (!h || !count)
            return fail(h, OKENV_ERR_INVALID, "okenv_batch_count: NULL argument");
        if (h->d_batch_count == nullptr)
            return fail(h, OKENV_ERR_STATE, "okenv_batch_count: call okenv_batch_prepare first");
        OK_HIP(h, hipSetDevice(h->device));
        OK_HIP(h, hipMemcpyAsync(count, h->d_batch_count, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        OK_HIP(h, hipStreamSynchronize(h->stream));
        return OKENV_OK;
    }

    int okenv_debug_batch_timing(okenv_t h, double *ms5)
    {
        OK_QUIESCE(h);
        return updateTiming(h, &okenv::batch_scratch, "okenv_debug_batch_timing", "okenv_batch_prepare", ms5, 5);
    }

    int okenv_batch_prepare_host(const okenv_batch_params *params, const okenv_batch_input *in, const okenv_batch_output *out, int32_t *count)
    {
        if (const char *why = okBatchCheck(params, in, out))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_batch_prepare_host: ") + why);
        const int32_t m = okBatchPrepareHost(*params, *in, *out);
        if (count != nullptr)
            *count = m;
        return OKENV_OK;
    }

    // ---- PPO's update: losses, gradients and Adam (ok_learn.h) --------------------------------------------------------------

    int okenv_learner_create(okenv_t h, const okenv_learner_params *params)
    {
        OK_QUIESCE(h);
        if (!h)
            return fail(h, OKENV_ERR_INVALID, "okenv_learner_create: NULL handle");
        if (const char *why = okLearnCheckParams(params))
            return fail(h, OKENV_ERR_INVALID, std::string("okenv_learner_create: ") + why);
        if (!h->actor_drv.ok || !h->actor_drv.set[0] || (h->actor.value_hidden > 0 && !h->actor_drv.set[1]))
            return fail(h, OKENV_ERR_STATE, "okenv_learner_create: needs an actor whose networks have their parameters (okenv_actor_create, okenv_actor_set_params)");
        OK_HIP(h, hipSetDevice(h->device));
        h->learn_cap = static_cast<size_t>(ok_actor_num_params(h->shape.R, OK_ACTOR_MAX_HIDDEN, OK_ACTOR_MAX_ACTIONS)) + 4U;
        const int rc = devEnsure(h, &h->d_learn_moments, 4U * h->learn_cap);
        if (rc != OKENV_OK)
            return rc;
        if (const int lrc = raiseLdsLimit(h, {kernelOf(okLearnGradKernel), kernelOf(okReinforceGradKernel)}))
            return lrc;
        OK_HIP(h, hipMemsetAsync(h->d_learn_moments, 0, 4U * h->learn_cap * sizeof(float), h->stream));
        h->learner    = *params;
        h->learn_t    = 0;
        h->learner_ok = true;
        return OKENV_OK;
    }

    int okenv_learner_reset(okenv_t h)
    {
        OK_QUIESCE(h);
        if (!h || !h->learner_ok)
            return fail(h, OKENV_ERR_STATE, "okenv_learner_reset: call okenv_learner_create first");
        OK_HIP(h, hipSetDevice(h->device));
        OK_HIP(h, hipMemsetAsync(h->d_learn_moments, 0, 4U * h->learn_cap * sizeof(float), h->stream));
        h->learn_t = 0;
        return OKENV_OK;
    }

    int okenv_ppo_update(okenv_t h, const okenv_ppo_batch *batch, int32_t M, int32_t B, int32_t epochs, const int32_t *order, const okenv_ppo_output *out)
    {
        OK_QUIESCE(h);
        if (!h)
            return fail(h, OKENV_ERR_INVALID, "okenv_ppo_update: NULL handle");
        if (!h->learner_ok || !h->actor_drv.ok)
            return fail(h, OKENV_ERR_STATE, "okenv_ppo_update: call okenv_learner_create first");
        if (h->actor_dropout > 0.F)
            return fail(h, OKENV_ERR_STATE, "okenv_ppo_update: the actor's dropout is on (okenv_actor_set_dropout) and this update's forward knows no mask");
        if (const char *why = okLearnCheckCall(batch, M, B, epochs, h->actor.value_hidden))
            return fail(h, OKENV_ERR_INVALID, std::string("okenv_ppo_update: ") + why);
        OK_HIP(h, hipSetDevice(h->device));
        OkLearnParams p{};
        p.R    = h->shape.R;
        p.H    = h->actor.hidden;
        p.A    = h->actor.num_actions;
        p.Hv   = h->actor.value_hidden;
        p.M    = M;
        p.Pp   = ok_actor_num_params(p.R, p.H, p.A);
        p.Pv   = p.Hv > 0 ? ok_actor_num_params(p.R, p.Hv, 1) : 0;
        p.cols = p.Pp + p.Pv + 2;
        p.in   = *batch;
        p.lo   = okLearnClipLo(h->learner.clip);
        p.hi   = okLearnClipHi(h->learner.clip);
        p.policy = h->actor_drv.d;
        p.value  = h->actor_drv.d2;
        p.pol_m  = h->d_learn_moments;
        p.pol_v  = h->d_learn_moments + h->learn_cap;
        p.val_m  = h->d_learn_moments + 2U * h->learn_cap;
        p.val_v  = h->d_learn_moments + 3U * h->learn_cap;
        const okenv_ppo_output none{};
        const okenv_ppo_output &o = out != nullptr ? *out : none;
        p.grad_policy = o.grad_policy;
        p.grad_value  = o.grad_value;
        // the scratch: [chunk partials | clip counts], each piece 256-aligned
        const auto   up    = [](const size_t b) { return (b + 255U) & ~static_cast<size_t>(255U); };
        const size_t c_max = (static_cast<size_t>(std::min(B, M)) + OK_LEARN_CHUNK - 1U) / OK_LEARN_CHUNK;
        const size_t parts = up(sizeof(float) * c_max * static_cast<size_t>(p.cols)), bytes = parts + up(sizeof(uint32_t) * c_max);
        if (const int rc = growScratch(h, h->learn_scratch, bytes))
            return rc;
        p.part      = reinterpret_cast<float *>(h->learn_scratch.part);
        p.part_clip = reinterpret_cast<uint32_t *>(h->learn_scratch.part + parts);
        const int    per_epoch = okLearnMinibatches(M, B);
        const size_t launches  = 2U * static_cast<size_t>(epochs) * static_cast<size_t>(per_epoch);
        if (const int rc = eventsBegin(h, h->learn_scratch.log, launches))
            return rc;
        const size_t lds = okLearnLdsBytes(p.R, p.H, p.A, p.Hv);
        for (int e = 0; e < epochs; ++e)
            for (int k = 0; k < per_epoch; ++k)
            {
                const size_t slot = static_cast<size_t>(e) * per_epoch + k;
                p.base  = static_cast<long>(k) * B;
                p.Bk    = static_cast<int>(std::min<long>(B, M - p.base));
                p.C     = (p.Bk + OK_LEARN_CHUNK - 1) / OK_LEARN_CHUNK;
                p.order = order != nullptr ? order + static_cast<size_t>(e) * M : nullptr;
                p.adam        = okLearnAdamConsts(h->learner, h->learn_t + 1);
                p.actor_loss  = o.actor_loss != nullptr ? o.actor_loss + slot : nullptr;
                p.critic_loss = o.critic_loss != nullptr ? o.critic_loss + slot : nullptr;
                p.clipped     = o.clipped != nullptr ? o.clipped + slot : nullptr;
                // The step number advances only once both kernels of the minibatch are enqueued: after a failed launch the handle's t
                // is the number of steps the device's moments have taken, and the call reports the error.
                hipLaunchKernelGGL(okLearnGradKernel, dim3(static_cast<unsigned>(p.C)), dim3(kLearnThreads), lds, h->stream, p);
                OK_HIP(h, hipGetLastError());
                if (const int rc = eventsMark(h, h->learn_scratch.log))
                    return rc;
                hipLaunchKernelGGL(okLearnStepKernel, dim3(static_cast<unsigned>((p.cols + kLearnStepCols - 1) / kLearnStepCols)),
                                   dim3(kLearnStepCols * kLearnStepRows), 0, h->stream, p);
                OK_HIP(h, hipGetLastError());
                h->learn_t += 1;
                if (const int rc = eventsMark(h, h->learn_scratch.log))
                    return rc;
            }
        return OKENV_OK;
    }

    int okenv_debug_update_timing(okenv_t h, double *ms2)
    {
        OK_QUIESCE(h);
        return updateTiming(h, &okenv::learn_scratch, "okenv_debug_update_timing", "okenv_ppo_update", ms2, 2);
    }

    int okenv_actor_get_params(okenv_t h, float *policy, float *value)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kActorDriver, "get_params", kGateCreated))
            return rc;
        if ((policy != nullptr && !h->actor_drv.set[0]) || (value != nullptr && !h->actor_drv.set[1]))
            return fail(h, OKENV_ERR_STATE, "okenv_actor_get_params: the network has no parameters yet (okenv_actor_set_params)");
        return driverGet(h, {vectorOf(h->actor_drv.d, policy, actorPolicyParams(h)), vectorOf(h->actor_drv.d2, value, actorValueParams(h))});
    }

    int okenv_learner_get_state(okenv_t h, float *policy_m, float *policy_v, float *value_m, float *value_v, int64_t *t)
    {
        OK_QUIESCE(h);
        if (!h || !h->learner_ok)
            return fail(h, OKENV_ERR_STATE, "okenv_learner_get_state: call okenv_learner_create first");
        OK_HIP(h, hipSetDevice(h->device));
        const size_t np = sizeof(float) * static_cast<size_t>(ok_actor_num_params(h->shape.R, h->actor.hidden, h->actor.num_actions));
        const size_t nv = h->actor.value_hidden > 0 ? sizeof(float) * static_cast<size_t>(ok_actor_num_params(h->shape.R, h->actor.value_hidden, 1)) : 0U;
        float *const dst[4]   = {policy_m, policy_v, value_m, value_v};
        const size_t bytes[4] = {np, np, nv, nv};
        for (int k = 0; k < 4; ++k)
            if (dst[k] != nullptr)
            {
                const int rc = copyAny(h, dst[k], h->d_learn_moments + static_cast<size_t>(k) * h->learn_cap, bytes[k]);
                if (rc != OKENV_OK)
                    return rc;
            }
        OK_HIP(h, hipStreamSynchronize(h->stream));
        if (t != nullptr)
            *t = h->learn_t;
        return OKENV_OK;
    }

    int okenv_ppo_update_host(const okenv_learner_params *params, int32_t num_rays, int32_t hidden, int32_t num_actions, int32_t value_hidden,
                              okenv_learner_state *state, const okenv_ppo_batch *batch, int32_t M, int32_t B, int32_t epochs, const int32_t *order,
                              const okenv_ppo_output *out)
    {
        if (const char *why = okLearnCheckParams(params))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_ppo_update_host: ") + why);
        if (num_rays < 1 || num_rays > OK_ACTOR_MAX_RAYS || hidden < 1 || hidden > OK_ACTOR_MAX_HIDDEN || num_actions < 2 ||
            num_actions > OK_ACTOR_MAX_ACTIONS || value_hidden < 0 || value_hidden > OK_ACTOR_MAX_HIDDEN)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_ppo_update_host: a network width outside the actor's limits");
        if (const char *why = okLearnCheckCall(batch, M, B, epochs, value_hidden))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_ppo_update_host: ") + why);
        if (state == nullptr || state->policy == nullptr || state->policy_m == nullptr || state->policy_v == nullptr || state->t < 0 ||
            (value_hidden > 0 && (state->value == nullptr || state->value_m == nullptr || state->value_v == nullptr)))
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_ppo_update_host: state lacks a parameter or moment vector, or t < 0");
        const okenv_ppo_output none{};
        okLearnUpdateHost(*params, num_rays, hidden, num_actions, value_hidden, *state, *batch, M, B, epochs, order, out != nullptr ? *out : none);
        return OKENV_OK;
    }

    // ---- REINFORCE: the dropout actor and the whole-episode update (ok_reinforce.h) -------------------------------------------

    int okenv_actor_set_dropout(okenv_t h, float p, uint32_t seed)
    {
        OK_QUIESCE(h);
        if (!h)
            return fail(h, OKENV_ERR_INVALID, "okenv_actor_set_dropout: NULL handle");
        if (!h->actor_drv.ok)
            return fail(h, OKENV_ERR_STATE, "okenv_actor_set_dropout: call okenv_actor_create first");
        if (!(p >= 0.F && p < 1.F))
            return fail(h, OKENV_ERR_INVALID, "okenv_actor_set_dropout: p outside [0, 1)");
        h->actor_dropout      = p;
        h->actor_dropout_seed = seed;
        return OKENV_OK;
    }

    int okenv_actor_act_dropout_host(const okenv_actor_params *params, float p, uint32_t dropout_seed, const float *policy, const float *value,
                                     int32_t num_rays, int32_t n, const float *dist, const uint8_t *crashed, uint32_t draw_index, float *throttle,
                                     float *steer, int64_t *action, float *prob, float *value_out, float *state, uint8_t *alive)
    {
        if (const char *why = okActorCheckParams(params, num_rays))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_actor_act_dropout_host: ") + why);
        if (!(p >= 0.F && p < 1.F))
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_actor_act_dropout_host: p outside [0, 1)");
        if (!policy || n < 0 || !dist || (params->value_hidden > 0 && !value))
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_actor_act_dropout_host: bad argument");
        okActorActDropoutHost(*params, p, dropout_seed, policy, value, num_rays, n, dist, crashed, draw_index, throttle, steer, action, prob, value_out,
                              state, alive);
        return OKENV_OK;
    }

    int okenv_reinforce_update(okenv_t h, const okenv_reinforce_config *config, const okenv_reinforce_batch *batch, int32_t M, int32_t B,
                               const int32_t *order, const okenv_reinforce_output *out)
    {
        OK_QUIESCE(h);
        if (!h)
            return fail(h, OKENV_ERR_INVALID, "okenv_reinforce_update: NULL handle");
        if (!h->learner_ok || !h->actor_drv.ok)
            return fail(h, OKENV_ERR_STATE, "okenv_reinforce_update: call okenv_learner_create first");
        if (const char *why = okReinforceCheckCall(config, batch, M, B, h->actor_dropout > 0.F))
            return fail(h, OKENV_ERR_INVALID, std::string("okenv_reinforce_update: ") + why);
        OK_HIP(h, hipSetDevice(h->device));
        OkReinforceParams p{};
        p.R          = h->shape.R;
        p.H          = h->actor.hidden;
        p.A          = h->actor.num_actions;
        p.M          = M;
        p.Pp         = ok_actor_num_params(p.R, p.H, p.A);
        p.cols       = p.Pp + 1;
        p.in         = *batch;
        p.drop       = ok_reinforce_mask{h->actor_dropout, ok_reinforce_scale(h->actor_dropout), h->actor_dropout_seed, 0U, 0U};
        p.agent_base = h->actor.agent_base;
        p.draw_first = config->draw_first;
        p.N          = config->num_agents;
        p.order      = order;
        p.policy     = h->actor_drv.d;
        const okenv_reinforce_output none{};
        const okenv_reinforce_output &o = out != nullptr ? *out : none;
        const OkJoinParams j   = okJoinOn(p.Pp, h->actor_drv.d, h->d_learn_moments, h->d_learn_moments + h->learn_cap, config->reduce, o.grad_policy);
        const size_t       lds = okReinforceLdsBytes(p.R, p.H, p.A);
        return sliceUpdate(h, h->reinforce_scratch, M, B, config->accumulate != 0, j, h->learn_t, h->learner, o.loss,
                           [&](const long base, const int Bk, const int C)
                           {
                               p.base = base;
                               p.Bk   = Bk;
                               p.part = reinterpret_cast<float *>(h->reinforce_scratch.part);
                               hipLaunchKernelGGL(okReinforceGradKernel, dim3(static_cast<unsigned>(C)), dim3(kLearnThreads), lds, h->stream, p);
                           });
    }

    int okenv_debug_reinforce_timing(okenv_t h, double *ms2)
    {
        OK_QUIESCE(h);
        return updateTiming(h, &okenv::reinforce_scratch, "okenv_debug_reinforce_timing", "okenv_reinforce_update", ms2, 2);
    }

    int okenv_reinforce_update_host(const okenv_learner_params *params, const okenv_reinforce_config *config, float p, uint32_t dropout_seed,
                                    uint32_t agent_base, int32_t num_rays, int32_t hidden, int32_t num_actions, okenv_learner_state *state,
                                    const okenv_reinforce_batch *batch, int32_t M, int32_t B, const int32_t *order, const okenv_reinforce_output *out)
    {
        if (const char *why = okLearnCheckParams(params))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_reinforce_update_host: ") + why);
        if (num_rays < 1 || num_rays > OK_ACTOR_MAX_RAYS || hidden < 1 || hidden > OK_ACTOR_MAX_HIDDEN || num_actions < 2 ||
            num_actions > OK_ACTOR_MAX_ACTIONS)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_reinforce_update_host: a network width outside the actor's limits");
        if (!(p >= 0.F && p < 1.F))
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_reinforce_update_host: p outside [0, 1)");
        if (const char *why = okReinforceCheckCall(config, batch, M, B, p > 0.F))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_reinforce_update_host: ") + why);
        if (state == nullptr || state->policy == nullptr || state->policy_m == nullptr || state->policy_v == nullptr || state->t < 0)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_reinforce_update_host: state lacks a parameter or moment vector, or t < 0");
        const okenv_reinforce_output none{};
        okReinforceUpdateHost(*params, *config, p, dropout_seed, agent_base, num_rays, hidden, num_actions, *state, *batch, M, B, order,
                              out != nullptr ? *out : none);
        return OKENV_OK;
    }

    int okenv_debug_logf(const float *x, float *out, int32_t n)
    {
        if (!x || !out || n < 0)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_debug_logf: bad argument");
        for (int32_t i = 0; i < n; ++i)
            out[i] = ok_logf(x[i]);
        return OKENV_OK;
    }

    int okenv_debug_reinforce_mask(float p, uint32_t seed, uint32_t agent, uint32_t draw, int32_t hidden, uint8_t *out)
    {
        if (!(p >= 0.F && p < 1.F) || hidden < 0 || !out)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_debug_reinforce_mask: bad argument");
        const ok_reinforce_mask m{p, ok_reinforce_scale(p), seed, agent, draw};
        for (int32_t j = 0; j < hidden; ++j)
            out[j] = ok_reinforce_kept(m, j) ? 1 : 0;
        return OKENV_OK;
    }

    // ---- Deep-Q learning: replay ring, sampling and the TD update (ok_dqn.h) ------------------------------------------------

    int okenv_replay_create(okenv_t h, int32_t capacity, uint32_t flags)
    {
        OK_QUIESCE(h);
        return ringCreate(h, kDqnRing, capacity, flags, reinterpret_cast<const void *>(&okDqnGradKernel));
    }

    int okenv_replay_reset(okenv_t h)
    {
        OK_QUIESCE(h);
        return ringReset(h, kDqnRing);
    }

    int okenv_replay_push(okenv_t h, const okenv_actor_record *rec, const float *reward)
    {
        OK_QUIESCE(h);
        return ringPush<OkReplayParams>(h, kDqnRing, rec, reward);
    }

    int okenv_replay_size(okenv_t h, int64_t *size, int64_t *pushed)
    {
        OK_QUIESCE(h);
        return ringSize(h, kDqnRing, size, pushed);
    }

    int okenv_replay_get(okenv_t h, const okenv_replay_ring *out)
    {
        OK_QUIESCE(h);
        return ringGet(h, kDqnRing, out);
    }

    int okenv_dqn_sync_target(okenv_t h)
    {
        OK_QUIESCE(h);
        if (!h)
            return fail(h, OKENV_ERR_INVALID, "okenv_dqn_sync_target: NULL handle");
        if (h->dqn.target_network == 0 || h->d_dqn_target == nullptr)
            return fail(h, OKENV_ERR_STATE, "okenv_dqn_sync_target: okenv_dqn_params has not turned the target network on");
        if (!h->actor_drv.ok || !h->actor_drv.set[0])
            return fail(h, OKENV_ERR_STATE, "okenv_dqn_sync_target: the actor has no parameters yet (okenv_actor_create, okenv_actor_set_params)");
        OK_HIP(h, hipSetDevice(h->device));
        // (whole float4s: the kernels stage a network in 16-byte loads, and the actor's vector is padded the same way)
        const size_t n = (static_cast<size_t>(ok_actor_num_params(h->shape.R, h->actor.hidden, h->actor.num_actions)) + 3U) & ~static_cast<size_t>(3U);
        OK_HIP(h, hipMemcpyAsync(h->d_dqn_target, h->actor_drv.d, n * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        h->dqn_target_set = true;
        return OKENV_OK;
    }

    int okenv_dqn_params(okenv_t h, const okenv_dqn_config *config)
    {
        OK_QUIESCE(h);
        if (!h)
            return fail(h, OKENV_ERR_INVALID, "okenv_dqn_params: NULL handle");
        if (const char *why = okDqnCheckConfig(config))
            return fail(h, OKENV_ERR_INVALID, std::string("okenv_dqn_params: ") + why);
        if (config->target_network == 0)
        {
            h->dqn = *config;
            return OKENV_OK;
        }
        OK_HIP(h, hipSetDevice(h->device));
        const int rc = devEnsure(h, &h->d_dqn_target, static_cast<size_t>(ok_actor_num_params(OK_ACTOR_MAX_RAYS, OK_ACTOR_MAX_HIDDEN, OK_ACTOR_MAX_ACTIONS)) + 4U);
        if (rc != OKENV_OK)
            return rc;
        const bool turned_on = h->dqn.target_network == 0;
        h->dqn               = *config;
        if (turned_on)
        { // (an earlier copy is stale: the switch going on is a sync, or the wait for one)
            h->dqn_target_set = false;
            if (h->actor_drv.ok && h->actor_drv.set[0])
                return okenv_dqn_sync_target(h);
        }
        return OKENV_OK;
    }

    int okenv_dqn_update(okenv_t h, int32_t B, int32_t iterations, int32_t resample, uint32_t draw_base, const okenv_dqn_output *out)
    {
        OK_QUIESCE(h);
        if (!h)
            return fail(h, OKENV_ERR_INVALID, "okenv_dqn_update: NULL handle");
        if (!h->learner_ok || !h->actor_drv.ok)
            return fail(h, OKENV_ERR_STATE, "okenv_dqn_update: call okenv_learner_create first");
        if (h->actor_dropout > 0.F)
            return fail(h, OKENV_ERR_STATE, "okenv_dqn_update: the actor's dropout is on (okenv_actor_set_dropout) and this update's forward knows no mask");
        if (!h->replay.ok)
            return fail(h, OKENV_ERR_STATE, "okenv_dqn_update: call okenv_replay_create first");
        if (h->dqn.target_network != 0 && !h->dqn_target_set)
            return fail(h, OKENV_ERR_STATE, "okenv_dqn_update: the target network was never filled (okenv_dqn_sync_target)");
        if (const char *why = okDqnCheckCall(B, iterations, h->actor.num_actions))
            return fail(h, OKENV_ERR_INVALID, std::string("okenv_dqn_update: ") + why);
        OK_HIP(h, hipSetDevice(h->device));
        OkDqnParams p{};
        p.R        = h->shape.R;
        p.H        = h->actor.hidden;
        p.A        = h->actor.num_actions;
        p.B        = B;
        p.C        = (B + OK_LEARN_CHUNK - 1) / OK_LEARN_CHUNK;
        p.Pp       = ok_actor_num_params(p.R, p.H, p.A);
        p.cols     = p.Pp + 1;
        p.capacity = static_cast<uint64_t>(h->replay.capacity);
        p.pushed   = h->replay.d_words;
        p.ring     = ringFields<okenv_replay_ring>(h->replay);
        p.policy   = h->actor_drv.d;
        p.pol_m    = h->d_learn_moments;
        p.pol_v    = h->d_learn_moments + h->learn_cap;
        p.target   = h->dqn.target_network != 0 ? h->d_dqn_target : h->actor_drv.d;
        p.gamma    = h->dqn.gamma;
        p.flags    = h->dqn.flags;
        p.seed     = h->dqn.seed;
        const okenv_dqn_output none{};
        const okenv_dqn_output &o = out != nullptr ? *out : none;
        p.grad_policy = o.grad_policy;
        p.index       = o.index;
        const size_t bytes = sizeof(float) * static_cast<size_t>(p.C) * static_cast<size_t>(p.cols);
        if (const int rc = growScratch(h, h->dqn_scratch, bytes))
            return rc;
        p.part = reinterpret_cast<float *>(h->dqn_scratch.part);
        const size_t launches = 2U * static_cast<size_t>(iterations);
        if (const int rc = eventsBegin(h, h->dqn_scratch.log, launches))
            return rc;
        const size_t lds = okDqnLdsBytes(p.R, p.H, p.A);
        for (int it = 0; it < iterations; ++it)
        {
            p.draw = draw_base + (resample != 0 ? static_cast<uint32_t>(it) : 0U);
            p.adam = okLearnAdamConsts(h->learner, h->learn_t + 1);
            p.loss = o.loss != nullptr ? o.loss + it : nullptr;
            // (the step number advances once both kernels of the iteration are enqueued, as in okenv_ppo_update)
            hipLaunchKernelGGL(okDqnGradKernel, dim3(static_cast<unsigned>(p.C)), dim3(kLearnThreads), lds, h->stream, p);
            OK_HIP(h, hipGetLastError());
            if (const int rc = eventsMark(h, h->dqn_scratch.log))
                return rc;
            hipLaunchKernelGGL(okDqnStepKernel, dim3(static_cast<unsigned>((p.cols + kLearnStepCols - 1) / kLearnStepCols)),
                               dim3(kLearnStepCols * kLearnStepRows), 0, h->stream, p);
            OK_HIP(h, hipGetLastError());
            h->learn_t += 1;
            if (const int rc = eventsMark(h, h->dqn_scratch.log))
                return rc;
        }
        return OKENV_OK;
    }

    int okenv_debug_dqn_timing(okenv_t h, double *ms2)
    {
        OK_QUIESCE(h);
        return updateTiming(h, &okenv::dqn_scratch, "okenv_debug_dqn_timing", "okenv_dqn_update", ms2, 2);
    }

    int okenv_replay_push_host(const okenv_replay_ring *ring, int32_t capacity, int32_t num_rays, uint64_t *pushed, uint32_t flags, int32_t n,
                               const float *state, const int64_t *action, const uint8_t *alive, const float *dist, const uint8_t *crashed,
                               const float *reward)
    {
        if (const char *why = okReplayCheckCreate(capacity, flags))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_replay_push_host: ") + why);
        if (!okReplayRingComplete(ring) || !pushed)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_replay_push_host: the ring needs every field and its counter");
        if (num_rays < 1 || num_rays > OK_ACTOR_MAX_RAYS || n < 0)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_replay_push_host: the fan needs 1 .. 64 rays and n >= 0");
        if (!state || !action)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_replay_push_host: the record needs state and action");
        if (!alive && (flags & OKENV_REPLAY_PUSH_ALL) == 0U)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_replay_push_host: the record needs alive (or pass OKENV_REPLAY_PUSH_ALL)");
        if (!dist || !crashed)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_replay_push_host: dist and crashed are required");
        okReplayPushHost(*ring, static_cast<uint64_t>(capacity), num_rays, pushed, flags, n, state, action, alive, dist, crashed, reward);
        return OKENV_OK;
    }

    int okenv_dqn_update_host(const okenv_learner_params *params, const okenv_dqn_config *config, int32_t num_rays, int32_t hidden, int32_t num_actions,
                              okenv_learner_state *state, const float *target, const okenv_replay_ring *ring, int64_t size, int32_t B,
                              int32_t iterations, int32_t resample, uint32_t draw_base, const okenv_dqn_output *out)
    {
        if (const char *why = okLearnCheckParams(params))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_dqn_update_host: ") + why);
        if (const char *why = okDqnCheckConfig(config))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_dqn_update_host: ") + why);
        if (num_rays < 1 || num_rays > OK_ACTOR_MAX_RAYS || hidden < 1 || hidden > OK_ACTOR_MAX_HIDDEN || num_actions < 2 || num_actions > OK_ACTOR_MAX_ACTIONS)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_dqn_update_host: a network width outside the actor's limits");
        if (const char *why = okDqnCheckCall(B, iterations, num_actions))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_dqn_update_host: ") + why);
        if (state == nullptr || state->policy == nullptr || state->policy_m == nullptr || state->policy_v == nullptr || state->t < 0)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_dqn_update_host: state lacks a parameter or moment vector, or t < 0");
        if ((config->target_network != 0) != (target != nullptr))
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_dqn_update_host: target is required exactly when the target network is on");
        if (size < 0 || size >= (INT64_C(1) << 31) || (size > 0 && !okReplayRingComplete(ring)))
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_dqn_update_host: size outside 0 .. 2^31 - 1, or a ring without every field");
        const okenv_dqn_output  none{};
        const okenv_replay_ring empty{};
        okDqnUpdateHost(*params, *config, num_rays, hidden, num_actions, *state, target, ring != nullptr ? *ring : empty, static_cast<uint32_t>(size), B,
                        iterations, resample != 0, draw_base, out != nullptr ? *out : none);
        return OKENV_OK;
    }

    // ---- Continuous REINFORCE: two-hidden-layer Gaussian actor and whole-episode update (ok_gauss.h) ---------------------------

    int64_t okenv_gauss_lds_bytes(int32_t num_rays, int32_t hidden1, int32_t hidden2, int32_t num_actions)
    {
        return static_cast<int64_t>(okGaussLdsBytes(num_rays, hidden1, hidden2, num_actions));
    }

    int okenv_gauss_create(okenv_t h, const okenv_gauss_config *config)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kGaussDriver, "create", kGateHandle))
            return rc;
        if (const char *why = okGaussCheckConfig(config, h->shape.R))
            return driverRefuses(h, OKENV_ERR_INVALID, kGaussDriver, "create", why);
        OK_HIP(h, hipSetDevice(h->device));
        // room for the widest network, so that a later create with other widths allocates nothing: [params | m | v]
        const size_t cap = (static_cast<size_t>(ok_gauss_num_params(OK_ACTOR_MAX_RAYS, OK_GAUSS_MAX_HIDDEN, OK_GAUSS_MAX_HIDDEN, 2)) + 3U) & ~static_cast<size_t>(3U);
        if (const int rc = driverCreateFixed(h, kGaussDriver, cap, 3, 0, true, {kernelOf(okGaussActKernel), kernelOf(okGaussGradKernel)}))
            return rc;
        h->gauss            = *config;
        h->gauss_t          = 0;
        h->gauss_learner_ok = false;
        return OKENV_OK;
    }

    int okenv_gauss_num_params(okenv_t h, int32_t *num_params)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kGaussDriver, "num_params", kGateCreated))
            return rc;
        if (num_params)
            *num_params = gaussNumParams(h);
        return OKENV_OK;
    }

    int okenv_gauss_set_params(okenv_t h, const float *params)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kGaussDriver, "set_params", kGateCreated | kGateArgLast, params != nullptr))
            return rc;
        return driverSet(h, kGaussDriver, {vectorOf(h->gauss_drv.d, params, gaussNumParams(h))});
    }

    int okenv_gauss_get_state(okenv_t h, okenv_gauss_state *out)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kGaussDriver, "get_state", kGateArgFirst | kGateStored, out != nullptr, 1U))
            return rc;
        const OkDriver &d = h->gauss_drv;
        const int       n = gaussNumParams(h);
        if (const int rc = driverGet(h, {vectorOf(d.d, out->params, n), vectorOf(d.d + d.cap, out->m, n), vectorOf(d.d + 2U * d.cap, out->v, n)}))
            return rc;
        out->t = h->gauss_t;
        return OKENV_OK;
    }

    int okenv_gauss_get_params(okenv_t h, float *params)
    {
        OK_QUIESCE(h);
        if (!params)
            return fail(h, OKENV_ERR_INVALID, "okenv_gauss_get_params: NULL argument");
        okenv_gauss_state st{params, nullptr, nullptr, 0};
        return okenv_gauss_get_state(h, &st);
    }

    int okenv_gauss_set_draw_offset(okenv_t h, const uint32_t *device_word)
    {
        OK_QUIESCE(h);
        return driverSetDrawOffset(h, kGaussDriver, device_word);
    }

    int okenv_gauss_set_greedy(okenv_t h, int32_t greedy)
    {
        OK_QUIESCE(h);
        return driverSetGreedy(h, kGaussDriver, &okenv::gauss, greedy);
    }

    int okenv_gauss_act(okenv_t h, const okenv_gauss_record *rec)
    {
        OK_QUIESCE(h);
        if (const int rc = actBegin(h, kGaussDriver, 1U))
            return rc;
        OkGaussActParams p{};
        p.f      = actFrame(h);
        p.draw   = actDrawWords(h, h->gauss_drv.draw_offset);
        p.H1     = h->gauss.hidden1;
        p.H2     = h->gauss.hidden2;
        p.params = h->gauss_drv.d;
        for (int k = 0; k < 2; ++k)
        {
            p.scale[k] = h->gauss.scale[k];
            p.bias[k]  = h->gauss.bias[k];
        }
        p.greedy     = h->gauss.greedy;
        p.seed       = h->gauss.seed;
        p.agent_base = h->gauss.agent_base;
        if (rec != nullptr)
            p.rec = *rec;
        return actLaunch(h, okGaussActKernel, kActorAgents, kActorThreads, okGaussActLdsBytes(p.f.R, p.H1, p.H2), p);
    }

    int okenv_gauss_learner_create(okenv_t h, const okenv_learner_params *params)
    {
        OK_QUIESCE(h);
        if (!h)
            return fail(h, OKENV_ERR_INVALID, "okenv_gauss_learner_create: NULL handle");
        if (const char *why = okLearnCheckParams(params))
            return fail(h, OKENV_ERR_INVALID, std::string("okenv_gauss_learner_create: ") + why);
        if (!h->gauss_drv.ok || !h->gauss_drv.set[0])
            return fail(h, OKENV_ERR_STATE, "okenv_gauss_learner_create: needs a Gaussian actor with its parameters (okenv_gauss_create, okenv_gauss_set_params)");
        OK_HIP(h, hipSetDevice(h->device));
        OK_HIP(h, hipMemsetAsync(h->gauss_drv.d + h->gauss_drv.cap, 0, 2U * h->gauss_drv.cap * sizeof(float), h->stream));
        h->gauss_learner    = *params;
        h->gauss_t          = 0;
        h->gauss_learner_ok = true;
        return OKENV_OK;
    }

    int okenv_gauss_update(okenv_t h, const okenv_gauss_update_config *config, const okenv_gauss_batch *batch, int32_t M, int32_t B, const int32_t *order,
                           const okenv_gauss_output *out)
    {
        OK_QUIESCE(h);
        if (!h)
            return fail(h, OKENV_ERR_INVALID, "okenv_gauss_update: NULL handle");
        if (!h->gauss_drv.ok || !h->gauss_learner_ok)
            return fail(h, OKENV_ERR_STATE, "okenv_gauss_update: call okenv_gauss_learner_create first");
        if (const char *why = okGaussCheckCall(config, batch, M, B))
            return fail(h, OKENV_ERR_INVALID, std::string("okenv_gauss_update: ") + why);
        OK_HIP(h, hipSetDevice(h->device));
        OkGaussParams p{};
        p.R      = h->shape.R;
        p.H1     = h->gauss.hidden1;
        p.H2     = h->gauss.hidden2;
        p.A      = 2;
        p.M      = M;
        p.P      = ok_gauss_num_params(p.R, p.H1, p.H2, p.A);
        p.cols   = p.P + 1;
        p.in     = *batch;
        p.mode   = config->grad_mode;
        p.order  = order;
        p.params = h->gauss_drv.d;
        // the join kernels are section 19's, on this parameter vector
        const okenv_gauss_output none{};
        const okenv_gauss_output &o = out != nullptr ? *out : none;
        const OkJoinParams j   = okJoinOn(p.P, h->gauss_drv.d, h->gauss_drv.d + h->gauss_drv.cap, h->gauss_drv.d + 2U * h->gauss_drv.cap, config->reduce, o.grad);
        const size_t       lds = okGaussLdsBytes(p.R, p.H1, p.H2, p.A);
        return sliceUpdate(h, h->gauss_scratch, M, B, config->accumulate != 0, j, h->gauss_t, h->gauss_learner, o.loss,
                           [&](const long base, const int Bk, const int C)
                           {
                               p.base = base;
                               p.Bk   = Bk;
                               p.part = reinterpret_cast<float *>(h->gauss_scratch.part);
                               hipLaunchKernelGGL(okGaussGradKernel, dim3(static_cast<unsigned>(C)), dim3(kLearnThreads), lds, h->stream, p);
                           });
    }

    int okenv_debug_gauss_timing(okenv_t h, double *ms2)
    {
        OK_QUIESCE(h);
        return updateTiming(h, &okenv::gauss_scratch, "okenv_debug_gauss_timing", "okenv_gauss_update", ms2, 2);
    }

    int okenv_gauss_act_host(const okenv_gauss_config *config, const float *params, int32_t num_rays, int32_t n, const float *dist, const uint8_t *crashed,
                             uint32_t draw_index, float *throttle, float *steer, float *eps, float *pre, float *action, float *logp, float *state,
                             uint8_t *alive)
    {
        if (const char *why = okGaussCheckConfig(config, num_rays))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_gauss_act_host: ") + why);
        if (!params || n < 0 || !dist)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_gauss_act_host: bad argument");
        okGaussActHost(*config, params, num_rays, n, dist, crashed, draw_index, throttle, steer, eps, pre, action, logp, state, alive);
        return OKENV_OK;
    }

    int okenv_gauss_update_host(const okenv_learner_params *params, const okenv_gauss_update_config *config, int32_t num_rays, int32_t hidden1,
                                int32_t hidden2, int32_t num_actions, okenv_gauss_state *state, const okenv_gauss_batch *batch, int32_t M, int32_t B,
                                const int32_t *order, const okenv_gauss_output *out)
    {
        if (const char *why = okLearnCheckParams(params))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_gauss_update_host: ") + why);
        if (const char *why = okGaussCheckShape(num_rays, hidden1, hidden2, num_actions))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_gauss_update_host: ") + why);
        if (const char *why = okGaussCheckCall(config, batch, M, B))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_gauss_update_host: ") + why);
        if (state == nullptr || state->params == nullptr || state->m == nullptr || state->v == nullptr || state->t < 0)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_gauss_update_host: state lacks a parameter or moment vector, or t < 0");
        const okenv_gauss_output none{};
        okGaussUpdateHost(*params, *config, num_rays, hidden1, hidden2, num_actions, *state, *batch, M, B, order, out != nullptr ? *out : none);
        return OKENV_OK;
    }

    int okenv_debug_normal(int32_t device, const uint32_t *w0, const uint32_t *w1, float *out0, float *out1, int32_t n)
    {
        if (!w0 || !w1 || !out0 || !out1 || n < 0)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_debug_normal: bad argument");
        const size_t count = static_cast<size_t>(n);
        if (device == OKENV_DEBUG_ON_HOST)
        {
            for (size_t i = 0; i < count; ++i)
                ok_gauss_normal_pair(w0[i], w1[i], out0 + i, out1 + i);
            return OKENV_OK;
        }
        if (const int rc = debugNeedsDevice("okenv_debug_normal"))
            return rc;
        if (n == 0)
            return OKENV_OK;
        OK_HIP(nullptr, hipSetDevice(device));
        // four arrays of n words: w0, w1, out0, out1
        DebugBuffer buf;
        OK_HIP(nullptr, hipMalloc(reinterpret_cast<void **>(&buf.d), 16U * count));
        uint32_t *d0 = reinterpret_cast<uint32_t *>(buf.d), *d1 = d0 + count;
        float    *o0 = buf.d + 2U * count, *o1 = buf.d + 3U * count;
        OK_HIP(nullptr, hipMemcpy(d0, w0, 4U * count, hipMemcpyHostToDevice));
        OK_HIP(nullptr, hipMemcpy(d1, w1, 4U * count, hipMemcpyHostToDevice));
        const unsigned un = static_cast<unsigned>(n);
        hipLaunchKernelGGL(okDebugNormalKernel, dim3((un + 255U) / 256U), dim3(256), 0, nullptr, d0, d1, o0, o1, un);
        OK_HIP(nullptr, hipGetLastError());
        OK_HIP(nullptr, hipMemcpy(out0, o0, 4U * count, hipMemcpyDeviceToHost));
        OK_HIP(nullptr, hipMemcpy(out1, o1, 4U * count, hipMemcpyDeviceToHost));
        return OKENV_OK;
    }

    // ---- Guided cost learning: cost, policy and value networks (ok_gcl.h) --------------------------------------------------------

    int64_t okenv_gcl_lds_bytes(int32_t num_rays, int32_t hidden1, int32_t hidden2, int32_t cost_hidden1, int32_t cost_hidden2)
    {
        return static_cast<int64_t>(okGclLdsBytes(num_rays, hidden1, hidden2, cost_hidden1, cost_hidden2));
    }

    int okenv_gcl_create(okenv_t h, const okenv_gcl_config *config)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kGclDriver, "create", kGateHandle))
            return rc;
        if (const char *why = okGclCheckConfig(config, h->shape.R))
            return driverRefuses(h, OKENV_ERR_INVALID, kGclDriver, "create", why);
        OK_HIP(h, hipSetDevice(h->device));
        // room for the widest network, so that a later create with other widths allocates nothing: three networks of [params | m | v]
        const size_t cap = (static_cast<size_t>(ok_gauss_num_params(OK_ACTOR_MAX_RAYS, OK_GAUSS_MAX_HIDDEN, OK_GAUSS_MAX_HIDDEN, 2)) + 3U) & ~static_cast<size_t>(3U);
        if (const int rc = driverCreateFixed(h, kGclDriver, cap, 9, 0, true,
                                             {kernelOf(okGclActKernel), kernelOf(okGclForwardKernel<false>), kernelOf(okGclForwardKernel<true>),
                                              kernelOf(okGclGradKernel<OK_GCL_POLICY>), kernelOf(okGclGradKernel<OK_GCL_VALUE>),
                                              kernelOf(okGclGradKernel<OK_GCL_COST>)}))
            return rc;
        h->gcl = *config;
        h->gcl_t = h->gcl_cost_t = 0;
        h->gcl_learner_ok = false;
        h->gcl_bank_rows  = 0;
        return OKENV_OK;
    }

    int okenv_gcl_num_params(okenv_t h, int32_t which, int32_t *num_params)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kGclDriver, "num_params", kGateCreated))
            return rc;
        if (which < OKENV_GCL_POLICY || which > OKENV_GCL_COST)
            return fail(h, OKENV_ERR_INVALID, "okenv_gcl_num_params: unknown network (OKENV_GCL_POLICY / _VALUE / _COST)");
        if (num_params)
            *num_params = gclNumParams(h, which);
        return OKENV_OK;
    }

    int okenv_gcl_set_params(okenv_t h, int32_t which, const float *params)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kGclDriver, "set_params", kGateCreated))
            return rc;
        if (!params || which < OKENV_GCL_POLICY || which > OKENV_GCL_COST)
            return fail(h, OKENV_ERR_INVALID, "okenv_gcl_set_params: NULL argument or unknown network");
        return driverSet(h, kGclDriver, {vectorOf(gclVector(h, which, 0), params, gclNumParams(h, which), which)});
    }

    int okenv_gcl_get_state(okenv_t h, int32_t which, okenv_gcl_state *out)
    {
        OK_QUIESCE(h);
        if (!h || !out || which < OKENV_GCL_POLICY || which > OKENV_GCL_COST)
            return fail(h, OKENV_ERR_INVALID, "okenv_gcl_get_state: NULL argument or unknown network");
        if (const int rc = driverGate(h, kGclDriver, "get_state", kGateStored, true, 1U << which))
            return rc;
        const int n = gclNumParams(h, which);
        if (const int rc = driverGet(h, {vectorOf(gclVector(h, which, 0), out->params, n), vectorOf(gclVector(h, which, 1), out->m, n),
                                         vectorOf(gclVector(h, which, 2), out->v, n)}))
            return rc;
        out->t = which == OKENV_GCL_COST ? h->gcl_cost_t : h->gcl_t;
        return OKENV_OK;
    }

    int okenv_gcl_get_params(okenv_t h, int32_t which, float *params)
    {
        OK_QUIESCE(h);
        if (!params)
            return fail(h, OKENV_ERR_INVALID, "okenv_gcl_get_params: NULL argument");
        okenv_gcl_state st{params, nullptr, nullptr, 0};
        return okenv_gcl_get_state(h, which, &st);
    }

    int okenv_gcl_set_draw_offset(okenv_t h, const uint32_t *device_word)
    {
        OK_QUIESCE(h);
        return driverSetDrawOffset(h, kGclDriver, device_word);
    }

    int okenv_gcl_set_greedy(okenv_t h, int32_t greedy)
    {
        OK_QUIESCE(h);
        return driverSetGreedy(h, kGclDriver, &okenv::gcl, greedy);
    }

    int okenv_gcl_act(okenv_t h, const okenv_gcl_record *rec)
    {
        OK_QUIESCE(h);
        if (const int rc = actBegin(h, kGclDriver, 1U << OKENV_GCL_POLICY))
            return rc;
        OkGclActParams p{};
        p.f      = actFrame(h);
        p.draw   = actDrawWords(h, h->gcl_drv.draw_offset);
        p.H1     = h->gcl.hidden1;
        p.H2     = h->gcl.hidden2;
        p.params = gclVector(h, OKENV_GCL_POLICY, 0);
        for (int k = 0; k < 2; ++k)
        {
            p.scale[k] = h->gcl.scale[k];
            p.bias[k]  = h->gcl.bias[k];
        }
        p.greedy     = h->gcl.greedy;
        p.seed       = h->gcl.seed;
        p.agent_base = h->gcl.agent_base;
        if (rec != nullptr)
            p.rec = *rec;
        return actLaunch(h, okGclActKernel, kActorAgents, kActorThreads, okGaussActLdsBytes(p.f.R, p.H1, p.H2), p);
    }

    int okenv_gcl_set_expert(okenv_t h, const float *state, const float *action, int32_t E)
    {
        OK_QUIESCE(h);
        if (!h || !h->gcl_drv.ok)
            return fail(h, OKENV_ERR_STATE, "okenv_gcl_set_expert: call okenv_gcl_create first");
        if (!state || !action || E < 1)
            return fail(h, OKENV_ERR_INVALID, "okenv_gcl_set_expert: NULL argument or an empty bank");
        OK_HIP(h, hipSetDevice(h->device));
        const size_t R = static_cast<size_t>(h->shape.R), rows = static_cast<size_t>(E);
        if (rows * (R + 2U) > h->gcl_bank.cap)
            h->gcl_bank_rows = 0; // (a failed allocation leaves no bank)
        if (const int rc = growBuffers(h, {grown(h->gcl_bank, rows * (R + 2U))}))
            return rc;
        if (const int rc = copyAny(h, h->gcl_bank.d, state, sizeof(float) * rows * R))
            return rc;
        if (const int rc = copyAny(h, h->gcl_bank.d + rows * R, action, sizeof(float) * rows * 2U))
            return rc;
        h->gcl_bank_rows = E;
        return OKENV_OK;
    }

    int okenv_gcl_cost(okenv_t h, const float *state, const float *squashed, int32_t M, float *out)
    {
        OK_QUIESCE(h);
        if (!h)
            return fail(h, OKENV_ERR_INVALID, "okenv_gcl_cost: NULL handle");
        if (!h->gcl_drv.ok || !h->gcl_drv.set[OKENV_GCL_COST])
            return fail(h, OKENV_ERR_STATE, "okenv_gcl_cost: the cost network needs its parameters first (okenv_gcl_create, okenv_gcl_set_params)");
        if (!state || !squashed || !out || M < 1)
            return fail(h, OKENV_ERR_INVALID, "okenv_gcl_cost: NULL argument or M < 1");
        OK_HIP(h, hipSetDevice(h->device));
        OkGclForwardParams p{};
        p.R        = h->shape.R;
        p.in       = p.R + 2;
        p.H1       = h->gcl.cost_hidden1;
        p.H2       = h->gcl.cost_hidden2;
        p.M        = M;
        p.state    = state;
        p.squashed = squashed;
        p.params   = gclVector(h, OKENV_GCL_COST, 0);
        p.out      = out;
        p.C        = (M + OK_LEARN_CHUNK - 1) / OK_LEARN_CHUNK;
        hipLaunchKernelGGL(okGclForwardKernel<true>, dim3(static_cast<unsigned>(p.C)), dim3(kLearnThreads), okGclForwardLdsBytes(p.in, p.H1, p.H2), h->stream, p);
        OK_HIP(h, hipGetLastError());
        return OKENV_OK;
    }

    int okenv_gcl_learner_create(okenv_t h, const okenv_learner_params *policy_value, const okenv_learner_params *cost)
    {
        OK_QUIESCE(h);
        if (!h)
            return fail(h, OKENV_ERR_INVALID, "okenv_gcl_learner_create: NULL handle");
        for (const okenv_learner_params *lp : {policy_value, cost})
            if (const char *why = okLearnCheckParams(lp))
                return fail(h, OKENV_ERR_INVALID, std::string("okenv_gcl_learner_create: ") + why);
        if (!h->gcl_drv.ok || !h->gcl_drv.set[0] || !h->gcl_drv.set[1] || !h->gcl_drv.set[2])
            return fail(h, OKENV_ERR_STATE, "okenv_gcl_learner_create: needs a GCL object whose three networks have their parameters (okenv_gcl_create, okenv_gcl_set_params)");
        OK_HIP(h, hipSetDevice(h->device));
        for (int which = 0; which < 3; ++which)
            OK_HIP(h, hipMemsetAsync(gclVector(h, which, 1), 0, 2U * h->gcl_drv.cap * sizeof(float), h->stream));
        h->gcl_learner      = *policy_value;
        h->gcl_cost_learner = *cost;
        h->gcl_t = h->gcl_cost_t = 0;
        h->gcl_learner_ok        = true;
        return OKENV_OK;
    }

    int okenv_gcl_cost_update(okenv_t h, const okenv_gcl_cost_batch *batch, int32_t Mp, int32_t Me, const okenv_gcl_cost_output *out)
    {
        OK_QUIESCE(h);
        if (!h)
            return fail(h, OKENV_ERR_INVALID, "okenv_gcl_cost_update: NULL handle");
        if (!h->gcl_drv.ok || !h->gcl_learner_ok)
            return fail(h, OKENV_ERR_STATE, "okenv_gcl_cost_update: call okenv_gcl_learner_create first");
        if (h->gcl_bank_rows < 1)
            return fail(h, OKENV_ERR_STATE, "okenv_gcl_cost_update: call okenv_gcl_set_expert first (the bank is empty)");
        if (const char *why = okGclCheckCostCall(batch, Mp, Me))
            return fail(h, OKENV_ERR_INVALID, std::string("okenv_gcl_cost_update: ") + why);
        OK_HIP(h, hipSetDevice(h->device));
        OkUpdateScratch &u = h->gcl_scratch[OKENV_GCL_COST];
        OkGclGradParams  p{};
        p.R           = h->shape.R;
        p.in          = p.R + 2;
        p.H1          = h->gcl.cost_hidden1;
        p.H2          = h->gcl.cost_hidden2;
        p.Bk          = Mp;
        p.P           = gclNumParams(h, OKENV_GCL_COST);
        p.cols        = p.P + 1;
        p.state       = batch->state;
        p.squashed    = batch->squashed;
        p.bank_state  = h->gcl_bank.d;
        p.bank_action = h->gcl_bank.d + static_cast<size_t>(h->gcl_bank_rows) * static_cast<size_t>(p.R);
        p.E           = h->gcl_bank_rows;
        p.Me          = Me;
        p.Ce          = (Me + OK_LEARN_CHUNK - 1) / OK_LEARN_CHUNK;
        p.seed        = h->gcl.seed;
        p.draw        = static_cast<uint32_t>(h->gcl_cost_t);
        p.params      = gclVector(h, OKENV_GCL_COST, 0);
        const int Cp  = (Mp + OK_LEARN_CHUNK - 1) / OK_LEARN_CHUNK;
        if (const int rc = growScratch(h, u, sizeof(float) * static_cast<size_t>(p.Ce + Cp) * static_cast<size_t>(p.cols)))
            return rc;
        p.part = reinterpret_cast<float *>(u.part);
        if (const int rc = eventsBegin(h, u.log, 2U))
            return rc;
        hipLaunchKernelGGL(okGclGradKernel<OK_GCL_COST>, dim3(static_cast<unsigned>(p.Ce + Cp)), dim3(kLearnThreads), okGclGradLdsBytes(p.in, p.H1, p.H2, 1),
                           h->stream, p);
        OK_HIP(h, hipGetLastError());
        if (const int rc = eventsMark(h, u.log))
            return rc;
        OkGclCostJoinParams j{};
        j.P      = p.P;
        j.cols   = p.cols;
        j.Ce     = p.Ce;
        j.Cp     = Cp;
        j.part   = p.part;
        j.me     = static_cast<float>(Me);
        j.mp     = static_cast<float>(Mp);
        j.params = gclVector(h, OKENV_GCL_COST, 0);
        j.m      = gclVector(h, OKENV_GCL_COST, 1);
        j.v      = gclVector(h, OKENV_GCL_COST, 2);
        j.adam   = okLearnAdamConsts(h->gcl_cost_learner, h->gcl_cost_t + 1);
        j.loss   = out != nullptr ? out->loss : nullptr;
        j.grad   = out != nullptr ? out->grad : nullptr;
        hipLaunchKernelGGL(okGclCostStepKernel, dim3(static_cast<unsigned>((j.cols + kLearnStepCols - 1) / kLearnStepCols)), dim3(kLearnStepCols * kLearnStepRows), 0,
                           h->stream, j);
        OK_HIP(h, hipGetLastError());
        h->gcl_cost_t += 1;
        return eventsMark(h, u.log);
    }

    int okenv_gcl_policy_update(okenv_t h, const okenv_gcl_update_config *config, const okenv_gcl_batch *batch, int32_t M, int32_t B, const int32_t *order,
                                const okenv_gcl_output *out)
    {
        OK_QUIESCE(h);
        if (!h)
            return fail(h, OKENV_ERR_INVALID, "okenv_gcl_policy_update: NULL handle");
        if (!h->gcl_drv.ok || !h->gcl_learner_ok)
            return fail(h, OKENV_ERR_STATE, "okenv_gcl_policy_update: call okenv_gcl_learner_create first");
        if (const char *why = okGclCheckCall(config, batch, M, B))
            return fail(h, OKENV_ERR_INVALID, std::string("okenv_gcl_policy_update: ") + why);
        OK_HIP(h, hipSetDevice(h->device));
        const okenv_gcl_output  none{};
        const okenv_gcl_output &o = out != nullptr ? *out : none;
        const bool              accumulate = config->accumulate != 0;
        const int               R = h->shape.R, H1 = h->gcl.hidden1, H2 = h->gcl.hidden2;
        // the advantages' scratch: [S, Q partials | adv | mean, std | the policy chunks' clip counts], each piece 256-aligned
        const auto   up    = [](const size_t b) { return (b + 255U) & ~static_cast<size_t>(255U); };
        const int    Cm    = (M + OK_LEARN_CHUNK - 1) / OK_LEARN_CHUNK;
        const size_t c_max = (static_cast<size_t>(std::min(B, M)) + OK_LEARN_CHUNK - 1U) / OK_LEARN_CHUNK;
        const size_t stat_bytes = up(sizeof(double) * 2U * static_cast<size_t>(Cm)), adv_bytes = up(sizeof(float) * static_cast<size_t>(M));
        if (const int rc = growScratch(h, h->gcl_adv_scratch, stat_bytes + adv_bytes + 256U + up(sizeof(uint32_t) * c_max)))
            return rc;
        double   *stat = reinterpret_cast<double *>(h->gcl_adv_scratch.part);
        float    *adv = reinterpret_cast<float *>(h->gcl_adv_scratch.part + stat_bytes), *ms = reinterpret_cast<float *>(h->gcl_adv_scratch.part + stat_bytes + adv_bytes);
        uint32_t *part_clip = reinterpret_cast<uint32_t *>(h->gcl_adv_scratch.part + stat_bytes + adv_bytes + 256U);
        // the value sweep with the parameters the call starts with, the statistics, the normalisation
        OkGclForwardParams f{};
        f.R      = R;
        f.in     = R;
        f.H1     = H1;
        f.H2     = H2;
        f.M      = M;
        f.state  = batch->state;
        f.ret    = batch->ret;
        f.params = gclVector(h, OKENV_GCL_VALUE, 0);
        f.out    = adv;
        f.stat   = stat;
        f.C      = Cm;
        hipLaunchKernelGGL(okGclForwardKernel<false>, dim3(static_cast<unsigned>(Cm)), dim3(kLearnThreads), okGclForwardLdsBytes(R, H1, H2), h->stream, f);
        OK_HIP(h, hipGetLastError());
        hipLaunchKernelGGL(okGclAdvStatsKernel, dim3(1), dim3(kGclStatsThreads), 0, h->stream, stat, Cm, M, ms);
        OK_HIP(h, hipGetLastError());
        hipLaunchKernelGGL(okGclAdvNormKernel, dim3(static_cast<unsigned>((M + 255) / 256)), dim3(256), 0, h->stream, adv, ms, M, o.adv);
        OK_HIP(h, hipGetLastError());
        if (o.clipped != nullptr)
            OK_HIP(h, hipMemsetAsync(o.clipped, 0, sizeof(int32_t) * static_cast<size_t>(accumulate ? 1 : okLearnMinibatches(M, B)), h->stream));
        OkGclGradParams p{};
        p.R     = R;
        p.in    = R;
        p.H1    = H1;
        p.H2    = H2;
        p.M     = M;
        p.order = order;
        p.state = batch->state;
        p.pre   = batch->pre;
        p.logp  = batch->logp;
        p.ret   = batch->ret;
        p.adv   = adv;
        p.lo    = okLearnClipLo(h->gcl_learner.clip);
        p.hi    = okLearnClipHi(h->gcl_learner.clip);
        // the policy's slices, then the value's: the join kernels are section 19's, on either parameter vector; both count the same steps
        int64_t t_policy = h->gcl_t, t_value = h->gcl_t;
        p.P         = gclNumParams(h, OKENV_GCL_POLICY);
        p.cols      = p.P + 1;
        p.params    = gclVector(h, OKENV_GCL_POLICY, 0);
        p.part_clip = o.clipped != nullptr ? part_clip : nullptr;
        if (const int rc = sliceUpdate(h, h->gcl_scratch[OKENV_GCL_POLICY], M, B, accumulate,
                                       okJoinOn(p.P, gclVector(h, OKENV_GCL_POLICY, 0), gclVector(h, OKENV_GCL_POLICY, 1), gclVector(h, OKENV_GCL_POLICY, 2), config->reduce,
                                                o.grad_policy),
                                       t_policy, h->gcl_learner, o.policy_loss,
                                       [&](const long base, const int Bk, const int C)
                                       {
                                           p.base = base;
                                           p.Bk   = Bk;
                                           p.part = reinterpret_cast<float *>(h->gcl_scratch[OKENV_GCL_POLICY].part);
                                           hipLaunchKernelGGL(okGclGradKernel<OK_GCL_POLICY>, dim3(static_cast<unsigned>(C)), dim3(kLearnThreads),
                                                              okGclGradLdsBytes(R, H1, H2, 2), h->stream, p);
                                           if (o.clipped != nullptr)
                                               hipLaunchKernelGGL(okGclClipCountKernel, dim3(1), dim3(256), 0, h->stream, part_clip, C, o.clipped + (accumulate ? 0 : base / B));
                                       }))
            return rc;
        p.P         = gclNumParams(h, OKENV_GCL_VALUE);
        p.cols      = p.P + 1;
        p.params    = gclVector(h, OKENV_GCL_VALUE, 0);
        p.part_clip = nullptr;
        if (const int rc = sliceUpdate(h, h->gcl_scratch[OKENV_GCL_VALUE], M, B, accumulate,
                                       okJoinOn(p.P, gclVector(h, OKENV_GCL_VALUE, 0), gclVector(h, OKENV_GCL_VALUE, 1), gclVector(h, OKENV_GCL_VALUE, 2), config->reduce,
                                                o.grad_value),
                                       t_value, h->gcl_learner, o.value_loss,
                                       [&](const long base, const int Bk, const int C)
                                       {
                                           p.base = base;
                                           p.Bk   = Bk;
                                           p.part = reinterpret_cast<float *>(h->gcl_scratch[OKENV_GCL_VALUE].part);
                                           hipLaunchKernelGGL(okGclGradKernel<OK_GCL_VALUE>, dim3(static_cast<unsigned>(C)), dim3(kLearnThreads),
                                                              okGclGradLdsBytes(R, H1, H2, 1), h->stream, p);
                                       }))
            return rc;
        h->gcl_t = t_policy;
        return OKENV_OK;
    }

    int okenv_debug_gcl_timing(okenv_t h, int32_t which, double *ms2)
    {
        OK_QUIESCE(h);
        if (!h || !ms2 || which < OKENV_GCL_POLICY || which > OKENV_GCL_COST)
            return fail(h, OKENV_ERR_INVALID, "okenv_debug_gcl_timing: NULL argument or unknown network");
        if (h->gcl_scratch[which].log.timed < 3U)
            return fail(h, OKENV_ERR_STATE, "okenv_debug_gcl_timing: no update of this network has run with okenv_set_timing on");
        return eventsSums(h, h->gcl_scratch[which].log, ms2, 2);
    }

    int okenv_gcl_act_host(const okenv_gcl_config *config, const float *policy, int32_t num_rays, int32_t n, const float *rel_x, const float *rel_y,
                           const uint8_t *crashed, uint32_t draw_index, float *throttle, float *steer, float *eps, float *pre, float *squashed, float *action,
                           float *logp, float *state, uint8_t *alive)
    {
        if (const char *why = okGclCheckConfig(config, num_rays))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_gcl_act_host: ") + why);
        if (!policy || n < 0 || !rel_x || !rel_y)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_gcl_act_host: bad argument");
        okGclActHost(*config, policy, num_rays, n, rel_x, rel_y, crashed, draw_index, throttle, steer, eps, pre, squashed, action, logp, state, alive);
        return OKENV_OK;
    }

    int okenv_gcl_cost_host(const float *cost, int32_t num_rays, int32_t cost_hidden1, int32_t cost_hidden2, const float *state, const float *squashed,
                            int32_t M, float *out)
    {
        if (const char *why = okGclCheckShape(num_rays, 1, 1, cost_hidden1, cost_hidden2))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_gcl_cost_host: ") + why);
        if (!cost || !state || !squashed || !out || M < 0)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_gcl_cost_host: bad argument");
        okGclForwardHost(okGclHostNet(OK_GCL_COST, num_rays, cost_hidden1, cost_hidden2, cost), num_rays, state, squashed, M, out);
        return OKENV_OK;
    }

    int okenv_gcl_cost_update_host(const okenv_learner_params *params, uint32_t seed, int32_t num_rays, int32_t cost_hidden1, int32_t cost_hidden2,
                                   okenv_gcl_state *state, const float *bank_state, const float *bank_action, int32_t E, const okenv_gcl_cost_batch *batch,
                                   int32_t Mp, int32_t Me, const okenv_gcl_cost_output *out)
    {
        if (const char *why = okLearnCheckParams(params))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_gcl_cost_update_host: ") + why);
        if (const char *why = okGclCheckShape(num_rays, 1, 1, cost_hidden1, cost_hidden2))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_gcl_cost_update_host: ") + why);
        if (const char *why = okGclCheckCostCall(batch, Mp, Me))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_gcl_cost_update_host: ") + why);
        if (!bank_state || !bank_action || E < 1)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_gcl_cost_update_host: the expert bank is NULL or empty");
        if (!okGclStateComplete(state))
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_gcl_cost_update_host: state lacks a parameter or moment vector, or t < 0");
        const okenv_gcl_cost_output none{};
        okGclCostUpdateHost(*params, seed, num_rays, cost_hidden1, cost_hidden2, *state, bank_state, bank_action, E, *batch, Mp, Me, out != nullptr ? *out : none);
        return OKENV_OK;
    }

    int okenv_gcl_policy_update_host(const okenv_learner_params *params, const okenv_gcl_update_config *config, int32_t num_rays, int32_t hidden1,
                                     int32_t hidden2, okenv_gcl_state *policy, okenv_gcl_state *value, const okenv_gcl_batch *batch, int32_t M, int32_t B,
                                     const int32_t *order, const okenv_gcl_output *out)
    {
        if (const char *why = okLearnCheckParams(params))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_gcl_policy_update_host: ") + why);
        if (const char *why = okGclCheckShape(num_rays, hidden1, hidden2, 1, 1))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_gcl_policy_update_host: ") + why);
        if (const char *why = okGclCheckCall(config, batch, M, B))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_gcl_policy_update_host: ") + why);
        if (!okGclStateComplete(policy) || !okGclStateComplete(value))
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_gcl_policy_update_host: a state lacks a parameter or moment vector, or t < 0");
        const okenv_gcl_output none{};
        okGclPolicyUpdateHost(*params, *config, num_rays, hidden1, hidden2, *policy, *value, *batch, M, B, order, out != nullptr ? *out : none);
        return OKENV_OK;
    }

    // ---- Lidar transformer driver (ok_lidar.h) -----------------------------------------------------------------------------------

    int64_t okenv_lidar_lds_bytes(const okenv_lidar_config *config)
    {
        return config != nullptr ? static_cast<int64_t>(okLidarLdsBytes(okLidarShape(*config))) : 0;
    }

    int okenv_lidar_create(okenv_t h, const okenv_lidar_config *config)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kLidarDriver, "create", kGateHandle))
            return rc;
        if (const char *why = okLidarCheckConfig(config))
            return driverRefuses(h, OKENV_ERR_INVALID, kLidarDriver, "create", why);
        if (config->num_points != h->shape.R)
            return fail(h, OKENV_ERR_INVALID, "okenv_lidar_create: num_points must equal the handle's ray count");
        if (const int rc = driverCreateFlat(h, kLidarDriver, static_cast<size_t>(ok_lidar_offsets(okLidarShape(*config)).total), {kernelOf(okLidarActKernel)}))
            return rc;
        h->lidar        = *config;
        h->lidar_drv.ok = true;
        return OKENV_OK;
    }

    int okenv_lidar_num_params(okenv_t h, int32_t *num_params)
    {
        OK_QUIESCE(h);
        return flatNumParams(h, kLidarDriver, num_params);
    }

    int okenv_lidar_set_params(okenv_t h, const float *params)
    {
        OK_QUIESCE(h);
        return flatSetParams(h, kLidarDriver, 0, params);
    }

    int okenv_lidar_get_params(okenv_t h, float *params)
    {
        OK_QUIESCE(h);
        return flatGetParams(h, kLidarDriver, 0, params);
    }

    int okenv_lidar_act(okenv_t h, const okenv_lidar_record *rec)
    {
        OK_QUIESCE(h);
        if (const int rc = actBegin(h, kLidarDriver, 1U))
            return rc;
        OkLidarActParams p{};
        p.st     = h->st;
        p.N      = h->shape.N;
        p.s      = okLidarShape(h->lidar);
        p.params = h->lidar_drv.d;
        for (int k = 0; k < 2; ++k)
        {
            p.lo[k] = h->lidar.action_lo[k];
            p.hi[k] = h->lidar.action_hi[k];
        }
        p.range = h->lidar.sensor_range;
        p.scale = ok_lidar_scale(p.s.d / p.s.nhead);
        if (rec != nullptr)
            p.rec = *rec;
        return actLaunch(h, okLidarActKernel, kLidarAgents, kLidarThreads, okLidarLdsBytes(p.s), p);
    }

    int okenv_lidar_act_host(const okenv_lidar_config *config, const float *params, int32_t n, const float *rel_xy, const uint8_t *crashed, float *throttle,
                             float *steer, float *input, uint8_t *alive)
    {
        if (const char *why = okLidarCheckConfig(config))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_lidar_act_host: ") + why);
        if (!params || n < 0 || !rel_xy)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_lidar_act_host: bad argument");
        okLidarActHost(*config, params, n, rel_xy, crashed, throttle, steer, input, alive);
        return OKENV_OK;
    }

    int okenv_debug_lidar_linear(int32_t device, int32_t M, int32_t K, int32_t N, const float *x, const float *w, const float *bias, int32_t relu, float *out)
    {
        if (!x || !w || !bias || !out || M < 0 || K < 16 || K > 4096 || K % 16 != 0 || N < 16 || N > 4096 || N % 16 != 0)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_debug_lidar_linear: bad argument (K and N multiples of 16 up to 4096)");
        if (device < 0)
        {
            okLidarLinearHost(M, K, N, x, w, bias, relu, out);
            return OKENV_OK;
        }
        const size_t lds = okDebugLidarLinearLdsBytes(K, N);
        if (lds > kLdsBudget)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_debug_lidar_linear: 16 rows of x and out do not fit the LDS");
        if (const int rc = debugNeedsDevice("okenv_debug_lidar_linear"))
            return rc;
        if (M == 0)
            return OKENV_OK;
        OK_HIP(nullptr, hipSetDevice(device));
        // [x M K | w N K | bias N | out M N]
        const size_t nx = static_cast<size_t>(M) * K, nw = static_cast<size_t>(N) * K, nb = static_cast<size_t>(N), no = static_cast<size_t>(M) * N;
        DebugBuffer  buf;
        OK_HIP(nullptr, hipMalloc(reinterpret_cast<void **>(&buf.d), 4U * (nx + nw + nb + no)));
        float *dx = buf.d, *dw = dx + nx, *db = dw + nw, *dout = db + nb;
        OK_HIP(nullptr, hipMemcpy(dx, x, 4U * nx, hipMemcpyHostToDevice));
        OK_HIP(nullptr, hipMemcpy(dw, w, 4U * nw, hipMemcpyHostToDevice));
        OK_HIP(nullptr, hipMemcpy(db, bias, 4U * nb, hipMemcpyHostToDevice));
        if (const int rc = raiseLdsLimit(nullptr, {kernelOf(okDebugLidarLinearKernel)}))
            return rc;
        hipLaunchKernelGGL(okDebugLidarLinearKernel, dim3(static_cast<unsigned>((M + kLidarAgents - 1) / kLidarAgents)), dim3(kLidarThreads), lds, nullptr, M, K, N,
                           dx, dw, db, relu, dout);
        OK_HIP(nullptr, hipGetLastError());
        OK_HIP(nullptr, hipMemcpy(out, dout, 4U * no, hipMemcpyDeviceToHost));
        return OKENV_OK;
    }

    // ---- Image transformer driver (ok_vit.h) -----------------------------------------------------------------------------------

    int64_t okenv_vit_lds_bytes(const okenv_vit_config *config)
    {
        return config != nullptr ? static_cast<int64_t>(okVitLdsBytes(okVitShape(*config))) : 0;
    }

    int okenv_vit_create(okenv_t h, const okenv_vit_config *config)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kVitDriver, "create", kGateHandle))
            return rc;
        if (const char *why = okVitCheckConfig(config))
            return driverRefuses(h, OKENV_ERR_INVALID, kVitDriver, "create", why);
        const ok_vit_shape s = okVitShape(*config);
        const size_t       pass = okVitAgentsPerPass(*config, static_cast<size_t>(h->shape.N));
        if (const char *why = okVitWorkspaceBad(*config, pass))
            return driverRefuses(h, OKENV_ERR_INVALID, kVitDriver, "create", why);
        h->vit_head_ok = false; // (the head's learner belongs to the policy that goes)
        if (const int rc = driverCreateFlat(h, kVitDriver, static_cast<size_t>(ok_vit_offsets(s).total), {kernelOf(okVitAttendKernel), kernelOf(okVitFinalKernel)},
                                            {grown(h->vit_work, pass * ok_vit_agent_floats(s))}))
            return rc;
        h->vit        = *config;
        h->vit_pass   = pass;
        h->vit_drv.ok = true;
        return OKENV_OK;
    }

    int okenv_vit_num_params(okenv_t h, int32_t *num_params)
    {
        OK_QUIESCE(h);
        return flatNumParams(h, kVitDriver, num_params);
    }

    int okenv_vit_set_params(okenv_t h, const float *params)
    {
        OK_QUIESCE(h);
        return flatSetParams(h, kVitDriver, 0, params);
    }

    int okenv_vit_get_params(okenv_t h, float *params)
    {
        OK_QUIESCE(h);
        return flatGetParams(h, kVitDriver, 0, params);
    }

    int okenv_vit_act(okenv_t h, const uint8_t *frames, int64_t frame_bytes, const okenv_vit_record *rec)
    {
        OK_QUIESCE(h);
        return vitAct(h, frames, frame_bytes, rec);
    }

    int okenv_vit_act_host(const okenv_vit_config *config, const float *params, int32_t n, const uint8_t *frames, const uint8_t *crashed, float *throttle,
                           float *steer, float *output, float *embedding, uint8_t *alive)
    {
        if (const char *why = okVitCheckConfig(config))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_vit_act_host: ") + why);
        if (!params || !frames || n < 0)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_vit_act_host: bad argument");
        okVitActHost(*config, params, n, frames, crashed, throttle, steer, output, embedding, alive);
        return OKENV_OK;
    }

    int okenv_debug_vit_attend(int32_t device, int32_t seqs, int32_t T, int32_t heads, int32_t dh, const float *qkv, float *ctx)
    {
        if (!qkv || !ctx || seqs < 0 || T < 1 || T > OK_VIT_MAX_TOKENS || heads < 1 || heads > OK_VIT_MAX_DIM / 16 || dh < 16 || dh > OK_VIT_MAX_HEAD_DIM ||
            dh % 16 != 0 || heads * dh > OK_VIT_MAX_DIM || seqs > 65536)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_debug_vit_attend: bad argument (T 1 .. 1024, dh a multiple of 16 up to 64, heads x dh up to 768)");
        if (device < 0)
        {
            okVitAttendHost(seqs, T, heads, dh, qkv, ctx);
            return OKENV_OK;
        }
        if (const int rc = debugNeedsDevice("okenv_debug_vit_attend"))
            return rc;
        if (seqs == 0)
            return OKENV_OK;
        OK_HIP(nullptr, hipSetDevice(device));
        const size_t D = static_cast<size_t>(heads) * dh, nq = static_cast<size_t>(seqs) * T * 3U * D, nc = static_cast<size_t>(seqs) * T * D;
        DebugBuffer  buf;
        OK_HIP(nullptr, hipMalloc(reinterpret_cast<void **>(&buf.d), 4U * (nq + nc)));
        float *dq = buf.d, *dc = dq + nq;
        OK_HIP(nullptr, hipMemcpy(dq, qkv, 4U * nq, hipMemcpyHostToDevice));
        if (const int rc = raiseLdsLimit(nullptr, {kernelOf(okVitAttendKernel)}))
            return rc;
        OkVitAttendParams ap{};
        ap.T = T, ap.D = static_cast<int>(D), ap.heads = heads, ap.dh = dh, ap.qtiles = (T + kVitQueries - 1) / kVitQueries;
        ap.scale = ok_lidar_scale(dh), ap.qkv = dq, ap.ctx = dc;
        hipLaunchKernelGGL(okVitAttendKernel, dim3(static_cast<unsigned>(static_cast<size_t>(seqs) * heads * ap.qtiles)), dim3(kVitThreads),
                           okVitAttendLdsBytes(T, dh), nullptr, ap);
        OK_HIP(nullptr, hipGetLastError());
        OK_HIP(nullptr, hipMemcpy(ctx, dc, 4U * nc, hipMemcpyDeviceToHost));
        return OKENV_OK;
    }

    // ---- The image transformer driver's training (ok_vithead.h) ---------------------------------------------------------------------

    int okenv_vit_embed(okenv_t h, const uint8_t *frames, int32_t m, int64_t frame_bytes, float *embedding)
    {
        OK_QUIESCE(h);
        return vitEmbed(h, frames, m, frame_bytes, embedding);
    }

    int64_t okenv_vit_head_lds_bytes(int32_t dim, int32_t hidden1, int32_t hidden2)
    {
        return static_cast<int64_t>(okVitHeadLdsBytes(dim, hidden1, hidden2));
    }

    int okenv_vit_head_learner_create(okenv_t h, const okenv_vit_head_params *params)
    {
        OK_QUIESCE(h);
        if (!h)
            return fail(h, OKENV_ERR_INVALID, "okenv_vit_head_learner_create: NULL handle");
        if (const char *why = okVitHeadCheckParams(params))
            return fail(h, OKENV_ERR_INVALID, std::string("okenv_vit_head_learner_create: ") + why);
        if (!h->vit_drv.ok || !h->vit_drv.set[0])
            return fail(h, OKENV_ERR_STATE, "okenv_vit_head_learner_create: needs a policy that has its parameters (okenv_vit_create, okenv_vit_set_params)");
        if (const char *why = okVitHeadCheckShape(h->vit.dim, h->vit.head_hidden1, h->vit.head_hidden2, h->vit.steer_scale))
            return fail(h, OKENV_ERR_INVALID, std::string("okenv_vit_head_learner_create: ") + why);
        OK_HIP(h, hipSetDevice(h->device));
        h->vit_head_ok = false;
        if (const int rc = growBuffers(h, {grown(h->vit_head_mv, 2U * static_cast<size_t>(vitHeadTotal(h)))})) // [m | v], each half the room
            return rc;
        if (const int rc = raiseLdsLimit(h, {kernelOf(okVitHeadForwardKernel)}))
            return rc;
        OK_HIP(h, hipMemsetAsync(h->vit_head_mv.d, 0, h->vit_head_mv.cap * sizeof(float), h->stream));
        h->vit_head    = *params;
        h->vit_head_t  = 0;
        h->vit_head_ok = true;
        return OKENV_OK;
    }

    int okenv_vit_head_learner_reset(okenv_t h)
    {
        OK_QUIESCE(h);
        if (!h || !h->vit_drv.ok || !h->vit_head_ok)
            return fail(h, OKENV_ERR_STATE, "okenv_vit_head_learner_reset: call okenv_vit_head_learner_create first");
        OK_HIP(h, hipSetDevice(h->device));
        OK_HIP(h, hipMemsetAsync(h->vit_head_mv.d, 0, h->vit_head_mv.cap * sizeof(float), h->stream));
        h->vit_head_t = 0;
        return OKENV_OK;
    }

    int okenv_vit_head_learner_get_state(okenv_t h, okenv_vit_head_state *out)
    {
        OK_QUIESCE(h);
        if (!h || !out)
            return fail(h, OKENV_ERR_INVALID, "okenv_vit_head_learner_get_state: NULL argument");
        if (!h->vit_drv.ok || !h->vit_head_ok)
            return fail(h, OKENV_ERR_STATE, "okenv_vit_head_learner_get_state: call okenv_vit_head_learner_create first");
        const int n = vitHeadTotal(h);
        if (const int rc = driverGet(h, {vectorOf(vitHeadParams(h), out->params, n), vectorOf(vitHeadMoment(h, 0), out->m, n), vectorOf(vitHeadMoment(h, 1), out->v, n)}))
            return rc;
        out->t = h->vit_head_t;
        return OKENV_OK;
    }

    int okenv_vit_head_update(okenv_t h, const float *embedding, const float *steer, int32_t M, int32_t B, int32_t epochs, const int32_t *order,
                              const okenv_vit_head_output *out)
    {
        OK_QUIESCE(h);
        return vitHeadRun(h, "okenv_vit_head_update", true, embedding, steer, M, B, epochs, order, out != nullptr ? out->loss : nullptr,
                          out != nullptr ? out->grad : nullptr);
    }

    int okenv_vit_head_eval(okenv_t h, const float *embedding, const float *steer, int32_t M, int32_t B, float *loss)
    {
        OK_QUIESCE(h);
        if (h != nullptr && h->vit_head_ok && loss == nullptr)
            return fail(h, OKENV_ERR_INVALID, "okenv_vit_head_eval: NULL argument");
        return vitHeadRun(h, "okenv_vit_head_eval", false, embedding, steer, M, B, 1, nullptr, loss, nullptr);
    }

    int okenv_vit_head_update_host(const okenv_vit_head_params *params, int32_t dim, int32_t hidden1, int32_t hidden2, float steer_scale,
                                   okenv_vit_head_state *state, const float *embedding, const float *steer, int32_t M, int32_t B, int32_t epochs,
                                   const int32_t *order, const okenv_vit_head_output *out)
    {
        if (const char *why = okVitHeadCheckParams(params))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_vit_head_update_host: ") + why);
        if (const char *why = okVitHeadCheckShape(dim, hidden1, hidden2, steer_scale))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_vit_head_update_host: ") + why);
        if (const char *why = okVitHeadCheckCall(embedding, steer, M, B, epochs))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_vit_head_update_host: ") + why);
        if (state == nullptr || state->params == nullptr || state->m == nullptr || state->v == nullptr || state->t < 0)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_vit_head_update_host: state is NULL, lacks a parameter or moment vector (NULL argument), or t < 0");
        const okenv_vit_head_output none{};
        okVitHeadUpdateHost(*params, dim, hidden1, hidden2, steer_scale, *state, embedding, steer, M, B, epochs, order, out != nullptr ? *out : none);
        return OKENV_OK;
    }

    int okenv_vit_head_eval_host(const okenv_vit_head_params *params, int32_t dim, int32_t hidden1, int32_t hidden2, float steer_scale, const float *head,
                                 const float *embedding, const float *steer, int32_t M, int32_t B, float *loss)
    {
        if (const char *why = okVitHeadCheckParams(params))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_vit_head_eval_host: ") + why);
        if (const char *why = okVitHeadCheckShape(dim, hidden1, hidden2, steer_scale))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_vit_head_eval_host: ") + why);
        if (const char *why = okVitHeadCheckCall(embedding, steer, M, B, 1))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_vit_head_eval_host: ") + why);
        if (head == nullptr || loss == nullptr)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_vit_head_eval_host: NULL argument");
        okVitHeadEvalHost(*params, dim, hidden1, hidden2, steer_scale, head, embedding, steer, M, B, loss);
        return OKENV_OK;
    }

    // ---- Flow-matching driver (ok_flow.h) ----------------------------------------------------------------------------------------

    int64_t okenv_flow_lds_bytes(const okenv_flow_config *config)
    {
        return config != nullptr ? static_cast<int64_t>(okFlowLdsBytes(okFlowShape(*config))) : 0;
    }

    int okenv_flow_create(okenv_t h, const okenv_flow_config *config)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kFlowDriver, "create", kGateHandle))
            return rc;
        if (const char *why = okFlowCheckConfig(config))
            return driverRefuses(h, OKENV_ERR_INVALID, kFlowDriver, "create", why);
        if (const int rc = driverCreateFlat(h, kFlowDriver, static_cast<size_t>(ok_flow_offsets(okFlowShape(*config)).total), {kernelOf(okFlowActKernel)}))
            return rc;
        h->flow        = *config;
        h->flow_drv.ok = true;
        return OKENV_OK;
    }

    int okenv_flow_num_params(okenv_t h, int32_t *num_params)
    {
        OK_QUIESCE(h);
        return flatNumParams(h, kFlowDriver, num_params);
    }

    int okenv_flow_set_params(okenv_t h, const float *params)
    {
        OK_QUIESCE(h);
        return flatSetParams(h, kFlowDriver, 0, params);
    }

    int okenv_flow_get_params(okenv_t h, float *params)
    {
        OK_QUIESCE(h);
        return flatGetParams(h, kFlowDriver, 0, params);
    }

    int okenv_flow_set_draw_offset(okenv_t h, const uint32_t *device_word)
    {
        OK_QUIESCE(h);
        return driverSetDrawOffset(h, kFlowDriver, device_word);
    }

    int okenv_flow_act(okenv_t h, const float *cond, const okenv_flow_record *rec)
    {
        OK_QUIESCE(h);
        if (const int rc = actBegin(h, kFlowDriver, 1U, cond != nullptr ? nullptr : "cond is NULL"))
            return rc;
        OkFlowActParams p{};
        p.st     = h->st;
        p.N      = h->shape.N;
        p.s      = okFlowShape(h->flow);
        p.params = h->flow_drv.d;
        p.cond   = cond;
        p.draw   = actDrawWords(h, h->flow_drv.draw_offset);
        for (int k = 0; k < 2; ++k)
        {
            p.lo[k] = h->flow.action_lo[k];
            p.hi[k] = h->flow.action_hi[k];
        }
        p.noise      = h->flow.noise;
        p.seed       = h->flow.seed;
        p.agent_base = h->flow.agent_base;
        if (rec != nullptr)
            p.rec = *rec;
        return actLaunch(h, okFlowActKernel, kFlowAgents, kLidarThreads, okFlowLdsBytes(p.s), p);
    }

    int okenv_flow_act_host(const okenv_flow_config *config, const float *params, int32_t n, const float *cond, const uint8_t *crashed,
                            uint32_t draw_index, float *throttle, float *steer, float *x0, float *x, uint8_t *alive)
    {
        if (const char *why = okFlowCheckConfig(config))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_flow_act_host: ") + why);
        if (!params || n < 0 || !cond)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_flow_act_host: bad argument");
        okFlowActHost(*config, params, n, cond, crashed, draw_index, throttle, steer, x0, x, alive);
        return OKENV_OK;
    }

    // ---- Behavioural-cloning image policy (ok_cnn.h) -------------------------------------------------------------------------------

    int64_t okenv_cnn_lds_bytes(const okenv_cnn_config *config)
    {
        return config != nullptr ? static_cast<int64_t>(okCnnLdsBytes(okCnnShape(*config))) : 0;
    }

    int okenv_cnn_plan(const okenv_cnn_config *config, int32_t *plan)
    {
        if (const char *why = okCnnCheckConfig(config))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_cnn_plan: ") + why);
        if (!plan)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_cnn_plan: bad argument");
        const OkCnnPlaces pl = okCnnPlaces(okCnnShape(*config));
        plan[0] = pl.ct;
        plan[1] = pl.region;
        return OKENV_OK;
    }

    int okenv_cnn_create(okenv_t h, const okenv_cnn_config *config)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kCnnDriver, "create", kGateHandle))
            return rc;
        if (const char *why = okCnnCheckConfig(config))
            return driverRefuses(h, OKENV_ERR_INVALID, kCnnDriver, "create", why);
        const ok_cnn_shape s = okCnnShape(*config);
        if (const int rc = driverCreateFlat(h, kCnnDriver, static_cast<size_t>(ok_cnn_offsets(s).total), {kernelOf(okCnnConvKernel)},
                                            {grown(h->cnn_pack, static_cast<size_t>(okCnnPlaces(s).pack_total)),
                                             grown(h->cnn_feat, static_cast<size_t>(h->shape.N) * ok_cnn_features(s))}))
            return rc;
        h->cnn        = *config;
        h->cnn_drv.ok = true;
        return OKENV_OK;
    }

    int okenv_cnn_num_params(okenv_t h, int32_t *num_params)
    {
        OK_QUIESCE(h);
        return flatNumParams(h, kCnnDriver, num_params);
    }

    int okenv_cnn_set_params(okenv_t h, const float *params)
    {
        OK_QUIESCE(h);
        return flatSetParams(h, kCnnDriver, 0, params);
    }

    int okenv_cnn_get_params(okenv_t h, float *params)
    {
        OK_QUIESCE(h);
        return flatGetParams(h, kCnnDriver, 0, params);
    }

    int okenv_cnn_act(okenv_t h, const uint8_t *frames, int64_t frame_bytes, const okenv_cnn_record *rec)
    {
        OK_QUIESCE(h);
        return cnnAct(h, frames, frame_bytes, rec, OKENV_CNN_STAGE_CONV | OKENV_CNN_STAGE_HEAD);
    }

    int okenv_debug_cnn_stages(okenv_t h, const uint8_t *frames, int64_t frame_bytes, const okenv_cnn_record *rec, uint32_t stages)
    {
        OK_QUIESCE(h);
        return cnnAct(h, frames, frame_bytes, rec, stages);
    }

    int okenv_cnn_act_host(const okenv_cnn_config *config, const float *params, int32_t n, const uint8_t *frames, const uint8_t *crashed,
                           float *throttle, float *steer, float *out, uint8_t *alive)
    {
        if (const char *why = okCnnCheckConfig(config))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_cnn_act_host: ") + why);
        if (!params || n < 0 || !frames)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_cnn_act_host: bad argument");
        okCnnActHost(*config, params, n, frames, crashed, throttle, steer, out, alive);
        return OKENV_OK;
    }

    // ---- World-model racers (ok_world.h) -------------------------------------------------------------------------------------------

    int64_t okenv_world_lds_bytes(const okenv_world_config *config)
    {
        return config != nullptr ? static_cast<int64_t>(okWorldLdsBytes(okWorldShape(*config))) : 0;
    }

    int okenv_world_plan(const okenv_world_config *config, int32_t *plan)
    {
        if (const char *why = okWorldCheckConfig(config))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_world_plan: ") + why);
        if (!plan)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_world_plan: bad argument");
        okWorldPlan(okWorldShape(*config), plan);
        return OKENV_OK;
    }

    int64_t okenv_world_workspace_bytes(const okenv_world_config *config, int32_t num_agents)
    {
        if (okWorldCheckConfig(config) != nullptr || num_agents < 1)
            return 0;
        const ok_world_shape s = okWorldShape(*config);
        return static_cast<int64_t>(sizeof(float) * (okWorldPlaces(s, static_cast<size_t>(num_agents)).words + static_cast<size_t>(ok_world_offsets(s).total)));
    }

    int okenv_world_create(okenv_t h, const okenv_world_config *config)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kWorldDriver, "create", kGateHandle))
            return rc;
        if (const char *why = okWorldCheckConfig(config))
            return driverRefuses(h, OKENV_ERR_INVALID, kWorldDriver, "create", why);
        const ok_world_shape s = okWorldShape(*config);
        h->mem_drv.ok          = false; // (a memory belongs to the racers it was created on: okenv_memory_create attaches a new one)
        h->mem_learn_ok        = false; // (and a learner to its memory)
        const OkWorldPlaces  pl = okWorldPlaces(s, static_cast<size_t>(h->shape.N));
        // (the conv kernels' 16.5 KB and their row table fit the default limit; the latent kernel, up to 32.1 KB, has the limit raised)
        if (const int rc = driverCreateFlat(h, kWorldDriver, static_cast<size_t>(ok_world_offsets(s).total), {kernelOf(okWorldLatentKernel)},
                                            {grown(h->world_ws, pl.words)}))
            return rc;
        OK_HIP(h, hipMemsetAsync(h->world_ws.d + pl.fitness, 0, sizeof(float) * static_cast<size_t>(h->shape.N), h->stream));
        h->world        = *config;
        h->world_drv.ok = true;
        return OKENV_OK;
    }

    int okenv_world_num_params(okenv_t h, int32_t *encoder, int32_t *controller)
    {
        OK_QUIESCE(h);
        return flatNumParams(h, kWorldDriver, encoder, controller);
    }

    int okenv_world_set_params(okenv_t h, int32_t which, const float *params)
    {
        OK_QUIESCE(h);
        return flatSetParams(h, kWorldDriver, which, params);
    }

    int okenv_world_get_params(okenv_t h, int32_t which, float *params)
    {
        OK_QUIESCE(h);
        return flatGetParams(h, kWorldDriver, which, params);
    }

    int okenv_world_act(okenv_t h, const uint8_t *frames, int64_t frame_bytes, const okenv_world_record *rec)
    {
        OK_QUIESCE(h);
        return worldAct(h, frames, frame_bytes, rec, ~0U);
    }

    int okenv_debug_world_stages(okenv_t h, const uint8_t *frames, int64_t frame_bytes, const okenv_world_record *rec, uint32_t stages)
    {
        OK_QUIESCE(h);
        return worldAct(h, frames, frame_bytes, rec, stages);
    }

    int okenv_world_set_lane_widths(okenv_t h, const float *w_left, const float *w_right, int32_t num_points)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kWorldDriver, "set_lane_widths", kGateArgFirst | kGateCreated, w_left != nullptr && w_right != nullptr))
            return rc;
        if (num_points < 1 || num_points != h->P)
            return driverRefuses(h, OKENV_ERR_INVALID, kWorldDriver, "set_lane_widths", "num_points is not the centre line's (okenv_set_centerline)");
        h->world_widths = false;
        if (const int rc = regrow(h, {fresh(h->d_world_widths, 2U * static_cast<size_t>(num_points))}))
            return rc;
        const size_t bytes = sizeof(float) * static_cast<size_t>(num_points);
        int          rc    = copyAny(h, h->d_world_widths, w_left, bytes);
        if (rc == OKENV_OK)
            rc = copyAny(h, h->d_world_widths + num_points, w_right, bytes);
        h->world_widths = rc == OKENV_OK;
        return rc;
    }

    int okenv_world_score_begin(okenv_t h)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kWorldDriver, "score_begin", kGateHandle | kGateCreated))
            return rc;
        const size_t at = okWorldPlaces(okWorldShape(h->world), static_cast<size_t>(h->shape.N)).fitness;
        OK_HIP(h, hipMemsetAsync(h->world_ws.d + at, 0, sizeof(float) * static_cast<size_t>(h->shape.N), h->stream));
        return OKENV_OK;
    }

    int okenv_world_score(okenv_t h)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kWorldDriver, "score", kGateHandle | kGateCreated))
            return rc;
        if (!h->world_widths || h->P < 1)
            return driverRefuses(h, OKENV_ERR_STATE, kWorldDriver, "score", "call okenv_world_set_lane_widths first");
        OK_HIP(h, hipSetDevice(h->device));
        const size_t at = okWorldPlaces(okWorldShape(h->world), static_cast<size_t>(h->shape.N)).fitness;
        hipLaunchKernelGGL(okWorldScoreKernel, dim3((h->shape.N + 255) / 256), dim3(256), 0, h->stream, h->st, h->shape.N, h->d_cx, h->d_cy,
                           h->d_world_widths, h->d_world_widths + h->P, h->P, h->world_ws.d + at);
        OK_HIP(h, hipGetLastError());
        return OKENV_OK;
    }

    int okenv_world_fitness(okenv_t h, float *out)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kWorldDriver, "fitness", kGateArgFirst | kGateCreated, out != nullptr))
            return rc;
        const size_t at = okWorldPlaces(okWorldShape(h->world), static_cast<size_t>(h->shape.N)).fitness;
        return driverGet(h, {vectorOf(h->world_ws.d + at, out, h->shape.N)});
    }

    int okenv_world_fitness_device(okenv_t h, float **ptr)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kWorldDriver, "fitness_device", kGateArgFirst | kGateCreated, ptr != nullptr))
            return rc;
        *ptr = h->world_ws.d + okWorldPlaces(okWorldShape(h->world), static_cast<size_t>(h->shape.N)).fitness;
        return OKENV_OK;
    }

    int okenv_world_act_host(const okenv_world_config *config, const float *encoder, const float *controllers, int32_t n, const uint8_t *frames,
                             const float *rot, const uint8_t *crashed, float *mu, float *state, float *out, float *throttle, float *steer,
                             uint8_t *alive)
    {
        if (const char *why = okWorldCheckConfig(config))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_world_act_host: ") + why);
        if (!encoder || !controllers || n < 0 || !frames || !rot)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_world_act_host: bad argument");
        okWorldActHost(*config, encoder, controllers, n, frames, rot, crashed, mu, state, out, throttle, steer, alive);
        return OKENV_OK;
    }

    int okenv_world_score_host(const float *cx, const float *cy, const float *w_left, const float *w_right, int32_t num_points, int32_t n,
                               const float *x, const float *y, const uint8_t *crashed, const uint8_t *timed_out, float *fitness)
    {
        if (!cx || !cy || !w_left || !w_right || num_points < 1 || n < 0 || !x || !y || !crashed || !timed_out || !fitness)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_world_score_host: bad argument");
        okWorldScoreHost(cx, cy, w_left, w_right, num_points, n, x, y, crashed, timed_out, fitness);
        return OKENV_OK;
    }

    // ---- The racers' memory (ok_memory.h) -----------------------------------------------------------------------------------------

    int64_t okenv_memory_lds_bytes(const okenv_world_config *world, const okenv_memory_config *config)
    {
        return okMemoryCheckConfig(world, config) == nullptr ? static_cast<int64_t>(okMemoryLdsBytes(okMemoryShape(*world, *config))) : 0;
    }

    int okenv_memory_plan(const okenv_world_config *world, const okenv_memory_config *config, int32_t *plan)
    {
        if (const char *why = okMemoryCheckConfig(world, config))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_memory_plan: ") + why);
        if (!plan)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_memory_plan: bad argument");
        okMemoryPlan(okMemoryShape(*world, *config), plan);
        return OKENV_OK;
    }

    int64_t okenv_memory_workspace_bytes(const okenv_world_config *world, const okenv_memory_config *config, int32_t num_agents)
    {
        if (okMemoryCheckConfig(world, config) != nullptr || num_agents < 1)
            return 0;
        const ok_memory_shape s = okMemoryShape(*world, *config);
        return static_cast<int64_t>(sizeof(float) * (okMemoryPlaces(s, static_cast<size_t>(num_agents)).words + static_cast<size_t>(ok_memory_offsets(s).total)));
    }

    int okenv_memory_create(okenv_t h, const okenv_memory_config *config)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kMemoryDriver, "create", kGateHandle))
            return rc;
        if (!h->world_drv.ok)
            return driverRefuses(h, OKENV_ERR_STATE, kMemoryDriver, "create", "call okenv_world_create first");
        if (const char *why = okMemoryCheckConfig(&h->world, config))
            return driverRefuses(h, OKENV_ERR_INVALID, kMemoryDriver, "create", why);
        const ok_memory_shape s = okMemoryShape(h->world, *config);
        const OkMemoryPlaces pl = okMemoryPlaces(s, static_cast<size_t>(h->shape.N));
        h->mem_learn_ok         = false; // (the learner belongs to the memory that goes)
        if (const int rc = driverCreateFlat(h, kMemoryDriver, static_cast<size_t>(ok_memory_offsets(s).total), {kernelOf(okMemoryLayerKernel)},
                                            {grown(h->mem_ws, pl.words)}))
            return rc;
        OK_HIP(h, hipMemsetAsync(h->mem_ws.d + pl.hidden, 0, sizeof(float) * static_cast<size_t>(h->shape.N) * s.L * s.H, h->stream));
        h->mem        = *config;
        h->mem_drv.ok = true;
        return OKENV_OK;
    }

    int okenv_memory_num_params(okenv_t h, int32_t *network, int32_t *controller)
    {
        OK_QUIESCE(h);
        return flatNumParams(h, kMemoryDriver, network, controller);
    }

    int okenv_memory_set_params(okenv_t h, int32_t which, const float *params)
    {
        OK_QUIESCE(h);
        return flatSetParams(h, kMemoryDriver, which, params);
    }

    int okenv_memory_get_params(okenv_t h, int32_t which, float *params)
    {
        OK_QUIESCE(h);
        return flatGetParams(h, kMemoryDriver, which, params);
    }

    int okenv_memory_reset(okenv_t h)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kMemoryDriver, "reset", kGateHandle | kGateCreated))
            return rc;
        OK_HIP(h, hipSetDevice(h->device));
        const ok_memory_shape s     = memoryShape(h);
        const long            words = static_cast<long>(h->shape.N) * s.L * s.H;
        hipLaunchKernelGGL(okMemoryResetKernel, dim3(static_cast<unsigned>((words + 255) / 256)), dim3(256), 0, h->stream,
                           h->mem_ws.d + okMemoryPlaces(s, static_cast<size_t>(h->shape.N)).hidden, words);
        OK_HIP(h, hipGetLastError());
        return OKENV_OK;
    }

    int okenv_memory_set_hidden(okenv_t h, const float *hidden)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kMemoryDriver, "set_hidden", kGateArgFirst | kGateCreated, hidden != nullptr))
            return rc;
        OK_HIP(h, hipSetDevice(h->device));
        const ok_memory_shape s = memoryShape(h);
        return copyAny(h, h->mem_ws.d + okMemoryPlaces(s, static_cast<size_t>(h->shape.N)).hidden, hidden,
                       sizeof(float) * static_cast<size_t>(h->shape.N) * s.L * s.H);
    }

    int okenv_memory_get_hidden(okenv_t h, float *hidden)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kMemoryDriver, "get_hidden", kGateArgFirst | kGateCreated, hidden != nullptr))
            return rc;
        const ok_memory_shape s = memoryShape(h);
        return driverGet(h, {vectorOf(h->mem_ws.d + okMemoryPlaces(s, static_cast<size_t>(h->shape.N)).hidden, hidden, h->shape.N * s.L * s.H)});
    }

    int okenv_memory_act(okenv_t h, const uint8_t *frames, int64_t frame_bytes, const okenv_memory_record *rec)
    {
        OK_QUIESCE(h);
        return memoryAct(h, frames, frame_bytes, rec, ~0U);
    }

    int okenv_debug_memory_stages(okenv_t h, const uint8_t *frames, int64_t frame_bytes, const okenv_memory_record *rec, uint32_t stages)
    {
        OK_QUIESCE(h);
        return memoryAct(h, frames, frame_bytes, rec, stages);
    }

    int okenv_memory_act_host(const okenv_world_config *world, const okenv_memory_config *config, const float *encoder, const float *network,
                              const float *controllers, int32_t n, const uint8_t *frames, const uint8_t *crashed, float *hidden, float *throttle,
                              float *steer, const okenv_memory_record *rec)
    {
        if (const char *why = okMemoryCheckConfig(world, config))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_memory_act_host: ") + why);
        if (!encoder || !network || !controllers || n < 0 || !frames || !hidden || !throttle || !steer)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_memory_act_host: bad argument");
        if (ok_memory_params_bad(okMemoryShape(*world, *config), network))
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_memory_act_host: the network vector holds a non-finite value or a std that is not > 0");
        okMemoryActHost(*world, *config, encoder, network, controllers, n, frames, crashed, hidden, throttle, steer, rec != nullptr ? *rec : okenv_memory_record{});
        return OKENV_OK;
    }

    // ---- The memory's training (ok_memtrain.h) ------------------------------------------------------------------------------------

    int64_t okenv_memory_learner_workspace_bytes(const okenv_world_config *world, const okenv_memory_config *config, const okenv_memory_learner_config *learner)
    {
        if (okMemoryCheckConfig(world, config) != nullptr || okMemTrainCheckConfig(learner) != nullptr)
            return 0;
        return static_cast<int64_t>(sizeof(float) * okMemTrainPlaces(okMemoryShape(*world, *config), learner->seq_len, learner->max_batch).words);
    }

    int64_t okenv_memory_learner_lds_bytes(const okenv_world_config *world, const okenv_memory_config *config)
    {
        return okMemoryCheckConfig(world, config) == nullptr ? static_cast<int64_t>(okMemTrainLdsBytes(okMemoryShape(*world, *config))) : 0;
    }

    int okenv_memory_learner_create(okenv_t h, const okenv_memory_learner_config *config)
    {
        OK_QUIESCE(h);
        if (!h)
            return fail(h, OKENV_ERR_INVALID, "okenv_memory_learner_create: NULL handle");
        if (const char *why = okMemTrainCheckConfig(config))
            return fail(h, OKENV_ERR_INVALID, std::string("okenv_memory_learner_create: ") + why);
        if (!h->mem_drv.ok || !h->mem_drv.set[0])
            return fail(h, OKENV_ERR_STATE, "okenv_memory_learner_create: needs a memory whose network has its parameters (okenv_memory_create, okenv_memory_set_params)");
        OK_HIP(h, hipSetDevice(h->device));
        h->mem_learn_ok = false;
        const OkMemTrainPlaces pl = okMemTrainPlaces(memoryShape(h), config->seq_len, config->max_batch);
        if (okMemTrainLdsBytes(memoryShape(h)) > kLidarLdsBudget)
            return fail(h, OKENV_ERR_INVALID, "okenv_memory_learner_create: the kernels' LDS (okenv_memory_learner_lds_bytes) does not fit 160 KB");
        if (const int rc = growBuffers(h, {grown(h->mem_learn_ws, pl.words)}))
            return rc;
        // (everything: the moments, the step number, and the rows of zeros in front of every layer's hidden states)
        OK_HIP(h, hipMemsetAsync(h->mem_learn_ws.d, 0, h->mem_learn_ws.cap * sizeof(float), h->stream));
        h->mem_learn    = *config;
        h->mem_learn_ok = true;
        return OKENV_OK;
    }

    int okenv_memory_learner_reset(okenv_t h)
    {
        OK_QUIESCE(h);
        if (!h || !h->mem_drv.ok || !h->mem_learn_ok)
            return fail(h, OKENV_ERR_STATE, "okenv_memory_learner_reset: call okenv_memory_learner_create first");
        OK_HIP(h, hipSetDevice(h->device));
        const OkMemTrainPlaces pl = okMemTrainPlaces(memoryShape(h), h->mem_learn.seq_len, h->mem_learn.max_batch);
        // [scalars | m | v] lie together at the workspace's start
        OK_HIP(h, hipMemsetAsync(h->mem_learn_ws.d, 0, sizeof(float) * pl.grad, h->stream));
        return OKENV_OK;
    }

    int okenv_memory_learner_get_state(okenv_t h, okenv_memory_learner_state *out)
    {
        OK_QUIESCE(h);
        if (!h || !out)
            return fail(h, OKENV_ERR_INVALID, "okenv_memory_learner_get_state: NULL argument");
        if (!h->mem_drv.ok || !h->mem_learn_ok)
            return fail(h, OKENV_ERR_STATE, "okenv_memory_learner_get_state: call okenv_memory_learner_create first");
        const ok_memory_shape  s  = memoryShape(h);
        const OkMemTrainPlaces pl = okMemTrainPlaces(s, h->mem_learn.seq_len, h->mem_learn.max_batch);
        const int              T = ok_memtrain_trainable(s);
        float                 *ws = h->mem_learn_ws.d;
        if (const int rc = driverGet(h, {vectorOf(h->mem_drv.d, out->params, ok_memory_offsets(s).total), vectorOf(ws + pl.m, out->m, T), vectorOf(ws + pl.v, out->v, T)}))
            return rc;
        long long t = 0;
        OK_HIP(h, hipMemcpyAsync(&t, ws + pl.scalars + kMemTrainStepAt, sizeof(t), hipMemcpyDeviceToHost, h->stream));
        OK_HIP(h, hipStreamSynchronize(h->stream));
        out->t = static_cast<int64_t>(t);
        return OKENV_OK;
    }

    int okenv_memory_update(okenv_t h, const float *latent, const float *action, int32_t rows, const int32_t *start, int32_t M, int32_t stride, int32_t B,
                            int32_t epochs, const int32_t *order, const float *lr_schedule, const okenv_memory_learner_output *out)
    {
        OK_QUIESCE(h);
        return memoryLearnRun(h, "okenv_memory_update", true, latent, action, rows, start, M, stride, B, epochs, order, lr_schedule,
                              out != nullptr ? out->loss : nullptr, out != nullptr ? out->norm : nullptr, out != nullptr ? out->grad : nullptr);
    }

    int okenv_memory_eval(okenv_t h, const float *latent, const float *action, int32_t rows, const int32_t *start, int32_t M, int32_t stride, int32_t B, float *loss)
    {
        OK_QUIESCE(h);
        if (h != nullptr && h->mem_learn_ok && loss == nullptr)
            return fail(h, OKENV_ERR_INVALID, "okenv_memory_eval: NULL argument");
        return memoryLearnRun(h, "okenv_memory_eval", false, latent, action, rows, start, M, stride, B, 1, nullptr, nullptr, loss, nullptr, nullptr);
    }

    int okenv_memory_update_host(const okenv_world_config *world, const okenv_memory_config *config, const okenv_memory_learner_config *learner,
                                 okenv_memory_learner_state *state, const float *latent, const float *action, int32_t rows, const int32_t *start, int32_t M,
                                 int32_t stride, int32_t B, int32_t epochs, const int32_t *order, const float *lr_schedule, const okenv_memory_learner_output *out)
    {
        if (const char *why = okMemoryCheckConfig(world, config))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_memory_update_host: ") + why);
        if (const char *why = okMemTrainCheckConfig(learner))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_memory_update_host: ") + why);
        if (const char *why = okMemTrainCheckCall(latent, action, rows, start, M, B, epochs))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_memory_update_host: ") + why);
        if (std::min(B, M) > learner->max_batch)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_memory_update_host: a minibatch of min(B, M) windows is beyond the learner's max_batch");
        if (!state || !state->params || !state->m || !state->v || state->t < 0)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_memory_update_host: state is NULL, lacks a parameter or moment vector (NULL argument), or t < 0");
        const ok_memory_shape s = okMemoryShape(*world, *config);
        if (ok_memory_params_bad(s, state->params))
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_memory_update_host: the network vector holds a non-finite value or a std that is not > 0");
        const okenv_memory_learner_output none{};
        okMemTrainUpdateHost(*learner, s, *state, latent, action, rows, start, M, stride, B, epochs, order, lr_schedule, out != nullptr ? *out : none);
        return OKENV_OK;
    }

    int okenv_memory_eval_host(const okenv_world_config *world, const okenv_memory_config *config, const okenv_memory_learner_config *learner, const float *network,
                               const float *latent, const float *action, int32_t rows, const int32_t *start, int32_t M, int32_t stride, int32_t B, float *loss)
    {
        if (const char *why = okMemoryCheckConfig(world, config))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_memory_eval_host: ") + why);
        if (const char *why = okMemTrainCheckConfig(learner))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_memory_eval_host: ") + why);
        if (const char *why = okMemTrainCheckCall(latent, action, rows, start, M, B, 1))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_memory_eval_host: ") + why);
        if (!network || !loss)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_memory_eval_host: NULL argument");
        const ok_memory_shape s = okMemoryShape(*world, *config);
        if (ok_memory_params_bad(s, network))
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_memory_eval_host: the network vector holds a non-finite value or a std that is not > 0");
        okMemTrainEvalHost(s, learner->seq_len, network, latent, action, rows, start, M, stride, B, loss);
        return OKENV_OK;
    }

    int okenv_memory_window_host(const okenv_world_config *world, const okenv_memory_config *config, const float *network, const float *latent, const float *action,
                                 int32_t rows, int32_t start, int32_t stride, int32_t seq_len, float *hidden, float *zn)
    {
        if (const char *why = okMemoryCheckConfig(world, config))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_memory_window_host: ") + why);
        if (!network || !latent || !action || rows < 1 || seq_len < 1 || seq_len > OK_MEMTRAIN_MAX_SEQ || !hidden || !zn)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_memory_window_host: bad argument");
        const ok_memory_shape s = okMemoryShape(*world, *config);
        if (ok_memory_params_bad(s, network))
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_memory_window_host: the network vector holds a non-finite value or a std that is not > 0");
        OkMemTrainSaved sv;
        okMemTrainForwardHost(s, network, latent, action, rows, stride, seq_len, std::vector<int>{start}, sv);
        for (int st = 0; st < seq_len; ++st)
            for (int l = 0; l < s.L; ++l)
                std::copy(sv.h.begin() + (static_cast<long>(l) * seq_len + st) * s.H, sv.h.begin() + (static_cast<long>(l) * seq_len + st + 1) * s.H,
                          hidden + (static_cast<long>(st) * s.L + l) * s.H);
        std::copy(sv.zn.begin(), sv.zn.end(), zn);
        return OKENV_OK;
    }

    // ---- Deep-Q image racers (ok_qcnn.h) ---------------------------------------------------------------------------------------------

    int64_t okenv_qcnn_lds_bytes(const okenv_qcnn_config *config)
    {
        return config != nullptr ? static_cast<int64_t>(okQcnnLdsBytes(okQcnnShape(*config))) : 0;
    }

    int okenv_qcnn_plan(const okenv_qcnn_config *config, int32_t *plan)
    {
        if (const char *why = okQcnnCheckConfig(config))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_qcnn_plan: ") + why);
        if (!plan)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_qcnn_plan: bad argument");
        const OkQcnnPlaces pl = okQcnnPlaces(okQcnnShape(*config));
        plan[0] = pl.ct;
        plan[1] = pl.region;
        plan[2] = pl.vec;
        return OKENV_OK;
    }

    int okenv_qcnn_create(okenv_t h, const okenv_qcnn_config *config)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kQcnnDriver, "create", kGateHandle))
            return rc;
        if (const char *why = okQcnnCheckConfig(config))
            return driverRefuses(h, OKENV_ERR_INVALID, kQcnnDriver, "create", why);
        const ok_qcnn_shape s = okQcnnShape(*config);
        if (const int rc = driverCreateFlat(h, kQcnnDriver, static_cast<size_t>(ok_qcnn_offsets(s).total),
                                            {kernelOf(okQcnnConvKernel), kernelOf(okQcnnHeadKernel<1, 1>), kernelOf(okQcnnHeadKernel<2, 1>),
                                             kernelOf(okQcnnHeadKernel<3, 1>), kernelOf(okQcnnHeadKernel<4, 1>), kernelOf(okQcnnHeadKernel<1, 2>),
                                             kernelOf(okQcnnHeadKernel<2, 2>), kernelOf(okQcnnHeadKernel<3, 2>), kernelOf(okQcnnHeadKernel<4, 2>)},
                                            {grown(h->qcnn_pack, static_cast<size_t>(okQcnnPlaces(s).pack_total)),
                                             grown(h->qcnn_feat, static_cast<size_t>(h->shape.N) * ok_qcnn_features(s))}))
            return rc;
        if (h->qcnn_ring.ok && h->qcnn_ring_side != config->image_size)
            h->qcnn_ring.ok = false; // (its planes had the earlier network's size)
        h->qcnn        = *config;
        h->qcnn_drv.ok = true;
        return OKENV_OK;
    }

    int okenv_qcnn_num_params(okenv_t h, int32_t *num_params)
    {
        OK_QUIESCE(h);
        return flatNumParams(h, kQcnnDriver, num_params);
    }

    int okenv_qcnn_set_params(okenv_t h, const float *params)
    {
        OK_QUIESCE(h);
        return flatSetParams(h, kQcnnDriver, 0, params);
    }

    int okenv_qcnn_get_params(okenv_t h, float *params)
    {
        OK_QUIESCE(h);
        return flatGetParams(h, kQcnnDriver, 0, params);
    }

    int okenv_qcnn_set_epsilon(okenv_t h, float epsilon)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kQcnnDriver, "set_epsilon", kGateCreated))
            return rc;
        if (!(epsilon >= 0.F && epsilon <= 1.F))
            return driverRefuses(h, OKENV_ERR_INVALID, kQcnnDriver, "set_epsilon", "epsilon outside [0, 1]");
        h->qcnn.epsilon = epsilon;
        return OKENV_OK;
    }

    int okenv_qcnn_set_draw_offset(okenv_t h, const uint32_t *device_word)
    {
        OK_QUIESCE(h);
        return driverSetDrawOffset(h, kQcnnDriver, device_word);
    }

    int okenv_qcnn_act(okenv_t h, const uint8_t *frames, int64_t frame_bytes, const okenv_qcnn_record *rec)
    {
        OK_QUIESCE(h);
        return qcnnAct(h, frames, frame_bytes, rec, OKENV_QCNN_STAGE_CONV | OKENV_QCNN_STAGE_HEAD);
    }

    int okenv_debug_qcnn_stages(okenv_t h, const uint8_t *frames, int64_t frame_bytes, const okenv_qcnn_record *rec, uint32_t stages)
    {
        OK_QUIESCE(h);
        return qcnnAct(h, frames, frame_bytes, rec, stages);
    }

    int okenv_qcnn_ring_create(okenv_t h, int32_t capacity, uint32_t flags)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kQcnnDriver, "ring_create", kGateHandle | kGateCreated))
            return rc;
        if (const char *why = okReplayCheckCreate(capacity, flags))
            return driverRefuses(h, OKENV_ERR_INVALID, kQcnnDriver, "ring_create", why);
        OkRing &r = h->qcnn_ring;
        OK_HIP(h, hipSetDevice(h->device));
        r.ok = false;
        const size_t C = static_cast<size_t>(capacity), px = static_cast<size_t>(h->qcnn.image_size) * static_cast<size_t>(h->qcnn.image_size);
        const size_t blocks = (static_cast<size_t>(h->shape.N) + kReplayThreads - 1U) / kReplayThreads;
        // (the wait: nobody is still working in an earlier ring)
        int rc = regrow(h, {fresh(r.state, C * px), fresh(r.next_state, C * px), fresh(r.action, C * r.action_bytes), fresh(r.reward, C), fresh(r.done, C)});
        if (rc != OKENV_OK || (rc = devEnsure(h, &r.d_words, 2)) != OKENV_OK || (rc = devEnsure(h, &r.d_counts, blocks)) != OKENV_OK ||
            (rc = devEnsure(h, &h->d_qcnn_slots, static_cast<size_t>(h->shape.N))) != OKENV_OK)
            return rc;
        OK_HIP(h, hipMemsetAsync(r.d_words, 0, 2U * sizeof(uint64_t), h->stream));
        OK_HIP(h, hipStreamSynchronize(h->stream));
        r.capacity        = capacity;
        r.flags           = flags;
        r.ok              = true;
        h->qcnn_ring_side = h->qcnn.image_size;
        return OKENV_OK;
    }

    int okenv_qcnn_ring_reset(okenv_t h)
    {
        OK_QUIESCE(h);
        if (!h || !h->qcnn_ring.ok)
            return driverRefuses(h, OKENV_ERR_STATE, kQcnnDriver, "ring_reset", "call okenv_qcnn_ring_create first");
        OK_HIP(h, hipSetDevice(h->device));
        OK_HIP(h, hipMemsetAsync(h->qcnn_ring.d_words, 0, 2U * sizeof(uint64_t), h->stream));
        return OKENV_OK;
    }

    int okenv_qcnn_ring_size(okenv_t h, int64_t *size, int64_t *pushed)
    {
        OK_QUIESCE(h);
        if (!h || !h->qcnn_ring.ok)
            return driverRefuses(h, OKENV_ERR_STATE, kQcnnDriver, "ring_size", "call okenv_qcnn_ring_create first");
        OK_HIP(h, hipSetDevice(h->device));
        uint64_t word = 0;
        OK_HIP(h, hipMemcpyAsync(&word, h->qcnn_ring.d_words, sizeof(word), hipMemcpyDeviceToHost, h->stream));
        OK_HIP(h, hipStreamSynchronize(h->stream));
        if (size)
            *size = static_cast<int64_t>(ok_dqn_size(word, static_cast<uint64_t>(h->qcnn_ring.capacity)));
        if (pushed)
            *pushed = static_cast<int64_t>(word);
        return OKENV_OK;
    }

    int okenv_qcnn_ring_get(okenv_t h, const okenv_qcnn_ring *out)
    {
        OK_QUIESCE(h);
        if (!h || !out)
            return driverRefuses(h, OKENV_ERR_INVALID, kQcnnDriver, "ring_get", "NULL argument");
        const OkRing &r = h->qcnn_ring;
        if (!r.ok)
            return driverRefuses(h, OKENV_ERR_STATE, kQcnnDriver, "ring_get", "call okenv_qcnn_ring_create first");
        OK_HIP(h, hipSetDevice(h->device));
        const size_t C = static_cast<size_t>(r.capacity), px = static_cast<size_t>(h->qcnn_ring_side) * static_cast<size_t>(h->qcnn_ring_side);
        void *const       dst[5]   = {out->state, out->next_state, out->action, out->reward, out->done};
        const void *const src[5]   = {r.state, r.next_state, r.action, r.reward, r.done};
        const size_t      bytes[5] = {C * px * sizeof(float), C * px * sizeof(float), C * r.action_bytes, C * sizeof(float), C * sizeof(float)};
        for (int i = 0; i < 5; ++i)
            if (dst[i] != nullptr)
                if (const int rc = copyAny(h, dst[i], src[i], bytes[i]))
                    return rc;
        OK_HIP(h, hipStreamSynchronize(h->stream));
        return OKENV_OK;
    }

    int okenv_qcnn_push(okenv_t h, const okenv_qcnn_record *rec, const uint8_t *frames, const uint8_t *next_frames, int64_t frame_bytes,
                        const float *reward)
    {
        OK_QUIESCE(h);
        if (!h)
            return driverRefuses(h, OKENV_ERR_INVALID, kQcnnDriver, "push", "NULL handle");
        const OkRing &r = h->qcnn_ring;
        if (!h->qcnn_drv.ok || !r.ok)
            return driverRefuses(h, OKENV_ERR_STATE, kQcnnDriver, "push", "call okenv_qcnn_ring_create first");
        if (!rec || !rec->action)
            return driverRefuses(h, OKENV_ERR_INVALID, kQcnnDriver, "push", "the record needs action");
        if (!rec->alive && (r.flags & OKENV_REPLAY_PUSH_ALL) == 0U)
            return driverRefuses(h, OKENV_ERR_INVALID, kQcnnDriver, "push", "the record needs alive (or create the ring with OKENV_REPLAY_PUSH_ALL)");
        for (const uint8_t *f : {frames, next_frames})
            if (const char *missing = qcnnFramesMissing(h, f, frame_bytes))
                return driverRefuses(h, OKENV_ERR_INVALID, kQcnnDriver, "push", missing);
        OK_HIP(h, hipSetDevice(h->device));
        OkQcnnPushParams p{};
        p.N           = h->shape.N;
        p.R           = h->shape.R;
        p.S           = h->qcnn.image_size;
        p.flags       = r.flags;
        p.capacity    = static_cast<uint64_t>(r.capacity);
        p.ring        = okenv_qcnn_ring{r.state, r.next_state, reinterpret_cast<int64_t *>(r.action), r.reward, r.done};
        p.pushed      = r.d_words;
        p.snapshot    = r.d_words + 1;
        p.counts      = r.d_counts;
        p.slots       = h->d_qcnn_slots;
        p.rec         = *rec;
        p.frames      = frames;
        p.next_frames = next_frames;
        p.crashed     = h->st.crashed;
        p.dist        = h->st.dist;
        p.reward      = reward;
        const unsigned blocks = static_cast<unsigned>((h->shape.N + kReplayThreads - 1) / kReplayThreads);
        hipLaunchKernelGGL(okReplayCountKernel<OkQcnnPushParams>, dim3(blocks), dim3(kReplayThreads), 0, h->stream, p);
        OK_HIP(h, hipGetLastError());
        hipLaunchKernelGGL(okQcnnRankKernel, dim3(blocks), dim3(kReplayThreads), 0, h->stream, p);
        OK_HIP(h, hipGetLastError());
        const bool     vec    = okQcnnPlaces(okQcnnShape(h->qcnn)).vec != 0;
        const unsigned pieces = static_cast<unsigned>((p.S * p.S / (vec ? 4 : 1) + kQcnnCopyThreads - 1) / kQcnnCopyThreads);
        hipLaunchKernelGGL(vec ? okQcnnFramesKernel<true> : okQcnnFramesKernel<false>, dim3(static_cast<unsigned>(p.N), pieces), dim3(kQcnnCopyThreads), 0,
                           h->stream, p);
        OK_HIP(h, hipGetLastError());
        return OKENV_OK;
    }

    int okenv_qcnn_batch(okenv_t h, int32_t B, int32_t mode, int64_t start_or_draw, const okenv_qcnn_batch_out *out)
    {
        OK_QUIESCE(h);
        if (!h)
            return driverRefuses(h, OKENV_ERR_INVALID, kQcnnDriver, "batch", "NULL handle");
        const OkRing &r = h->qcnn_ring;
        if (!h->qcnn_drv.ok || !r.ok)
            return driverRefuses(h, OKENV_ERR_STATE, kQcnnDriver, "batch", "call okenv_qcnn_ring_create first");
        if (!out || B < 1 || start_or_draw < 0 || (mode != OKENV_QCNN_BATCH_UNIFORM && mode != OKENV_QCNN_BATCH_SEQUENTIAL))
            return driverRefuses(h, OKENV_ERR_INVALID, kQcnnDriver, "batch", "out must not be NULL, B at least 1, start_or_draw at least 0, mode OKENV_QCNN_BATCH_UNIFORM or _SEQUENTIAL");
        const bool vec = okQcnnPlaces(okQcnnShape(h->qcnn)).vec != 0;
        if (vec && (reinterpret_cast<uintptr_t>(out->state) % 16U != 0U || reinterpret_cast<uintptr_t>(out->next_state) % 16U != 0U))
            return driverRefuses(h, OKENV_ERR_INVALID, kQcnnDriver, "batch", "state and next_state must be 16-byte aligned");
        OK_HIP(h, hipSetDevice(h->device));
        OkQcnnBatchParams p{};
        p.S             = h->qcnn.image_size;
        p.B             = B;
        p.mode          = mode;
        p.seed          = h->qcnn.seed;
        p.capacity      = static_cast<uint64_t>(r.capacity);
        p.start_or_draw = static_cast<uint64_t>(start_or_draw);
        p.pushed        = r.d_words;
        p.ring          = okenv_qcnn_ring{r.state, r.next_state, reinterpret_cast<int64_t *>(r.action), r.reward, r.done};
        p.out           = *out;
        const unsigned pieces = static_cast<unsigned>((p.S * p.S / (vec ? 4 : 1) + kQcnnCopyThreads - 1) / kQcnnCopyThreads);
        hipLaunchKernelGGL(vec ? okQcnnBatchKernel<true> : okQcnnBatchKernel<false>, dim3(static_cast<unsigned>(B), pieces), dim3(kQcnnCopyThreads), 0,
                           h->stream, p);
        OK_HIP(h, hipGetLastError());
        return OKENV_OK;
    }

    int okenv_qcnn_act_host(const okenv_qcnn_config *config, const float *params, int32_t n, const uint8_t *frames, const uint8_t *crashed,
                            uint32_t draw_index, float *throttle, float *steer, float *q, int64_t *action, float *value, uint8_t *alive)
    {
        if (const char *why = okQcnnCheckConfig(config))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_qcnn_act_host: ") + why);
        if (!params || n < 0 || !frames)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_qcnn_act_host: bad argument");
        okQcnnActHost(*config, params, n, frames, crashed, draw_index, throttle, steer, q, action, value, alive);
        return OKENV_OK;
    }

    int okenv_qcnn_push_host(const okenv_qcnn_ring *ring, int32_t capacity, int32_t image_size, uint64_t *pushed, uint32_t flags, int32_t n,
                             const int64_t *action, const uint8_t *alive, const uint8_t *frames, const uint8_t *next_frames, const uint8_t *crashed,
                             const float *reward, const float *dist, int32_t num_rays)
    {
        if (const char *why = okReplayCheckCreate(capacity, flags))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_qcnn_push_host: ") + why);
        if (!okReplayRingComplete(ring) || !pushed)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_qcnn_push_host: the ring needs every field and its counter");
        if (image_size < OK_CNN_MIN_SIDE || image_size > OK_CNN_MAX_SIDE || n < 0)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_qcnn_push_host: image_size 16 .. 128 and n >= 0");
        if (!action || !frames || !next_frames || !crashed)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_qcnn_push_host: action, frames, next_frames and crashed are required");
        if (!alive && (flags & OKENV_REPLAY_PUSH_ALL) == 0U)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_qcnn_push_host: alive is required (or pass OKENV_REPLAY_PUSH_ALL)");
        if (!reward && (!dist || num_rays < 1))
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_qcnn_push_host: without reward, dist and num_rays >= 1 are required");
        ok_qcnn_push(okQcnnRing(*ring), static_cast<uint64_t>(capacity), image_size, pushed, flags, n, action, alive, frames, next_frames, crashed, reward,
                     dist, num_rays);
        return OKENV_OK;
    }

    int okenv_qcnn_batch_host(const okenv_qcnn_ring *ring, int32_t capacity, int32_t image_size, uint64_t pushed, uint32_t seed, int32_t B, int32_t mode,
                              int64_t start_or_draw, const okenv_qcnn_batch_out *out)
    {
        if (!okReplayRingComplete(ring) || !out || capacity < 1 || B < 1 || start_or_draw < 0 || image_size < OK_CNN_MIN_SIDE ||
            image_size > OK_CNN_MAX_SIDE || (mode != OKENV_QCNN_BATCH_UNIFORM && mode != OKENV_QCNN_BATCH_SEQUENTIAL))
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_qcnn_batch_host: bad argument");
        const ok_qcnn_batch_out o{out->state, out->next_state, out->action, out->reward, out->done, out->index};
        ok_qcnn_batch(okQcnnRing(*ring), static_cast<uint64_t>(capacity), image_size, pushed, seed, B, mode, static_cast<uint64_t>(start_or_draw), o);
        return OKENV_OK;
    }

    int okenv_debug_qcnn_grey_host(int32_t image_size, int32_t n, const uint8_t *frames, float *planes)
    {
        if (image_size < 1 || n < 0 || !frames || !planes)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_debug_qcnn_grey_host: bad argument");
        const size_t px = static_cast<size_t>(image_size) * static_cast<size_t>(image_size);
        for (int a = 0; a < n; ++a)
            ok_qcnn_grey_plane(image_size, frames + static_cast<size_t>(a) * px * 4U, planes + static_cast<size_t>(a) * px);
        return OKENV_OK;
    }

    int okenv_debug_qcnn_forward_planes_host(const okenv_qcnn_config *config, const float *params, int32_t n, const float *planes, float *q)
    {
        if (const char *why = okQcnnCheckConfig(config))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_debug_qcnn_forward_planes_host: ") + why);
        if (!params || n < 0 || !planes || !q)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_debug_qcnn_forward_planes_host: bad argument");
        const ok_qcnn_shape s  = okQcnnShape(*config);
        const size_t        px = static_cast<size_t>(s.S) * static_cast<size_t>(s.S);
        std::vector<float>  work(static_cast<size_t>(ok_qcnn_work_floats(s)));
        for (int a = 0; a < n; ++a)
            ok_qcnn_forward_plane(s, params, planes + static_cast<size_t>(a) * px, work.data(), q + static_cast<size_t>(a) * s.A);
        return OKENV_OK;
    }

    // ---- The flow driver's image encoder (ok_bev.h) ------------------------------------------------------------------------------

    int64_t okenv_bev_lds_bytes(const okenv_bev_config *config)
    {
        return config != nullptr ? static_cast<int64_t>(okBevLdsBytes(okBevShape(*config))) : 0;
    }

    int okenv_bev_tiles(const okenv_bev_config *config, int32_t *tiles)
    {
        if (const char *why = okBevCheckConfig(config))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_bev_tiles: ") + why);
        if (!tiles)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_bev_tiles: bad argument");
        const OkBevPlaces pl = okBevPlaces(okBevShape(*config));
        tiles[0] = pl.ta;
        tiles[1] = pl.tb;
        return OKENV_OK;
    }

    int okenv_bev_create(okenv_t h, const okenv_bev_config *config)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kBevDriver, "create", kGateHandle))
            return rc;
        if (const char *why = okBevCheckConfig(config))
            return driverRefuses(h, OKENV_ERR_INVALID, kBevDriver, "create", why);
        const ok_bev_shape s = okBevShape(*config);
        const size_t N = static_cast<size_t>(h->shape.N), side1 = static_cast<size_t>(ok_bev_side(s, 1)), side2 = static_cast<size_t>(ok_bev_side(s, 2));
        if (const int rc = driverCreateFlat(h, kBevDriver, static_cast<size_t>(ok_bev_offsets(s).total),
                                            {kernelOf(okBevFrontKernel<8>), kernelOf(okBevFrontKernel<4>), kernelOf(okBevBackKernel<8>), kernelOf(okBevBackKernel<4>)},
                                            {grown(h->bev_pack, static_cast<size_t>(okBevPlaces(s).pack_total)), grown(h->bev_act1, N * side1 * side1 * s.c[1]),
                                             grown(h->bev_act2, N * side2 * side2 * s.c[2])}))
            return rc;
        h->bev        = *config;
        h->bev_drv.ok = true;
        return OKENV_OK;
    }

    int okenv_bev_num_params(okenv_t h, int32_t *num_params)
    {
        OK_QUIESCE(h);
        return flatNumParams(h, kBevDriver, num_params);
    }

    int okenv_bev_set_params(okenv_t h, const float *params)
    {
        OK_QUIESCE(h);
        return flatSetParams(h, kBevDriver, 0, params);
    }

    int okenv_bev_get_params(okenv_t h, float *params)
    {
        OK_QUIESCE(h);
        return flatGetParams(h, kBevDriver, 0, params);
    }

    int okenv_bev_encode(okenv_t h, const uint8_t *frames, int64_t frame_bytes, float *out)
    {
        OK_QUIESCE(h);
        return bevEncode(h, frames, frame_bytes, out, OKENV_BEV_STAGE_FRONT | OKENV_BEV_STAGE_BACK | OKENV_BEV_STAGE_HEAD);
    }

    int okenv_debug_bev_stages(okenv_t h, const uint8_t *frames, int64_t frame_bytes, float *out, uint32_t stages)
    {
        OK_QUIESCE(h);
        return bevEncode(h, frames, frame_bytes, out, stages);
    }

    int okenv_bev_encode_host(const okenv_bev_config *config, const float *params, int32_t n, const uint8_t *frames, float *out)
    {
        if (const char *why = okBevCheckConfig(config))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_bev_encode_host: ") + why);
        if (!params || n < 0 || !frames || !out)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_bev_encode_host: bad argument");
        okBevEncodeHost(*config, params, n, frames, out);
        return OKENV_OK;
    }

    // ---- DDPG: continuous actor, critic, replay ring and update (ok_ddpg.h) ---------------------------------------------------

    int okenv_ddpg_create(okenv_t h, const okenv_ddpg_config *config)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kDdpgDriver, "create", kGateHandle))
            return rc;
        if (const char *why = okDdpgCheckConfig(config, h->shape.R))
            return driverRefuses(h, OKENV_ERR_INVALID, kDdpgDriver, "create", why);
        OK_HIP(h, hipSetDevice(h->device));
        // room for the widest networks, so that a later create with other widths allocates nothing
        // (a multiple of four floats, with room for the last 16-byte load: okActorStage reads whole float4s from each vector)
        const size_t cap = ((static_cast<size_t>(ok_actor_num_params(OK_ACTOR_MAX_RAYS, OK_ACTOR_MAX_HIDDEN, 2)) + 3U) & ~static_cast<size_t>(3U)) + 4U;
        if (const int rc = driverCreateFixed(h, kDdpgDriver, cap, 4, 4, true,
                                             {kernelOf(okDdpgActKernel), kernelOf(okDdpgCriticGradKernel), kernelOf(okDdpgActorGradKernel)}))
            return rc;
        h->ddpg   = *config;
        h->ddpg_t = 0;
        return OKENV_OK;
    }

    int okenv_ddpg_num_params(okenv_t h, int32_t *actor, int32_t *critic)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kDdpgDriver, "num_params", kGateCreated))
            return rc;
        if (actor)
            *actor = ddpgActorParams(h);
        if (critic)
            *critic = ddpgCriticParams(h);
        return OKENV_OK;
    }

    int okenv_ddpg_set_params(okenv_t h, const float *actor, const float *critic)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kDdpgDriver, "set_params", kGateCreated))
            return rc;
        const OkDriver    &d          = h->ddpg_drv;
        const float *const src[2]     = {actor, critic};
        const size_t       floats[2]  = {static_cast<size_t>(ddpgActorParams(h)), static_cast<size_t>(ddpgCriticParams(h))};
        if (const int rc = driverSet(h, kDdpgDriver, {vectorOf(d.d, actor, ddpgActorParams(h), 0), vectorOf(d.d + d.cap, critic, ddpgCriticParams(h), 1)}))
            return rc;
        // each online network that arrived, into its target (DDPGAgent.hpp:65-74)
        for (size_t k = 0; k < 2U; ++k)
            if (src[k] != nullptr)
                OK_HIP(h, hipMemcpyAsync(d.d + (k + 2U) * d.cap, d.d + k * d.cap, sizeof(float) * floats[k], hipMemcpyDeviceToDevice, h->stream));
        return OKENV_OK;
    }

    int okenv_ddpg_get_state(okenv_t h, okenv_ddpg_state *out)
    {
        OK_QUIESCE(h);
        if (const int rc = driverGate(h, kDdpgDriver, "get_state", kGateArgFirst | kGateStored, out != nullptr, 3U))
            return rc;
        const OkDriver &d  = h->ddpg_drv;
        const int       na = ddpgActorParams(h), nc = ddpgCriticParams(h);
        if (const int rc = driverGet(h, {vectorOf(d.d, out->actor, na), vectorOf(d.d + d.cap, out->critic, nc), vectorOf(d.d + 2U * d.cap, out->actor_target, na),
                                         vectorOf(d.d + 3U * d.cap, out->critic_target, nc), vectorOf(d.d2, out->actor_m, na),
                                         vectorOf(d.d2 + d.cap, out->actor_v, na), vectorOf(d.d2 + 2U * d.cap, out->critic_m, nc),
                                         vectorOf(d.d2 + 3U * d.cap, out->critic_v, nc)}))
            return rc;
        out->t = h->ddpg_t;
        return OKENV_OK;
    }

    int okenv_ddpg_set_draw_offset(okenv_t h, const uint32_t *device_word)
    {
        OK_QUIESCE(h);
        return driverSetDrawOffset(h, kDdpgDriver, device_word);
    }

    int okenv_ddpg_act(okenv_t h, const okenv_ddpg_record *rec)
    {
        OK_QUIESCE(h);
        if (const int rc = actBegin(h, kDdpgDriver, 1U))
            return rc;
        OkDdpgActParams p{};
        p.f     = actFrame(h);
        p.draw  = actDrawWords(h, h->ddpg_drv.draw_offset);
        p.H     = h->ddpg.hidden;
        p.actor = h->ddpg_drv.d;
        for (int k = 0; k < 2; ++k)
        {
            p.scale[k] = h->ddpg.scale[k];
            p.bias[k]  = h->ddpg.bias[k];
            p.noise[k] = h->ddpg.noise[k];
        }
        p.seed       = h->ddpg.seed;
        p.agent_base = h->ddpg.agent_base;
        if (rec != nullptr)
            p.rec = *rec;
        return actLaunch(h, okDdpgActKernel, kActorAgents, kActorThreads, okDdpgActLdsBytes(p.f.R, p.H), p);
    }

    int okenv_ddpg_replay_create(okenv_t h, int32_t capacity, uint32_t flags)
    {
        OK_QUIESCE(h);
        return ringCreate(h, kDdpgRing, capacity, flags, nullptr);
    }

    int okenv_ddpg_replay_reset(okenv_t h)
    {
        OK_QUIESCE(h);
        return ringReset(h, kDdpgRing);
    }

    int okenv_ddpg_replay_push(okenv_t h, const okenv_ddpg_record *rec, const float *reward)
    {
        OK_QUIESCE(h);
        return ringPush<OkDdpgReplayParams>(h, kDdpgRing, rec, reward);
    }

    int okenv_ddpg_replay_size(okenv_t h, int64_t *size, int64_t *pushed)
    {
        OK_QUIESCE(h);
        return ringSize(h, kDdpgRing, size, pushed);
    }

    int okenv_ddpg_replay_get(okenv_t h, const okenv_ddpg_ring *out)
    {
        OK_QUIESCE(h);
        return ringGet(h, kDdpgRing, out);
    }

    int okenv_ddpg_update(okenv_t h, int32_t B, int32_t iterations, int32_t resample, uint32_t draw_base, const okenv_ddpg_output *out)
    {
        OK_QUIESCE(h);
        if (!h)
            return fail(h, OKENV_ERR_INVALID, "okenv_ddpg_update: NULL handle");
        if (!h->ddpg_drv.ok)
            return fail(h, OKENV_ERR_STATE, "okenv_ddpg_update: call okenv_ddpg_create first");
        if (!h->ddpg_drv.set[0] || !h->ddpg_drv.set[1])
            return fail(h, OKENV_ERR_STATE, "okenv_ddpg_update: both networks need their parameters first (okenv_ddpg_set_params)");
        if (!h->ddpg_ring.ok)
            return fail(h, OKENV_ERR_STATE, "okenv_ddpg_update: call okenv_ddpg_replay_create first");
        if (B < 1 || iterations < 1)
            return fail(h, OKENV_ERR_INVALID, "okenv_ddpg_update: B and iterations must be at least 1");
        OK_HIP(h, hipSetDevice(h->device));
        OkDdpgParams p{};
        p.R        = h->shape.R;
        p.H        = h->ddpg.hidden;
        p.Hc       = h->ddpg.critic_hidden;
        p.B        = B;
        p.C        = (B + OK_LEARN_CHUNK - 1) / OK_LEARN_CHUNK;
        p.Pa       = ok_actor_num_params(p.R, p.H, 2);
        p.Pc       = ok_ddpg_critic_params(p.R, p.Hc);
        p.capacity = static_cast<uint64_t>(h->ddpg_ring.capacity);
        p.pushed   = h->ddpg_ring.d_words;
        p.ring     = ringFields<okenv_ddpg_ring>(h->ddpg_ring);
        p.actor    = h->ddpg_drv.d;
        p.critic   = h->ddpg_drv.d + h->ddpg_drv.cap;
        p.actor_t  = h->ddpg_drv.d + 2U * h->ddpg_drv.cap;
        p.critic_t = h->ddpg_drv.d + 3U * h->ddpg_drv.cap;
        p.act_m    = h->ddpg_drv.d2;
        p.act_v    = h->ddpg_drv.d2 + h->ddpg_drv.cap;
        p.cri_m    = h->ddpg_drv.d2 + 2U * h->ddpg_drv.cap;
        p.cri_v    = h->ddpg_drv.d2 + 3U * h->ddpg_drv.cap;
        for (int k = 0; k < 2; ++k)
        {
            p.scale[k] = h->ddpg.scale[k];
            p.bias[k]  = h->ddpg.bias[k];
        }
        p.gamma = h->ddpg.gamma;
        p.tau   = h->ddpg.tau;
        p.omt   = 1.F - h->ddpg.tau;
        p.seed  = h->ddpg.sample_seed;
        const okenv_ddpg_output none{};
        const okenv_ddpg_output &o = out != nullptr ? *out : none;
        p.grad_critic = o.grad_critic;
        p.grad_actor  = o.grad_actor;
        p.index       = o.index;
        const size_t bytes = sizeof(float) * static_cast<size_t>(p.C) * (static_cast<size_t>(std::max(p.Pa, p.Pc)) + 1U);
        if (const int rc = growScratch(h, h->ddpg_scratch, bytes))
            return rc;
        p.part = reinterpret_cast<float *>(h->ddpg_scratch.part);
        const size_t launches = 4U * static_cast<size_t>(iterations);
        if (const int rc = eventsBegin(h, h->ddpg_scratch.log, launches))
            return rc;
        const size_t   lds = okDdpgLdsBytes(p.R, p.H, p.Hc);
        const unsigned chunks = static_cast<unsigned>(p.C), step_threads = kLearnStepCols * kLearnStepRows;
        const unsigned cols_c = static_cast<unsigned>((p.Pc + 1 + kLearnStepCols - 1) / kLearnStepCols), cols_a = static_cast<unsigned>((p.Pa + 1 + kLearnStepCols - 1) / kLearnStepCols);
        for (int it = 0; it < iterations; ++it)
        {
            p.draw        = draw_base + (resample != 0 ? static_cast<uint32_t>(it) : 0U);
            p.adam_actor  = okDdpgAdamConsts(h->ddpg, h->ddpg.lr_actor, h->ddpg_t + 1);
            p.adam_critic = okDdpgAdamConsts(h->ddpg, h->ddpg.lr_critic, h->ddpg_t + 1);
            p.critic_loss = o.critic_loss != nullptr ? o.critic_loss + it : nullptr;
            p.actor_loss  = o.actor_loss != nullptr ? o.actor_loss + it : nullptr;
            // (the step number advances once all four kernels of the iteration are enqueued, as in okenv_ppo_update)
            hipLaunchKernelGGL(okDdpgCriticGradKernel, dim3(chunks), dim3(kLearnThreads), lds, h->stream, p);
            OK_HIP(h, hipGetLastError());
            if (const int rc = eventsMark(h, h->ddpg_scratch.log))
                return rc;
            hipLaunchKernelGGL(okDdpgStepKernel<false>, dim3(cols_c), dim3(step_threads), 0, h->stream, p);
            OK_HIP(h, hipGetLastError());
            if (const int rc = eventsMark(h, h->ddpg_scratch.log))
                return rc;
            hipLaunchKernelGGL(okDdpgActorGradKernel, dim3(chunks), dim3(kLearnThreads), lds, h->stream, p);
            OK_HIP(h, hipGetLastError());
            if (const int rc = eventsMark(h, h->ddpg_scratch.log))
                return rc;
            hipLaunchKernelGGL(okDdpgStepKernel<true>, dim3(cols_a), dim3(step_threads), 0, h->stream, p);
            OK_HIP(h, hipGetLastError());
            if (const int rc = eventsMark(h, h->ddpg_scratch.log))
                return rc;
            h->ddpg_t += 1;
        }
        return OKENV_OK;
    }

    int okenv_debug_ddpg_timing(okenv_t h, double *ms4)
    {
        OK_QUIESCE(h);
        return updateTiming(h, &okenv::ddpg_scratch, "okenv_debug_ddpg_timing", "okenv_ddpg_update", ms4, 4);
    }

    int okenv_ddpg_act_host(const okenv_ddpg_config *config, const float *actor, int32_t num_rays, int32_t n, const float *dist, const uint8_t *crashed,
                            uint32_t draw_index, float *throttle, float *steer, float *action, float *state, uint8_t *alive)
    {
        if (const char *why = okDdpgCheckConfig(config, num_rays))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_ddpg_act_host: ") + why);
        if (!actor || n < 0 || !dist)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_ddpg_act_host: bad argument");
        okDdpgActHost(*config, actor, num_rays, n, dist, crashed, draw_index, throttle, steer, action, state, alive);
        return OKENV_OK;
    }

    int okenv_ddpg_replay_push_host(const okenv_ddpg_ring *ring, int32_t capacity, int32_t num_rays, uint64_t *pushed, uint32_t flags, int32_t n,
                                    const float *state, const float *action, const uint8_t *alive, const float *dist, const uint8_t *crashed,
                                    const float *reward)
    {
        if (const char *why = okReplayCheckCreate(capacity, flags))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_ddpg_replay_push_host: ") + why);
        if (!okReplayRingComplete(ring) || !pushed)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_ddpg_replay_push_host: the ring needs every field and its counter");
        if (num_rays < 1 || num_rays > OK_DDPG_MAX_RAYS || n < 0)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_ddpg_replay_push_host: the fan needs 1 .. 62 rays and n >= 0");
        if (!state || !action)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_ddpg_replay_push_host: the record needs state and action");
        if (!alive && (flags & OKENV_REPLAY_PUSH_ALL) == 0U)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_ddpg_replay_push_host: the record needs alive (or pass OKENV_REPLAY_PUSH_ALL)");
        if (!dist || !crashed)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_ddpg_replay_push_host: dist and crashed are required");
        okReplayPushHost(*ring, static_cast<uint64_t>(capacity), num_rays, pushed, flags, n, state, action, alive, dist, crashed, reward);
        return OKENV_OK;
    }

    int okenv_ddpg_update_host(const okenv_ddpg_config *config, int32_t num_rays, okenv_ddpg_state *state, const okenv_ddpg_ring *ring, int64_t size, int32_t B,
                               int32_t iterations, int32_t resample, uint32_t draw_base, const okenv_ddpg_output *out)
    {
        if (const char *why = okDdpgCheckConfig(config, num_rays))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_ddpg_update_host: ") + why);
        if (B < 1 || iterations < 1)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_ddpg_update_host: B and iterations must be at least 1");
        if (state == nullptr || state->actor == nullptr || state->critic == nullptr || state->actor_target == nullptr || state->critic_target == nullptr ||
            state->actor_m == nullptr || state->actor_v == nullptr || state->critic_m == nullptr || state->critic_v == nullptr || state->t < 0)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_ddpg_update_host: state lacks a parameter or moment vector, or t < 0");
        if (size < 0 || size >= (INT64_C(1) << 31) || (size > 0 && !okReplayRingComplete(ring)))
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_ddpg_update_host: size outside 0 .. 2^31 - 1, or a ring without every field");
        const okenv_ddpg_output none{};
        const okenv_ddpg_ring   empty{};
        okDdpgUpdateHost(*config, num_rays, *state, ring != nullptr ? *ring : empty, static_cast<uint32_t>(size), B, iterations, resample != 0, draw_base,
                         out != nullptr ? *out : none);
        return OKENV_OK;
    }

    int okenv_debug_adam(const okenv_learner_params *params, int64_t t, float *p, float *m, float *v, const float *g, int32_t n)
    {
        if (const char *why = okLearnCheckParams(params))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_debug_adam: ") + why);
        if (t < 1 || !p || !m || !v || !g || n < 0)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_debug_adam: bad argument");
        const ok_learn_adam_consts c = okLearnAdamConsts(*params, t);
        for (int32_t i = 0; i < n; ++i)
            ok_learn_adam(p + i, m + i, v + i, g[i], c);
        return OKENV_OK;
    }

    int okenv_debug_expf(const float *x, float *out, int32_t n)
    {
        if (!x || !out || n < 0)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_debug_expf: bad argument");
        for (int32_t i = 0; i < n; ++i)
            out[i] = ok_expf(x[i]);
        return OKENV_OK;
    }

    int okenv_rollout_controller(okenv_t h, int32_t n_steps, float throttle, float steering_scale)
    {
        OK_QUIESCE(h);
        if (!h || n_steps < 0)
            return fail(h, OKENV_ERR_INVALID, "okenv_rollout_controller: bad argument");
        if (!h->d_ctrl_params)
            return fail(h, OKENV_ERR_STATE, "okenv_rollout_controller: call okenv_controller_create first");
        if (h->tracker_kind < 0)
            return fail(h, OKENV_ERR_STATE, "okenv_rollout_controller: call okenv_tracker_create first");
        if (h->shape.grid_mode != kGridLds || !h->shape.coop || h->shape.rays_per_lane != 1 || h->shape.G < 8)
            return fail(h, OKENV_ERR_STATE, "okenv_rollout_controller: needs the LDS form of the step kernel with at most 64 rays "
                                            "(use okenv_controller_act + okenv_step + okenv_tracker_update)");
        if (h->ctrl_hidden > kCtrlUnitsPerLane * h->shape.G)
            return fail(h, OKENV_ERR_STATE, "okenv_rollout_controller: the hidden layer is too wide for this fan's lane groups (hidden <= 4 x lanes per agent); "
                                            "use okenv_controller_act + okenv_step + okenv_tracker_update");
        if (okCoopLdsBytes(h->shape.image_bytes) + qLdsBytes(h) > kLdsBudget)
            return fail(h, OKENV_ERR_STATE, "okenv_rollout_controller: track image + centre line do not fit the CU's LDS");
        if (n_steps == 0)
            return OKENV_OK;
        OK_HIP(h, hipSetDevice(h->device));
        const int brc = buildCenterlineBuckets(h);
        if (brc != OKENV_OK)
            return brc;
        if (h->episode)
        {
            if (h->ep_kind != 0 && h->ep_kind != kPolicyCtrl)
                return fail(h, OKENV_ERR_STATE, "okenv_rollout_controller: the running episode belongs to another rollout (okenv_rollout_policy / _q)");
            if ((h->reset_flags & kAutoResetOn) != 0U)
                return fail(h, OKENV_ERR_STATE, "okenv_rollout_controller: episodes need auto-reset off");
            // (an episode stops stepping an agent once it has crashed and taken one more step; the +1-per-step reward keeps counting
            // for crashed agents, so its bookkeeping would fall behind the per-step loop's)
            if (h->tracker_kind != kRewardProgress)
                return fail(h, OKENV_ERR_STATE, "okenv_rollout_controller: inside an episode the bookkeeping must be OKENV_REWARD_PROGRESS");
            const int prc = prelistEpisode(h, kActionsController);
            if (prc != OKENV_OK)
                return prc;
            h->ep_kind = kPolicyCtrl;
        }
        OkStepParams p     = baseParams(h);
        p.n_steps          = n_steps;
        p.action_source    = kActionsController;
        p.ctrl_throttle    = throttle;
        p.ctrl_steer_scale = steering_scale;
        int rc             = OKENV_OK;
        if (!(h->episode && h->n_active == 0)) // (nobody left to step: the steps still count)
            rc = launchStep(h, p);
        if (rc == OKENV_OK && h->episode)
            h->ep_steps += static_cast<uint32_t>(n_steps);
        return rc == OKENV_OK ? advanceStepCount(h, n_steps) : rc;
    }

    // ---- EvolutionaryRacer ---------------------------------------------------------------------------------------

    int okenv_policy_mlp_create(okenv_t h, int32_t hidden, uint32_t seed, uint32_t agent_base)
    {
        OK_QUIESCE(h);
        if (!h || hidden < 1 || hidden > OK_MLP_HID_PAD)
            return fail(h, OKENV_ERR_INVALID, "okenv_policy_mlp_create: hidden width must be in [1, 32]");
        if (h->shape.rays_per_lane != 1 || h->shape.R < 5 || h->shape.G < 8)
            return fail(h, OKENV_ERR_INVALID, "okenv_policy_mlp_create: the fused policy needs 5 <= rays <= 64");
        OK_HIP(h, hipSetDevice(h->device));
        const size_t total = static_cast<size_t>(h->shape.N) * OK_MLP_WEIGHTS(h->shape.R);
        int          rc;
        // (d_mlp_w, which the other entry points take as "a policy exists", comes last)
        if ((rc = devEnsure(h, &h->d_mlp_w_new, total)) || (rc = devEnsure(h, &h->d_score, static_cast<size_t>(h->shape.N))) ||
            (rc = devEnsure(h, &h->d_nearest, static_cast<size_t>(h->shape.N))) || (rc = devEnsure(h, &h->d_parents, 16U)) ||
            (rc = devEnsure(h, &h->d_parent_score, 16U)) || (rc = devEnsure(h, &h->d_alive, 4U)) || (rc = devEnsure(h, &h->d_mlp_w, total)))
            return rc;
        h->mlp_hidden = hidden;
        hipLaunchKernelGGL(okGaInitWeightsKernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, h->stream, h->d_mlp_w, h->shape.N,
                           h->shape.R, hidden, seed, agent_base);
        OK_HIP(h, hipGetLastError());
        return OKENV_OK;
    }

    int32_t okenv_policy_mlp_weights_per_agent(okenv_t h)
    {
        return h ? OK_MLP_WEIGHTS(h->shape.R) : 0;
    }

    int okenv_policy_mlp_get_weights(okenv_t h, float *out)
    {
        OK_QUIESCE(h);
        if (!h || !out || !h->d_mlp_w)
            return fail(h, OKENV_ERR_STATE, "okenv_policy_mlp_get_weights: no policy");
        int rc = copyAny(h, out, h->d_mlp_w, sizeof(float) * static_cast<size_t>(h->shape.N) * OK_MLP_WEIGHTS(h->shape.R));
        if (rc != OKENV_OK)
            return rc;
        OK_HIP(h, hipStreamSynchronize(h->stream));
        return OKENV_OK;
    }

    int okenv_policy_mlp_set_weights(okenv_t h, const float *in)
    {
        OK_QUIESCE(h);
        if (h)
            dropEpisode(h);
        if (!h || !in || !h->d_mlp_w)
            return fail(h, OKENV_ERR_STATE, "okenv_policy_mlp_set_weights: no policy");
        int rc = copyAny(h, h->d_mlp_w, in, sizeof(float) * static_cast<size_t>(h->shape.N) * OK_MLP_WEIGHTS(h->shape.R));
        if (rc != OKENV_OK)
            return rc;
        OK_HIP(h, hipStreamSynchronize(h->stream));
        return OKENV_OK;
    }

    int okenv_rollout_policy(okenv_t h, int32_t n_steps)
    {
        OK_QUIESCE(h);
        if (!h || n_steps < 0)
            return fail(h, OKENV_ERR_INVALID, "okenv_rollout_policy: bad argument");
        if (!h->d_mlp_w)
            return fail(h, OKENV_ERR_STATE, "okenv_rollout_policy: call okenv_policy_mlp_create first");
        if (n_steps == 0)
            return OKENV_OK;
        if (h->episode)
        {
            if (h->ep_kind != 0 && h->ep_kind != kPolicyMlp)
                return fail(h, OKENV_ERR_STATE, "okenv_rollout_policy: the running episode belongs to another rollout (okenv_rollout_q / _controller)");
            if ((h->reset_flags & kAutoResetOn) != 0U)
                return fail(h, OKENV_ERR_STATE, "okenv_rollout_policy: episodes need auto-reset off");
            const int prc = prelistEpisode(h, kActionsMlpPolicy);
            if (prc != OKENV_OK)
                return prc;
            h->ep_kind = kPolicyMlp;
        }
        OkStepParams p  = baseParams(h);
        p.n_steps       = n_steps;
        p.action_source = kActionsMlpPolicy;
        int rc          = OKENV_OK;
        if (!(h->episode && h->n_active == 0)) // (nobody left to step: the steps still count)
            rc = launchStep(h, p);
        if (rc == OKENV_OK && h->episode)
            h->ep_steps += static_cast<uint32_t>(n_steps);
        return rc == OKENV_OK ? advanceStepCount(h, n_steps) : rc;
    }

    int okenv_episode_begin(okenv_t h)
    {
        OK_QUIESCE(h);
        if (!h)
            return OKENV_ERR_INVALID;
        if ((h->reset_flags & kAutoResetOn) != 0U)
            return fail(h, OKENV_ERR_STATE, "okenv_episode_begin: episodes need auto-reset off (a crashed agent stays crashed until the caller resets it)");
        OK_HIP(h, hipSetDevice(h->device));
        const size_t N = static_cast<size_t>(h->shape.N);
        int          rc;
        if ((rc = devEnsure(h, &h->d_settled, N)) || (rc = devEnsure(h, &h->d_crash_step, N)) || (rc = devEnsure(h, &h->d_crash_thr, N)) ||
            (rc = devEnsure(h, &h->d_crash_steer, N)) || (rc = devEnsure(h, &h->d_active, N)) || (rc = devEnsure(h, &h->d_ep_counts, 2U)) ||
            (rc = devEnsure(h, &h->d_ep_out, 2U)) || (rc = devEnsure(h, &h->d_live, 1U)) || (rc = devEnsure(h, &h->d_q_next_state, N)))
            return rc;
        hipLaunchKernelGGL(okEpisodeBeginKernel, dim3((h->shape.N + 255) / 256), dim3(256), 0, h->stream, h->st.crashed, h->d_settled, h->d_crash_step,
                           h->d_live, h->shape.N);
        OK_HIP(h, hipGetLastError());
        h->episode    = true;
        h->n_active   = -1;
        h->ep_kind    = 0;
        h->ep_steps   = 0U;
        h->ep_prelist = true; // (the first rollout lists the population when it fits the tail kernel: prelistEpisode)
        return OKENV_OK;
    }

    int okenv_episode_compact(okenv_t h, int32_t *alive_out, int32_t *listed_out)
    {
        OK_QUIESCE(h);
        if (!h || !h->episode)
            return fail(h, OKENV_ERR_STATE, "okenv_episode_compact: no episode is running (okenv_episode_begin)");
        OK_HIP(h, hipSetDevice(h->device));
        hipLaunchKernelGGL(okEpisodeCompactKernel, dim3(1), dim3(1024), 0, h->stream, h->d_settled, h->st.crashed, h->shape.N, h->d_active, h->d_ep_counts);
        OK_HIP(h, hipGetLastError());
        int32_t counts[2] = {0, 0};
        OK_HIP(h, hipMemcpyAsync(counts, h->d_ep_counts, sizeof(counts), hipMemcpyDeviceToHost, h->stream));
        OK_HIP(h, hipStreamSynchronize(h->stream));
        h->n_active   = counts[1];
        h->ep_prelist = false;
        if (alive_out)
            *alive_out = counts[0];
        if (listed_out)
            *listed_out = counts[1];
        return OKENV_OK;
    }

    int okenv_episode_tail_limit(okenv_t h, int32_t *out)
    {
        OK_QUIESCE(h);
        if (!h || !out)
            return fail(h, OKENV_ERR_INVALID, "okenv_episode_tail_limit: NULL argument");
        const bool q    = h->ep_kind == kPolicyQ || (h->ep_kind == 0 && h->d_q_table != nullptr && h->d_mlp_w == nullptr);
        const bool ctrl = h->ep_kind == kPolicyCtrl || (h->ep_kind == 0 && h->d_ctrl_params != nullptr && h->d_mlp_w == nullptr && h->d_q_table == nullptr);
        *out            = ctrl ? 0 : static_cast<int32_t>(okTailLimit(h->shape, q, qLdsBytes(h))); // (the controller rollout has no one-agent-per-workgroup form)
        return OKENV_OK;
    }

    int okenv_episode_end(okenv_t h, int32_t *steps_out, uint64_t *live_agent_steps_out)
    {
        OK_QUIESCE(h);
        if (!h || !h->episode)
            return fail(h, OKENV_ERR_STATE, "okenv_episode_end: no episode is running (okenv_episode_begin)");
        OK_HIP(h, hipSetDevice(h->device));
        const unsigned blocks = static_cast<unsigned>((h->shape.N + 255) / 256);
        hipLaunchKernelGGL(okEpisodeEndKernel, dim3(1), dim3(1024), 0, h->stream, h->st.crashed, h->d_crash_step, h->shape.N, h->ep_steps, h->d_ep_out);
        if (h->ep_kind == kPolicyMlp || h->ep_kind == kPolicyCtrl)
            hipLaunchKernelGGL(okEpisodeFixupKernel, dim3(blocks), dim3(256), 0, h->stream, h->st, h->d_crash_step, h->d_crash_thr, h->d_crash_steer,
                               h->d_ep_out, h->shape.N);
        else if (h->ep_kind == kPolicyQ)
            hipLaunchKernelGGL(okQSettleKernel, dim3(static_cast<unsigned>((static_cast<long>(h->shape.N) * kSettleLanes + 255) / 256)), dim3(256), 0,
                               h->stream, h->st, h->d_q_table, h->d_q_state, h->d_q_action,
                               h->d_q_next_state, h->d_crash_step, h->d_ep_out, h->shape.N, h->ep_q_seed, h->ep_q_agent_base, h->ep_q_step_base,
                               h->ep_q_epsilon, h->shape.R, h->q_ray[0], h->q_ray[1], h->q_ray[2], h->q_ray[3], h->q_ray[4]);
        OK_HIP(h, hipGetLastError());
        uint32_t           out[2] = {0U, 0U};
        unsigned long long live   = 0ULL;
        OK_HIP(h, hipMemcpyAsync(out, h->d_ep_out, sizeof(out), hipMemcpyDeviceToHost, h->stream));
        OK_HIP(h, hipMemcpyAsync(&live, h->d_live, sizeof(live), hipMemcpyDeviceToHost, h->stream));
        OK_HIP(h, hipStreamSynchronize(h->stream));
        // the steps beyond T were taken by nobody who could still move: they do not count
        if (h->ep_kind == kPolicyMlp || h->ep_kind == kPolicyCtrl)
            h->step_count -= h->ep_steps - out[0];
        if (steps_out)
            *steps_out = static_cast<int32_t>(out[0]);
        if (live_agent_steps_out)
            *live_agent_steps_out = live;
        dropEpisode(h);
        return OKENV_OK;
    }

    int okenv_alive_count(okenv_t h, int32_t *out)
    {
        OK_QUIESCE(h);
        if (!h || !out)
            return fail(h, OKENV_ERR_INVALID, "okenv_alive_count: NULL argument");
        OK_HIP(h, hipSetDevice(h->device));
        int *d = h->d_alive;
        if (!d)
        {
            int rc = devAlloc(h, &h->d_alive, 4U);
            if (rc != OKENV_OK)
                return rc;
            d = h->d_alive;
        }
        OK_HIP(h, hipMemsetAsync(d, 0, sizeof(int), h->stream));
        hipLaunchKernelGGL(okAliveCountKernel, dim3((h->shape.N + 255) / 256), dim3(256), 0, h->stream, h->st.crashed, h->shape.N, d);
        OK_HIP(h, hipGetLastError());
        OK_HIP(h, hipMemcpyAsync(out, d, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        OK_HIP(h, hipStreamSynchronize(h->stream));
        return OKENV_OK;
    }

    int okenv_off_grid_count(okenv_t h, int32_t *alive_off_grid, int32_t *all_off_grid)
    {
        OK_QUIESCE(h);
        if (!h)
            return OKENV_ERR_INVALID;
        OK_HIP(h, hipSetDevice(h->device));
        void     *sp = nullptr;
        const int rc = deviceScratch(h, 2U * sizeof(int), &sp);
        if (rc != OKENV_OK)
            return rc;
        int *d = static_cast<int *>(sp);
        OK_HIP(h, hipMemsetAsync(d, 0, 2U * sizeof(int), h->stream));
        const OkGridGeom &g = h->grid.g;
        hipLaunchKernelGGL(okOffGridCountKernel, dim3((h->shape.N + 255) / 256), dim3(256), 0, h->stream, h->st.pos_x, h->st.pos_y, h->st.crashed, h->shape.N,
                           g.x0, g.y0, g.x1, g.y1, d);
        OK_HIP(h, hipGetLastError());
        int host[2] = {0, 0};
        OK_HIP(h, hipMemcpyAsync(host, d, 2U * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        OK_HIP(h, hipStreamSynchronize(h->stream));
        if (alive_off_grid)
            *alive_off_grid = host[0];
        if (all_off_grid)
            *all_off_grid = host[1];
        return OKENV_OK;
    }

    int okenv_reset_all(okenv_t h, float x, float y, float rot_deg)
    {
        OK_QUIESCE(h);
        if (h)
            dropEpisode(h);
        if (!h)
            return OKENV_ERR_INVALID;
        OK_HIP(h, hipSetDevice(h->device));
        hipLaunchKernelGGL(okResetAllKernel, dim3((h->shape.N + 255) / 256), dim3(256), 0, h->stream, h->st, x, y, rot_deg, h->shape.N);
        OK_HIP(h, hipGetLastError());
        return OKENV_OK;
    }

    int okenv_ga_scores(okenv_t h, float *out)
    {
        OK_QUIESCE(h);
        if (!h)
            return OKENV_ERR_INVALID;
        if (!h->d_mlp_w || h->P <= 0)
            return fail(h, OKENV_ERR_STATE, "okenv_ga_scores: needs okenv_policy_mlp_create and okenv_set_centerline");
        OK_HIP(h, hipSetDevice(h->device));
        hipLaunchKernelGGL(okNearestIdxKernel, dim3((h->shape.N * kNearestLanes + 255) / 256), dim3(256), 0, h->stream, h->d_cx, h->d_cy, h->P,
                           h->st.pos_x, h->st.pos_y, h->shape.N, h->d_nearest);
        hipLaunchKernelGGL(okGaScoreKernel, dim3((h->shape.N + 255) / 256), dim3(256), 0, h->stream, h->d_nearest, h->d_score, h->shape.N);
        OK_HIP(h, hipGetLastError());
        if (out)
        {
            int rc = copyAny(h, out, h->d_score, sizeof(float) * static_cast<size_t>(h->shape.N));
            if (rc != OKENV_OK)
                return rc;
            OK_HIP(h, hipStreamSynchronize(h->stream));
        }
        return OKENV_OK;
    }

    int okenv_ga_scores_device(okenv_t h, const float **ptr)
    {
        OK_QUIESCE(h);
        if (!h || !ptr)
            return OKENV_ERR_INVALID;
        if (!h->d_score)
            return fail(h, OKENV_ERR_STATE, "okenv_ga_scores_device: call okenv_policy_mlp_create first");
        *ptr = h->d_score;
        return OKENV_OK;
    }

    int okenv_get_stream(okenv_t h, void **hip_stream)
    {
        OK_QUIESCE(h);
        if (!h || !hip_stream)
            return OKENV_ERR_INVALID;
        *hip_stream = static_cast<void *>(h->stream);
        return OKENV_OK;
    }

    int okenv_ga_select_mate(okenv_t h, uint32_t seed, uint32_t generation, uint32_t agent_base, int32_t *parents_out)
    {
        OK_QUIESCE(h);
        if (h)
            dropEpisode(h);
        if (!h)
            return OKENV_ERR_INVALID;
        if (!h->d_mlp_w)
            return fail(h, OKENV_ERR_STATE, "okenv_ga_select_mate: call okenv_policy_mlp_create first");
        OK_HIP(h, hipSetDevice(h->device));
        const int    K     = h->shape.N < 5 ? h->shape.N : 5; // kNumParents (Mating.hpp:118)
        const size_t total = static_cast<size_t>(h->shape.N) * OK_MLP_WEIGHTS(h->shape.R);
        hipLaunchKernelGGL(okGaTopKernel, dim3(1), dim3(1024), 0, h->stream, h->d_score, h->shape.N, h->d_parents, h->d_parent_score, K);
        hipLaunchKernelGGL(okGaMateKernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, h->stream, h->d_mlp_w, h->d_mlp_w_new,
                           h->d_parents, h->d_parent_score, K, h->shape.N, h->shape.R, h->mlp_hidden, seed, generation, agent_base);
        OK_HIP(h, hipGetLastError());
        std::swap(h->d_mlp_w, h->d_mlp_w_new);
        if (parents_out)
        {
            OK_HIP(h, hipMemcpyAsync(parents_out, h->d_parents, sizeof(int32_t) * K, hipMemcpyDeviceToHost, h->stream));
            OK_HIP(h, hipStreamSynchronize(h->stream));
        }
        return OKENV_OK;
    }

    // ---- RLRacers/Q_Learning ------------------------------------------------------------------------------------

    int okenv_q_create(okenv_t h)
    {
        OK_QUIESCE(h);
        if (!h)
            return OKENV_ERR_INVALID;
        if (!h->shape.coop || h->shape.R < 5)
            return fail(h, OKENV_ERR_INVALID, "okenv_q_create: needs the LDS form with 5 <= rays <= 64");
        OK_HIP(h, hipSetDevice(h->device));
        const size_t n = static_cast<size_t>(h->shape.N) * OK_Q_STATES * OK_Q_ACTIONS;
        int          rc;
        // (d_q_table, which the other entry points take as "the tables exist", comes last)
        if ((rc = devEnsure(h, &h->d_q_state, static_cast<size_t>(h->shape.N))) || (rc = devEnsure(h, &h->d_q_action, static_cast<size_t>(h->shape.N))) ||
            (rc = devEnsure(h, &h->d_q_prev, static_cast<size_t>(h->shape.N))) || (rc = devEnsure(h, &h->d_q_reset_nearest, 4U)) ||
            (rc = devEnsure(h, &h->d_q_reset_query, 4U)) || (rc = devEnsure(h, &h->d_q_table, n)))
            return rc;
        hipLaunchKernelGGL(okQInitTableKernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, h->stream, h->d_q_table,
                           static_cast<long>(n));
        OK_HIP(h, hipGetLastError());
        // the five rays of the state: nearest to -70, -30, 0, 30, 70 degrees, ties to the lower index
        const float target[5] = {-70.F, -30.F, 0.F, 30.F, 70.F};
        for (int t = 0; t < 5; ++t)
        {
            int   arg  = 0;
            float best = std::fabs(h->host_ray_deg[0] - target[t]);
            for (int r = 1; r < h->shape.R; ++r)
            {
                const float d = std::fabs(h->host_ray_deg[r] - target[t]);
                if (d < best)
                {
                    best = d;
                    arg  = r;
                }
            }
            h->q_ray[t] = arg;
        }
        return OKENV_OK;
    }

    int okenv_q_begin_episode(okenv_t h, int32_t reset_idx)
    {
        OK_QUIESCE(h);
        if (!h || !h->d_q_table)
            return fail(h, OKENV_ERR_STATE, "okenv_q_begin_episode: call okenv_q_create first");
        if (h->P <= 0 || reset_idx < 0 || reset_idx >= h->P)
            return fail(h, OKENV_ERR_INVALID, "okenv_q_begin_episode: needs a centre line and a valid reset index");
        const float x = h->host_cx[reset_idx], y = h->host_cy[reset_idx];
        int         rc = okenv_reset_all(h, x, y, h->host_chead[reset_idx]);
        if (rc != OKENV_OK)
            return rc;
        // prev_track_idx_ = findNearestTrackIndexBruteForce(reset point) (q_racer_sim.cpp:134-139); one query on the device
        // (the query lives in the handle on both sides: an asynchronous copy out of a local variable may still be reading it
        // after this function has returned)
        h->q_reset_query[0] = x;
        h->q_reset_query[1] = y;
        float *dq           = h->d_q_reset_query;
        OK_HIP(h, hipMemcpyAsync(dq, h->q_reset_query, 8U, hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(okNearestIdxKernel, dim3(1), dim3(256), 0, h->stream, h->d_cx, h->d_cy, h->P, dq, dq + 1, 1, h->d_q_reset_nearest);
        OK_HIP(h, hipGetLastError());
        if ((rc = okenv_step(h, 1)) != OKENV_OK) // initial observation with the zero action Agent::reset leaves behind
            return rc;
        hipLaunchKernelGGL(okQBeginEpisodeKernel, dim3((h->shape.N + 255) / 256), dim3(256), 0, h->stream, h->st.dist, h->shape.R, h->q_ray[0], h->q_ray[1],
                           h->q_ray[2], h->q_ray[3], h->q_ray[4], h->d_q_state, h->d_q_prev, h->d_q_reset_nearest, h->shape.N);
        OK_HIP(h, hipGetLastError());
        return OKENV_OK;
    }

    int okenv_rollout_q(okenv_t h, int32_t n_steps, float epsilon, uint32_t seed, uint32_t agent_base, uint32_t step_base)
    {
        OK_QUIESCE(h);
        if (!h || n_steps < 0)
            return fail(h, OKENV_ERR_INVALID, "okenv_rollout_q: bad argument");
        if (!h->d_q_table)
            return fail(h, OKENV_ERR_STATE, "okenv_rollout_q: call okenv_q_create first");
        if (n_steps == 0)
            return OKENV_OK;
        if (okCoopLdsBytes(h->shape.image_bytes) + qLdsBytes(h) > kLdsBudget)
            return fail(h, OKENV_ERR_STATE, "okenv_rollout_q: track image + centre line do not fit the CU's LDS");
        OK_HIP(h, hipSetDevice(h->device));
        const int brc = buildCenterlineBuckets(h);
        if (brc != OKENV_OK)
            return brc;
        h->q_epsilon    = epsilon;
        if (h->episode)
        {
            if (h->ep_kind != 0 && h->ep_kind != kPolicyQ)
                return fail(h, OKENV_ERR_STATE, "okenv_rollout_q: the running episode belongs to another rollout (okenv_rollout_policy / _controller)");
            if (h->ep_kind == 0)
            {
                const int prc = prelistEpisode(h, kActionsQLearning);
                if (prc != OKENV_OK)
                    return prc;
                h->ep_kind         = kPolicyQ;
                h->ep_q_seed       = seed;
                h->ep_q_agent_base = agent_base;
                h->ep_q_epsilon    = epsilon;
                h->ep_q_step_base  = step_base - h->ep_steps;
            }
            else if (h->ep_q_seed != seed || h->ep_q_agent_base != agent_base || h->ep_q_epsilon != epsilon ||
                     h->ep_q_step_base + h->ep_steps != step_base)
                return fail(h, OKENV_ERR_INVALID, "okenv_rollout_q: inside an episode seed, agent_base and epsilon must stay the same and "
                                                  "step_base advance by the steps taken");
        }
        OkStepParams p  = baseParams(h);
        p.n_steps       = n_steps;
        p.action_source = kActionsQLearning;
        p.reset_flags   = 0; // episodes are restarted by okenv_q_begin_episode
        p.seed          = seed;
        p.agent_base    = agent_base;
        p.step_base     = step_base;
        int rc          = OKENV_OK;
        if (!(h->episode && h->n_active == 0))
            rc = launchStep(h, p);
        if (rc == OKENV_OK && h->episode)
            h->ep_steps += static_cast<uint32_t>(n_steps);
        return rc;
    }

    int okenv_q_get_table(okenv_t h, float *out)
    {
        OK_QUIESCE(h);
        if (!h || !out || !h->d_q_table)
            return fail(h, OKENV_ERR_STATE, "okenv_q_get_table: no table");
        int rc = copyAny(h, out, h->d_q_table, sizeof(float) * static_cast<size_t>(h->shape.N) * OK_Q_STATES * OK_Q_ACTIONS);
        if (rc != OKENV_OK)
            return rc;
        OK_HIP(h, hipStreamSynchronize(h->stream));
        return OKENV_OK;
    }

    int okenv_q_set_table(okenv_t h, const float *in)
    {
        OK_QUIESCE(h);
        if (h)
            dropEpisode(h);
        if (!h || !in || !h->d_q_table)
            return fail(h, OKENV_ERR_STATE, "okenv_q_set_table: no table");
        int rc = copyAny(h, h->d_q_table, in, sizeof(float) * static_cast<size_t>(h->shape.N) * OK_Q_STATES * OK_Q_ACTIONS);
        if (rc != OKENV_OK)
            return rc;
        OK_HIP(h, hipStreamSynchronize(h->stream));
        return OKENV_OK;
    }

    int okenv_q_get_state(okenv_t h, int32_t *state, int32_t *action, int32_t *prev_idx)
    {
        OK_QUIESCE(h);
        if (!h || !h->d_q_table)
            return fail(h, OKENV_ERR_STATE, "okenv_q_get_state: no table");
        int rc;
        if ((state && (rc = copyAny(h, state, h->d_q_state, 4U * h->shape.N))) || (action && (rc = copyAny(h, action, h->d_q_action, 4U * h->shape.N))) ||
            (prev_idx && (rc = copyAny(h, prev_idx, h->d_q_prev, 4U * h->shape.N))))
            return rc;
        OK_HIP(h, hipStreamSynchronize(h->stream));
        return OKENV_OK;
    }

    static int qSums(okenv_t h, float **d_out)
    {
        if (!h || !h->d_q_table)
            return fail(h, OKENV_ERR_STATE, "no Q table (call okenv_q_create first)");
        OK_HIP(h, hipSetDevice(h->device));
        if (!h->d_q_sums)
        {
            int rc = devAlloc(h, &h->d_q_sums, 2U * OK_Q_STATES * OK_Q_ACTIONS);
            if (rc != OKENV_OK)
                return rc;
        }
        constexpr int kEntries = OK_Q_STATES * OK_Q_ACTIONS;
        hipLaunchKernelGGL(okQTableSumsKernel, dim3((kEntries + 63) / 64), dim3(64), 0, h->stream, h->d_q_table, h->shape.N, h->d_q_sums,
                           h->d_q_sums + kEntries);
        OK_HIP(h, hipGetLastError());
        *d_out = h->d_q_sums;
        return OKENV_OK;
    }

    int okenv_q_table_sums(okenv_t h, float *sum, float *count)
    {
        OK_QUIESCE(h);
        if (!sum || !count)
            return fail(h, OKENV_ERR_INVALID, "okenv_q_table_sums: NULL argument");
        float *d  = nullptr;
        int    rc = qSums(h, &d);
        if (rc != OKENV_OK)
            return rc;
        constexpr size_t kBytes = sizeof(float) * OK_Q_STATES * OK_Q_ACTIONS;
        if ((rc = copyAny(h, sum, d, kBytes)) || (rc = copyAny(h, count, d + OK_Q_STATES * OK_Q_ACTIONS, kBytes)))
            return rc;
        OK_HIP(h, hipStreamSynchronize(h->stream));
        return OKENV_OK;
    }

    int okenv_q_assign_mean(okenv_t h, const float *sum, const float *count)
    {
        OK_QUIESCE(h);
        if (h)
            dropEpisode(h);
        if (!h || !h->d_q_table || !sum || !count)
            return fail(h, OKENV_ERR_STATE, "okenv_q_assign_mean: no Q table or NULL argument");
        OK_HIP(h, hipSetDevice(h->device));
        if (!h->d_q_sums)
        {
            int rc = devAlloc(h, &h->d_q_sums, 2U * OK_Q_STATES * OK_Q_ACTIONS);
            if (rc != OKENV_OK)
                return rc;
        }
        constexpr int    kEntries = OK_Q_STATES * OK_Q_ACTIONS;
        constexpr size_t kBytes   = sizeof(float) * kEntries;
        int              rc;
        if ((sum != h->d_q_sums && (rc = copyAny(h, h->d_q_sums, sum, kBytes))) ||
            (count != h->d_q_sums + kEntries && (rc = copyAny(h, h->d_q_sums + kEntries, count, kBytes))))
            return rc;
        const long total = static_cast<long>(h->shape.N) * kEntries;
        hipLaunchKernelGGL(okQAssignAllKernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, h->stream, h->d_q_table, h->shape.N,
                           h->d_q_sums, h->d_q_sums + kEntries);
        OK_HIP(h, hipGetLastError());
        OK_HIP(h, hipStreamSynchronize(h->stream));
        return OKENV_OK;
    }

    int okenv_q_share_knowledge(okenv_t h)
    {
        OK_QUIESCE(h);
        if (h)
            dropEpisode(h);
        float *d  = nullptr;
        int    rc = qSums(h, &d);
        if (rc != OKENV_OK)
            return rc;
        return okenv_q_assign_mean(h, d, d + OK_Q_STATES * OK_Q_ACTIONS);
    }

    int okenv_set_timing(okenv_t h, int32_t enabled)
    {
        OK_QUIESCE(h);
        if (!h)
            return OKENV_ERR_INVALID;
        h->timing = enabled != 0;
        return OKENV_OK;
    }

    int okenv_get_timing(okenv_t h, double *total_ms, uint64_t *launches)
    {
        OK_QUIESCE(h);
        if (!h || !total_ms || !launches)
            return fail(h, OKENV_ERR_INVALID, "okenv_get_timing: NULL argument");
        OK_HIP(h, hipStreamSynchronize(h->stream));
        double sum = 0.0;
        for (auto &e : h->events)
        {
            float ms = 0.F;
            OK_HIP(h, hipEventElapsedTime(&ms, e.start, e.stop));
            sum += ms;
        }
        *total_ms = sum + h->timing_carry_ms;
        *launches = h->events.size() + h->timing_carry_n;
        h->timing_carry_ms = 0.0;
        h->timing_carry_n  = 0;
        for (auto &e : h->events)
            h->event_pool.push_back(e);
        h->events.clear();
        return OKENV_OK;
    }

    // ---- track ------------------------------------------------------------------------------------------

    int okenv_track_load(okenv_track_t *out, const char *csv_path)
    {
        if (!out || !csv_path)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_track_load: NULL argument");
        *out = nullptr;
        std::unique_ptr<okenv_track> t(new okenv_track);
        t->track.reset(new RaceTrack(std::string(csv_path)));
        if (!t->track->loadedOk())
            return fail(nullptr, OKENV_ERR_IO, std::string("okenv_track_load: cannot read ") + csv_path);
        // TrackSegments (TrackSegments.cu:6-42): LI, LO, RI, RO polylines, then closers LI, RI, LO, RO
        const RaceTrack &rt   = *t->track;
        auto             run = [&](const std::vector<Vec2d> &poly) {
            for (size_t i = 0; i + 1 < poly.size(); ++i)
                t->segments.push_back({poly[i].x, poly[i].y, poly[i + 1].x, poly[i + 1].y});
        };
        auto closer = [&](const std::vector<Vec2d> &poly) {
            t->segments.push_back({poly.back().x, poly.back().y, poly.front().x, poly.front().y});
        };
        run(rt.left_bound_inner_);
        run(rt.left_bound_outer_);
        run(rt.right_bound_inner_);
        run(rt.right_bound_outer_);
        if (rt.left_bound_inner_.size() > 1)
        {
            closer(rt.left_bound_inner_);
            closer(rt.right_bound_inner_);
        }
        if (rt.left_bound_outer_.size() > 1)
        {
            closer(rt.left_bound_outer_);
            closer(rt.right_bound_outer_);
        }
        *out = t.release();
        return OKENV_OK;
    }

    int okenv_track_free(okenv_track_t t)
    {
        delete t;
        return OKENV_OK;
    }

    int32_t okenv_track_num_points(okenv_track_t t)
    {
        return t ? static_cast<int32_t>(t->track->track_data_points_.x_m.size()) : 0;
    }

    int32_t okenv_track_num_segments(okenv_track_t t)
    {
        return t ? static_cast<int32_t>(t->segments.size()) : 0;
    }

    int okenv_track_get(okenv_track_t t, int32_t which, float *out)
    {
        if (!t || !out)
            return OKENV_ERR_INVALID;
        const RaceTrack &rt  = *t->track;
        const auto      &d   = rt.track_data_points_;
        auto             vec = [&](const std::vector<float> &v) { std::memcpy(out, v.data(), v.size() * 4U); };
        auto             pts = [&](const std::vector<Vec2d> &v) {
            for (size_t i = 0; i < v.size(); ++i)
            {
                out[2 * i]     = v[i].x;
                out[2 * i + 1] = v[i].y;
            }
        };
        switch (which)
        {
        case 0: vec(d.x_m); break;
        case 1: vec(d.y_m); break;
        case 2: vec(d.w_tr_right_m); break;
        case 3: vec(d.w_tr_left_m); break;
        case 4: vec(rt.headings_); break;
        case 5: pts(rt.left_bound_inner_); break;
        case 6: pts(rt.left_bound_outer_); break;
        case 7: pts(rt.right_bound_inner_); break;
        case 8: pts(rt.right_bound_outer_); break;
        default: return OKENV_ERR_INVALID;
        }
        return OKENV_OK;
    }

    int okenv_track_queries(okenv_track_t t, const float *qx, const float *qy, int32_t n, float *out_boundary_distance,
                            float *out_lane_center_ratio)
    {
        if (!t || !qx || !qy || n < 0)
            return OKENV_ERR_INVALID;
        const RaceTrack &rt = *t->track;
        for (int32_t i = 0; i < n; ++i)
        {
            const Vec2d q{qx[i], qy[i]};
            if (out_boundary_distance)
                out_boundary_distance[i] = rt.getNearestDistanceToTrackBoundary(q);
            if (out_lane_center_ratio)
                out_lane_center_ratio[i] = rt.getDistanceToLaneCenter(q);
        }
        return OKENV_OK;
    }

    int okenv_track_segments(okenv_track_t t, float *out_xyxy)
    {
        if (!t || !out_xyxy)
            return OKENV_ERR_INVALID;
        std::memcpy(out_xyxy, t->segments.data(), t->segments.size() * sizeof(Segment2d));
        return OKENV_OK;
    }

    // ---- bird's-eye camera views (ok_render.h) ------------------------------------------------------------------------------

    int okenv_track_band_triangles(okenv_track_t t, float *xy6, uint8_t *ordinal, int32_t cap)
    {
        if (!t || cap < 0)
            return OKENV_ERR_INVALID;
        const RaceTrack &rt = *t->track;
        const size_t     P  = rt.left_bound_inner_.size();
        if (P < 2 || rt.left_bound_outer_.size() != P || rt.right_bound_inner_.size() != P || rt.right_bound_outer_.size() != P)
            return OKENV_ERR_STATE;
        auto xy = [](const std::vector<Vec2d> &v) {
            std::vector<float> o(2 * v.size());
            for (size_t i = 0; i < v.size(); ++i)
                o[2 * i] = v[i].x, o[2 * i + 1] = v[i].y;
            return o;
        };
        const std::vector<float> li = xy(rt.left_bound_inner_), lo = xy(rt.left_bound_outer_), ri = xy(rt.right_bound_inner_),
                                 ro = xy(rt.right_bound_outer_);
        const std::vector<OkRenderTri> list = okRenderDrawList(li.data(), lo.data(), ri.data(), ro.data(), static_cast<int>(P));
        const size_t                   n    = std::min(list.size(), static_cast<size_t>(cap));
        for (size_t i = 0; i < n; ++i)
        {
            if (xy6)
            {
                const OkRenderTri &q = list[i];
                const float        v[6] = {q.ax, q.ay, q.bx, q.by, q.cx, q.cy};
                std::memcpy(xy6 + 6 * i, v, sizeof(v));
            }
            if (ordinal)
                ordinal[i] = static_cast<uint8_t>(list[i].ord);
        }
        return static_cast<int>(list.size());
    }

    int okenv_render_create(okenv_t h, const float *left_inner_xy, const float *left_outer_xy, const float *right_inner_xy,
                            const float *right_outer_xy, int32_t num_points, const okenv_view_desc *desc)
    {
        OK_QUIESCE(h);
        if (!h || !desc || !left_inner_xy || !left_outer_xy || !right_inner_xy || !right_outer_xy)
            return fail(h, OKENV_ERR_INVALID, "okenv_render_create: NULL argument");
        if (num_points < 2)
            return fail(h, OKENV_ERR_INVALID, "okenv_render_create: need at least two points per boundary");
        const okenv_view_desc &d = *desc;
        if (d.width < 1 || d.width > 1024 || d.height < 1 || d.height > 1024)
            return fail(h, OKENV_ERR_INVALID, "okenv_render_create: width and height must be 1..1024");
        if (d.samples != 1 && d.samples != 2 && d.samples != 4)
            return fail(h, OKENV_ERR_INVALID, "okenv_render_create: samples must be 1, 2 or 4");
        if (d.format != OKENV_VIEW_RGBA8 && d.format != OKENV_VIEW_CLASS8)
            return fail(h, OKENV_ERR_INVALID, "okenv_render_create: unknown format");
        if (d.format == OKENV_VIEW_CLASS8 && d.samples != 1)
            return fail(h, OKENV_ERR_INVALID, "okenv_render_create: OKENV_VIEW_CLASS8 takes one sample per pixel");
        if (!(std::isfinite(d.view_w) && d.view_w > 0.F && std::isfinite(d.view_h) && d.view_h > 0.F))
            return fail(h, OKENV_ERR_INVALID, "okenv_render_create: the view extent must be finite and > 0");
        if (!(std::isfinite(d.radius) && d.radius > 0.F))
            return fail(h, OKENV_ERR_INVALID, "okenv_render_create: the radius must be finite and > 0");
        if ((d.flags & ~(OKENV_VIEW_DRAW_AGENT | OKENV_VIEW_DRAW_HEADING | OKENV_VIEW_HEADING_UP)) != 0U)
            return fail(h, OKENV_ERR_INVALID, "okenv_render_create: unknown flag");
        const std::vector<OkRenderTri> list =
            okRenderDrawList(left_inner_xy, left_outer_xy, right_inner_xy, right_outer_xy, num_points);
        float cell = kRenderCell;
        if (const char *e = std::getenv("OKENV_RENDER_CELL"))
            cell = static_cast<float>(std::atof(e));
        OkRenderGeom g;
        if (!okRenderBuildGrid(list, cell, g))
            return fail(h, OKENV_ERR_INVALID, "okenv_render_create: non-finite boundary coordinate");
        OK_HIP(h, hipSetDevice(h->device));
        // the buffers of an earlier setup go (behind the wait: nothing on the stream may still read them)
        h->render_ok = false;
        if (const int rc = regrow(h, {fresh(h->d_render_tris, g.cell_tris.size()), fresh(h->d_render_start, g.cell_start.size())}))
            return rc;
        if (!g.cell_tris.empty())
            OK_HIP(h, hipMemcpyAsync(h->d_render_tris, g.cell_tris.data(), sizeof(OkRenderTri) * g.cell_tris.size(), hipMemcpyHostToDevice,
                                     h->stream));
        OK_HIP(h, hipMemcpyAsync(h->d_render_start, g.cell_start.data(), sizeof(uint32_t) * g.cell_start.size(), hipMemcpyHostToDevice,
                                 h->stream));
        OK_HIP(h, hipStreamSynchronize(h->stream));
        h->render_refs = g.cell_tris.size();
        g.cell_tris    = {};
        g.cell_start   = {};
        h->render_geom = std::move(g);
        h->render_desc = d;
        h->render_ok   = true;
        return OKENV_OK;
    }

    int okenv_render_get_info(okenv_t h, okenv_render_info *out)
    {
        OK_QUIESCE(h);
        if (!h || !out)
            return fail(h, OKENV_ERR_INVALID, "okenv_render_get_info: NULL argument");
        if (!h->render_ok)
            return fail(h, OKENV_ERR_STATE, "okenv_render_get_info: call okenv_render_create first");
        const okenv_view_desc &d = h->render_desc;
        const OkRenderGeom    &g = h->render_geom;
        out->triangles      = g.triangles;
        out->grid_nx        = g.nx;
        out->grid_ny        = g.ny;
        out->grid_cell      = g.cell;
        out->registrations  = static_cast<int32_t>(h->render_refs);
        out->solid_cells    = 0;
        out->width          = d.width;
        out->height         = d.height;
        out->samples        = d.samples;
        out->channels       = d.format == OKENV_VIEW_RGBA8 ? 4 : 1;
        out->bytes_per_call = static_cast<uint64_t>(h->shape.N) * static_cast<uint64_t>(d.width) * static_cast<uint64_t>(d.height) *
                              static_cast<uint64_t>(out->channels);
        return OKENV_OK;
    }

    int okenv_render_views(okenv_t h, void *dst, uint64_t dst_bytes)
    {
        OK_QUIESCE(h);
        if (!h)
            return fail(h, OKENV_ERR_INVALID, "okenv_render_views: NULL handle");
        if (!h->render_ok)
            return fail(h, OKENV_ERR_STATE, "okenv_render_views: call okenv_render_create first");
        const okenv_view_desc &d  = h->render_desc;
        const uint64_t         C  = d.format == OKENV_VIEW_RGBA8 ? 4U : 1U;
        const uint64_t         hw = static_cast<uint64_t>(d.width) * static_cast<uint64_t>(d.height);
        if (!dst || dst_bytes < static_cast<uint64_t>(h->shape.N) * hw * C)
            return fail(h, OKENV_ERR_INVALID, "okenv_render_views: dst is NULL or smaller than N * H * W * C bytes");
        OK_HIP(h, hipSetDevice(h->device));
        hipPointerAttribute_t attr{};
        const hipError_t      pe = hipPointerGetAttributes(&attr, dst);
        if (pe != hipSuccess)
            (void)hipGetLastError(); // an unknown (host) pointer: clear the sticky error before the launch checks for one
        if (pe != hipSuccess || (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged) || attr.device != h->device)
            return fail(h, OKENV_ERR_INVALID, "okenv_render_views: dst must be device memory of the handle's device");
        const OkRenderGeom &g = h->render_geom;
        OkRenderParams      p{};
        p.pos_x      = h->st.pos_x;
        p.pos_y      = h->st.pos_y;
        p.rot        = h->st.rot;
        p.crashed    = h->st.crashed;
        p.tris       = h->d_render_tris;
        p.cell_start = h->d_render_start;
        p.dst        = static_cast<uint8_t *>(dst);
        p.x0         = g.x0;
        p.y0         = g.y0;
        p.inv_cell   = g.inv_cell;
        p.fnx        = static_cast<float>(g.nx);
        p.fny        = static_cast<float>(g.ny);
        p.nx         = g.nx;
        p.W          = static_cast<uint32_t>(d.width);
        p.hw         = static_cast<uint32_t>(hw);
        p.step_x     = d.view_w / static_cast<float>(d.width * d.samples);
        p.step_y     = d.view_h / static_cast<float>(d.height * d.samples);
        p.half_x     = d.view_w * 0.5F;
        p.half_y     = d.view_h * 0.5F;
        p.r2         = d.radius * d.radius;
        p.flags      = d.flags;
        p.agent_rgb  = d.agent_rgb[0] | static_cast<uint32_t>(d.agent_rgb[1]) << 8 | static_cast<uint32_t>(d.agent_rgb[2]) << 16;
        const uint32_t pix_per_block = kRenderThreads * (d.format == OKENV_VIEW_RGBA8 ? 4U : 16U);
        p.chunks                     = static_cast<uint32_t>((hw + pix_per_block - 1U) / pix_per_block);
        if (static_cast<uint64_t>(h->shape.N) * p.chunks > 0x7FFFFFFFULL)
            return fail(h, OKENV_ERR_INVALID, "okenv_render_views: too many workgroups for one launch (N * H * W too large)");
        const dim3 grid(static_cast<uint32_t>(h->shape.N) * p.chunks), block(kRenderThreads);
        const bool up = (d.flags & OKENV_VIEW_HEADING_UP) != 0U;
#define OK_RENDER_LAUNCH(F, S)                                                                                                 \
    do                                                                                                                         \
    {                                                                                                                          \
        if (up)                                                                                                                \
            hipLaunchKernelGGL((okRenderViewsKernel<F, S, true>), grid, block, 0, h->stream, p);                               \
        else                                                                                                                   \
            hipLaunchKernelGGL((okRenderViewsKernel<F, S, false>), grid, block, 0, h->stream, p);                              \
    } while (0)
        if (d.format == OKENV_VIEW_CLASS8)
            OK_RENDER_LAUNCH(kRenderClass, 1);
        else if (d.samples == 1)
            OK_RENDER_LAUNCH(kRenderRgba, 1);
        else if (d.samples == 2)
            OK_RENDER_LAUNCH(kRenderRgba, 2);
        else
            OK_RENDER_LAUNCH(kRenderRgba, 4);
#undef OK_RENDER_LAUNCH
        OK_HIP(h, hipGetLastError());
        return OKENV_OK;
    }

#if defined(OKENV_STAMPS)
    // stamps of the last step launch: kStampWords words per wave; returns the number of waves copied (<= waves) or an error (< 0)
    __attribute__((visibility("default"))) int okenv_debug_stamps(okenv_t h, unsigned long long *out, int waves)
    {
        OK_QUIESCE(h);
        OK_HIP(h, hipStreamSynchronize(h->stream));
        const size_t n = std::min(static_cast<size_t>(waves < 0 ? 0 : waves), h->stamp_waves);
        if (n > 0)
            OK_HIP(h, hipMemcpy(out, h->d_stamps, sizeof(unsigned long long) * kStampWords * n, hipMemcpyDeviceToHost));
        return static_cast<int>(n);
    }
#endif

    // ---- device self-checks ----------------------------------------------------------------------------------

    int okenv_debug_sincos(int32_t device, const float *x, float *s, float *c, int32_t n)
    {
        if (!x || !s || !c || n < 0)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_debug_sincos: bad argument");
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
            return fail(nullptr, OKENV_ERR_NO_DEVICE, "okenv_debug_sincos: no HIP device");
        if (n == 0)
            return OKENV_OK;
        OK_HIP(nullptr, hipSetDevice(device));
        float *d = nullptr;
        OK_HIP(nullptr, hipMalloc(reinterpret_cast<void **>(&d), 12U * static_cast<size_t>(n)));
        OK_HIP(nullptr, hipMemcpy(d, x, 4U * static_cast<size_t>(n), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(okDebugSincosKernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, d, d + n, d + 2 * static_cast<size_t>(n), n);
        OK_HIP(nullptr, hipGetLastError());
        OK_HIP(nullptr, hipMemcpy(s, d + n, 4U * static_cast<size_t>(n), hipMemcpyDeviceToHost));
        OK_HIP(nullptr, hipMemcpy(c, d + 2 * static_cast<size_t>(n), 4U * static_cast<size_t>(n), hipMemcpyDeviceToHost));
        OK_HIP(nullptr, hipFree(d));
        return OKENV_OK;
    }

    int okenv_debug_math(int32_t device, int32_t fn, const float *a, const float *b, float *out0, float *out1, int32_t n)
    {
        if (fn < 0 || fn >= OKENV_NUM_DEBUG_FNS || !a || !out0 || n < 0 || ((fn == OKENV_FN_ATAN2 || fn == OKENV_FN_SINCOS_PAIR) && !b) ||
            ((fn == OKENV_FN_SINCOS || fn == OKENV_FN_SINCOS_PAIR) && !out1))
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_debug_math: bad argument");
        switch (fn)
        {
        case OKENV_FN_SINCOS: return debugMath<OKENV_FN_SINCOS>(device, a, b, out0, out1, n);
        case OKENV_FN_TANH: return debugMath<OKENV_FN_TANH>(device, a, b, out0, out1, n);
        case OKENV_FN_EXP: return debugMath<OKENV_FN_EXP>(device, a, b, out0, out1, n);
        case OKENV_FN_LOG: return debugMath<OKENV_FN_LOG>(device, a, b, out0, out1, n);
        case OKENV_FN_ATAN2: return debugMath<OKENV_FN_ATAN2>(device, a, b, out0, out1, n);
        case OKENV_FN_NORMALIZE_ANGLE: return debugMath<OKENV_FN_NORMALIZE_ANGLE>(device, a, b, out0, out1, n);
        case OKENV_FN_SINCOS_PAIR: return debugMath<OKENV_FN_SINCOS_PAIR>(device, a, b, out0, out1, n);
        case OKENV_FN_ERF: return debugMath<OKENV_FN_ERF>(device, a, b, out0, out1, n);
        default: return debugMath<OKENV_FN_EXPERT_NORMALIZE_ANGLE>(device, a, b, out0, out1, n);
        }
    }

    int okenv_debug_adam_device(int32_t device, const okenv_learner_params *params, int64_t t, float *p, float *m, float *v, const float *g, int32_t n)
    {
        // okLearnCheckParams but for eps, which may be 0 here (include/okenv.h)
        okenv_learner_params checked{};
        if (params != nullptr)
        {
            checked = *params;
            if (checked.eps == 0.F)
                checked.eps = 1.F;
        }
        if (const char *why = okLearnCheckParams(params != nullptr ? &checked : nullptr))
            return fail(nullptr, OKENV_ERR_INVALID, std::string("okenv_debug_adam_device: ") + why);
        if (t < 1 || !p || !m || !v || !g || n < 0)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_debug_adam_device: bad argument");
        const ok_learn_adam_consts c     = okLearnAdamConsts(*params, t);
        const size_t               count = static_cast<size_t>(n);
        if (device == OKENV_DEBUG_ON_HOST)
        {
            for (size_t i = 0; i < count; ++i)
                ok_learn_adam(p + i, m + i, v + i, g[i], c);
            return OKENV_OK;
        }
        if (const int rc = debugNeedsDevice("okenv_debug_adam_device"))
            return rc;
        if (n == 0)
            return OKENV_OK;
        OK_HIP(nullptr, hipSetDevice(device));
        DebugBuffer buf;
        OK_HIP(nullptr, hipMalloc(reinterpret_cast<void **>(&buf.d), 16U * count));
        float *dp = buf.d, *dm = buf.d + count, *dv = buf.d + 2U * count, *dg = buf.d + 3U * count;
        OK_HIP(nullptr, hipMemcpy(dp, p, 4U * count, hipMemcpyHostToDevice));
        OK_HIP(nullptr, hipMemcpy(dm, m, 4U * count, hipMemcpyHostToDevice));
        OK_HIP(nullptr, hipMemcpy(dv, v, 4U * count, hipMemcpyHostToDevice));
        OK_HIP(nullptr, hipMemcpy(dg, g, 4U * count, hipMemcpyHostToDevice));
        const unsigned un = static_cast<unsigned>(n);
        hipLaunchKernelGGL(okDebugAdamKernel, dim3((un + 255U) / 256U), dim3(256), 0, nullptr, dp, dm, dv, dg, c, un);
        OK_HIP(nullptr, hipGetLastError());
        OK_HIP(nullptr, hipMemcpy(p, dp, 4U * count, hipMemcpyDeviceToHost));
        OK_HIP(nullptr, hipMemcpy(m, dm, 4U * count, hipMemcpyDeviceToHost));
        OK_HIP(nullptr, hipMemcpy(v, dv, 4U * count, hipMemcpyDeviceToHost));
        return OKENV_OK;
    }

    static int workStats(okenv_t h, uint64_t *out, const int n_out, const bool split, const char *who)
    {
        if (!h || !out)
            return fail(h, OKENV_ERR_INVALID, std::string(who) + ": NULL argument");
        if (h->shape.grid_mode != kGridLds)
            return fail(h, OKENV_ERR_STATE, std::string(who) + ": needs the LDS form of the grid");
        if (split && !h->shape.fb_ok)
            return fail(h, OKENV_ERR_STATE, std::string(who) + ": the segment set has no front / back split (okenv_info.front_back_bytes == 0)");
        OK_HIP(h, hipSetDevice(h->device));
        void     *sp  = nullptr;
        const int src = deviceScratch(h, 8U * sizeof(unsigned long long), &sp);
        if (src != OKENV_OK)
            return src;
        OK_HIP(h, hipMemsetAsync(sp, 0, 8U * sizeof(unsigned long long), h->stream));
        OkStepParams p = baseParams(h);
        if (split)
            useFrontBack(h, p);
        if (const int lrc = raiseLdsLimit(h, {kernelOf(okWorkStatsKernel)}))
            return lrc;
        const long total  = static_cast<long>(h->shape.N) * h->shape.R;
        const int  blocks = static_cast<int>(std::min<long>(256, (total + 1023) / 1024));
        hipLaunchKernelGGL(okWorkStatsKernel, dim3(blocks), dim3(1024), p.image_bytes, h->stream, p, static_cast<unsigned long long *>(sp));
        OK_HIP(h, hipGetLastError());
        unsigned long long host[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        OK_HIP(h, hipMemcpyAsync(host, sp, sizeof(host), hipMemcpyDeviceToHost, h->stream));
        OK_HIP(h, hipStreamSynchronize(h->stream));
        for (int i = 0; i < n_out; ++i)
            out[i] = host[i];
        return OKENV_OK;
    }

    int okenv_work_stats(okenv_t h, uint64_t out[4])
    {
        OK_QUIESCE(h);
        return workStats(h, out, 4, false, "okenv_work_stats");
    }

    int okenv_work_stats_split(okenv_t h, uint64_t out[8])
    {
        OK_QUIESCE(h);
        return workStats(h, out, 8, true, "okenv_work_stats_split");
    }

    int okenv_debug_cast_rays(okenv_t h, const float *ox, const float *oy, const float *angle_rad, int32_t n, float *out_t)
    {
        OK_QUIESCE(h);
        if (!h || !ox || !oy || !angle_rad || !out_t || n < 0)
            return fail(h, OKENV_ERR_INVALID, "okenv_debug_cast_rays: bad argument");
        if (n == 0)
            return OKENV_OK;
        OK_HIP(h, hipSetDevice(h->device));
        void     *sp  = nullptr;
        const int src = deviceScratch(h, 16U * static_cast<size_t>(n), &sp);
        if (src != OKENV_OK)
            return src;
        float *d = static_cast<float *>(sp);
        OK_HIP(h, hipMemcpyAsync(d, ox, 4U * static_cast<size_t>(n), hipMemcpyHostToDevice, h->stream));
        OK_HIP(h, hipMemcpyAsync(d + n, oy, 4U * static_cast<size_t>(n), hipMemcpyHostToDevice, h->stream));
        OK_HIP(h, hipMemcpyAsync(d + 2 * static_cast<size_t>(n), angle_rad, 4U * static_cast<size_t>(n), hipMemcpyHostToDevice, h->stream));
        const OkStepParams p      = baseParams(h);
        const int          blocks = std::min(1024, (n + 1023) / 1024);
        float             *dt     = d + 3 * static_cast<size_t>(n);
        switch (h->shape.grid_mode)
        {
        case kGridLds:
            hipLaunchKernelGGL(okDebugCastKernel<kGridLds>, dim3(blocks), dim3(1024), h->shape.image_bytes, h->stream, p, d, d + n,
                               d + 2 * static_cast<size_t>(n), n, dt);
            break;
        case kGridGlobal:
            hipLaunchKernelGGL(okDebugCastKernel<kGridGlobal>, dim3(blocks), dim3(1024), 0, h->stream, p, d, d + n,
                               d + 2 * static_cast<size_t>(n), n, dt);
            break;
        default:
            hipLaunchKernelGGL(okDebugCastKernel<kGridBrute>, dim3(blocks), dim3(1024), 0, h->stream, p, d, d + n,
                               d + 2 * static_cast<size_t>(n), n, dt);
            break;
        }
        OK_HIP(h, hipGetLastError());
        OK_HIP(h, hipMemcpyAsync(out_t, dt, 4U * static_cast<size_t>(n), hipMemcpyDeviceToHost, h->stream));
        OK_HIP(h, hipStreamSynchronize(h->stream));
        return OKENV_OK;
    }

    int okenv_debug_step_forms(okenv_t h, uint64_t *out, int32_t n_words, int32_t clear)
    {
        OK_QUIESCE(h);
        constexpr int32_t kWords = OKENV_NUM_STEP_FORMS * (1 + OKENV_NUM_STEP_FORM_ATTRS);
        if (!h || !out || n_words < kWords)
            return fail(h, OKENV_ERR_INVALID, "okenv_debug_step_forms: bad argument (out needs OKENV_NUM_STEP_FORMS * (1 + OKENV_NUM_STEP_FORM_ATTRS) words)");
        std::memcpy(out, h->form_counts, sizeof(h->form_counts));
        if (clear != 0)
            std::memset(h->form_counts, 0, sizeof(h->form_counts));
        return OKENV_OK;
    }

    // The launch policy on plain numbers: the same okPlanLanes / okPlanGeometry / okPlanStep a handle goes through, without one.
    int okenv_debug_plan_step(const okenv_plan_query *q, okenv_plan_result *out)
    {
        if (!q || !out || q->num_agents <= 0 || q->num_rays <= 0 || q->compute_units <= 0 || q->image_bytes < 0 || q->front_back_bytes < 0 ||
            q->q_bytes < 0)
            return fail(nullptr, OKENV_ERR_INVALID, "okenv_debug_plan_step: bad argument");
        OkKnobs k;
        k.lanes_per_agent  = q->lanes_per_agent;
        k.block_threads    = q->block_threads;
        k.coop             = q->coop;
        k.agents_per_block = q->agents_per_block;
        k.tail_max_agents  = q->tail_max_agents;
        k.phase1_range     = q->phase1_range;
        k.resident         = q->resident;
        k.front_back       = q->front_back;
        OkLaunchShape s = okPlanLanes(q->num_agents, q->num_rays, q->compute_units, k);
        okPlanGeometry(s, q->flags, q->image_fits_lds != 0, k);
        if (s.grid_mode == kGridLds)
        { // (what okenv_create learns from the grid builder and the front / back classification)
            s.image_bytes = static_cast<size_t>(q->image_bytes);
            s.fb_ok       = s.front_back && q->front_back_bytes > 0;
            s.fb_bytes    = s.fb_ok ? static_cast<size_t>(q->front_back_bytes) : 0U;
        }
        OkStepRequest rq;
        rq.action_source   = q->action_source;
        rq.n_listed        = q->n_listed;
        rq.packed          = q->packed != 0;
        rq.resident        = q->resident_launch != 0;
        rq.do_move         = q->do_move;
        rq.reset_flags     = q->reset_flags;
        rq.ctrl_num_params = q->ctrl_num_params;
        rq.q_bytes         = static_cast<size_t>(q->q_bytes);
        if (q->n_listed == OKENV_PLAN_FIRST_ROLLOUT)
            rq.n_listed = okPrelist(s, rq.action_source, rq.q_bytes) ? s.N : -1;
        const OkStepPlan pl    = okPlanStep(s, rq);
        out->lanes_per_agent   = s.G;
        out->natural_lanes     = s.natural_g;
        out->rays_per_lane     = s.rays_per_lane;
        out->phase1_range      = s.phase1_range;
        out->grid_cell         = s.cell_default;
        out->grid_mode         = s.grid_mode;
        out->front_back_built  = s.front_back ? 1 : 0;
        out->block_threads     = s.block_threads;
        out->grid_blocks       = s.grid_blocks;
        out->coop              = s.coop ? 1 : 0;
        out->agents_per_block  = s.agents_per_block;
        out->tail_max_agents   = s.tail_max_agents;
        out->resident_mode     = s.resident_mode;
        out->resident_eligible = okResidentShape(s) ? 1 : 0;
        out->tail_limit        = static_cast<int32_t>(okTailLimit(s, rq.action_source == kActionsQLearning, rq.q_bytes));
        out->form              = pl.form;
        out->launch_grid       = static_cast<int32_t>(pl.grid);
        out->launch_block      = static_cast<int32_t>(pl.block);
        out->launch_lds_bytes  = static_cast<int32_t>(pl.lds);
        out->launch_image_off  = static_cast<int32_t>(pl.image_off);
        out->launch_phase1     = pl.phase1;
        out->launch_lanes      = pl.G;
        out->launch_front_back = pl.front_back ? 1 : 0;
        out->launch_ctrl_lds_off = static_cast<int32_t>(pl.ctrl_lds_off);
        out->launch_waves        = static_cast<int32_t>(pl.waves());
        return OKENV_OK;
    }
}
