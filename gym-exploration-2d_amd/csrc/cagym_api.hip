// cagym_api.hip -- C ABI of libcagym_hip.so (include/cagym.h): handle, device buffers, launches.
// No torch types, no CPU fallback: without a HIP device cagym_create fails.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cagym.h"
#include "../../include/cagym_ig_observe.h"
#include "../../include/cagym_ig_context.h"
#include "../../include/cagym_ig_goals.h"
#include "../../include/cagym_ig_viewpoints.h"
#include "../../include/cagym_ig_headings.h"
#include "../../include/cagym_ig_assign.h"
#include "../../include/cagym_ig_route.h"
#include "../../include/cagym_ig_credit.h"
#include "../../include/cagym_ig_episode_log.h"
#include "cagym_gen1.h"
#include "cagym_sensors.h"
#include "cagym_kernels3.h"  // LDS layout helpers; the kernels themselves are instantiated in the cagym_k3_tu.hip units
#include "cagym_split3.h"
#include "cagym_launch3.h"
#ifdef CAGYM_MONOLITHIC  // diagnostic builds: every generation-3 specialisation in this one translation unit
#include "cagym_k3_all.inc"
#endif
#include "cagym_ig.h"
#include "cagym_ga3c.h"
#include "cagym_ga3c16.h"
#include "cagym_gen.h"
#include "cagym_gen2.h"
#include "cagym_dmcts.h"
#include "cagym_ig_episode.h"
#include "cagym_ig_greedy.h"
#include "cagym_ig_observe.h"
#include "cagym_ig_context.h"
#include "cagym_ig_geodesic.h"
#include "cagym_ig_viewpoints.h"
#include "cagym_ig_headings.h"
#include "cagym_ig_assign.h"
#include "cagym_ig_route.h"
#include "cagym_ig_credit.h"
#include "cagym_ig_episode_log.h"
#include "cagym_episode_records.h"
#include "cagym_episode_log.h"
#include "cagym_snapshot.h"
#include "cagym_stream.h"
#include "cagym_explore.h"
#include "cagym_replay.h"
#include "cagym_terminal.h"
#include "cagym_checkpoint.h"
#include "cagym_layout.h"

namespace {

thread_local std::string g_last_error;

struct Env {
    cagym_config cfg;
    CagymDev D;
    std::vector<void*> allocs;
    std::string err;
    bool scenarios_set = false;
    double* sc_obst = nullptr;
    float4* sc_obst_prep = nullptr;
    double* sc_heading_buf = nullptr;
    IgDev G{};
    uint32_t* ig_any = nullptr;
    IgEpisode ig_ep{};  // the team reward's per-world episode accumulators (cagym_ig_episode_boundary)
    int32_t* gen_failed = nullptr;  // device word: agents whose rejection loop hit max_tries (cagym_generate_scenarios)
    int32_t* ga3c_ctr = nullptr;    // device words of cagym_ga3c_act's list (k_ga3c_select): ticket, list start, list length
    unsigned char* ga3c_packed = nullptr;   // the weight blob as split f16 operand fragments (k_ga3c_pack16, cagym_ga3c16.h)
    const float* ga3c_packed_src = nullptr; // the blob it was packed from (cagym_ga3c_load_weights)
    int32_t* status_host = nullptr; // host-mapped word the kernels' bounded waits report into (CagymDev::dev_status, cagym_spin.h)
    bool ig_ready = false;
    int any_rvo = 1;
    int obst_rvo = 0;    // RVO agents in worlds with rectangles: the kernels build obstacle half-planes (OBST instantiations)
    int generation = 3;  // CAGYM_KERNEL=v1 selects the one-lane-per-agent kernels (bitwise A/B only)
    int wpw10 = 5;       // worlds per workgroup of the M = 10 kernels (4 while all workgroups are co-resident)
    size_t pre_lds_min = 0;  // CAGYM_PRE_LDS (bytes, read at creation): the PRE half asks for at least this much LDS per workgroup - a cap on how
                             // many of its workgroups share a CU with the caller's policy kernel (tools/cfg4_overlap.py)
    bool begun = false;  // cagym_step_begin was enqueued and no cagym_step_finish has consumed its velocities yet
    EpRec rec{};         // per-scenario episode records (cagym_episode_records_init allocates them)
    bool rec_ready = false;
    EpLog elog{};        // append-only episode log (cagym_episode_log_init allocates it: the running block once, the ring per capacity)
    bool log_ready = false;
    void* elog_ring = nullptr;  // the ring's one allocation (EpLog's row columns are carved from it)
    int n_ig = 0;        // IG robots (active CAGYM_POL_IGMCTS slots) of every scenario of the pool; N_IG_UNEQUAL when the scenarios
                         // differ, N_IG_RANDOM when cagym_generate_scenarios may have drawn some (cagym_ig_robot_inputs / _actions)
    bool streaming = false;          // cagym_stream_scenarios started the ring and no pool setter or cagym_stream_stop ended it
    StreamDev stream{};              // its device words (allocated by the first cagym_stream_scenarios; csrc/cagym_stream.h)
    cagym_gen2_params stream_P{};    // the parameter set cagym_stream_refill generates with (cagym_stream_set_params replaces it)
    bool explore_stream = false;     // while streaming: cagym_stream_exploration_scenarios started the ring (csrc/cagym_explore.h)
    ExploreTeam stream_team{};       // its team edit (cagym_stream_set_exploration_params replaces it together with stream_P)
    ExploreDev explore{};            // the field refresh's device words (allocated by the first cagym_stream_exploration_scenarios)
    bool replay_on = false;          // while streaming: cagym_stream_replay_init armed the replay refill (csrc/cagym_replay.h)
    ReplayDev replay{};              // its device words and per-slot tables (allocated by the first cagym_stream_replay_init)
    void* replay_ring = nullptr;     // the buffer's one allocation (once per capacity)
    double replay_p = 0.0;           // cagym_stream_replay_set
    uint32_t replay_mask = 0;
    uint64_t replay_seed = 0;
    uint32_t stream_gen = 1;         // parameter generation: 1 at the stream's start, + 1 with every cagym_stream_set_params
    uint8_t* go_scratch = nullptr;   // [N] game_over of cagym_step_autoreset_keep when the caller gives none
    TrajRing traj{};                 // trajectory ring (cagym_trajectory_init allocates it: the running block once, the ring per n_slices)
    bool traj_ready = false;
    void* traj_ring = nullptr;       // the ring's one allocation (TrajRing's planes are carved from it)
    IgEpLog iglog{};                 // the IG team's episode log (cagym_ig_episode_log_init allocates it: the running block once, the ring per capacity)
    bool iglog_ready = false;
    void* iglog_ring = nullptr;      // the ring's one allocation (IgEpLog's row columns are carved from it)
};
enum { N_IG_UNEQUAL = -1, N_IG_RANDOM = -2 };

int fail(Env* e, int code, const std::string& msg) {
    g_last_error = msg;
    if (e) e->err = msg;
    return code;
}

#define HIPCHK(e, call)                                                                              \
    do {                                                                                             \
        hipError_t _s = (call);                                                                      \
        if (_s != hipSuccess)                                                                        \
            return fail(e, CAGYM_E_HIP, std::string(#call) + ": " + hipGetErrorString(_s));          \
    } while (0)

// Every launching entry point runs with the handle's device current (a C caller may hold handles on several devices:
// "one process, 8 handles") and leaves the caller's current device as it found it.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t status = hipSuccess;
    explicit DeviceGuard(int dev) {
        status = hipGetDevice(&prev);
        if (status == hipSuccess && prev != dev) {
            status = hipSetDevice(dev);
            switched = status == hipSuccess;
        }
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};
// The prologue of a launching entry point is two statements.  ENTRY* turns `void* env` into `Env* e` and checks the handle and the
// state the call needs; ON_DEVICE makes the handle's device current and refuses after a void launch (device_status).  A function's
// own argument checks stay where they always were, before or after ON_DEVICE: which of two errors wins is part of the ABI.
#define ENTRY_IF(e, env, state_ok, msg)                                \
    Env* e = reinterpret_cast<Env*>(env);                              \
    if (!e) return fail(nullptr, CAGYM_E_INVALID, "null env");         \
    if (!(state_ok)) return fail(e, CAGYM_E_STATE, msg)
#define ENTRY(e, env) ENTRY_IF(e, env, true, "")
#define ENTRY_POOL(e, env, name) ENTRY_IF(e, env, e->scenarios_set, name " before cagym_set_scenarios")
#define ENTRY_IG(e, env, name) ENTRY_IF(e, env, e->ig_ready, name " before cagym_ig_init")
// ... behind ENTRY_POOL, of a call that needs what an *_init call sets up (a missing pool is reported first)
#define REQUIRE(e, ready, name, init) \
    if (!(ready)) return fail(e, CAGYM_E_STATE, name " before " init)
#define ON_DEVICE(e)                                                                                       \
    DeviceGuard _guard((e)->cfg.device);                                                                   \
    if (_guard.status != hipSuccess) return fail(e, CAGYM_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(_guard.status)); \
    if (int _rc = device_status(e)) return _rc
// ... of a call that moves the state a pending cagym_step_begin solved for: its velocities must not be consumed any more.
// (The scenario setters clear `begun` themselves, on success only: a refused call leaves the handle as it was.)
#define ON_DEVICE_VOIDS_BEGUN(e) \
    ON_DEVICE(e);                \
    (e)->begun = false

// A kernel whose bounded intra-workgroup wait expired (cagym_spin.h) wrote its CAGYM_DEVERR_* code into the handle's host-mapped
// status word: the launches since then produced void results.  Every launching entry point refuses to go on (the word is sticky
// until cagym_destroy: the state on the device is not trustworthy any more).
int device_status(Env* e) {
    const int32_t code = e->status_host ? *reinterpret_cast<volatile int32_t*>(e->status_host) : 0;
    if (code == CAGYM_DEVERR_NONE) return CAGYM_OK;
    return fail(e, CAGYM_E_DEVICE, std::string("a kernel of an earlier launch gave up a bounded wait (") +
                                       (code == CAGYM_DEVERR_LP_WAIT ? "LP waves" : code == CAGYM_DEVERR_LASER_WAIT ? "LaserScan passes" : code == CAGYM_DEVERR_PAIR_WAIT ? "pair phase" : "unknown") +
                                       "): results since then are void, destroy the handle");
}

template <typename T>
int dalloc(Env* e, T** p, size_t n) {
    void* q = nullptr;
    size_t bytes = (n ? n : 1) * sizeof(T);
    hipError_t s = hipMalloc(&q, bytes);
    if (s != hipSuccess) return fail(e, CAGYM_E_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(s));
    s = hipMemset(q, 0, bytes);
    if (s != hipSuccess) return fail(e, CAGYM_E_HIP, std::string("hipMemset: ") + hipGetErrorString(s));
    e->allocs.push_back(q);
    *p = reinterpret_cast<T*>(q);
    return CAGYM_OK;
}

// the kernels' view of the caller's outputs; a handle without a LaserScan sensor passes no laserscan pointer on
// (scan_as_given: cagym_reset hands k_reset the caller's pointer whatever the handle says, only its follow-up scan is conditional)
CagymOut to_out(const Env* e, const cagym_outputs* o, bool scan_as_given = false) {
    CagymOut r{};
    if (o) {
        r.obs_oas = o->obs_oas;
        r.obs_ego = o->obs_ego;
        r.laserscan = (e->cfg.laserscan || scan_as_given) ? o->laserscan : nullptr;
        r.reward = o->reward;
        r.flags = o->flags;
        r.game_over = o->game_over;
    }
    return r;
}

// worlds per workgroup of the compile-time specialisations (0 = generic: 64 / M worlds, LDS stride 64)
//   M = 4 : 16 worlds,  96 unordered pairs per phase round of 256 lanes
//   M = 10:  5 worlds (225 unordered / 500 directed pair slots, ~35 live agents = 2 rounds of 32 LP groups), or
//            4 worlds while every workgroup of the launch is co-resident (<= 5 per CU): ~28 live agents = one
//            round of LP groups; measured 4096 worlds: 259 vs 247 M env-steps/s, 65536 worlds: 342 vs 392
//   M = 20:  2 worlds, 380 unordered / 800 directed pair slots on 256 lanes (5 workgroups per CU instead of 2)
#define WPW20 2
#define NT20 256  /* lanes per workgroup of the M = 20 specialisation (512: 64 vs 78 M env-steps/s at 2048 x 20) */
// kernel specialisation of the handle: lanes per workgroup, compile-time M (0 = generic) and worlds per workgroup
// (0 = 64 / M worlds, LDS stride 64)
struct Spec2 {
    int nt, mt, wpw;
};
inline Spec2 spec2(int M, int wpw10) {
    if (M == 10) return {256, 10, wpw10};
    if (M == 4) return {256, 4, 0};
    if (M == 20) return {NT20, 20, WPW20};
    if (M <= 12) return {256, 0, 0};
    return {512, 0, 0};
}
inline Spec2 spec2(const Env* e) { return spec2(e->cfg.max_agents, e->wpw10); }
inline int wpw_spec(const Env* e) { return spec2(e).wpw; }
inline int n_wg2(const Env* e) {
    const int M = e->cfg.max_agents;
    const int wpw = wpw_spec(e) ? wpw_spec(e) : CAGYM_WAVE / M;
    return (e->cfg.n_worlds + wpw - 1) / wpw;
}
// obst: the OBST instantiation (worlds may hold rectangles); lines: RVO agents among them (obstacle half-plane rows)
inline size_t lds3_bytes(const cagym_config& cfg, const Spec2 sp, bool obst, bool lines) {
    const int M = cfg.max_agents;
    return cagym_lds3_bytes(M, cagym_as(M, sp.wpw), sp.nt, (obst && lines) ? 2 * cfg.max_obstacles : 0, cagym_lpl3(sp.mt, obst), obst, sp.mt);
}
inline size_t lds3_bytes(const Env* e, bool obst, bool lines) { return lds3_bytes(e->cfg, spec2(e), obst, lines); }
inline bool has_map(const Env* e) { return e->cfg.max_obstacles > 0; }
inline size_t scan_bytes(const Env* e) { return (size_t)e->cfg.n_worlds * e->cfg.max_agents * 16 * sizeof(float); }
inline size_t lds3_bytes(const Env* e) { return lds3_bytes(e, has_map(e), e->obst_rvo != 0); }
// the one-step launch of a handle with rectangles runs on the time-shared layout (carve_lds3_ovl)
inline size_t lds3_step_bytes(const Env* e) {
    if (!has_map(e)) return lds3_bytes(e);
    return cagym_lds3_ovl_bytes(e->cfg.max_agents, cagym_as(e->cfg.max_agents, wpw_spec(e)), spec2(e).nt, e->D.ko);
}
// LP group width of the handle's specialisation (run_steps3)
inline int lp_group_width(const Env* e) {
    const int mt = spec2(e).mt;
    return cagym_gw3(mt);
}

inline int n_waves(const Env* e) {
    int wpw = CAGYM_WAVE / e->cfg.max_agents;
    return (e->cfg.n_worlds + wpw - 1) / wpw;
}

// the one place that maps a handle to its kernel instantiation
// (the launchers live in the per-specialisation translation units, cagym_k3_tu.hip)
struct K3Entry {
    int nt, mt, wp;
    void (*launch[2])(const K3Launch&);  // [OBST]
    void (*setattr[2])(int);
};
#define K3_ROW(NT, MT, WP)                                                                     \
    {NT, MT, WP, {cagym_k3_launch_##NT##_##MT##_##WP##_0, cagym_k3_launch_##NT##_##MT##_##WP##_1}, \
     {cagym_k3_setattr_##NT##_##MT##_##WP##_0, cagym_k3_setattr_##NT##_##MT##_##WP##_1}},
const K3Entry k3_table[] = {CAGYM_K3_SPECS(K3_ROW)};
#undef K3_ROW
inline const K3Entry* k3_entry(const Env* e) {
    const Spec2 sp = spec2(e);
    for (const K3Entry& r : k3_table)
        if (r.nt == sp.nt && r.mt == sp.mt && r.wp == sp.wpw) return &r;
    return nullptr;
}
// one generation-3 launch of the handle's specialisation (free-space or OBST instantiation): the fused step or roll-out
// (K3_HALF_NONE) or one half of the split step, which differ in their LDS footprint and in who solves the RVO agents
inline void launch3(const Env* e, int half, bool rollout, bool auto_reset, const float* ext, int n_steps, const CagymOut& o, hipStream_t st) {
    const int M = e->cfg.max_agents, as = cagym_as(M, wpw_spec(e));
    K3Launch L;
    L.D = e->D; L.half = half; L.ext = ext; L.out = o; L.n_steps = n_steps; L.rollout = rollout; L.auto_reset = auto_reset;
    L.grid = (unsigned)n_wg2(e); L.stream = st;
    if (half == K3_HALF_PRE) {  // launched only when the pool has RVO agents
        L.any_rvo = 1;
        L.lds = cagym_lds3_pre_bytes(M, as, spec2(e).nt, has_map(e) ? e->D.ko : 0);
        if (L.lds < e->pre_lds_min && e->pre_lds_min <= 64 * 1024) L.lds = e->pre_lds_min;
    } else if (half == K3_HALF_POST) {  // the velocities are in CagymDev::lp_vel
        L.any_rvo = 0;
        L.lds = cagym_lds3_post_bytes(M, as, has_map(e) ? e->D.ko / 2 : 0, has_map(e));
    } else {
        L.any_rvo = e->any_rvo;
        L.lds = rollout ? lds3_bytes(e) : lds3_step_bytes(e);
#ifdef CAGYM_DIAG_LDS_PAD  // occupancy experiments only (tools/README.md): unused LDS bytes on top, to force fewer workgroups per CU
        if (const char* pad = getenv("CAGYM_LDS_PAD")) L.lds += (size_t)atoi(pad);
#endif
    }
    k3_entry(e)->launch[has_map(e) ? 1 : 0](L);
}
// A handle without rectangles runs the free-space kernels, which write no laserscan: every beam of an empty map reads 0.0
// (LaserScanSensor.py:27-58 on an all-free Map), in all n_steps slices of a roll-out.  Generation 1 scans through cagym_laserscan.
// (HIPCHK's message quotes the call, so both spellings are kept.)
inline int fill_empty_scan(Env* e, const CagymOut& o, hipStream_t st, int n_steps = 0) {
    if (e->generation != 3 || has_map(e) || !o.laserscan) return CAGYM_OK;
    if (n_steps) HIPCHK(e, hipMemsetAsync(o.laserscan, 0, (size_t)n_steps * scan_bytes(e), st));
    else HIPCHK(e, hipMemsetAsync(o.laserscan, 0, scan_bytes(e), st));
    return CAGYM_OK;
}

// the episode recorder's restart / clear launch (csrc/cagym_episode_records.h); a no-op for handles that never initialised it
inline int eprec_restart(Env* e, const uint8_t* world_mask, bool clear_table, hipStream_t st) {
    if (!e->rec_ready) return CAGYM_OK;
    const size_t rows = (size_t)std::max(e->cfg.n_worlds, clear_table ? e->cfg.n_scenarios : 0) * e->cfg.max_agents;
    const unsigned grid = (unsigned)std::min<size_t>((rows + 255) / 256, 4096);
    hipLaunchKernelGGL(k_episode_records_restart, dim3(grid), dim3(256), 0, st, e->D, e->rec, world_mask, clear_table ? 1 : 0);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

// the episode log's restart / clear launch (csrc/cagym_episode_log.h); a no-op for handles that never initialised it
inline int eplog_restart(Env* e, const uint8_t* world_mask, bool clear_rows, hipStream_t st) {
    if (!e->log_ready) return CAGYM_OK;
    const size_t rows = (size_t)std::max(e->cfg.n_worlds, clear_rows ? e->elog.capacity : 0) * e->cfg.max_agents;
    const unsigned grid = (unsigned)std::min<size_t>((rows + 255) / 256, 4096);
    hipLaunchKernelGGL(k_episode_log_restart, dim3(grid), dim3(256), 0, st, e->D, e->elog, world_mask, clear_rows ? 1 : 0);
    HIPCHK(e, hipGetLastError());
    if (clear_rows && e->replay.words)  // head restarts at 0: so does the row number the replay harvest has reached
        HIPCHK(e, hipMemsetAsync(e->replay.words + RPW_CURSOR, 0, sizeof(unsigned long long), st));
    return CAGYM_OK;
}
// the trajectory ring's restart / clear (csrc/cagym_terminal.h); a no-op for handles that never initialised it
inline int traj_restart(Env* e, const uint8_t* world_mask, bool clear, hipStream_t st) {
    if (!e->traj_ready) return CAGYM_OK;
    const size_t NM = (size_t)e->cfg.n_worlds * e->cfg.max_agents;
    if (clear) {  // every slice: `last` closes the ring; head, desync and the workgroups' copies of head open the running block (traj_*_members)
        const TrajRing& R = e->traj;
        const unsigned char* const ring_end = R.last + (size_t)e->cfg.n_worlds * R.L;
        const unsigned char* const words_end = reinterpret_cast<const unsigned char*>(R.head_wg + tcap_slice_wgs(e->cfg.n_worlds, e->cfg.max_agents));
        HIPCHK(e, hipMemsetAsync(e->traj_ring, 0, (size_t)(ring_end - static_cast<const unsigned char*>(e->traj_ring)), st));
        HIPCHK(e, hipMemsetAsync(e->traj.head, 0, (size_t)(words_end - reinterpret_cast<const unsigned char*>(R.head)), st));
    }
    hipLaunchKernelGGL(k_trajectory_restart, dim3((unsigned)std::min<size_t>((NM + 255) / 256, 4096)), dim3(256), 0, st, e->D, e->traj, world_mask);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}
// the IG team's episode log's restart / clear launch (csrc/cagym_ig_episode_log.h); a no-op for handles that never initialised it
inline int iglog_restart(Env* e, const uint8_t* world_mask, bool clear_rows, hipStream_t st) {
    if (!e->iglog_ready) return CAGYM_OK;
    const size_t rows = (size_t)std::max(e->cfg.n_worlds, clear_rows ? e->iglog.capacity : 0) * e->cfg.max_agents;
    const unsigned grid = (unsigned)std::min<size_t>((rows + 255) / 256, 4096);
    hipLaunchKernelGGL(k_ig_episode_log_restart, dim3(grid), dim3(256), 0, st, e->D, e->iglog, world_mask, clear_rows ? 1 : 0);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}
// The three behind cagym_reset - the episode the masked worlds abandon leaves no record, no row, and its rows in the ring without a
// `last` slice - and behind a new pool (every world): the records describe the pool (cleared); the log and the ring are history (their
// rows stay, the running values go)
inline int episodes_restart(Env* e, const uint8_t* world_mask, bool new_pool, hipStream_t st) {
    if (int rc = eprec_restart(e, world_mask, new_pool, st)) return rc;
    if (int rc = eplog_restart(e, world_mask, false, st)) return rc;
    if (int rc = iglog_restart(e, world_mask, false, st)) return rc;  // (the IG team's log: history too)
    return traj_restart(e, world_mask, false, st);
}
// every slot's raster from its rectangles (FIELD_RASTER); a handle without rectangles has none
inline int rasterize_pool(Env* e, hipStream_t st) {
    if (e->cfg.max_obstacles <= 0) return CAGYM_OK;
    hipLaunchKernelGGL(k_rasterize, dim3((unsigned)e->cfg.n_scenarios), dim3(256), 0, st, e->sc_obst, e->D.sc_nobst, e->cfg.max_obstacles,
                       const_cast<uint32_t*>(e->D.map_bits));
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}
// the reset kernel as cagym_reset and cagym_step_autoreset_keep launch it
inline int launch_reset(Env* e, const uint8_t* world_mask, int advance_episode, const CagymOut& o, hipStream_t st) {
    hipLaunchKernelGGL(k_reset, dim3(n_waves(e)), dim3(64), cagym_lds_bytes(e->cfg.max_agents), st, e->D, world_mask,
                       advance_episode, o);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

// ---- the handle's per-world and per-slot arrays: ONE list each, walked by alloc_state and by the field tables of csrc/cagym_snapshot.h.
// The order of a list is the order of its allocations and the order inside a blob row.  A new array is one new row here, and a
// CAGYM_SNAP_VERSION / CAGYM_CKPT_VERSION bump if the row rides in a blob.
enum {
    FIELD_SNAP = 1,    // state: rides in a snapshot's blob row
    FIELD_FORK = 2,    // cagym_fork copies it
    FIELD_MAP = 4,     // pool: exists only on a handle with rectangles (max_obstacles > 0)
    FIELD_RASTER = 8,  // pool: a pure function of the rectangles - a checkpoint's row leaves it out, the load rasterizes again
    FIELD_SF = FIELD_SNAP | FIELD_FORK
};
// X(pointer, elements per world, flags), in terms of D (the handle's CagymDev) and M.  lp_vel is the split step's hand-over: restore
// and fork void a pending begin.  cagym_fork leaves dst its episode index and stat_*.
#define CAGYM_STATE_FIELDS(X) \
    X(D.px, M, FIELD_SF) X(D.py, M, FIELD_SF) X(D.vx, M, FIELD_SF) X(D.vy, M, FIELD_SF) X(D.heading, M, FIELD_SF) X(D.heading_ego, M, FIELD_SF) \
    X(D.dist_goal, M, FIELD_SF) X(D.time_rem, M, FIELD_SF) X(D.t, M, FIELD_SF) X(D.gx, M, FIELD_SF) X(D.gy, M, FIELD_SF) X(D.radius, M, FIELD_SF) \
    X(D.pref, M, FIELD_SF) X(D.speed, M, FIELD_SF) X(D.dhead, M, FIELD_SF) X(D.aux0, M, FIELD_SF) X(D.aux1, M, FIELD_SF) X(D.coop, M, FIELD_SF) \
    X(D.action, 2 * M, FIELD_SF) X(D.status, M, FIELD_SF) X(D.step_num, M, FIELD_SF) X(D.n_observed, M, FIELD_SF) X(D.lp_vel, M, 0) \
    X(D.n_agents, 1, FIELD_SF) X(D.episode, 1, FIELD_SNAP) X(D.ep_len, 1, FIELD_SF) X(D.ep_return, 1, FIELD_SF) \
    X(D.stat_return, 1, FIELD_SNAP) X(D.stat_episodes, 1, FIELD_SNAP) X(D.stat_steps, 1, FIELD_SNAP) X(D.stat_outcomes, 3, FIELD_SNAP)
// the tail of a blob row after cagym_ig_init, which allocates them (there is no fork on such a handle); e is the Env
#define CAGYM_IG_STATE_FIELDS(X) \
    X(e->G.belief, IG_BEL * IG_BEL, FIELD_SNAP) X(e->G.mi, IG_BEL * IG_BEL, FIELD_SNAP) \
    X(e->ig_ep.running, 1, FIELD_SNAP) X(e->ig_ep.sum, 1, FIELD_SNAP) X(e->ig_ep.last, 1, FIELD_SNAP) X(e->ig_ep.episodes, 1, FIELD_SNAP)
// X(pointer, elements per scenario slot, flags), in terms of D, e, M and K = max_obstacles
#define CAGYM_POOL_FIELDS(X) \
    X(D.sc_agents6, 6 * M, FIELD_FORK) X(e->sc_heading_buf, M, FIELD_FORK) X(D.sc_coop, M, FIELD_FORK) X(D.sc_policy, M, FIELD_FORK) \
    X(D.sc_dyn, M, FIELD_FORK) X(D.sc_nagents, 1, FIELD_FORK) X(D.sc_nobst, 1, FIELD_FORK) \
    X(D.map_bits, CAGYM_MAPD * CAGYM_MAPW, FIELD_FORK | FIELD_MAP | FIELD_RASTER) \
    X(e->sc_obst, 4 * K, FIELD_FORK | FIELD_MAP) X(e->sc_obst_prep, 4 * K, FIELD_FORK | FIELD_MAP)
#define FIELD_COUNT(p, elems, flags) +1
static_assert(0 CAGYM_STATE_FIELDS(FIELD_COUNT) CAGYM_IG_STATE_FIELDS(FIELD_COUNT) <= SNAP_MAX_FIELDS && 0 CAGYM_POOL_FIELDS(FIELD_COUNT) <= SNAP_MAX_FIELDS,
              "SnapTable holds every field of a row");
// alloc_state: one zero-filled array per row, `rows` worlds or slots long (the kernels read the pool through pointers to const)
template <typename T>
inline T*& field_mut(const T*& p) { return const_cast<T*&>(p); }
template <typename T>
inline T*& field_mut(T*& p) { return p; }
#define FIELD_ALLOC(p, elems, flags) \
    if (int rc = ((flags) & skip) ? CAGYM_OK : dalloc(e, &field_mut(p), rows * (elems))) return rc;

// The table of k_snapshot_copy over the rows of a list that have the flag `need` (0: any) and none of `skip`: each field at the next
// multiple of 16 behind the 16-byte header.  (SNAP_FORK / SNAP_POOL have no blob: the offsets only spread the lanes over the fields.)
struct SnapBuilder {
    SnapTable T;
    int need, skip;
    SnapBuilder(const Env* e, int mode, int need, int skip) : T{mode, 0, e->cfg.n_worlds, e->cfg.n_scenarios, e->D.episode, SNAP_HEADER_BYTES, {}}, need(need), skip(skip) {}
    void operator()(const void* base, size_t bytes, int flags) {
        if ((flags & need) != need || (flags & skip)) return;
        T.f[T.n_fields++] = {reinterpret_cast<unsigned char*>(const_cast<void*>(base)), (uint32_t)bytes, (uint32_t)T.row_bytes};
        T.row_bytes += layout_round16(bytes);
    }
};
#define FIELD_ADD(p, elems, flags) add(p, (elems) * sizeof(*(p)), flags);
// a snapshot's blob row (after cagym_ig_init with the IG tail), or with fork_only the table of cagym_fork's world -> world copy
inline SnapTable snap_state_table(const Env* e, int mode, bool fork_only = false) {
    const CagymDev& D = e->D;
    const size_t M = (size_t)e->cfg.max_agents;
    SnapBuilder add(e, mode, fork_only ? FIELD_FORK : FIELD_SNAP, 0);
    CAGYM_STATE_FIELDS(FIELD_ADD)
    if (e->ig_ready) { CAGYM_IG_STATE_FIELDS(FIELD_ADD) }
    return add.T;
}
// the pool rows of one scenario slot: what cagym_fork copies (SNAP_POOL: src's current slot over dst's), or a checkpoint's row
inline SnapTable snap_pool_table(const Env* e, int mode = SNAP_POOL) {
    const CagymDev& D = e->D;
    const size_t M = (size_t)e->cfg.max_agents, K = (size_t)e->cfg.max_obstacles;
    SnapBuilder add(e, mode, mode == SNAP_POOL ? FIELD_FORK : 0, (has_map(e) ? 0 : FIELD_MAP) | (mode == SNAP_POOL ? 0 : FIELD_RASTER));
    CAGYM_POOL_FIELDS(FIELD_ADD)
    return add.T;
}

inline cagym_snapshot_layout snap_layout(const Env* e) {
    cagym_snapshot_layout L{};
    L.magic = CAGYM_SNAP_MAGIC; L.version = CAGYM_SNAP_VERSION;
    L.n_worlds = e->cfg.n_worlds; L.max_agents = e->cfg.max_agents; L.n_scenarios = e->cfg.n_scenarios; L.max_obstacles = e->cfg.max_obstacles;
    L.fields = CAGYM_SNAP_CORE | (e->ig_ready ? CAGYM_SNAP_IG : 0u);
    L.row_bytes = snap_state_table(e, SNAP_GATHER).row_bytes;
    return L;
}

inline int snap_launch(Env* e, const SnapTable& T, const int32_t* ids, const int32_t* ids2, void* blob, int n, hipStream_t st) {
    if (n == 0) return CAGYM_OK;
    hipLaunchKernelGGL(k_snapshot_copy, dim3((unsigned)n), dim3(SNAP_NT), 0, st, T, ids, ids2, reinterpret_cast<unsigned char*>(blob));
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

// ---- the blocks of arrays that share one allocation (csrc/cagym_layout.h) ----------------------------------------------------------
// Each block's members are listed ONCE, with their element counts.  The listing gives the allocation's size, the members' pointers
// and - listing order is blob order - the entries of a checkpoint's flat sections (ckpt_flat_table).  A new member is one new v(...),
// and a CAGYM_CKPT_VERSION bump unless it is LAYOUT_SCRATCH or its block is in no checkpoint.
// the stream's words: `generated` with n_failed and n_lapped behind it is ONE 16-byte member (one memset, one field of a checkpoint)
template <class V> constexpr void stream_members(StreamDev& W, size_t N, V& v) { v(W.generated, 2); v(W.next_episode, N); }
// the exploration stream's field refresh: `fields_built` with n_list behind it (one memset), then field_next and the slot list
template <class V> constexpr void explore_members(ExploreDev& X, size_t N, size_t S, V& v) { v(X.fields_built, 2); v(X.field_next, N); v(X.list, S - N); }
// the episode log's ring of L rows, and its running block (pos and cnt live between the launches of one update)
template <class V> constexpr void eplog_ring_members(EpLog& G, size_t L, size_t M, V& v) {
    v(G.slice, L); v(G.ret, L); v(G.t, L * M); v(G.extra_t, L * M); v(G.key, L); v(G.world, L); v(G.episode, L); v(G.steps, L);
    v(G.outcome, L); v(G.n_agents, L); v(G.n_obst, L); v(G.flags, L * M);
}
template <class V> constexpr void eplog_run_members(EpLog& G, size_t N, size_t M, V& v) {
    v(G.run.t_run, N * M); v(G.run.ret_run, N); v(G.run.steps_run, N); v(G.run.atgoal_run, N); v(G.run.cursor, N); v(G.run.desync, 1);
    v(G.seq, 1); v(G.head, 1); v(G.pos, N, LAYOUT_SCRATCH); v(G.cnt, N, LAYOUT_SCRATCH);
}
// the IG team's episode log (in no checkpoint): its ring of L rows, and its running block (pos lives between the launches of one update)
template <class V> constexpr void iglog_ring_members(IgEpLog& G, size_t L, size_t M, V& v) {
    v(G.slice, L); v(G.ret, L); v(G.entropy, L); v(G.residual_mi, L); v(G.key, L); v(G.world, L); v(G.episode, L); v(G.steps, L);
    v(G.n_targets, L); v(G.n_found, L); v(G.n_touched, L); v(G.found_at, L * M);
}
template <class V> constexpr void iglog_run_members(IgEpLog& G, size_t N, size_t M, V& v) {
    v(G.head, 1); v(G.seq, 1); v(G.desync, 1); v(G.steps_run, N); v(G.cursor, N); v(G.found_run, N * M); v(G.pos, N, LAYOUT_SCRATCH);
}
// the replay's buffer of Q keys, and its words and per-slot tables
template <class V> constexpr void replay_ring_members(ReplayDev& R, size_t Q, V& v) { v(R.buf_key, Q); }
template <class V> constexpr void replay_table_members(ReplayDev& R, size_t S, V& v) { v(R.words, RPW_WORDS); v(R.buf_gen, 1); v(R.slot_key, S); v(R.slot_gen, S); }
// the trajectory ring's running block and its ring of L slices (in no checkpoint).  traj_restart clears head, desync and head_wg with
// one memset - they stay first and adjacent - and the ring up to the end of `last`, which stays its last member
template <class V> constexpr void traj_run_members(TrajRing& R, size_t NM, size_t n_wg, V& v) { v(R.head, 1); v(R.desync, 1); v(R.head_wg, n_wg); v(R.t_prev, NM); v(R.seen, NM); }
template <class V> constexpr void traj_ring_members(TrajRing& R, size_t N, size_t NM, size_t L, V& v) {
    v(R.rows, TRAJ_COLS * NM * L); v(R.episode, N * L); v(R.moved, NM * L); v(R.last, N * L);
}

// members: a block's listing with its sizes bound, [&](auto& v) { ..._members(G, ..., v); }
template <class F> inline size_t block_bytes(F members) {
    LayoutBytes b;
    members(b);
    return b.bytes;
}
// a zero-filled allocation of its own for the block, once per handle; the members point into it afterwards
template <class F> inline int block_alloc(Env* e, F members) {
    LayoutCarve carve{nullptr};
    if (int rc = dalloc(e, &carve.base, block_bytes(members))) return rc;
    members(carve);
    return CAGYM_OK;
}
// The one allocation of a ring's block (e->elog_ring, e->replay_ring, e->traj_ring: `name`), made again when its size changes: the
// new block first, and only when there is one the old block goes, behind a device sync (no launch may still use it).  quiet: a
// refused allocation must not surface as the next launch's error - the handle goes on as it was.
template <class F> inline int ring_alloc(Env* e, void** ring, const char* name, bool quiet, F members) {
    LayoutCarve carve{nullptr};
    if (int rc = dalloc(e, &carve.base, block_bytes(members))) {
        if (quiet) (void)hipGetLastError();
        return rc;
    }
    if (*ring) {
        HIPCHK(e, hipDeviceSynchronize());
        e->allocs.erase(std::find(e->allocs.begin(), e->allocs.end(), *ring));
        const hipError_t s = hipFree(*ring);
        if (s != hipSuccess) return fail(e, CAGYM_E_HIP, std::string("hipFree(e->") + name + "): " + hipGetErrorString(s));
    }
    *ring = carve.base;
    members(carve);
    return CAGYM_OK;
}

// the stream's device words, once per handle
inline int stream_alloc(Env* e) {
    const int N = e->cfg.n_worlds;
    StreamDev& W = e->stream;
    if (!W.next_episode) {
        if (int rc = block_alloc(e, [&](auto& v) { stream_members(W, N, v); })) return rc;
        W.n_failed = reinterpret_cast<int32_t*>(W.generated + 1); W.n_lapped = W.n_failed + 1;
    }
    W.episode = e->D.episode;
    W.map_bits = const_cast<uint32_t*>(e->D.map_bits);
    W.N = N;
    W.depth = e->cfg.n_scenarios / N;
    return CAGYM_OK;
}
// the log's running block (once per handle) and its ring (once per capacity); e->elog is complete afterwards
inline int eplog_alloc(Env* e, int capacity) {
    const size_t N = e->cfg.n_worlds, M = e->cfg.max_agents, L = (size_t)capacity;
    EpLog G = e->elog;
    if (!G.run.t_run) {
        if (int rc = block_alloc(e, [&](auto& v) { eplog_run_members(G, N, M, v); })) return rc;
        e->elog = G;  // kept whatever becomes of the ring's allocation
    }
    if (!e->elog_ring || G.capacity != capacity) {
        if (int rc = ring_alloc(e, &e->elog_ring, "elog_ring", false, [&](auto& v) { eplog_ring_members(G, L, M, v); })) return rc;
        G.capacity = capacity;
    }
    e->elog = G;
    return CAGYM_OK;
}
// the IG team's log: the running block (once per handle) and the ring (once per capacity); e->iglog is complete afterwards
inline int iglog_alloc(Env* e, int capacity) {
    const size_t N = e->cfg.n_worlds, M = e->cfg.max_agents, L = (size_t)capacity;
    IgEpLog G = e->iglog;
    if (!G.steps_run) {
        if (int rc = block_alloc(e, [&](auto& v) { iglog_run_members(G, N, M, v); })) return rc;
        e->iglog = G;  // kept whatever becomes of the ring's allocation
    }
    if (!e->iglog_ring || G.capacity != capacity) {
        if (int rc = ring_alloc(e, &e->iglog_ring, "iglog_ring", false, [&](auto& v) { iglog_ring_members(G, L, M, v); })) return rc;
        G.capacity = capacity;
    }
    e->iglog = G;
    return CAGYM_OK;
}
// the replay's words and per-slot tables (once per handle) and its buffer (once per capacity); e->replay is complete afterwards
inline int replay_alloc(Env* e, int capacity) {
    const size_t S = (size_t)e->cfg.n_scenarios;
    ReplayDev R = e->replay;
    if (!R.words) {
        if (int rc = block_alloc(e, [&](auto& v) { replay_table_members(R, S, v); })) return rc;
        e->replay = R;  // kept whatever becomes of the buffer's allocation
    }
    if (!e->replay_ring || R.Q != capacity) {
        if (int rc = ring_alloc(e, &e->replay_ring, "replay_ring", false, [&](auto& v) { replay_ring_members(R, (size_t)capacity, v); })) return rc;
        R.Q = capacity;
    }
    e->replay = R;
    return CAGYM_OK;
}

// ---- whole-handle checkpoint (csrc/cagym_checkpoint.h) -----------------------------------------------------------------------------------
// The host header of a checkpoint: opaque to the caller, plain words to the library.  Every member is written (the struct has no
// padding: static_assert below), so two saves of the same state give the same bytes.
struct CkptHost {
    uint32_t magic, version;
    uint64_t sizes[CAGYM_CKPT_SECTIONS];
    // cagym_config without `device`
    int32_t n_worlds, max_agents, n_scenarios, max_obstacles, game_over_mode, collide_with_static, laserscan, rvo_max_neighbors;
    double dt;
    int32_t cfg_reserved;
    // the pool's host state (cagym_set_scenarios / cagym_generate_*)
    int32_t scenarios_set, heading0_set, any_rvo, obst_rvo, n_ig;
    // cagym_stream_scenarios / cagym_stream_set_params
    int32_t streaming;
    uint32_t stream_gen;
    int32_t log_ready, log_capacity;  // cagym_episode_log_init
    // cagym_stream_replay_init / _set
    int32_t replay_on, replay_capacity;
    uint32_t replay_mask, reserved;
    double replay_p;
    uint64_t replay_seed;
    cagym_gen2_params stream_P;
};
static_assert(sizeof(CkptHost) == 8 + 8 * CAGYM_CKPT_SECTIONS + 8 * 4 + 8 + 4 + 5 * 4 + 2 * 4 + 2 * 4 + 4 * 4 + 8 + 8 + sizeof(cagym_gen2_params) &&
                  sizeof(cagym_gen2_params) == 64,
              "CkptHost has no padding");

// what a checkpoint does not carry
inline int ckpt_refuse(Env* e, const char* what) {
    const std::string w(what);
    if (e->streaming && e->explore_stream)
        return fail(e, CAGYM_E_UNSUPPORTED, w + " on an exploration stream: the per-slot distance fields are not part of a checkpoint");
    if (e->ig_ready)
        return fail(e, CAGYM_E_UNSUPPORTED, w + " after cagym_ig_init: per-slot distance fields and planner workspaces are not part of a checkpoint");
    if (e->traj_ready) return fail(e, CAGYM_E_STATE, w + " with a trajectory ring initialised: its slices are not part of a checkpoint");
    if (e->rec_ready) return fail(e, CAGYM_E_STATE, w + " with episode records initialised: their table is not part of a checkpoint");
    return CAGYM_OK;
}

// The flat sections of a handle whose stream / log / replay state is (streaming, log capacity or 0, replay capacity or 0): the
// listings of their blocks, ring before running block, in blob order.  with_pointers = false: sizes alone, while the arrays are not
// allocated (or not at these capacities) - the listings applied to empty structs; else the table of k_checkpoint_flat as well.
inline CkptTable ckpt_flat_table(const Env* e, bool streaming, int log_capacity, int replay_capacity, uint64_t* sizes, bool with_pointers) {
    const size_t N = e->cfg.n_worlds, M = e->cfg.max_agents, S = e->cfg.n_scenarios;
    CkptTable T{};
    uint64_t off = 0;
    LayoutCkpt<CkptTable> v{T, off};
    StreamDev W = with_pointers ? e->stream : StreamDev{};
    EpLog G = with_pointers ? e->elog : EpLog{};
    ReplayDev R = with_pointers ? e->replay : ReplayDev{};
    if (streaming) stream_members(W, N, v);
    sizes[CAGYM_CKPT_STREAM] = off;
    if (log_capacity > 0) { eplog_ring_members(G, (size_t)log_capacity, M, v); eplog_run_members(G, N, M, v); }
    sizes[CAGYM_CKPT_LOG] = off - sizes[CAGYM_CKPT_STREAM];
    if (replay_capacity > 0) { replay_ring_members(R, (size_t)replay_capacity, v); replay_table_members(R, S, v); }
    sizes[CAGYM_CKPT_REPLAY] = off - sizes[CAGYM_CKPT_STREAM] - sizes[CAGYM_CKPT_LOG];
    T.bytes = off;
    return T;
}
constexpr int ckpt_flat_fields() {
    LayoutCount n;
    StreamDev W{}; EpLog G{}; ReplayDev R{};
    stream_members(W, 1, n); eplog_ring_members(G, 1, 1, n); eplog_run_members(G, 1, 1, n); replay_ring_members(R, 1, n); replay_table_members(R, 1, n);
    return n.n;
}
static_assert(ckpt_flat_fields() <= CKPT_MAX_FIELDS, "CkptTable holds every flat field");

// every section size of a handle in the given stream / log / replay state
inline void ckpt_sizes(const Env* e, bool streaming, int log_capacity, int replay_capacity, uint64_t* sizes) {
    sizes[CAGYM_CKPT_HOST] = sizeof(CkptHost);
    sizes[CAGYM_CKPT_STATE] = (uint64_t)e->cfg.n_worlds * snap_state_table(e, SNAP_GATHER).row_bytes;
    sizes[CAGYM_CKPT_POOL] = (uint64_t)e->cfg.n_scenarios * snap_pool_table(e, SNAP_SLOT_GATHER).row_bytes;
    (void)ckpt_flat_table(e, streaming, log_capacity, replay_capacity, sizes, false);
}
inline void ckpt_sizes(const Env* e, uint64_t* sizes) {
    ckpt_sizes(e, e->streaming, e->log_ready ? e->elog.capacity : 0, e->replay_on ? e->replay.Q : 0, sizes);
}
inline uint64_t ckpt_blob_bytes(const uint64_t* sizes) {
    uint64_t b = 0;
    for (int k = CAGYM_CKPT_STATE; k < CAGYM_CKPT_SECTIONS; k++) b += sizes[k];
    return b;
}

// the three copy launches of a save (to_blob) or a load, for a blob whose flat sections are those of (streaming, log_capacity, replay_capacity)
inline int ckpt_copy(Env* e, bool to_blob, unsigned char* blob, bool streaming, int log_capacity, int replay_capacity, hipStream_t st) {
    uint64_t sizes[CAGYM_CKPT_SECTIONS];
    ckpt_sizes(e, streaming, log_capacity, replay_capacity, sizes);
    if (int rc = snap_launch(e, snap_state_table(e, to_blob ? SNAP_GATHER : SNAP_SCATTER), nullptr, nullptr, blob, e->cfg.n_worlds, st)) return rc;
    blob += sizes[CAGYM_CKPT_STATE];
    if (int rc = snap_launch(e, snap_pool_table(e, to_blob ? SNAP_SLOT_GATHER : SNAP_SLOT_SCATTER), nullptr, nullptr, blob, e->cfg.n_scenarios, st))
        return rc;
    blob += sizes[CAGYM_CKPT_POOL];
    CkptTable T = ckpt_flat_table(e, streaming, log_capacity, replay_capacity, sizes, true);
    T.to_blob = to_blob ? 1 : 0;
    if (T.bytes == 0) return CAGYM_OK;
    const unsigned grid = (unsigned)std::min<uint64_t>((T.bytes / 16 + CKPT_NT - 1) / CKPT_NT, CKPT_MAX_GRID);
    hipLaunchKernelGGL(k_checkpoint_flat, dim3(grid), dim3(CKPT_NT), 0, st, T, blob);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

}  // namespace

extern "C" {

int cagym_version(void) { return CAGYM_VERSION; }

const char* cagym_last_error(void* env) {
    Env* e = reinterpret_cast<Env*>(env);
    return e ? e->err.c_str() : g_last_error.c_str();
}

// ---- cagym_create, step by step (every step reports through fail(); cagym_create destroys the half-made handle on the first error) ----
static int validate_config(const cagym_config* cfg) {
    if (cfg->n_worlds < 1) return fail(nullptr, CAGYM_E_INVALID, "n_worlds must be >= 1");
    if (cfg->max_agents < 2 || cfg->max_agents > 32)
        return fail(nullptr, CAGYM_E_UNSUPPORTED, "max_agents must be in [2, 32] (a world may not straddle a wavefront)");
    if (cfg->n_scenarios < cfg->n_worlds) return fail(nullptr, CAGYM_E_INVALID, "n_scenarios must be >= n_worlds");
    if ((long long)cfg->n_worlds * cfg->max_agents >= (1ll << 31) || (long long)cfg->n_scenarios * cfg->max_agents >= (1ll << 31))
        return fail(nullptr, CAGYM_E_UNSUPPORTED, "n_worlds * max_agents (and n_scenarios * max_agents) must stay below 2^31: the kernels keep flat agent indices in 32 bits");
    if (cfg->max_obstacles < 0 || !(cfg->dt > 0)) return fail(nullptr, CAGYM_E_INVALID, "bad max_obstacles / dt");
    if (cfg->rvo_max_neighbors < 0) return fail(nullptr, CAGYM_E_INVALID, "rvo_max_neighbors must be >= 0 (0 = max_agents)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(nullptr, CAGYM_E_NODEVICE, "no HIP device: libcagym_hip has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, CAGYM_E_INVALID, "device ordinal out of range");
    return CAGYM_OK;
}

// the scenario pool, the per-agent and per-world state and the GA3C words, zero-filled
static int alloc_state(Env* e) {
    const cagym_config* cfg = &e->cfg;
    CagymDev& D = e->D;
    memset(&D, 0, sizeof(D));
    const size_t N = cfg->n_worlds, M = cfg->max_agents, S = cfg->n_scenarios, K = cfg->max_obstacles;
    D.N = (int)N; D.M = (int)M; D.S = (int)S; D.Kobs = cfg->max_obstacles;
    D.go_mode = cfg->game_over_mode; D.collide_static = cfg->collide_with_static; D.laserscan = cfg->laserscan;
    D.dt = cfg->dt;
    D.inv_dt = 1.0 / cfg->dt;
    D.maxnb = cfg->rvo_max_neighbors > 0 ? cfg->rvo_max_neighbors : (int)M;  // RVOPolicy.py:15: Config.MAX_NUM_AGENTS_IN_ENVIRONMENT
    if (D.maxnb > (int)M - 1) D.maxnb = (int)M - 1;                            // there are at most M - 1 other agents
    // the pool first, then the state: one allocation per row of the lists, in their order (sc_heading0 stays null: no headings yet)
    size_t rows = S;
    int skip = K > 0 ? 0 : FIELD_MAP;
    CAGYM_POOL_FIELDS(FIELD_ALLOC)
    D.sc_obst = e->sc_obst; D.sc_obst_prep = e->sc_obst_prep;
    rows = N; skip = 0;
    CAGYM_STATE_FIELDS(FIELD_ALLOC)
    if (int rc = dalloc(e, &e->ga3c_ctr, 4)) return rc;  // at creation: cagym_ga3c_act may run inside a stream capture (no allocation there)
    if (int rc = dalloc(e, &e->ga3c_packed, GA16_PACKED_BYTES)) return rc;
    return dalloc(e, &e->go_scratch, N);  // at creation, as the GA3C words: cagym_step_autoreset_keep may run inside a stream capture
}

// the kernels' status word: pinned host memory mapped into the device's address space (written only when a bounded wait expires)
static int alloc_status_word(Env* e) {
    void* hp = nullptr;
    void* dp = nullptr;
    if (hipHostMalloc(&hp, 64, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess) {
        if (hp) (void)hipHostFree(hp);
        return fail(nullptr, CAGYM_E_NOMEM, "hipHostMalloc of the device status word failed");
    }
    memset(hp, 0, 64);
    e->status_host = reinterpret_cast<int32_t*>(hp);
    e->D.dev_status = reinterpret_cast<int32_t*>(dp);
    return CAGYM_OK;
}

// Worlds per workgroup of the M = 10 kernels: 4 while 4 workgroups per CU hold the whole launch (128 VGPRs; 30.9 KB of LDS with 4
// worlds, 37.7 KB with 5), else 5.  A handle with rectangles (OBST instantiation) that would take 5 takes 4 when the smaller
// footprint buys a workgroup per CU.  What is priced: lds_obst4 / lds_obst5, the ROLL-OUT layout's bytes with 4 / 5 worlds
// (lds3_bytes with obstacle half-plane rows, without them when those exceed the CU's 160 KB), and at most 3 workgroups per CU
// are counted (cfg4: 53.4 KB -> 3 per CU, 65.9 KB with 5 worlds -> 2; profiles/r3/cfg4_occupancy_ab.txt).
// override: CAGYM_WPW10 = 4 | 5 (diagnostics) wins.
static int choose_wpw10(const cagym_config& cfg, int cus, const char* override, size_t lds_obst4, size_t lds_obst5) {
    if (override && (override[0] == '4' || override[0] == '5')) return override[0] - '0';
    const int wpw = (cfg.n_worlds + 3) / 4 <= 4 * cus ? 4 : 5;
    if (cfg.max_obstacles <= 0 || wpw == 4) return wpw;
    auto per_cu = [](size_t b) {
        const int n = (int)((size_t)160 * 1024 / b);
        return n < 3 ? n : 3;
    };
    return per_cu(lds_obst4) > per_cu(lds_obst5) ? 4 : 5;
}

// the kernel generation (CAGYM_KERNEL, or 1 when generation 3 does not fit the LDS), worlds per workgroup and CAGYM_PRE_LDS
static int choose_kernels(Env* e) {
    const int M = e->cfg.max_agents;
    if (cagym_lds_bytes(M) > 160 * 1024) return fail(nullptr, CAGYM_E_UNSUPPORTED, "LDS budget exceeded");
    const char* g = getenv("CAGYM_KERNEL");
    if (g && (!strcmp(g, "v1") || !strcmp(g, "1"))) e->generation = 1;
    else if (g && g[0] && strcmp(g, "v3") && strcmp(g, "3"))  // a retired or misspelt generation must not silently run the default
        return fail(nullptr, CAGYM_E_INVALID, std::string("CAGYM_KERNEL=") + g + ": unknown kernel generation (v1 or v3)");
    hipDeviceProp_t prop;
    int cus = 256;
    if (hipGetDeviceProperties(&prop, e->cfg.device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
    auto lds_obst = [&](int wpw) {
        const size_t b = lds3_bytes(e->cfg, spec2(M, wpw), true, true);
        return b > 160 * 1024 ? lds3_bytes(e->cfg, spec2(M, wpw), true, false) : b;
    };
    e->wpw10 = choose_wpw10(e->cfg, cus, getenv("CAGYM_WPW10"), lds_obst(4), lds_obst(5));
    if (const char* pl = getenv("CAGYM_PRE_LDS")) e->pre_lds_min = (size_t)atol(pl);
    if (e->generation == 3 && lds3_bytes(e, false, false) > 160 * 1024) e->generation = 1;
    // the free-space kernels keep the neighbour keys in the LP scratch (cagym_dsq_aliased): it must hold them
    if (e->generation == 3 && cagym_dsq_aliased(false, spec2(e).mt) &&
        (size_t)cagym_as(M, wpw_spec(e)) * cagym_mp(M) * 8 > (size_t)cagym_lpl3(spec2(e).mt, false) * spec2(e).nt * 16)
        return fail(nullptr, CAGYM_E_UNSUPPORTED, "neighbour keys do not fit the LP scratch of this specialisation");
    if (!k3_entry(e)) return fail(nullptr, CAGYM_E_UNSUPPORTED, "no kernel specialisation for this shape");
    return CAGYM_OK;
}

// > 64 KiB of dynamic LDS needs the attribute raised
static void raise_lds_attributes(Env* e) {
    const int lds = (int)cagym_lds_bytes(e->cfg.max_agents);
    hipFuncSetAttribute(reinterpret_cast<const void*>(k_step), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipFuncSetAttribute(reinterpret_cast<const void*>(k_rollout<true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipFuncSetAttribute(reinterpret_cast<const void*>(k_rollout<false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipFuncSetAttribute(reinterpret_cast<const void*>(k_reset), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    int lds3 = (int)lds3_bytes(e, false, false), lds3_obst = (int)lds3_bytes(e, true, true);
    if (lds3_obst > 160 * 1024) lds3_obst = (int)lds3_bytes(e, true, false);  // too many rectangles for RVO agents: refused at set_scenarios
#ifdef CAGYM_DIAG_LDS_PAD
    if (const char* pad = getenv("CAGYM_LDS_PAD")) { lds3 += atoi(pad); lds3_obst += atoi(pad); }
#endif
    k3_entry(e)->setattr[0](lds3);
    if (lds3_obst <= 160 * 1024) k3_entry(e)->setattr[1](lds3_obst);
    (void)hipGetLastError();
}

int cagym_create(const cagym_config* cfg, void** env_out) {
    if (!cfg || !env_out) return fail(nullptr, CAGYM_E_INVALID, "cagym_create: null argument");
    *env_out = nullptr;
    if (int rc = validate_config(cfg)) return rc;
    Env* e = new Env();
    e->cfg = *cfg;
    DeviceGuard guard(cfg->device);
    int rc = guard.status == hipSuccess ? CAGYM_OK : fail(nullptr, CAGYM_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(guard.status));
    if (!rc) rc = alloc_state(e);
    if (!rc) rc = alloc_status_word(e);
    if (!rc) rc = choose_kernels(e);
    if (rc) {
        cagym_destroy(e);
        return rc;
    }
    raise_lds_attributes(e);
    e->err.clear();
    *env_out = e;
    return CAGYM_OK;
}

int cagym_destroy(void* env) {
    Env* e = reinterpret_cast<Env*>(env);
    if (!e) return CAGYM_OK;
    for (void* p : e->allocs)
        if (p) (void)hipFree(p);
    if (e->status_host) (void)hipHostFree(e->status_host);
    delete e;
    return CAGYM_OK;
}

// A pool with RVO agents among rectangles: the kernels build obstacle half-planes (RVOPolicy.py:56-57).  The handle's max_obstacles
// must fit an LP group (4 half-planes per lane; an agent sees at most 2 edges of a rectangle from their right side), the coverage bit
// masks (<= 32 obstacle lines per ego), the obstacle-neighbour lists (8 B per candidate + 4 B per work item + 1 B per rank, in the LP3
// scratch) and the roll-out's LDS.
static int check_obst_rvo_capacity(Env* e) {
    const int K = e->cfg.max_obstacles, M = e->cfg.max_agents, gw = lp_group_width(e);
    const Spec2 sp = spec2(e);
    const int as = cagym_as(M, sp.wpw);
    if (e->generation != 3) return fail(e, CAGYM_E_UNSUPPORTED, "RVO agents among obstacles need the generation-3 kernels");
    if (2 * K + M - 1 > 4 * gw || 2 * K > 32 || (size_t)2 * K * as * 13 > (size_t)4 * sp.nt * 16 || lds3_bytes(e, true, true) > 160 * 1024)
        return fail(e, CAGYM_E_UNSUPPORTED, "too many rectangles per world for RVO agents at this max_agents (2 * max_obstacles + max_agents - 1 half-planes per ego)");
    return CAGYM_OK;
}

int cagym_set_scenarios(void* env, const double* agents6, const double* heading0, const int32_t* policy_id,
                        const int32_t* dynamics_id, const int32_t* n_agents, const double* coop,
                        const double* obstacles, const int32_t* n_obst, void* stream) {
    ENTRY(e, env);
    if (!agents6 || !policy_id || !dynamics_id) return fail(e, CAGYM_E_INVALID, "agents6 / policy_id / dynamics_id are required");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ON_DEVICE(e);
    const size_t S = e->cfg.n_scenarios, M = e->cfg.max_agents, SM = S * M;
    // validate ids on the host: the kernels index switch tables with them
    for (size_t k = 0; k < SM; k++) {
        if (policy_id[k] < 0 || policy_id[k] > CAGYM_POL_IGMCTS) return fail(e, CAGYM_E_INVALID, "policy id out of range");
        if (dynamics_id[k] < 0 || dynamics_id[k] > CAGYM_DYN_FIRSTORDER) return fail(e, CAGYM_E_INVALID, "dynamics id out of range");
    }
    // decided on locals, committed only after every validation and copy below succeeded: a refused call leaves the handle as it was
    int new_any_rvo = 0, new_obst_rvo = 0, new_ko = 0;
    for (size_t k = 0; k < SM; k++)
        if (policy_id[k] == CAGYM_POL_RVO) new_any_rvo = 1;
    std::vector<int32_t> na(S), no(S, 0);
    int new_n_ig = 0;
    for (size_t s = 0; s < S; s++) {
        na[s] = n_agents ? n_agents[s] : (int32_t)M;
        if (na[s] < 0 || na[s] > (int32_t)M) return fail(e, CAGYM_E_INVALID, "n_agents out of range");
        int c = 0;
        for (int k = 0; k < na[s]; k++) c += policy_id[s * M + k] == CAGYM_POL_IGMCTS;
        new_n_ig = s == 0 ? c : (c == new_n_ig ? new_n_ig : N_IG_UNEQUAL);
        if (n_obst && e->cfg.max_obstacles > 0) {
            no[s] = n_obst[s];
            if (no[s] < 0 || no[s] > e->cfg.max_obstacles) return fail(e, CAGYM_E_INVALID, "n_obst out of range");
        }
    }
    // RVO agents among rectangles: the kernels build obstacle half-planes (RVOPolicy.py:56-57).  Capacity of an LP group:
    // 4 half-planes per lane; an agent sees at most 2 edges of a rectangle from their right side.
    {
        bool any_obst = false;
        for (size_t sc = 0; sc < S; sc++) any_obst |= no[sc] > 0;
        if (any_obst && !obstacles) return fail(e, CAGYM_E_INVALID, "n_obst > 0 needs the obstacles array");
        new_obst_rvo = (any_obst && new_any_rvo) ? 1 : 0;
        new_ko = new_obst_rvo ? 2 * e->cfg.max_obstacles : 0;
        if (new_obst_rvo) {
            const int K = e->cfg.max_obstacles;
            const int rc = check_obst_rvo_capacity(e);
            if (rc != CAGYM_OK) return rc;
            for (size_t sc = 0; sc < S; sc++)
                    for (int k = 0; k < no[sc]; k++) {
                        const double* r = obstacles + (sc * K + k) * 4;
                        if (!(r[2] > r[0]) || !(r[3] > r[1]))
                            return fail(e, CAGYM_E_INVALID, "RVO agents need non-degenerate rectangles (xl < xu, yl < yu)");
                    }
        }
    }
    std::vector<double> cp(SM, 1.0);  // agent.py:10
    if (coop) memcpy(cp.data(), coop, SM * sizeof(double));
    CagymDev& D = e->D;
    double* dh0 = e->sc_heading_buf;
    HIPCHK(e, hipMemcpyAsync(const_cast<double*>(D.sc_agents6), agents6, SM * 6 * sizeof(double), hipMemcpyHostToDevice, st));
    if (heading0) {
        HIPCHK(e, hipMemcpyAsync(dh0, heading0, SM * sizeof(double), hipMemcpyHostToDevice, st));
        D.sc_heading0 = dh0;
    } else {
        D.sc_heading0 = nullptr;
    }
    HIPCHK(e, hipMemcpyAsync(const_cast<int32_t*>(D.sc_policy), policy_id, SM * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(const_cast<int32_t*>(D.sc_dyn), dynamics_id, SM * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(const_cast<int32_t*>(D.sc_nagents), na.data(), S * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(const_cast<double*>(D.sc_coop), cp.data(), SM * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(const_cast<int32_t*>(D.sc_nobst), no.data(), S * sizeof(int32_t), hipMemcpyHostToDevice, st));
    std::vector<float> prep;  // staged until the stream synchronisation below
    if (e->cfg.max_obstacles > 0) {
        if (obstacles) {
            HIPCHK(e, hipMemcpyAsync(e->sc_obst, obstacles, S * (size_t)e->cfg.max_obstacles * 4 * sizeof(double), hipMemcpyHostToDevice, st));
            // RVOSimulator::addObstacle per rectangle (vertices narrowed to float as Cython does): unit directions
            // normalize(next - this) = v * (1.0f / |v|) and convexity leftOf(prev, this, next) >= 0, in plain IEEE fp32
            const size_t K = (size_t)e->cfg.max_obstacles;
            prep.assign(S * K * 16, 0.0f);
            for (size_t r = 0; r < S * K; r++) {
                const float xl = (float)obstacles[4 * r], yl = (float)obstacles[4 * r + 1], xu = (float)obstacles[4 * r + 2], yu = (float)obstacles[4 * r + 3];
                const float X[4] = {xu, xl, xl, xu}, Y[4] = {yu, yu, yl, yl};
                float* q = prep.data() + 16 * r;
                q[0] = xl; q[1] = yl; q[2] = xu; q[3] = yu;
                uint32_t convex = 0;
                for (int k = 0; k < 4; k++) {
                    const int nx = (k + 1) & 3, pv = (k + 3) & 3;
                    const volatile float ex = X[nx] - X[k], ey = Y[nx] - Y[k];
                    const volatile float sq = ex * ex;
                    const volatile float sq2 = ey * ey;
                    const volatile float len2 = sq + sq2;
                    const volatile float inv = 1.0f / sqrtf(len2);
                    q[4 + 2 * k] = ex * inv;
                    q[5 + 2 * k] = ey * inv;
                    const volatile float a0 = X[pv] - X[nx], a1 = Y[pv] - Y[nx], b0 = X[k] - X[pv], b1 = Y[k] - Y[pv];
                    const volatile float m0 = a0 * b1;
                    const volatile float m1 = a1 * b0;
                    if (m0 - m1 >= 0.0f) convex |= 1u << k;
                }
                memcpy(&q[12], &convex, 4);
                // its raster footprint needs neither numpy's negative-index wrap nor clamping (laser_chunk3's shortcut)
                q[13] = (xl > -14.7f && yl > -14.7f && xu < 14.7f && yu < 14.7f) ? 1.0f : 0.0f;
            }
            HIPCHK(e, hipMemcpyAsync(e->sc_obst_prep, prep.data(), prep.size() * sizeof(float), hipMemcpyHostToDevice, st));
        }
    }
    if (int rc = rasterize_pool(e, st)) return rc;
    // host staging vectors die at return: the copies above must have consumed them
    HIPCHK(e, hipStreamSynchronize(st));
    // a new pool restarts the episode numbering
    HIPCHK(e, hipMemsetAsync(D.episode, 0, e->cfg.n_worlds * sizeof(int32_t), st));
    e->any_rvo = new_any_rvo;
    e->n_ig = new_n_ig;
    e->obst_rvo = new_obst_rvo;
    e->D.ko = new_ko;
    e->scenarios_set = true;
    e->streaming = e->replay_on = false;  // the pool is the caller's again
    e->begun = false;  // a pending cagym_step_begin solved the old pool's worlds: its velocities are void
    return episodes_restart(e, nullptr, true, st);
}

// the handle's scenario pool as the generator kernels write it
static GenDev gen_dev(const Env* e) {
    const CagymDev& D = e->D;
    GenDev G;
    G.agents6 = const_cast<double*>(D.sc_agents6);
    G.policy = const_cast<int32_t*>(D.sc_policy);
    G.dyn = const_cast<int32_t*>(D.sc_dyn);
    G.nagents = const_cast<int32_t*>(D.sc_nagents);
    G.coop = const_cast<double*>(D.sc_coop);
    G.nobst = const_cast<int32_t*>(D.sc_nobst);
    G.S = e->cfg.n_scenarios;
    G.M = e->cfg.max_agents;
    return G;
}
// Env::gen_failed, allocated by the first generator call
static int gen_failed_word(Env* e) { return e->gen_failed ? CAGYM_OK : dalloc(e, &e->gen_failed, 1); }

int cagym_generate_scenarios(void* env, const cagym_gen_params* params, int32_t* n_failed_host, void* stream) {
    ENTRY(e, env);
    if (!params) return fail(e, CAGYM_E_INVALID, "null params");
    const cagym_gen_params& P = *params;
    const int M = e->cfg.max_agents;
    if (P.n_min < 1 || P.n_max > M || P.n_min > P.n_max) return fail(e, CAGYM_E_INVALID, "need 1 <= n_min <= n_max <= max_agents");
    const int32_t pols[3] = {P.ego_policy, P.policy_a, P.policy_b};
    for (int32_t q : pols)
        if (q < 0 || q > CAGYM_POL_IGMCTS) return fail(e, CAGYM_E_INVALID, "policy id out of range");
    if (P.ego_dynamics < 0 || P.ego_dynamics > CAGYM_DYN_FIRSTORDER || P.other_dynamics < 0 || P.other_dynamics > CAGYM_DYN_FIRSTORDER)
        return fail(e, CAGYM_E_INVALID, "dynamics id out of range");
    if (P.max_tries < 1 || !(P.side > 0) || !(P.p_b >= 0 && P.p_b <= 1)) return fail(e, CAGYM_E_INVALID, "bad generator parameters");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ON_DEVICE(e);
    CagymDev& D = e->D;
    const GenDev G = gen_dev(e);
    if (int rc = gen_failed_word(e)) return rc;
    int32_t* d_failed = e->gen_failed;
    HIPCHK(e, hipMemsetAsync(d_failed, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(k_generate_scenarios, dim3((G.S + 63) / 64), dim3(64), 0, st, G, P, d_failed);
    HIPCHK(e, hipGetLastError());
    D.sc_heading0 = nullptr;  // toward the goal (agent.py:29-31)
    e->any_rvo = (P.ego_policy == CAGYM_POL_RVO || P.policy_a == CAGYM_POL_RVO || P.policy_b == CAGYM_POL_RVO) ? 1 : 0;
    e->n_ig = (P.ego_policy == CAGYM_POL_IGMCTS || P.policy_a == CAGYM_POL_IGMCTS || P.policy_b == CAGYM_POL_IGMCTS) ? N_IG_RANDOM : 0;
    e->obst_rvo = 0;  // the generator draws free-space worlds
    e->D.ko = 0;
    if (int rc = rasterize_pool(e, st)) return rc;  // free space: empty rasters
    if (n_failed_host) {
        HIPCHK(e, hipMemcpyAsync(n_failed_host, d_failed, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(e, hipStreamSynchronize(st));
    }
    HIPCHK(e, hipMemsetAsync(D.episode, 0, e->cfg.n_worlds * sizeof(int32_t), st));  // a new pool restarts the episode numbering
    e->scenarios_set = true;
    e->streaming = e->replay_on = false;
    e->begun = false;  // as in cagym_set_scenarios: a pending cagym_step_begin is void
    return episodes_restart(e, nullptr, true, st);
}

// what a parameter set of the reference samplers implies for the handle (gen2_validate)
struct Gen2Flags {
    bool any_rvo = false, any_ig = false, obst_rvo = false;
};

// the argument checks of cagym_generate_reference_scenarios, shared with cagym_stream_scenarios / cagym_stream_set_params
static int gen2_validate(Env* e, const cagym_gen2_params* params, Gen2Flags& F) {
    if (!params) return fail(e, CAGYM_E_INVALID, "null params");
    const cagym_gen2_params& P = *params;
    const int M = e->cfg.max_agents, K = e->cfg.max_obstacles;
    if (P.kinds_mask == 0 || (P.kinds_mask >> CAGYM_GEN_NKINDS) != 0) return fail(e, CAGYM_E_INVALID, "kinds_mask: no kind or an unknown kind");
    if ((P.number_of_agents > 2 ? P.number_of_agents : 2) > M) return fail(e, CAGYM_E_INVALID, "max(number_of_agents, 2) exceeds max_agents");
    const int32_t pols[3] = {P.ego_policy, P.policy_a, P.policy_b};
    for (int32_t q : pols)
        if (q < 0 || q > CAGYM_POL_IGMCTS) return fail(e, CAGYM_E_INVALID, "policy id out of range");
    if (P.ego_dynamics < 0 || P.ego_dynamics > CAGYM_DYN_FIRSTORDER || P.other_dynamics < 0 || P.other_dynamics > CAGYM_DYN_FIRSTORDER)
        return fail(e, CAGYM_E_INVALID, "dynamics id out of range");
    if (P.max_tries < 1 || !(P.p_b >= 0 && P.p_b <= 1)) return fail(e, CAGYM_E_INVALID, "bad generator parameters");
    if (P.n_obst_max > K) return fail(e, CAGYM_E_INVALID, "n_obst_max exceeds the handle's max_obstacles");
    if (P.n_obst_min >= 0 && P.n_obst_max >= 0 && P.n_obst_min > P.n_obst_max) return fail(e, CAGYM_E_INVALID, "n_obst_min exceeds n_obst_max");
    // the policies the pool may hold (each kind's rule unless overridden: RVO / NonCooperative, stages RVO only)
    const bool own = P.override_policies != 0;
    auto may = [&](int pol, int kind) {
        if (P.ego_policy == pol) return true;
        const int pa = own ? P.policy_a : CAGYM_POL_RVO;
        const int pb = own ? P.policy_b : (kind >= CAGYM_GEN_STAGE_1 ? CAGYM_POL_RVO : CAGYM_POL_NONCOOP);
        const double p_b = own ? P.p_b : (kind >= CAGYM_GEN_STAGE_1 ? 0.0 : 0.5);
        return (pa == pol && p_b < 1.0) || (pb == pol && p_b > 0.0);
    };
    for (int kind = 0; kind < CAGYM_GEN_NKINDS; kind++) {
        if (!((P.kinds_mask >> kind) & 1u)) continue;
        F.any_rvo |= may(CAGYM_POL_RVO, kind);
        F.any_ig |= may(CAGYM_POL_IGMCTS, kind);
        if (kind == CAGYM_GEN_STAGE_1 || kind == CAGYM_GEN_STAGE_2) {
            // the reference's randint range (tc.py:2377, 2482) narrowed by the caller's bounds, as the kernel narrows it
            const int rlo = kind == CAGYM_GEN_STAGE_1 ? 0 : 2, rhi = kind == CAGYM_GEN_STAGE_1 ? 4 : 10;
            const int lo = P.n_obst_min >= 0 ? std::max(rlo, (int)P.n_obst_min) : rlo;
            const int hi = P.n_obst_max >= 0 ? std::min(rhi, (int)P.n_obst_max) : rhi;
            const std::string name = kind == CAGYM_GEN_STAGE_1 ? "train_stage_1" : "train_stage_2";
            if (hi > K)
                return fail(e, CAGYM_E_INVALID, "the rectangle count of " + name + " (up to " + std::to_string(hi) +
                                                    ") exceeds the handle's max_obstacles: cap it with n_obst_max");
            if (lo > hi)
                return fail(e, CAGYM_E_INVALID, "the n_obst bounds leave " + name + " no rectangle count (its range is " +
                                                    std::to_string(rlo) + ".." + std::to_string(rhi) + ")");
            F.obst_rvo |= hi > 0 && may(CAGYM_POL_RVO, kind);
        }
    }
    // the counts are drawn on the device: the handle's max_obstacles decides, as cagym_set_scenarios decides it for a pool with a full world
    if (F.obst_rvo) {
        const int rc = check_obst_rvo_capacity(e);
        if (rc != CAGYM_OK) return rc;
    }
    return CAGYM_OK;
}

static Gen2Dev gen2_dev(const Env* e) {
    Gen2Dev G;
    G.G = gen_dev(e);
    G.obst = e->sc_obst;
    G.prep = reinterpret_cast<float*>(e->sc_obst_prep);
    G.K = e->cfg.max_obstacles;
    return G;
}

// every slot of the pool from the samplers (slot r from stream key r), its rasters, and the handle state a new pool commits;
// d_failed: the device word the rejection loops report into (zeroed by the caller)
// team: NULL, or the team edit of an exploration pool (k_generate_exploration_scenarios; every slot then holds team->R IG robots)
static int gen2_fill(Env* e, const cagym_gen2_params& P, const Gen2Flags& F, int32_t* d_failed, int32_t* n_failed_host, hipStream_t st,
                     const ExploreTeam* team = nullptr) {
    CagymDev& D = e->D;
    const int K = e->cfg.max_obstacles;
    const Gen2Dev G = gen2_dev(e);
    if (team)
        hipLaunchKernelGGL(k_generate_exploration_scenarios, dim3((G.G.S + 63) / 64), dim3(64), 0, st, G, P, *team, d_failed);
    else
        hipLaunchKernelGGL(k_generate_reference_scenarios, dim3((G.G.S + 63) / 64), dim3(64), 0, st, G, P, d_failed);
    HIPCHK(e, hipGetLastError());
    if (int rc = rasterize_pool(e, st)) return rc;
    HIPCHK(e, hipMemsetAsync(D.episode, 0, e->cfg.n_worlds * sizeof(int32_t), st));  // a new pool restarts the episode numbering
    if (n_failed_host) {
        HIPCHK(e, hipMemcpyAsync(n_failed_host, d_failed, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(e, hipStreamSynchronize(st));
    }
    D.sc_heading0 = nullptr;  // toward the goal (agent.py:29-31)
    e->any_rvo = F.any_rvo ? 1 : 0;
    e->n_ig = team ? team->R : F.any_ig ? N_IG_RANDOM : 0;
    e->obst_rvo = F.obst_rvo ? 1 : 0;
    e->D.ko = F.obst_rvo ? 2 * K : 0;
    e->scenarios_set = true;
    e->streaming = e->replay_on = false;
    e->begun = false;  // as in cagym_set_scenarios: a pending cagym_step_begin is void
    return episodes_restart(e, nullptr, true, st);
}

int cagym_generate_reference_scenarios(void* env, const cagym_gen2_params* params, int32_t* n_failed_host, void* stream) {
    ENTRY(e, env);
    Gen2Flags F;
    if (int rc = gen2_validate(e, params, F)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ON_DEVICE(e);
    if (int rc = gen_failed_word(e)) return rc;
    HIPCHK(e, hipMemsetAsync(e->gen_failed, 0, sizeof(int32_t), st));
    return gen2_fill(e, *params, F, e->gen_failed, n_failed_host, st);
}

// ---- streamed scenarios (csrc/cagym_stream.h) -------------------------------------------------------------------------------------------
// what cagym_stream_scenarios and cagym_stream_set_params refuse beyond the generator's own checks
enum { EXPLORE_COLS_GRID = 256, EXPLORE_ROWS_GRID = 2048 };  // the field refresh's fixed grids (cagym_stream_refill)
static int stream_check(Env* e, const char* what, const cagym_gen2_params* params, Gen2Flags& F) {
    if (int rc = gen2_validate(e, params, F)) return rc;
    const int N = e->cfg.n_worlds, S = e->cfg.n_scenarios;
    if (S % N != 0 || S < 2 * N)
        return fail(e, CAGYM_E_INVALID, std::string(what) + ": n_scenarios must be a multiple of n_worlds and at least 2 * n_worlds (a ring of depth >= 2 per world)");
    if (e->ig_ready) return fail(e, CAGYM_E_UNSUPPORTED, std::string(what) + " after cagym_ig_init: the per-slot distance field is not rebuilt");
    if (F.any_ig) return fail(e, CAGYM_E_UNSUPPORTED, std::string(what) + ": the parameter set can place CAGYM_POL_IGMCTS agents");
    if (e->rec_ready)
        return fail(e, CAGYM_E_STATE, std::string(what) + " with episode records initialised: their table has one row per pool slot, "
                                                          "which a streamed pool reuses");
    return CAGYM_OK;
}

int cagym_stream_scenarios(void* env, const cagym_gen2_params* params, int32_t* n_failed_host, void* stream) {
    ENTRY(e, env);
    Gen2Flags F;
    if (int rc = stream_check(e, "cagym_stream_scenarios", params, F)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ON_DEVICE(e);
    const int N = e->cfg.n_worlds, S = e->cfg.n_scenarios;
    if (int rc = stream_alloc(e)) return rc;
    StreamDev& T = e->stream;
    // the first fill counts: generated = S, n_failed = its failures
    HIPCHK(e, hipMemsetAsync(T.generated, 0, 16, st));
    HIPCHK(e, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(T.generated), S, 1, st));
    HIPCHK(e, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(T.next_episode), T.depth, (size_t)N, st));
    if (int rc = gen2_fill(e, *params, F, T.n_failed, n_failed_host, st)) return rc;
    e->stream_P = *params;
    e->streaming = true;
    e->explore_stream = false;
    e->stream_gen = 1;
    return CAGYM_OK;
}

int cagym_stream_set_params(void* env, const cagym_gen2_params* params) {
    ENTRY_IF(e, env, e->streaming, "cagym_stream_set_params on a handle that is not streaming");
    if (e->explore_stream)
        return fail(e, CAGYM_E_UNSUPPORTED, "cagym_stream_set_params on an exploration stream: its switch is cagym_stream_set_exploration_params");
    Gen2Flags F;
    if (int rc = stream_check(e, "cagym_stream_set_params", params, F)) return rc;
    // slots of both parameter sets are in the ring from now on: the handle's flags cover both
    const int any_rvo = (e->any_rvo || F.any_rvo) ? 1 : 0, obst_rvo = (e->obst_rvo || F.obst_rvo) ? 1 : 0;
    if (any_rvo != e->any_rvo || obst_rvo != e->obst_rvo) e->begun = false;  // a pending cagym_step_begin solved for the old flags
    e->any_rvo = any_rvo;
    e->obst_rvo = obst_rvo;
    e->D.ko = obst_rvo ? 2 * e->cfg.max_obstacles : 0;
    e->stream_P = *params;
    e->stream_gen += 1;  // a key redrawn under another set is another scenario: the replay buffer holds for one generation
    return CAGYM_OK;
}

int cagym_stream_refill(void* env, void* stream) {
    ENTRY_IF(e, env, e->streaming, "cagym_stream_refill on a handle that is not streaming");
    ON_DEVICE(e);
    const unsigned grid = (unsigned)((e->cfg.n_worlds + CAGYM_WAVE - 1) / CAGYM_WAVE);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (e->explore_stream) {  // 1 launch, or 4 once cagym_ig_init ran: the refill, then the field refresh's list, columns, rows
        hipLaunchKernelGGL(k_explore_refill, dim3(grid), dim3(CAGYM_WAVE), 0, st, gen2_dev(e), e->stream_P, e->stream_team, e->stream, e->explore.n_list);
        if (e->ig_ready) {
            hipLaunchKernelGGL(k_explore_field_list, dim3(grid), dim3(CAGYM_WAVE), 0, st, e->stream, e->explore, e->cfg.n_scenarios);
            hipLaunchKernelGGL(k_explore_field_cols, dim3(EXPLORE_COLS_GRID), dim3(320), 0, st, e->G, e->explore, e->ig_any);
            hipLaunchKernelGGL(k_explore_field_rows, dim3(EXPLORE_ROWS_GRID), dim3(320), 0, st, e->G, e->explore, e->ig_any);
        }
    } else if (e->replay_on) {
        hipLaunchKernelGGL(k_stream_refill_replay, dim3(grid), dim3(CAGYM_WAVE), 0, st, gen2_dev(e), e->stream_P, e->stream, e->replay, e->replay_p,
                           e->replay_seed, e->stream_gen);
    } else {
        hipLaunchKernelGGL(k_stream_refill, dim3(grid), dim3(CAGYM_WAVE), 0, st, gen2_dev(e), e->stream_P, e->stream);
    }
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

int cagym_stream_get(void* env, cagym_stream_ptrs* out) {
    ENTRY_IF(e, env, e->stream.next_episode != nullptr, "cagym_stream_get before cagym_stream_scenarios");
    if (!out) return fail(e, CAGYM_E_INVALID, "null out");
    out->next_episode = e->stream.next_episode;
    out->generated = reinterpret_cast<const uint64_t*>(e->stream.generated);
    out->n_failed = e->stream.n_failed;
    out->n_lapped = e->stream.n_lapped;
    return CAGYM_OK;
}

int cagym_stream_stop(void* env) {
    ENTRY(e, env);
    e->streaming = e->replay_on = false;
    return CAGYM_OK;
}

// ---- replay of logged scenarios in the stream (csrc/cagym_replay.h) -----------------------------------------------------------------------
int cagym_stream_replay_init(void* env, int capacity, uint64_t seed, void* stream) {
    ENTRY_IF(e, env, e->streaming, "cagym_stream_replay_init on a handle that is not streaming");
    if (e->explore_stream)
        return fail(e, CAGYM_E_UNSUPPORTED, "cagym_stream_replay_init on an exploration stream: its refill also rebuilds distance fields");
    if (capacity < 1) return fail(e, CAGYM_E_INVALID, "cagym_stream_replay_init: capacity must be >= 1");
    ON_DEVICE(e);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t S = (size_t)e->cfg.n_scenarios;
    if (int rc = replay_alloc(e, capacity)) return rc;
    const ReplayDev R = e->replay;
    e->replay_seed = seed;
    // a handle that is armed already keeps its tables (they name replayed keys): only the buffer and the counters are cleared
    const unsigned grid = (unsigned)((e->cfg.n_worlds + CAGYM_WAVE - 1) / CAGYM_WAVE);
    hipLaunchKernelGGL(k_replay_arm, dim3(grid), dim3(CAGYM_WAVE), 0, st, R, e->stream, (int)S, e->stream_gen, e->replay_on ? 0 : 1,
                       e->stream_gen == 1 ? 1 : 0, e->log_ready ? e->elog.head : nullptr);
    HIPCHK(e, hipGetLastError());
    if (!e->replay_on) {
        e->replay_p = 0.0;
        e->replay_mask = 0;
    }
    e->replay_on = true;
    return CAGYM_OK;
}

int cagym_stream_replay_set(void* env, double p, uint32_t outcome_mask) {
    ENTRY_IF(e, env, e->replay_on, "cagym_stream_replay_set before cagym_stream_replay_init");
    if (!(p >= 0.0 && p <= 1.0)) return fail(e, CAGYM_E_INVALID, "cagym_stream_replay_set: p must lie in [0, 1]");
    if (outcome_mask & ~7u) return fail(e, CAGYM_E_INVALID, "cagym_stream_replay_set: outcome_mask takes the bits 1 (collision), 2 (all at goal), 4 (stuck)");
    e->replay_p = p;
    e->replay_mask = outcome_mask;
    return CAGYM_OK;
}

int cagym_stream_replay_push(void* env, const uint32_t* keys, int n, void* stream) {
    ENTRY_IF(e, env, e->replay_on, "cagym_stream_replay_push before cagym_stream_replay_init");
    if (n < 0 || (n > 0 && !keys)) return fail(e, CAGYM_E_INVALID, "cagym_stream_replay_push: need n >= 0 and a device array of n keys");
    if (n == 0) return CAGYM_OK;
    ON_DEVICE(e);
    hipLaunchKernelGGL(k_replay_push, dim3(1), dim3(REPLAY_NT), 0, reinterpret_cast<hipStream_t>(stream), e->replay, keys, n, e->stream_gen);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

int cagym_stream_replay_harvest(void* env, void* stream) {
    ENTRY_IF(e, env, e->replay_on, "cagym_stream_replay_harvest before cagym_stream_replay_init");
    REQUIRE(e, e->log_ready, "cagym_stream_replay_harvest", "cagym_episode_log_init");
    ON_DEVICE(e);
    hipLaunchKernelGGL(k_replay_harvest, dim3(1), dim3(REPLAY_NT), 0, reinterpret_cast<hipStream_t>(stream), e->elog, e->replay, e->cfg.n_worlds,
                       e->cfg.n_scenarios, e->replay_mask, e->stream_gen);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

int cagym_stream_replay_get(void* env, const uint32_t** buf_key, const uint64_t** words, const uint32_t** slot_key, const uint32_t** slot_gen,
                            int* capacity) {
    ENTRY_IF(e, env, e->replay.words != nullptr, "cagym_stream_replay_get before cagym_stream_replay_init");
    if (buf_key) *buf_key = e->replay.buf_key;
    if (words) *words = reinterpret_cast<const uint64_t*>(e->replay.words);
    if (slot_key) *slot_key = e->replay.slot_key;
    if (slot_gen) *slot_gen = e->replay.slot_gen;
    if (capacity) *capacity = e->replay.Q;
    return CAGYM_OK;
}

// ---- exploration worlds and their stream (csrc/cagym_explore.h) -------------------------------------------------------------------------
// the checks of cagym_generate_exploration_scenarios, shared with the stream entries; P: the internal stage parameter set, Tm: the team edit
static int explore_validate(Env* e, const char* what, const cagym_explore_params* params, cagym_gen2_params& P, ExploreTeam& Tm, Gen2Flags& F) {
    if (!params) return fail(e, CAGYM_E_INVALID, "null params");
    const cagym_explore_params& X = *params;
    const uint32_t stages = (1u << CAGYM_GEN_STAGE_1) | (1u << CAGYM_GEN_STAGE_2);
    if (X.kinds_mask == 0 || (X.kinds_mask & ~stages) != 0)
        return fail(e, CAGYM_E_INVALID, std::string(what) + ": kinds_mask takes the CAGYM_GEN_STAGE_1 / CAGYM_GEN_STAGE_2 bits only, and at least one");
    if (X.n_robots < 1 || X.n_targets < 0 || (long long)X.n_robots + X.n_targets < 2 || (long long)X.n_robots + X.n_targets > e->cfg.max_agents)
        return fail(e, CAGYM_E_INVALID, std::string(what) + ": need n_robots >= 1, n_targets >= 0 and 2 <= n_robots + n_targets <= max_agents");
    if (!(X.target_radius > 0) || !(X.robot_pref_speed > 0) || std::isinf(X.target_radius) || std::isinf(X.robot_pref_speed))
        return fail(e, CAGYM_E_INVALID, std::string(what) + ": target_radius and robot_pref_speed must be positive");
    if (e->cfg.max_obstacles <= 0)
        return fail(e, CAGYM_E_UNSUPPORTED, std::string(what) + ": exploration worlds need obstacle rasters (max_obstacles > 0)");
    P = cagym_gen2_params{};
    P.seed = X.seed;
    P.kinds_mask = X.kinds_mask;
    P.number_of_agents = X.n_robots + X.n_targets;
    P.fixed_count = 1;
    P.ego_policy = CAGYM_POL_IGMCTS;
    P.ego_dynamics = CAGYM_DYN_FIRSTORDER;
    P.override_policies = 1;
    P.policy_a = P.policy_b = CAGYM_POL_STATIC;
    P.other_dynamics = CAGYM_DYN_FIRSTORDER;
    P.n_obst_min = X.n_obst_min;
    P.n_obst_max = X.n_obst_max;
    P.max_tries = X.max_tries;
    P.p_b = 0.0;
    Tm = ExploreTeam{X.n_robots, X.n_targets, X.target_radius, X.robot_pref_speed};
    return gen2_validate(e, &P, F);  // max_tries, the stage ranges against the bounds and max_obstacles
}

// every slot's distance field again, on a handle cagym_ig_init has set up: its two EDT launches over S (the beliefs stay)
static int ig_rebuild_fields(Env* e, hipStream_t st) {
    const size_t S = e->cfg.n_scenarios;
    HIPCHK(e, hipMemsetAsync(e->ig_any, 0, S * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_ig_edt_cols, dim3((unsigned)S), dim3(320), 0, st, e->G, e->ig_any);
    hipLaunchKernelGGL(k_ig_edt_rows, dim3((unsigned)(S * CAGYM_MAPD)), dim3(320), 0, st, e->G, e->ig_any);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

int cagym_generate_exploration_scenarios(void* env, const cagym_explore_params* params, int32_t* n_failed_host, void* stream) {
    ENTRY(e, env);
    cagym_gen2_params P;
    ExploreTeam Tm;
    Gen2Flags F;
    if (int rc = explore_validate(e, "cagym_generate_exploration_scenarios", params, P, Tm, F)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ON_DEVICE(e);
    if (int rc = gen_failed_word(e)) return rc;
    HIPCHK(e, hipMemsetAsync(e->gen_failed, 0, sizeof(int32_t), st));
    if (int rc = gen2_fill(e, P, F, e->gen_failed, n_failed_host, st, &Tm)) return rc;
    return e->ig_ready ? ig_rebuild_fields(e, st) : CAGYM_OK;
}

// what the exploration stream's entries refuse beyond the generator's own checks (stream_check's list without its two IG refusals)
static int explore_stream_check(Env* e, const char* what, const cagym_explore_params* params, cagym_gen2_params& P, ExploreTeam& Tm, Gen2Flags& F) {
    if (int rc = explore_validate(e, what, params, P, Tm, F)) return rc;
    const int N = e->cfg.n_worlds, S = e->cfg.n_scenarios;
    if (S % N != 0 || S < 2 * N)
        return fail(e, CAGYM_E_INVALID, std::string(what) + ": n_scenarios must be a multiple of n_worlds and at least 2 * n_worlds (a ring of depth >= 2 per world)");
    if (e->rec_ready)
        return fail(e, CAGYM_E_STATE, std::string(what) + " with episode records initialised: their table has one row per pool slot, "
                                                          "which a streamed pool reuses");
    return CAGYM_OK;
}

int cagym_stream_exploration_scenarios(void* env, const cagym_explore_params* params, int32_t* n_failed_host, void* stream) {
    ENTRY(e, env);
    cagym_gen2_params P;
    ExploreTeam Tm;
    Gen2Flags F;
    if (int rc = explore_stream_check(e, "cagym_stream_exploration_scenarios", params, P, Tm, F)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ON_DEVICE(e);
    const int N = e->cfg.n_worlds, S = e->cfg.n_scenarios;
    if (int rc = stream_alloc(e)) return rc;  // as cagym_stream_scenarios
    ExploreDev& X = e->explore;
    if (!X.field_next) {
        if (int rc = block_alloc(e, [&](auto& v) { explore_members(X, (size_t)N, (size_t)S, v); })) return rc;
        X.n_list = reinterpret_cast<int32_t*>(X.fields_built + 1); X.cap = S - N;
    }
    StreamDev& T = e->stream;
    HIPCHK(e, hipMemsetAsync(T.generated, 0, 16, st));
    HIPCHK(e, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(T.generated), S, 1, st));
    HIPCHK(e, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(T.next_episode), T.depth, (size_t)N, st));
    HIPCHK(e, hipMemsetAsync(e->explore.fields_built, 0, 16, st));
    HIPCHK(e, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(e->explore.field_next), T.depth, (size_t)N, st));
    if (int rc = gen2_fill(e, P, F, T.n_failed, n_failed_host, st, &Tm)) return rc;
    e->stream_P = P;
    e->stream_team = Tm;
    e->streaming = true;
    e->explore_stream = true;
    return e->ig_ready ? ig_rebuild_fields(e, st) : CAGYM_OK;
}

int cagym_stream_set_exploration_params(void* env, const cagym_explore_params* params) {
    ENTRY_IF(e, env, e->streaming && e->explore_stream, "cagym_stream_set_exploration_params on a handle that streams no exploration worlds");
    cagym_gen2_params P;
    ExploreTeam Tm;
    Gen2Flags F;
    if (int rc = explore_stream_check(e, "cagym_stream_set_exploration_params", params, P, Tm, F)) return rc;
    if (Tm.R != e->stream_team.R)
        return fail(e, CAGYM_E_INVALID, "cagym_stream_set_exploration_params: n_robots is fixed while the stream runs (every slot of the ring holds the same team)");
    e->stream_P = P;  // (the handle's flags do not move: no RVO agents before or after)
    e->stream_team = Tm;
    return CAGYM_OK;
}

int cagym_explore_stream_get(void* env, const int32_t** field_next, const uint64_t** fields_built) {
    ENTRY_IF(e, env, e->explore.field_next != nullptr, "cagym_explore_stream_get before cagym_stream_exploration_scenarios");
    if (field_next) *field_next = e->explore.field_next;
    if (fields_built) *fields_built = reinterpret_cast<const uint64_t*>(e->explore.fields_built);
    return CAGYM_OK;
}

int cagym_get_obstacles(void* env, const double** obst, const int32_t** n_obst) {
    ENTRY(e, env);
    if (!obst || !n_obst) return fail(e, CAGYM_E_INVALID, "null out");
    *obst = e->cfg.max_obstacles > 0 ? e->sc_obst : nullptr;
    *n_obst = e->cfg.max_obstacles > 0 ? e->D.sc_nobst : nullptr;
    return CAGYM_OK;
}

int cagym_get_scenarios(void* env, cagym_scenario_ptrs* out) {
    ENTRY(e, env);
    if (!out) return fail(e, CAGYM_E_INVALID, "null out");
    out->agents6 = e->D.sc_agents6;
    out->policy = e->D.sc_policy;
    out->dynamics = e->D.sc_dyn;
    out->n_agents = e->D.sc_nagents;
    out->coop = e->D.sc_coop;
    return CAGYM_OK;
}

int cagym_reset(void* env, const uint8_t* world_mask, int advance_episode, const cagym_outputs* out, void* stream) {
    ENTRY_POOL(e, env, "cagym_reset");
    ON_DEVICE_VOIDS_BEGUN(e);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const CagymOut o = to_out(e, out, true);
    if (int rc = launch_reset(e, world_mask, advance_episode, o, st)) return rc;
    if (int rc = episodes_restart(e, world_mask, false, st)) return rc;
    if (e->cfg.laserscan && o.laserscan) return cagym_laserscan(env, o.laserscan, stream);
    return CAGYM_OK;
}

int cagym_step(void* env, const float* ext_actions, const cagym_outputs* out, void* stream) {
    ENTRY_POOL(e, env, "cagym_step");
    ON_DEVICE_VOIDS_BEGUN(e);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const CagymOut o = to_out(e, out);
    if (e->generation == 3) launch3(e, K3_HALF_NONE, false, false, ext_actions, 1, o, st);
    else hipLaunchKernelGGL(k_step, dim3(n_waves(e)), dim3(64), cagym_lds_bytes(e->cfg.max_agents), st, e->D, ext_actions, o);
    HIPCHK(e, hipGetLastError());
    if (e->generation != 3 && o.laserscan) return cagym_laserscan(env, o.laserscan, stream);  // generation 3 scans in-kernel ...
    return fill_empty_scan(e, o, st);                                                         // ... in its OBST instantiation
}

int cagym_step_autoreset(void* env, const float* ext_actions, const cagym_outputs* out, void* stream) {
    ENTRY_POOL(e, env, "cagym_step_autoreset");
    ON_DEVICE_VOIDS_BEGUN(e);
    if (e->generation != 3) return fail(e, CAGYM_E_UNSUPPORTED, "cagym_step_autoreset needs the generation-3 kernels");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const CagymOut o = to_out(e, out);
    launch3(e, K3_HALF_NONE, false, true, ext_actions, 1, o, st);
    HIPCHK(e, hipGetLastError());
    return fill_empty_scan(e, o, st);  // the scan of the (possibly restarted) worlds is part of the launch
}

// ---- terminal observations and the trajectory ring (csrc/cagym_terminal.h) ---------------------------------------------------------
int cagym_step_autoreset_keep(void* env, const float* ext_actions, const cagym_outputs* out, const cagym_terminal_outputs* term, void* stream) {
    ENTRY_POOL(e, env, "cagym_step_autoreset_keep");
    ON_DEVICE_VOIDS_BEGUN(e);
    if (e->generation != 3) return fail(e, CAGYM_E_UNSUPPORTED, "cagym_step_autoreset_keep needs the generation-3 kernels");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    CagymOut o = to_out(e, out);
    if (!o.game_over) o.game_over = e->go_scratch;
    // 1. the step, without the restart: `out` and the state hold the terminal observation and the terminal state
    launch3(e, K3_HALF_NONE, false, false, ext_actions, 1, o, st);
    HIPCHK(e, hipGetLastError());
    if (int rc = fill_empty_scan(e, o, st)) return rc;
    // 2. the finished worlds' rows into `term`, and the ring's slice
    TermOut t{};
    if (term) {
        t.obs_oas = o.obs_oas ? term->obs_oas : nullptr;
        t.obs_ego = o.obs_ego ? term->obs_ego : nullptr;
        t.laserscan = o.laserscan ? term->laserscan : nullptr;
    }
    const unsigned n_row_wg = (t.obs_oas || t.obs_ego || t.laserscan) ? tcap_row_wgs(e->cfg.n_worlds) : 0u;
    const unsigned n_slice_wg = e->traj_ready ? tcap_slice_wgs(e->cfg.n_worlds, e->cfg.max_agents) : 0u;
    if (n_row_wg + n_slice_wg) {
        hipLaunchKernelGGL(k_terminal_capture, dim3(n_row_wg + n_slice_wg), dim3(TCAP_NT), 0, st, e->D, o, t, e->traj, n_row_wg);
        HIPCHK(e, hipGetLastError());
    }
    // 3. DummyVecEnv's restart of exactly those worlds: only their observations are rewritten, the terminal reward / flags / game_over stay
    CagymOut r = to_out(e, out, true);
    r.reward = nullptr; r.flags = nullptr; r.game_over = nullptr;
    if (int rc = launch_reset(e, o.game_over, 1, r, st)) return rc;
    if (e->cfg.laserscan && r.laserscan) return cagym_laserscan(env, r.laserscan, stream);
    return CAGYM_OK;
}

int cagym_trajectory_init(void* env, int n_slices, void* stream) {
    ENTRY_POOL(e, env, "cagym_trajectory_init");
    if (n_slices < 1) return fail(e, CAGYM_E_INVALID, "cagym_trajectory_init: n_slices must be >= 1");
    if (e->generation != 3) return fail(e, CAGYM_E_UNSUPPORTED, "the trajectory ring is fed by cagym_step_autoreset_keep, which needs the generation-3 kernels");
    ON_DEVICE(e);
    const size_t N = e->cfg.n_worlds, M = e->cfg.max_agents, NM = N * M, L = (size_t)n_slices, n_wg = tcap_slice_wgs((int)N, (int)M);
    TrajRing R = e->traj;
    if (!R.t_prev) {  // the running block: once per handle
        if (int rc = block_alloc(e, [&](auto& v) { traj_run_members(R, NM, n_wg, v); })) return rc;
        e->traj = R;  // kept whatever becomes of the ring's allocation
    }
    if (!e->traj_ring || R.L != n_slices) {  // the ring: once per n_slices
        const size_t per_slice = block_bytes([&](auto& v) { traj_ring_members(R, N, NM, 1, v); });
        if (L > ((size_t)1 << 46) / per_slice) return fail(e, CAGYM_E_NOMEM, "cagym_trajectory_init: the ring does not fit");
        if (int rc = ring_alloc(e, &e->traj_ring, "traj_ring", true, [&](auto& v) { traj_ring_members(R, N, NM, L, v); })) return rc;
        R.L = n_slices;
    }
    e->traj = R;
    e->traj_ready = true;
    return traj_restart(e, nullptr, true, reinterpret_cast<hipStream_t>(stream));
}

int cagym_trajectory_restart(void* env, const uint8_t* world_mask, int clear, void* stream) {
    ENTRY_POOL(e, env, "cagym_trajectory_restart");
    REQUIRE(e, e->traj_ready, "cagym_trajectory_restart", "cagym_trajectory_init");
    ON_DEVICE(e);
    return traj_restart(e, world_mask, clear != 0, reinterpret_cast<hipStream_t>(stream));
}

int cagym_trajectory_get(void* env, cagym_trajectory_ptrs* out) {
    ENTRY_POOL(e, env, "cagym_trajectory_get");
    REQUIRE(e, e->traj_ready, "cagym_trajectory_get", "cagym_trajectory_init");
    if (!out) return fail(e, CAGYM_E_INVALID, "null out");
    const TrajRing& R = e->traj;
    out->rows = R.rows; out->moved = R.moved; out->episode = R.episode; out->last = R.last;
    out->head = reinterpret_cast<const uint64_t*>(R.head); out->desync = R.desync; out->t_prev = R.t_prev; out->seen = R.seen;
    out->n_slices = R.L;
    return CAGYM_OK;
}

// ---- the split step (csrc/cagym_split3.h) -----------------------------------------------------------------------------------------
int cagym_step_begin(void* env, void* stream) {
    ENTRY_POOL(e, env, "cagym_step_begin");
    if (e->generation != 3) return fail(e, CAGYM_E_UNSUPPORTED, "the split step needs the generation-3 kernels");
    ON_DEVICE(e);
    e->begun = true;
    if (!e->any_rvo) return CAGYM_OK;  // no internal RVO policy: nothing to solve ahead of the external actions
    launch3(e, K3_HALF_PRE, false, false, nullptr, 1, CagymOut{}, reinterpret_cast<hipStream_t>(stream));
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

int cagym_step_finish(void* env, const float* ext_actions, const cagym_outputs* out, int auto_reset, void* stream) {
    ENTRY_POOL(e, env, "cagym_step_finish");
    if (e->generation != 3) return fail(e, CAGYM_E_UNSUPPORTED, "the split step needs the generation-3 kernels");
    if (!e->begun) return fail(e, CAGYM_E_STATE, "cagym_step_finish without a cagym_step_begin on the current state");
    ON_DEVICE_VOIDS_BEGUN(e);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const CagymOut o = to_out(e, out);
    launch3(e, K3_HALF_POST, false, auto_reset != 0, ext_actions, 1, o, st);
    HIPCHK(e, hipGetLastError());
    return fill_empty_scan(e, o, st);
}

int cagym_rollout(void* env, int n_steps, int auto_reset, const cagym_outputs* out, void* stream) {
    ENTRY_POOL(e, env, "cagym_rollout");
    ON_DEVICE_VOIDS_BEGUN(e);
    if (n_steps < 1) return fail(e, CAGYM_E_INVALID, "n_steps must be >= 1");
    if (e->cfg.laserscan && out && out->laserscan && e->generation != 3)
        return fail(e, CAGYM_E_UNSUPPORTED, "cagym_rollout produces laserscan with the generation-3 kernels only");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const CagymOut o = to_out(e, out);
    const size_t lds = cagym_lds_bytes(e->cfg.max_agents);
    if (e->generation == 3) launch3(e, K3_HALF_NONE, true, auto_reset != 0, nullptr, n_steps, o, st);
    else if (auto_reset) hipLaunchKernelGGL(k_rollout<true>, dim3(n_waves(e)), dim3(64), lds, st, e->D, n_steps, o);
    else hipLaunchKernelGGL(k_rollout<false>, dim3(n_waves(e)), dim3(64), lds, st, e->D, n_steps, o);
    HIPCHK(e, hipGetLastError());
    return fill_empty_scan(e, o, st, n_steps);
}

int cagym_kernel_name(void* env, int rollout, int auto_reset, char* buf, int buf_len) {
    Env* e = reinterpret_cast<Env*>(env);
    if (!e || !buf || buf_len < 1) return fail(e, CAGYM_E_INVALID, "bad arguments");
    if (e->generation == 3) {
        const Spec2 sp = spec2(e);
        snprintf(buf, (size_t)buf_len, "%s%d<%d, %d, %d, %s, %s>", rollout ? "k_rollout" : "k_step", e->generation, sp.nt, sp.mt,
                 sp.wpw, auto_reset ? "true" : "false", has_map(e) ? "true" : "false");
    } else if (rollout) {
        snprintf(buf, (size_t)buf_len, "k_rollout<%s>", auto_reset ? "true" : "false");
    } else {
        snprintf(buf, (size_t)buf_len, "k_step");
    }
    return CAGYM_OK;
}

int cagym_laserscan(void* env, float* laserscan, void* stream) {
    ENTRY(e, env);
    if (!laserscan) return fail(e, CAGYM_E_INVALID, "null laserscan buffer");
    ON_DEVICE(e);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    size_t total = (size_t)e->cfg.n_worlds * e->cfg.max_agents * 16;
    hipLaunchKernelGGL(k_laserscan, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, e->D, laserscan);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

int cagym_occupancy_grid(void* env, uint8_t* grid, void* stream) {
    ENTRY(e, env);
    if (!grid) return fail(e, CAGYM_E_INVALID, "null grid buffer");
    if (e->cfg.max_obstacles <= 0) return fail(e, CAGYM_E_STATE, "cagym_occupancy_grid needs an env created with max_obstacles > 0");
    ON_DEVICE(e);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_occupancy_grid, dim3((unsigned)((size_t)e->cfg.n_worlds * e->cfg.max_agents)), dim3(256), 0, st, e->D, grid);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

int cagym_get_state(void* env, cagym_state_ptrs* out) {
    Env* e = reinterpret_cast<Env*>(env);
    if (!e || !out) return fail(e, CAGYM_E_INVALID, "null argument");
    const CagymDev& D = e->D;
    out->pos_x = D.px; out->pos_y = D.py; out->vel_x = D.vx; out->vel_y = D.vy; out->heading = D.heading;
    out->heading_ego = D.heading_ego; out->dist_to_goal = D.dist_goal; out->time_remaining = D.time_rem; out->t = D.t;
    out->goal_x = D.gx; out->goal_y = D.gy; out->radius = D.radius; out->pref_speed = D.pref; out->speed = D.speed;
    out->delta_heading = D.dhead; out->aux0 = D.aux0; out->aux1 = D.aux1;
    out->action = D.action; out->status = D.status; out->step_num = D.step_num; out->n_agents = D.n_agents;
    out->n_observed = D.n_observed; out->episode = D.episode; out->map_bits = const_cast<uint32_t*>(D.map_bits);
    out->stat_return = D.stat_return; out->stat_episodes = D.stat_episodes; out->stat_steps = D.stat_steps;
    out->stat_outcomes = D.stat_outcomes;
    return CAGYM_OK;
}

// one 24-byte record per world (cagym.h: cagym_pack_episode_stats)
__global__ void __launch_bounds__(256) k_pack_stats(CagymDev D, int32_t* __restrict__ rec) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= D.N) return;
    int2* r = reinterpret_cast<int2*>(rec + (size_t)w * 6);  // 24-byte records: 8-byte aligned
    r[0] = make_int2(__float_as_int(D.stat_return[w]), D.stat_episodes[w]);
    r[1] = make_int2(D.stat_steps[w], D.stat_outcomes[3 * w]);
    r[2] = make_int2(D.stat_outcomes[3 * w + 1], D.stat_outcomes[3 * w + 2]);
}

int cagym_pack_episode_stats(void* env, int32_t* records, void* stream) {
    ENTRY(e, env);
    if (!records) return fail(e, CAGYM_E_INVALID, "null records buffer");
    ON_DEVICE(e);
    hipLaunchKernelGGL(k_pack_stats, dim3((unsigned)((e->cfg.n_worlds + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), e->D, records);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

// which forward kernel (read per call: the A/B tests flip it inside one process): default = split-f16 matrix cores
// (cagym_ga3c16.h); CAGYM_GA3C=mfma32: round 2's exact-fp32 matrix-core kernel; =valu: round 1's vector kernel
enum { GA_KERNEL_H16 = 0, GA_KERNEL_MFMA32 = 1, GA_KERNEL_VALU = 2 };
static int ga3c_kernel_choice(Env* e, int* kernel) {
    const char* which = getenv("CAGYM_GA3C");
    if (!which || !which[0] || !strcmp(which, "h16")) *kernel = GA_KERNEL_H16;
    else if (!strcmp(which, "mfma32")) *kernel = GA_KERNEL_MFMA32;
    else if (!strcmp(which, "valu")) *kernel = GA_KERNEL_VALU;
    else return fail(e, CAGYM_E_INVALID, "CAGYM_GA3C: unknown forward kernel (h16, mfma32 or valu)");
    return CAGYM_OK;
}

// the handle's packed copy of `weights`: made on `st` the first time a blob (by address) is used; a caller that rewrites the
// blob in place says so with cagym_ga3c_load_weights
static int ga3c_pack(Env* e, const float* weights, hipStream_t st, bool force) {
    if (!force && e->ga3c_packed_src == weights) return CAGYM_OK;
    hipLaunchKernelGGL(k_ga3c_pack16, dim3((GA16_PACK_THREADS + 255) / 256), dim3(256), 0, st, weights, e->ga3c_packed);
    const hipError_t s = hipGetLastError();
    if (s != hipSuccess) {
        e->ga3c_packed_src = nullptr;
        return fail(e, CAGYM_E_HIP, std::string("k_ga3c_pack16: ") + hipGetErrorString(s));
    }
    e->ga3c_packed_src = weights;
    return CAGYM_OK;
}

int cagym_ga3c_load_weights(void* env, const float* weights, void* stream) {
    ENTRY(e, env);
    if (!weights) return fail(e, CAGYM_E_INVALID, "null weights");
    ON_DEVICE(e);
    return ga3c_pack(e, weights, reinterpret_cast<hipStream_t>(stream), true);
}

static void launch_ga3c_state(Env* e, int max_observed, const int32_t* agent_idx, long long rows, uint32_t* ctr, float* state,
                              hipStream_t st) {
    if (e->cfg.max_agents <= 16)
        hipLaunchKernelGGL(k_ga3c_state<16>, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, st, e->D, max_observed, agent_idx, (int)rows, ctr, state);
    else
        hipLaunchKernelGGL(k_ga3c_state<32>, dim3((unsigned)((rows + 7) / 8)), dim3(256), 0, st, e->D, max_observed, agent_idx, (int)rows, ctr, state);
}

int cagym_ga3c_state(void* env, int max_observed, float* state, void* stream) {
    ENTRY(e, env);
    if (!state || max_observed < 1 || max_observed > 10) return fail(e, CAGYM_E_INVALID, "bad arguments (max_observed in 1..10)");
    ON_DEVICE(e);
    launch_ga3c_state(e, max_observed, nullptr, (long long)e->cfg.n_worlds * e->cfg.max_agents, nullptr, state, reinterpret_cast<hipStream_t>(stream));
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

// The default forward kernel of cagym_ga3c_act / cagym_ga3c_act_merge, one launch: list, state rows and network per workgroup of
// 32 worlds (cagym_ga3c16.h).  merge: the status lanes also copy the rows of every other agent from ext_in (null: zeros).
static int ga3c_act_h16(Env* e, const float* weights, int max_observed, float* actions, bool merge, const float* ext_in, hipStream_t st) {
    if (int rc = ga3c_pack(e, weights, st, false)) return rc;
    const bool lpa16 = e->cfg.max_agents <= 16;
    auto* kernel = merge ? (lpa16 ? k_ga3c_act_h16<16, true> : k_ga3c_act_h16<32, true>) : (lpa16 ? k_ga3c_act_h16<16, false> : k_ga3c_act_h16<32, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)((e->cfg.n_worlds + 31) / 32)), dim3(512), 0, st, e->D, e->ga3c_packed, max_observed, actions, ext_in);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

size_t cagym_ga3c_act_workspace_bytes(void* env) {
    Env* e = reinterpret_cast<Env*>(env);
    if (!e) return 0;
    const size_t total = (size_t)e->cfg.n_worlds * e->cfg.max_agents;
    return 256 + a16(total * sizeof(int32_t)) + total * 76 * sizeof(float);  // [count | agent list | state rows]
}

int cagym_ga3c_act(void* env, const float* weights, int max_observed, void* work, float* ext_actions, void* stream) {
    ENTRY(e, env);
    if (!weights || !work || !ext_actions || max_observed < 1 || max_observed > 10)
        return fail(e, CAGYM_E_INVALID, "bad arguments (max_observed in 1..10)");
    ON_DEVICE(e);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int which;
    if (int rc = ga3c_kernel_choice(e, &which)) return rc;
    if (which == GA_KERNEL_H16) return ga3c_act_h16(e, weights, max_observed, ext_actions, false, nullptr, st);  // `work` is not used
    // CAGYM_GA3C=mfma32 / valu (A/B): the three-launch chain of rounds 2 - 3
    const size_t total = (size_t)e->cfg.n_worlds * e->cfg.max_agents;
    int32_t* idx = reinterpret_cast<int32_t*>(reinterpret_cast<unsigned char*>(work) + 256);
    float* state = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(work) + 256 + a16(total * sizeof(int32_t)));
    // no memset in front of the chain: the handle's ticket words carry the list from call to call (k_ga3c_select)
    uint32_t* ctr = reinterpret_cast<uint32_t*>(e->ga3c_ctr);
    // a launch that fails cuts the chain: the forward kernel is the one that starts the next list, so the ticket words are
    // re-zeroed (on the same stream) before the error is returned and the next call starts from an empty list again
    auto launched = [&](const char* what) -> int {
        const hipError_t s = hipGetLastError();
        if (s == hipSuccess) return CAGYM_OK;
        (void)hipMemsetAsync(e->ga3c_ctr, 0, 4 * sizeof(int32_t), st);
        return fail(e, CAGYM_E_HIP, std::string(what) + ": " + hipGetErrorString(s));
    };
    hipLaunchKernelGGL(k_ga3c_select, dim3((unsigned)((total + 1023) / 1024)), dim3(1024), 0, st, e->D, idx, ctr);
    if (int rc = launched("k_ga3c_select")) return rc;
    // the list length stays on the device: both kernels are launched for the worst case and leave beyond it
    launch_ga3c_state(e, max_observed, idx, (long long)total, ctr, state, st);
    if (int rc = launched("k_ga3c_state")) return rc;
    hipLaunchKernelGGL(k_ga3c_forward_mfma, dim3((unsigned)((total + 31) / 32)), dim3(256), 0, st, weights, state, idx, 0, e->ga3c_ctr + 2, e->D.pref,
                       ext_actions, (int32_t*)nullptr, (float*)nullptr, ctr);
    if (int rc = launched("k_ga3c_forward")) return rc;
    return CAGYM_OK;
}

int cagym_ga3c_act_merge(void* env, const float* weights, int max_observed, void* work, const float* ext_in, float* actions, void* stream) {
    ENTRY(e, env);
    if (!weights || !work || !actions || max_observed < 1 || max_observed > 10)
        return fail(e, CAGYM_E_INVALID, "bad arguments (max_observed in 1..10)");
    const size_t total = (size_t)e->cfg.n_worlds * e->cfg.max_agents;
    if (ext_in && ext_in < actions + 2 * total && actions < ext_in + 2 * total) return fail(e, CAGYM_E_INVALID, "ext_in aliases actions");
    if ((reinterpret_cast<uintptr_t>(actions) | reinterpret_cast<uintptr_t>(ext_in)) & 7)
        return fail(e, CAGYM_E_INVALID, "actions / ext_in must be 8-byte aligned");
    ON_DEVICE(e);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int which;
    if (int rc = ga3c_kernel_choice(e, &which)) return rc;
    if (which == GA_KERNEL_H16) return ga3c_act_h16(e, weights, max_observed, actions, true, ext_in, st);
    // CAGYM_GA3C=mfma32 / valu (A/B): the table first, then cagym_ga3c_act's chain over it
    if (ext_in) HIPCHK(e, hipMemcpyAsync(actions, ext_in, total * 2 * sizeof(float), hipMemcpyDeviceToDevice, st));
    else HIPCHK(e, hipMemsetAsync(actions, 0, total * 2 * sizeof(float), st));
    return cagym_ga3c_act(env, weights, max_observed, work, actions, stream);
}

#ifdef CAGYM_STAMPS
int cagym_debug_stamps(unsigned long long* out16, int reset) {
    if (out16) hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 16);
    if (reset) {
        unsigned long long z[16] = {0};
        hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof(z));
    }
    return 0;
}
#endif

#ifdef CAGYM_WAVETRACE
int cagym_debug_wavetrace_select(int wg) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_wt_wg), &wg, sizeof(int)); }
int cagym_debug_wavetrace(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wavetrace), sizeof(unsigned long long) * CAGYM_WT_STEPS * CAGYM_WT_POINTS * 8);
}
#endif

#ifdef CAGYM_XTRACE
int cagym_debug_xtrace(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_xtrace), sizeof(unsigned long long) * CAGYM_XT_WGS * CAGYM_XT_STEPS * 8);
}
#endif

#ifdef CAGYM_WGTRACE
int cagym_debug_wgtrace(unsigned long long* out, int n_wg) {
    if (n_wg > CAGYM_WGTRACE_MAXWG) n_wg = CAGYM_WGTRACE_MAXWG;
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wgtrace), sizeof(unsigned long long) * CAGYM_WGTRACE_W * (size_t)n_wg);
}
#endif

int cagym_ga3c_forward(void* env, const float* weights, const float* state, const int32_t* agent_idx, int B,
                       float* ext_actions, int32_t* action_index, float* probs, void* stream) {
    ENTRY(e, env);
    if (!weights || !state || !agent_idx || B < 0) return fail(e, CAGYM_E_INVALID, "bad arguments");
    if (B == 0) return CAGYM_OK;
    ON_DEVICE(e);
    // 32 agents per workgroup reuse every weight 32 times; small batches take 16 so that each CU still gets >= 2 workgroups
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int which;
    if (int rc = ga3c_kernel_choice(e, &which)) return rc;
    if (which == GA_KERNEL_H16) {
        if (int rc = ga3c_pack(e, weights, st, false)) return rc;
        hipLaunchKernelGGL(k_ga3c_forward_h16, dim3((unsigned)((B + 31) / 32)), dim3(512), 0, st, e->ga3c_packed, state, agent_idx, B, e->D.pref,
                           ext_actions, action_index, probs);
    } else if (which == GA_KERNEL_MFMA32)
        hipLaunchKernelGGL(k_ga3c_forward_mfma, dim3((unsigned)((B + 31) / 32)), dim3(256), 0, st, weights, state, agent_idx, B,
                           (const int32_t*)nullptr, e->D.pref, ext_actions, action_index, probs, (uint32_t*)nullptr);
    else if (B <= 16 * 1024)
        hipLaunchKernelGGL(k_ga3c_forward<16>, dim3((unsigned)((B + 15) / 16)), dim3(256), 0, st, weights, state, agent_idx, B,
                           e->D.pref, ext_actions, action_index, probs);
    else
        hipLaunchKernelGGL(k_ga3c_forward<32>, dim3((unsigned)((B + 31) / 32)), dim3(256), 0, st, weights, state, agent_idx, B,
                           e->D.pref, ext_actions, action_index, probs);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

// ---- information-gain primitives -----------------------------------------------------------------
int cagym_ig_init(void* env, void* stream) {
    ENTRY_POOL(e, env, "cagym_ig_init");
    if (e->streaming && !e->explore_stream)
        return fail(e, CAGYM_E_UNSUPPORTED, "cagym_ig_init on a streaming handle: the per-slot distance field is not rebuilt by cagym_stream_refill");
    if (e->cfg.max_obstacles <= 0 || !e->D.map_bits)
        return fail(e, CAGYM_E_UNSUPPORTED, "information-gain primitives need obstacle rasters (max_obstacles > 0)");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ON_DEVICE(e);
    const size_t S = e->cfg.n_scenarios, N = e->cfg.n_worlds;
    if (!e->G.d2) {
        int rc;
        if ((rc = dalloc(e, &e->G.d2, S * CAGYM_MAPD * CAGYM_MAPD)) != CAGYM_OK) return rc;
        if ((rc = dalloc(e, &e->G.belief, N * IG_BEL * IG_BEL)) != CAGYM_OK) return rc;
        if ((rc = dalloc(e, &e->G.mi, N * IG_BEL * IG_BEL)) != CAGYM_OK) return rc;
        if ((rc = dalloc(e, &e->ig_any, S)) != CAGYM_OK) return rc;
        if ((rc = dalloc(e, &e->ig_ep.running, N)) != CAGYM_OK) return rc;
        if ((rc = dalloc(e, &e->ig_ep.sum, N)) != CAGYM_OK) return rc;
        if ((rc = dalloc(e, &e->ig_ep.last, N)) != CAGYM_OK) return rc;
        if ((rc = dalloc(e, &e->ig_ep.episodes, N)) != CAGYM_OK) return rc;
    }
    e->G.N = (int)N; e->G.S = (int)S; e->G.map_bits = e->D.map_bits; e->G.sc_nobst = e->D.sc_nobst; e->G.episode = e->D.episode;
    HIPCHK(e, hipMemsetAsync(e->ig_any, 0, S * sizeof(uint32_t), st));
    HIPCHK(e, hipMemsetAsync(e->ig_ep.running, 0, N * sizeof(double), st));
    HIPCHK(e, hipMemsetAsync(e->ig_ep.sum, 0, N * sizeof(double), st));
    HIPCHK(e, hipMemsetAsync(e->ig_ep.last, 0, N * sizeof(double), st));
    HIPCHK(e, hipMemsetAsync(e->ig_ep.episodes, 0, N * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_ig_edt_cols, dim3((unsigned)S), dim3(320), 0, st, e->G, e->ig_any);
    hipLaunchKernelGGL(k_ig_edt_rows, dim3((unsigned)(S * CAGYM_MAPD)), dim3(320), 0, st, e->G, e->ig_any);
    hipLaunchKernelGGL(k_ig_fill_belief, dim3((unsigned)N), dim3(256), 0, st, e->G, (const uint8_t*)nullptr);
    HIPCHK(e, hipGetLastError());
    if (e->streaming)  // an exploration stream: every field is current, which arms the refresh behind cagym_stream_refill
        HIPCHK(e, hipMemcpyAsync(e->explore.field_next, e->stream.next_episode, N * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    e->ig_ready = true;
    return CAGYM_OK;
}

int cagym_ig_reset_belief(void* env, const uint8_t* world_mask, void* stream) {
    ENTRY_IG(e, env, "cagym_ig_reset_belief");
    ON_DEVICE(e);
    hipLaunchKernelGGL(k_ig_fill_belief, dim3((unsigned)e->cfg.n_worlds), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), e->G, world_mask);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

int cagym_ig_get(void* env, uint32_t** edf_d2, double** belief) {
    ENTRY_IG(e, env, "cagym_ig_get");
    ON_DEVICE(e);
    if (edf_d2) *edf_d2 = e->G.d2;
    if (belief) *belief = e->G.belief;
    return CAGYM_OK;
}

int cagym_ig_get_episode_stats(void* env, double** running, double** sum, double** last, int32_t** episodes) {
    ENTRY_IG(e, env, "cagym_ig_get_episode_stats");
    ON_DEVICE(e);
    if (running) *running = e->ig_ep.running;
    if (sum) *sum = e->ig_ep.sum;
    if (last) *last = e->ig_ep.last;
    if (episodes) *episodes = e->ig_ep.episodes;
    return CAGYM_OK;
}

int cagym_ig_visible_cells(void* env, const double* poses, const int32_t* world, int Q, double fov_rad, double range,
                           uint64_t* masks, void* stream) {
    ENTRY_IG(e, env, "cagym_ig_visible_cells");
    ON_DEVICE(e);
    if (Q < 0 || !poses || !world || !masks) return fail(e, CAGYM_E_INVALID, "bad arguments");
    if (Q == 0) return CAGYM_OK;
    hipLaunchKernelGGL(k_ig_visible, dim3((unsigned)Q), dim3(128), 0, reinterpret_cast<hipStream_t>(stream), e->G, poses,
                       world, fov_rad, range, reinterpret_cast<unsigned long long*>(masks));
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

int cagym_ig_update_belief(void* env, const double* poses, const int32_t* n_poses, const double* detections,
                           const int32_t* n_det, int P, int Dmax, double fov_rad, double range, uint64_t* observed,
                           void* stream) {
    ENTRY_IG(e, env, "cagym_ig_update_belief");
    ON_DEVICE(e);
    if (P < 1 || Dmax < 1 || !poses || !detections || !n_det) return fail(e, CAGYM_E_INVALID, "bad arguments");
    hipLaunchKernelGGL(k_ig_update, dim3((unsigned)e->cfg.n_worlds), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       e->G, poses, n_poses, detections, n_det, P, Dmax, fov_rad, range,
                       reinterpret_cast<unsigned long long*>(observed));
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

int cagym_ig_mi_reward(void* env, const uint64_t* masks, const int32_t* world, int Q, double* reward, void* stream) {
    ENTRY_IG(e, env, "cagym_ig_mi_reward");
    ON_DEVICE(e);
    if (Q < 0 || !masks || !world || !reward) return fail(e, CAGYM_E_INVALID, "bad arguments");
    if (Q == 0) return CAGYM_OK;
    hipLaunchKernelGGL(k_ig_reward, dim3((unsigned)Q), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), e->G,
                       reinterpret_cast<const unsigned long long*>(masks), world, reward);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

int cagym_ig_next_pose(void* env, const double* poses, const double* actions, const int32_t* world,
                       const double* radius, int Q, int xdt, double dt, double* next, uint8_t* feasible, void* stream) {
    ENTRY_IG(e, env, "cagym_ig_next_pose");
    ON_DEVICE(e);
    if (Q < 0 || xdt < 1 || xdt > 1000 || !poses || !actions || !world || !radius || !next || !feasible)
        return fail(e, CAGYM_E_INVALID, "bad arguments");
    if (Q == 0) return CAGYM_OK;
    hipLaunchKernelGGL(k_ig_next_pose, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), e->G, poses, actions, world, radius, Q, xdt, dt, next,
                       feasible);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

int cagym_ig_rollouts(void* env, const double* pose0, const uint64_t* observed0, const uint64_t* exclude,
                      const int32_t* world, const int32_t* n_steps, const double* radius, int Q, int nsims,
                      int max_steps, int xdt, double dt, double fov_rad, double range, uint64_t seed, double* rewards,
                      uint8_t* actions, double* final_pose, uint64_t* observed_out, void* stream) {
    ENTRY_IG(e, env, "cagym_ig_rollouts");
    ON_DEVICE(e);
    if (Q < 0 || nsims < 1 || max_steps < 0 || max_steps > 255 || xdt < 1 || xdt > 1000 || !pose0 || !observed0 ||
        !exclude || !world || !n_steps || !radius || !rewards)
        return fail(e, CAGYM_E_INVALID, "bad arguments");
    if (Q == 0) return CAGYM_OK;
    hipLaunchKernelGGL(k_ig_rollouts, dim3((unsigned)((size_t)Q * nsims)), dim3(128), 0,
                       reinterpret_cast<hipStream_t>(stream), e->G, pose0,
                       reinterpret_cast<const unsigned long long*>(observed0),
                       reinterpret_cast<const unsigned long long*>(exclude), world, n_steps, radius, nsims, max_steps, xdt,
                       dt, fov_rad, range, (unsigned long long)seed, rewards, actions, final_pose,
                       reinterpret_cast<unsigned long long*>(observed_out));
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

static int ig_robots_check(Env* e, int n_robots, const char* what) {
    if (!e->scenarios_set) return fail(e, CAGYM_E_STATE, std::string(what) + " before cagym_set_scenarios");
    if (e->n_ig == N_IG_RANDOM)
        return fail(e, CAGYM_E_STATE, std::string(what) + ": the generated pool's IG robot count is random (cagym_generate_scenarios)");
    if (n_robots < 1 || e->n_ig != n_robots)
        return fail(e, CAGYM_E_INVALID, std::string(what) + ": every scenario of the pool must hold exactly n_robots IG agents (" +
                                            (e->n_ig == N_IG_UNEQUAL ? std::string("the counts differ") : std::to_string(e->n_ig) + " per scenario") + ")");
    return CAGYM_OK;
}

// The argument checks the learner entries share; `name`: the entry, for the message.  Which of two errors wins is part of the ABI
// (tests/test_ig_learner_refusals.py): the team's range is checked in front of a parameter block, the pool's team (ig_robots_check) behind it.
static int ig_team_check(Env* e, const std::string& name, int n_robots) {
    return (n_robots < 1 || n_robots > IG_MAXR) ? fail(e, CAGYM_E_INVALID, name + ": n_robots must be 1..8") : CAGYM_OK;
}
static int ig_flags_check(Env* e, const std::string& name, uint32_t flags, uint32_t known) {
    return (flags & ~known) ? fail(e, CAGYM_E_INVALID, name + ": unknown flags") : CAGYM_OK;
}
// the head of a window's parameter block: team, window, rotate, flags
static int ig_frame_check(Env* e, const std::string& name, int n_robots, int window, int rotate, uint32_t flags, uint32_t known) {
    if (int rc = ig_team_check(e, name, n_robots)) return rc;
    if (window < 4 || window > 64 || (window & 1)) return fail(e, CAGYM_E_INVALID, name + ": window must be even and within 4..64");
    if (rotate != 0 && rotate != 1) return fail(e, CAGYM_E_INVALID, name + ": rotate must be 0 or 1");
    return ig_flags_check(e, name, flags, known);
}
static int ig_positive_check(Env* e, const std::string& name, std::initializer_list<double> values, const char* what) {
    for (double v : values)
        if (!(v > 0.0) || !std::isfinite(v))  // (the negated comparison refuses NaN)
            return fail(e, CAGYM_E_INVALID, name + ": " + what);
    return CAGYM_OK;
}
// the workgroups of a view-gain launch: IGV_PER_WG viewpoints of one world each (no int sum near INT_MAX); refused beyond one launch
static int igv_blocks(Env* e, const std::string& name, int n_points, long long* blocks) {
    *blocks = (long long)e->cfg.n_worlds * (((long long)n_points + IGV_PER_WG - 1) / IGV_PER_WG);
    return *blocks > 0x7fffffffll ? fail(e, CAGYM_E_INVALID, name + ": n_worlds * n_points is too large for one launch") : CAGYM_OK;
}

int cagym_ig_robot_inputs(void* env, int n_robots, double detect_range, const float* obs_oas, double* poses, double* detections,
                          int32_t* n_det, void* stream) {
    ENTRY(e, env);
    if (!obs_oas || !poses || !detections || !n_det) return fail(e, CAGYM_E_INVALID, "null argument");
    if (int rc = ig_robots_check(e, n_robots, "cagym_ig_robot_inputs")) return rc;
    ON_DEVICE(e);
    hipLaunchKernelGGL(k_ig_robot_inputs, dim3((unsigned)e->cfg.n_worlds), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), e->D,
                       n_robots, (float)detect_range, obs_oas, poses, detections, n_det);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

int cagym_ig_robot_actions(void* env, int n_robots, const double* planner_actions, float* actions, void* stream) {
    ENTRY(e, env);
    if (!planner_actions || !actions) return fail(e, CAGYM_E_INVALID, "null argument");
    if (reinterpret_cast<uintptr_t>(actions) & 7) return fail(e, CAGYM_E_INVALID, "actions must be 8-byte aligned");
    if (int rc = ig_robots_check(e, n_robots, "cagym_ig_robot_actions")) return rc;
    ON_DEVICE(e);
    hipLaunchKernelGGL(k_ig_robot_actions, dim3((unsigned)e->cfg.n_worlds), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), e->D,
                       n_robots, planner_actions, actions);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

namespace {
inline int dm_node_cap(const cagym_dmcts_params& p) { return 1 + 9 * (p.Ntree * p.Ncycles + 1); }
inline int dm_mask_cap(const cagym_dmcts_params& p) { return 1 + p.Ntree * p.Ncycles; }  // the root + one newly selected node per grow
inline size_t dm_align(size_t x) { return (x + 255) & ~(size_t)255; }
}  // namespace

size_t cagym_dmcts_workspace_bytes(int n_worlds, const cagym_dmcts_params* p) {
    if (!p || n_worlds < 1 || p->n_robots < 1 || p->Ntree < 1 || p->Ncycles < 1) return 0;
    const size_t trees = (size_t)n_worlds * p->n_robots;
    const size_t bytes = dm_align(trees * sizeof(DmPublished)) + dm_align(trees * 2 * sizeof(int32_t)) + dm_align(trees * (size_t)dm_node_cap(*p) * sizeof(DmNode)) +
                         dm_align(trees * (size_t)dm_mask_cap(*p) * sizeof(DmMasks)) + trees * (size_t)dm_node_cap(*p) * sizeof(double);  // (last: the trees' compact value arrays)
    if (p->parallel_agents != 1) return bytes;
    // agent-parallel mode: behind the above, the second publication buffer and the robots' distributions between the launches
    return dm_align(bytes) + dm_align(trees * sizeof(DmPublished)) + trees * sizeof(DmDist);
}

int cagym_dmcts_plan(void* env, const cagym_dmcts_params* params, const double* poses, void* workspace,
                     size_t workspace_bytes, double* actions, uint8_t* paths, double* stats, void* stream) {
    ENTRY_IG(e, env, "cagym_dmcts_plan");
    ON_DEVICE(e);
    if (!params || !poses || !workspace || !actions || !paths || !stats) return fail(e, CAGYM_E_INVALID, "null argument");
    const cagym_dmcts_params& p = *params;
    if (p.n_robots < 1 || p.n_robots > DM_MAXR || p.horizon < 1 || p.horizon > DM_MAXH || p.Nsims < 1 || p.Nsims > DM_MAXSIMS ||
        p.comm_n < 1 || p.comm_n > DM_MAXCOMM || p.Ntree < 1 || p.Ncycles < 1 || p.xdt < 1 || p.xdt > 1000 ||
        (size_t)p.Ntree * p.Ncycles > 100000)
        return fail(e, CAGYM_E_INVALID, "Dec-MCTS parameters out of range (n_robots<=8, horizon<=8, Nsims<=32, comm_n<=8)");
    if (p.parallel_agents > 1) return fail(e, CAGYM_E_INVALID, "Dec-MCTS parallel_agents must be 0 or 1");
    const int N = e->cfg.n_worlds;
    if (workspace_bytes < cagym_dmcts_workspace_bytes(N, params)) return fail(e, CAGYM_E_INVALID, "workspace too small");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t trees = (size_t)N * p.n_robots;
    unsigned char* base = reinterpret_cast<unsigned char*>(workspace);
    DmPublished* pub = reinterpret_cast<DmPublished*>(base);
    int32_t* nn = reinterpret_cast<int32_t*>(base + dm_align(trees * sizeof(DmPublished)));
    DmNode* nodes = reinterpret_cast<DmNode*>(base + dm_align(trees * sizeof(DmPublished)) + dm_align(trees * 2 * sizeof(int32_t)));
    DmMasks* masks = reinterpret_cast<DmMasks*>(reinterpret_cast<unsigned char*>(nodes) + dm_align(trees * (size_t)dm_node_cap(p) * sizeof(DmNode)));
    double* mu = reinterpret_cast<double*>(reinterpret_cast<unsigned char*>(masks) + dm_align(trees * (size_t)dm_mask_cap(p) * sizeof(DmMasks)));
    // agent-parallel mode: the second publication buffer and the distributions (cagym_dmcts_workspace_bytes)
    DmPublished* pub2 = reinterpret_cast<DmPublished*>(reinterpret_cast<unsigned char*>(mu) + dm_align(trees * (size_t)dm_node_cap(p) * sizeof(double)));
    DmDist* dist = reinterpret_cast<DmDist*>(reinterpret_cast<unsigned char*>(pub2) + dm_align(trees * sizeof(DmPublished)));
    if (p.reset_comms) {
        HIPCHK(e, hipMemsetAsync(pub, 0, trees * sizeof(DmPublished), st));
        if (p.parallel_agents) HIPCHK(e, hipMemsetAsync(pub2, 0, trees * sizeof(DmPublished), st));
    }
    DmParams P;
    P.R = p.n_robots; P.Ntree = p.Ntree; P.Nsims = p.Nsims; P.horizon = p.horizon; P.Ncycles = p.Ncycles; P.comm_n = p.comm_n;
    P.node_cap = dm_node_cap(p); P.mask_cap = dm_mask_cap(p); P.xdt = p.xdt; P.call_base = p.call_base;
    P.c_p = p.c_p; P.gamma = p.gamma; P.radius = p.radius; P.dt = p.dt; P.fov = p.fov_rad; P.range = p.range; P.seed = p.seed;
    if (!p.parallel_agents) {
        hipLaunchKernelGGL(k_dmcts_plan, dim3((unsigned)N), dim3(DM_THREADS), 0, st, e->G, P, poses, nodes, masks, mu, nn, pub, actions, paths, stats);
        HIPCHK(e, hipGetLastError());
        return CAGYM_OK;
    }
    // one launch per cycle, each reading the publications of the one before from one buffer and writing the other.  The last
    // cycle writes `pub`, which both modes read at the next call; with an odd number of cycles the first reads a copy of it.
    DmPublished* buf[2] = {pub, pub2};
    if (p.Ncycles & 1) HIPCHK(e, hipMemcpyAsync(pub2, pub, trees * sizeof(DmPublished), hipMemcpyDeviceToDevice, st));
    for (int c = 0; c < p.Ncycles; c++) {
        hipLaunchKernelGGL(k_dmcts_plan_cycle, dim3((unsigned)trees), dim3(DM_THREADS), 0, st, e->G, P, c, poses, nodes, masks, mu, nn,
                           buf[(p.Ncycles - c) & 1], buf[(p.Ncycles - c - 1) & 1], dist, actions, paths, stats);
        HIPCHK(e, hipGetLastError());
    }
    return CAGYM_OK;
}

int cagym_ig_episode_boundary(void* env, const cagym_dmcts_params* params, const double* team_reward, const uint8_t* restart_mask,
                              uint32_t flags, void* workspace, size_t workspace_bytes, void* stream) {
    ENTRY_IG(e, env, "cagym_ig_episode_boundary");
    ON_DEVICE(e);
    if (!params || !workspace) return fail(e, CAGYM_E_INVALID, "null argument");
    cagym_dmcts_params p = *params;
    if (p.n_robots < 1 || p.n_robots > DM_MAXR || p.Ntree < 1 || p.Ncycles < 1 || (size_t)p.Ntree * p.Ncycles > 100000)
        return fail(e, CAGYM_E_INVALID, "Dec-MCTS parameters out of range (n_robots<=8, horizon<=8, Nsims<=32, comm_n<=8)");
    if (p.parallel_agents > 1) return fail(e, CAGYM_E_INVALID, "Dec-MCTS parallel_agents must be 0 or 1");
    if (flags & ~(uint32_t)(CAGYM_IG_EPISODE_FOLD | CAGYM_IG_EPISODE_PLANS_ONLY))
        return fail(e, CAGYM_E_INVALID, "cagym_ig_episode_boundary: unknown flags");
    const int N = e->cfg.n_worlds;
    if (workspace_bytes < cagym_dmcts_workspace_bytes(N, &p)) return fail(e, CAGYM_E_INVALID, "workspace too small");
    // the second publication buffer sits behind the sequential layout (cagym_dmcts_workspace_bytes); it is there when the
    // workspace is large enough for the agent-parallel mode, whatever the mode of this call
    p.parallel_agents = 0;
    const size_t seq_bytes = cagym_dmcts_workspace_bytes(N, &p);
    p.parallel_agents = 1;
    const bool has_pub2 = workspace_bytes >= cagym_dmcts_workspace_bytes(N, &p);
    unsigned char* base = reinterpret_cast<unsigned char*>(workspace);
    DmPublished* pub = reinterpret_cast<DmPublished*>(base);
    DmPublished* pub2 = has_pub2 ? reinterpret_cast<DmPublished*>(base + dm_align(seq_bytes)) : nullptr;
    hipLaunchKernelGGL(k_ig_episode_boundary, dim3((unsigned)N), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), e->G, e->ig_ep,
                       p.n_robots, (unsigned int)flags, team_reward, restart_mask, pub, pub2);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

int cagym_ig_greedy_plan(void* env, const cagym_ig_greedy_params* params, const double* poses, double* actions, uint8_t* choice,
                         double* mi, uint64_t* claimed, void* stream) {
    ENTRY_IG(e, env, "cagym_ig_greedy_plan");
    ON_DEVICE(e);
    if (!params || !poses || !actions || !choice) return fail(e, CAGYM_E_INVALID, "null argument");
    const cagym_ig_greedy_params& p = *params;
    if (int rc = ig_team_check(e, "cagym_ig_greedy_plan", p.n_robots)) return rc;
    if (p.coordinate != 0 && p.coordinate != 1) return fail(e, CAGYM_E_INVALID, "cagym_ig_greedy_plan: coordinate must be 0 or 1");
    const char* what = "dt, fov_rad and range must be finite and positive, radius finite and not negative";
    if (int rc = ig_positive_check(e, "cagym_ig_greedy_plan", {p.dt, p.fov_rad, p.range}, what)) return rc;
    if (!(p.radius >= 0.0) || !std::isfinite(p.radius)) return fail(e, CAGYM_E_INVALID, std::string("cagym_ig_greedy_plan: ") + what);
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(p.v[k]) || !std::isfinite(p.w[k])) return fail(e, CAGYM_E_INVALID, "cagym_ig_greedy_plan: non-finite candidate");
    IgGreedyParams P;
    P.R = p.n_robots; P.coordinate = p.coordinate; P.dt = p.dt; P.radius = p.radius; P.fov = p.fov_rad; P.range = p.range;
    P.v0 = p.v[0]; P.v1 = p.v[1]; P.v2 = p.v[2]; P.w0 = p.w[0]; P.w1 = p.w[1]; P.w2 = p.w[2];
    const size_t N = (size_t)e->cfg.n_worlds;
    hipLaunchKernelGGL(k_ig_greedy, dim3((unsigned)(p.coordinate ? N : N * p.n_robots)), dim3(IGG_THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream), e->G, P, poses, actions, choice, mi,
                       reinterpret_cast<unsigned long long*>(claimed));
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

int cagym_ig_observe(void* env, const cagym_ig_observe_params* params, const float* obs_oas, const uint8_t* restart_mask,
                     double* team_reward, double* gain, uint64_t* observed, float* belief_window, void* stream) {
    ENTRY_IG(e, env, "cagym_ig_observe");
    if (!params || !obs_oas) return fail(e, CAGYM_E_INVALID, "cagym_ig_observe: null argument");
    const cagym_ig_observe_params& p = *params;
    const char* name = "cagym_ig_observe";
    if (int rc = ig_frame_check(e, name, p.n_robots, p.window, p.rotate, p.flags, CAGYM_IG_EPISODE_FOLD | CAGYM_IG_OBSERVE_ONLY_RESTARTED)) return rc;
    if (int rc = ig_positive_check(e, name, {p.fov_rad, p.range, p.detect_range}, "fov_rad, range and detect_range must be finite and positive"))
        return rc;
    if (int rc = ig_robots_check(e, p.n_robots, name)) return rc;
    ON_DEVICE(e);
    IgObserveParams P;
    P.R = p.n_robots; P.G = p.window; P.rotate = p.rotate; P.flags = p.flags; P.det_range = (float)p.detect_range; P.fov = p.fov_rad; P.range = p.range;
    hipLaunchKernelGGL(k_ig_observe, dim3((unsigned)e->cfg.n_worlds), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), e->D, e->G, e->ig_ep,
                       P, obs_oas, restart_mask, team_reward, gain, reinterpret_cast<unsigned long long*>(observed), belief_window);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

int cagym_ig_context_window(void* env, const cagym_ig_context_params* params, const uint64_t* observed, const uint8_t* world_mask,
                            float* context_window, void* stream) {
    ENTRY_IG(e, env, "cagym_ig_context_window");
    if (!params || !context_window) return fail(e, CAGYM_E_INVALID, "cagym_ig_context_window: null argument");
    const cagym_ig_context_params& p = *params;
    const char* name = "cagym_ig_context_window";
    if (int rc = ig_frame_check(e, name, p.n_robots, p.window, p.rotate, p.flags, CAGYM_IG_CONTEXT_ONLY_MASKED)) return rc;
    if (int rc = ig_positive_check(e, name, {p.clear_max}, "clear_max must be finite and positive")) return rc;
    if (int rc = ig_robots_check(e, p.n_robots, name)) return rc;
    ON_DEVICE(e);
    IgContextParams P;
    P.R = p.n_robots; P.G = p.window; P.rotate = p.rotate; P.flags = p.flags; P.clear_max = p.clear_max;
    hipLaunchKernelGGL(k_ig_context_window, dim3((unsigned)e->cfg.n_worlds), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), e->D, e->G,
                       P, reinterpret_cast<const unsigned long long*>(observed), world_mask, context_window);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

int cagym_ig_credit(void* env, const cagym_ig_credit_params* params, const float* obs_oas, const uint8_t* restart_mask, double* gain,
                    uint64_t* robot_observed, double* credit, double* loo, double* reward, double* running, double* sum, double* last,
                    int32_t* episodes, void* stream) {
    ENTRY_IG(e, env, "cagym_ig_credit");
    if (!params || !obs_oas) return fail(e, CAGYM_E_INVALID, "cagym_ig_credit: null argument");
    const cagym_ig_credit_params& p = *params;
    const char* name = "cagym_ig_credit";
    if (int rc = ig_team_check(e, name, p.n_robots)) return rc;  // (R may exceed the pool's team: the rows past it are zero)
    if (int rc = ig_flags_check(e, name, p.flags, CAGYM_IG_EPISODE_FOLD | CAGYM_IG_OBSERVE_ONLY_RESTARTED)) return rc;
    if (int rc = ig_positive_check(e, name, {p.fov_rad, p.range, (double)p.detect_range}, "fov_rad, range and detect_range must be finite and positive"))
        return rc;
    ON_DEVICE(e);
    IgCreditParams P;
    P.R = p.n_robots; P.flags = p.flags; P.det_range = p.detect_range; P.fov = p.fov_rad; P.range = p.range;
    IgCreditOut O;
    O.gain = gain; O.robot_observed = reinterpret_cast<unsigned long long*>(robot_observed); O.credit = credit; O.loo = loo; O.reward = reward;
    O.running = running; O.sum = sum; O.last = last; O.episodes = episodes;
    hipLaunchKernelGGL(k_ig_credit, dim3((unsigned)e->cfg.n_worlds), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), e->D, e->G, P, obs_oas,
                       restart_mask, O);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

// ---- goal actions for the learner's robots (csrc/cagym_ig_geodesic.h) -----------------------------------------------------------------
// The checks of the three entries on their shared parameter block; `name`: the entry, for the message.
static int ig_goal_params_check(Env* e, const cagym_ig_goal_params* params, const char* name, IgGoalParams* P) {
    const std::string n(name);
    if (!params) return fail(e, CAGYM_E_INVALID, n + ": null argument");
    const cagym_ig_goal_params& p = *params;
    if (int rc = ig_frame_check(e, n, p.n_robots, p.window, p.rotate, p.flags, 0)) return rc;
    if (int rc = ig_positive_check(e, n, {p.radius, p.v_max, p.w_max, p.align_tol, p.goal_tol, p.dt},
                                   "radius, v_max, w_max, align_tol, goal_tol and dt must be finite and positive"))
        return rc;
    if (int rc = ig_robots_check(e, p.n_robots, name)) return rc;
    P->R = p.n_robots; P->G = p.window; P->rotate = p.rotate;
    P->radius = p.radius; P->v_max = p.v_max; P->w_max = p.w_max; P->align_tol = p.align_tol; P->goal_tol = p.goal_tol; P->dt = p.dt;
    return CAGYM_OK;
}

int cagym_ig_geodesic(void* env, const cagym_ig_goal_params* params, const uint8_t* mask, const double* goals_xy, const int32_t* goals_ab,
                      float* field, double* goal_xy, uint8_t* active, int32_t* sweeps, void* stream) {
    ENTRY_IG(e, env, "cagym_ig_geodesic");
    if (!field || !goal_xy || !active) return fail(e, CAGYM_E_INVALID, "cagym_ig_geodesic: null argument");
    if ((goals_xy != nullptr) == (goals_ab != nullptr))
        return fail(e, CAGYM_E_INVALID, "cagym_ig_geodesic: exactly one of goals_xy and goals_ab must be given");
    IgGoalParams P;
    if (int rc = ig_goal_params_check(e, params, "cagym_ig_geodesic", &P)) return rc;
    ON_DEVICE(e);
    hipLaunchKernelGGL(k_ig_geodesic, dim3((unsigned)(e->cfg.n_worlds * P.R)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), e->D, e->G,
                       P, mask, goals_xy, goals_ab, field, goal_xy, active, sweeps);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

int cagym_ig_goal_actions(void* env, const cagym_ig_goal_params* params, const float* field, const double* goal_xy,
                          const uint8_t* active, float* actions, uint8_t* choice, void* stream) {
    ENTRY_IG(e, env, "cagym_ig_goal_actions");
    if (!field || !goal_xy || !active || !actions) return fail(e, CAGYM_E_INVALID, "cagym_ig_goal_actions: null argument");
    if (reinterpret_cast<uintptr_t>(actions) & 7) return fail(e, CAGYM_E_INVALID, "cagym_ig_goal_actions: actions must be 8-byte aligned");
    IgGoalParams P;
    if (int rc = ig_goal_params_check(e, params, "cagym_ig_goal_actions", &P)) return rc;
    ON_DEVICE(e);
    hipLaunchKernelGGL(k_ig_goal_actions, dim3((unsigned)e->cfg.n_worlds), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), e->D, P, field,
                       goal_xy, active, actions, choice);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

int cagym_ig_goal_status(void* env, const cagym_ig_goal_params* params, const uint8_t* restart_mask, const float* field,
                         const double* goal_xy, uint8_t* active, float* goal_distance, uint8_t* goal_reached, void* stream) {
    ENTRY_IG(e, env, "cagym_ig_goal_status");
    if (!field || !goal_xy || !active || !goal_distance || !goal_reached)
        return fail(e, CAGYM_E_INVALID, "cagym_ig_goal_status: null argument");
    IgGoalParams P;
    if (int rc = ig_goal_params_check(e, params, "cagym_ig_goal_status", &P)) return rc;
    ON_DEVICE(e);
    hipLaunchKernelGGL(k_ig_goal_status, dim3((unsigned)e->cfg.n_worlds), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), e->D, P,
                       restart_mask, field, goal_xy, active, goal_distance, goal_reached);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

// ---- view gains and goal proposals (csrc/cagym_ig_viewpoints.h) -----------------------------------------------------------------------
// The checks of the two entries on their shared parameter block; `name`: the entry, for the message.
static int ig_view_params_check(Env* e, const cagym_ig_view_params* params, const char* name, IgViewParams* P) {
    const std::string n(name);
    if (!params) return fail(e, CAGYM_E_INVALID, n + ": null argument");
    const cagym_ig_view_params& p = *params;
    if (p.n_points < 0) return fail(e, CAGYM_E_INVALID, n + ": n_points must not be negative");
    if (int rc = ig_team_check(e, n, p.n_robots)) return rc;
    if (p.k < 1 || p.k > IGV_MAXK) return fail(e, CAGYM_E_INVALID, n + ": k must be 1..16");
    if (int rc = ig_flags_check(e, n, p.flags, 0)) return rc;
    if (int rc = ig_positive_check(e, n, {p.radius, p.range, p.min_sep, p.d0}, "radius, range, min_sep and d0 must be finite and positive")) return rc;
    P->P = p.n_points; P->R = p.n_robots; P->k = p.k;
    P->radius = p.radius; P->range = p.range; P->min_sep = p.min_sep; P->d0 = p.d0;
    return CAGYM_OK;
}

int cagym_ig_view_gain(void* env, const cagym_ig_view_params* params, const uint8_t* world_mask, const double* points_xy, double* gain,
                       int32_t* n_visible, uint8_t* valid, void* stream) {
    ENTRY_IG(e, env, "cagym_ig_view_gain");
    if (!gain || !n_visible || !valid) return fail(e, CAGYM_E_INVALID, "cagym_ig_view_gain: null argument");
    IgViewParams P;
    if (int rc = ig_view_params_check(e, params, "cagym_ig_view_gain", &P)) return rc;
    if (!points_xy) P.P = IGV_CELLS;  // the map: the kernel generates the cell centres
    long long blocks;
    if (int rc = igv_blocks(e, "cagym_ig_view_gain", P.P, &blocks)) return rc;
    ON_DEVICE(e);
    if (blocks == 0) return CAGYM_OK;
    hipLaunchKernelGGL(k_ig_view_gain, dim3((unsigned)blocks), dim3(IGV_THREADS), 0, reinterpret_cast<hipStream_t>(stream), e->G, P,
                       world_mask, points_xy, gain, n_visible, valid);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

int cagym_ig_propose_goals(void* env, const cagym_ig_view_params* params, const uint8_t* mask, const double* gain_map,
                           const uint8_t* valid_map, const float* field, int32_t* cells, double* xy, double* utility, double* gain,
                           float* distance, int32_t* n_found, void* stream) {
    ENTRY_IG(e, env, "cagym_ig_propose_goals");
    if (!gain_map || !valid_map || !field || !cells || !xy || !utility || !gain || !distance || !n_found)
        return fail(e, CAGYM_E_INVALID, "cagym_ig_propose_goals: null argument");
    IgViewParams P;
    if (int rc = ig_view_params_check(e, params, "cagym_ig_propose_goals", &P)) return rc;
    ON_DEVICE(e);
    hipLaunchKernelGGL(k_ig_propose_goals, dim3((unsigned)(e->cfg.n_worlds * P.R)), dim3(IGV_THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream), P, mask, gain_map, valid_map, field, cells, xy, utility, gain, distance,
                       n_found);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

// ---- heading-resolved view gains, goal headings and facing (csrc/cagym_ig_headings.h) -------------------------------------------------
int cagym_ig_view_gain_headings(void* env, const cagym_ig_heading_params* params, const uint8_t* world_mask, const double* points_xy,
                                double* gain_h, int32_t* n_visible_h, int32_t* best_heading, double* best_gain, uint8_t* valid,
                                void* stream) {
    ENTRY_IG(e, env, "cagym_ig_view_gain_headings");
    if (!params || !best_heading || !best_gain || !valid) return fail(e, CAGYM_E_INVALID, "cagym_ig_view_gain_headings: null argument");
    const cagym_ig_heading_params& p = *params;
    const char* name = "cagym_ig_view_gain_headings";
    if (p.n_points < 0) return fail(e, CAGYM_E_INVALID, "cagym_ig_view_gain_headings: n_points must not be negative");
    if (p.n_headings < 1 || p.n_headings > IGH_MAXH) return fail(e, CAGYM_E_INVALID, "cagym_ig_view_gain_headings: n_headings must be 1..16");
    if (int rc = ig_flags_check(e, name, p.flags, 0)) return rc;
    if (int rc = ig_positive_check(e, name, {p.radius, p.range, p.fov}, "radius, range and fov must be finite and positive")) return rc;
    IgHeadingParams P;
    P.P = points_xy ? p.n_points : IGV_CELLS;  // the map: the kernel generates the cell centres
    P.H = p.n_headings;
    P.radius = p.radius; P.range = p.range; P.fov = p.fov;
    for (int h = 0; h < IGH_MAXH; h++) {
        if (h < p.n_headings && !std::isfinite(p.headings[h]))
            return fail(e, CAGYM_E_INVALID, "cagym_ig_view_gain_headings: the first n_headings headings must be finite");
        P.headings[h] = h < p.n_headings ? p.headings[h] : 0.0;
    }
    long long blocks;
    if (int rc = igv_blocks(e, name, P.P, &blocks)) return rc;
    ON_DEVICE(e);
    if (blocks == 0) return CAGYM_OK;
    hipLaunchKernelGGL(k_ig_view_gain_headings, dim3((unsigned)blocks), dim3(IGV_THREADS), 0, reinterpret_cast<hipStream_t>(stream), e->G,
                       P, world_mask, points_xy, gain_h, n_visible_h, best_heading, best_gain, valid);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

// ---- team goal assignment (csrc/cagym_ig_assign.h) --------------------------------------------------------------------------------------
int cagym_ig_assign_goals(void* env, const cagym_ig_assign_params* params, const uint8_t* mask, const double* cand_xy,
                          const double* cand_heading, const float* cand_distance, const uint8_t* claim, const double* claim_xy,
                          const double* claim_heading, int32_t* choice, int32_t* order, double* marginal, double* utility,
                          uint64_t* claimed, uint64_t* masks, double* round_gain, void* stream) {
    ENTRY_IG(e, env, "cagym_ig_assign_goals");
    const char* name = "cagym_ig_assign_goals";
    if (!params || !cand_xy || !cand_distance || !choice || !order || !marginal || !utility || !claimed || !masks)
        return fail(e, CAGYM_E_INVALID, "cagym_ig_assign_goals: null argument");
    const cagym_ig_assign_params& p = *params;
    if (int rc = ig_team_check(e, name, p.n_robots)) return rc;
    if (p.k < 1 || p.k > IGV_MAXK) return fail(e, CAGYM_E_INVALID, "cagym_ig_assign_goals: k must be 1..16");
    if (p.mode != CAGYM_IG_ASSIGN_SLOT && p.mode != CAGYM_IG_ASSIGN_BEST)
        return fail(e, CAGYM_E_INVALID, "cagym_ig_assign_goals: mode must be 0 (slot order) or 1 (best first)");
    if (int rc = ig_flags_check(e, name, p.flags, 0)) return rc;
    if (int rc = ig_positive_check(e, name, {p.radius, p.range, p.d0, p.fov}, "radius, range, d0 and fov must be finite and positive")) return rc;
    if (claim && !claim_xy) return fail(e, CAGYM_E_INVALID, "cagym_ig_assign_goals: claim needs claim_xy");
    IgAssignParams P;
    P.R = p.n_robots; P.k = p.k; P.mode = p.mode;
    P.radius = p.radius; P.range = p.range; P.fov = p.fov; P.d0 = p.d0;
    ON_DEVICE(e);
    hipLaunchKernelGGL(k_ig_assign_goals, dim3((unsigned)e->cfg.n_worlds), dim3(IGV_THREADS), 0, reinterpret_cast<hipStream_t>(stream), e->G,
                       P, mask, cand_xy, cand_heading, cand_distance, claim, claim_xy, claim_heading, choice, order, marginal, utility,
                       reinterpret_cast<unsigned long long*>(claimed), reinterpret_cast<unsigned long long*>(masks), round_gain);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

// ---- route gains (csrc/cagym_ig_route.h) ------------------------------------------------------------------------------------------------
int cagym_ig_route_gains(void* env, const cagym_ig_route_params* params, const uint8_t* mask, const float* field,
                         const int32_t* cand_cells, const double* cand_heading, const uint64_t* exclude, uint64_t* route_masks,
                         uint64_t* total_masks, double* route_gain, double* total_gain, double* utility, int32_t* n_path,
                         int32_t* n_way, uint8_t* truncated, int32_t* best, int32_t* way_cells, int8_t* way_dir, void* stream) {
    ENTRY_IG(e, env, "cagym_ig_route_gains");
    const char* name = "cagym_ig_route_gains";
    if (!params || !field || !cand_cells || !route_masks || !total_masks || !route_gain || !total_gain || !utility || !n_path || !n_way ||
        !truncated || !best)
        return fail(e, CAGYM_E_INVALID, "cagym_ig_route_gains: null argument");
    const cagym_ig_route_params& p = *params;
    if (int rc = ig_team_check(e, name, p.n_robots)) return rc;
    if (p.k < 1 || p.k > IGV_MAXK) return fail(e, CAGYM_E_INVALID, "cagym_ig_route_gains: k must be 1..16");
    if (p.stride < 1) return fail(e, CAGYM_E_INVALID, "cagym_ig_route_gains: stride must be at least 1");
    if (int rc = ig_flags_check(e, name, p.flags, 0)) return rc;
    if (int rc = ig_positive_check(e, name, {p.radius, p.range, p.fov, p.d0}, "radius, range, fov and d0 must be finite and positive")) return rc;
    IgRouteParams P;
    P.R = p.n_robots; P.k = p.k;
    P.stride = std::min(p.stride, IGR_WALK_CAP + 1);  // (no path has more moves: the same way-points, and no product near INT_MAX)
    P.radius = p.radius; P.range = p.range; P.fov = p.fov; P.d0 = p.d0;
    IgRouteOut O;
    O.route_masks = reinterpret_cast<unsigned long long*>(route_masks);
    O.total_masks = reinterpret_cast<unsigned long long*>(total_masks);
    O.route_gain = route_gain; O.total_gain = total_gain; O.utility = utility;
    O.n_path = n_path; O.n_way = n_way; O.truncated = truncated; O.best = best;
    O.way_cells = way_cells; O.way_dir = way_dir;
    ON_DEVICE(e);
    hipLaunchKernelGGL(k_ig_route_gains, dim3((unsigned)e->cfg.n_worlds), dim3(IGV_THREADS), 0, reinterpret_cast<hipStream_t>(stream), e->G,
                       P, mask, field, cand_cells, cand_heading, reinterpret_cast<const unsigned long long*>(exclude), O);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

int cagym_ig_goal_face_actions(void* env, const cagym_ig_goal_params* params, const double* goal_xy, const uint8_t* active,
                               const double* goal_heading, float* actions, void* stream) {
    ENTRY_IG(e, env, "cagym_ig_goal_face_actions");
    if (!goal_xy || !active || !goal_heading || !actions) return fail(e, CAGYM_E_INVALID, "cagym_ig_goal_face_actions: null argument");
    if (reinterpret_cast<uintptr_t>(actions) & 7)
        return fail(e, CAGYM_E_INVALID, "cagym_ig_goal_face_actions: actions must be 8-byte aligned");
    IgGoalParams P;
    if (int rc = ig_goal_params_check(e, params, "cagym_ig_goal_face_actions", &P)) return rc;
    ON_DEVICE(e);
    hipLaunchKernelGGL(k_ig_goal_face_actions, dim3((unsigned)e->cfg.n_worlds), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), e->D, P,
                       goal_xy, active, goal_heading, actions);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

int cagym_ig_goal_face_status(void* env, const cagym_ig_goal_params* params, double face_tol, const double* goal_xy,
                              const uint8_t* active, const double* goal_heading, uint8_t* goal_facing, void* stream) {
    ENTRY_IG(e, env, "cagym_ig_goal_face_status");
    if (!goal_xy || !active || !goal_heading || !goal_facing) return fail(e, CAGYM_E_INVALID, "cagym_ig_goal_face_status: null argument");
    if (int rc = ig_positive_check(e, "cagym_ig_goal_face_status", {face_tol}, "face_tol must be finite and positive")) return rc;
    IgGoalParams P;
    if (int rc = ig_goal_params_check(e, params, "cagym_ig_goal_face_status", &P)) return rc;
    ON_DEVICE(e);
    hipLaunchKernelGGL(k_ig_goal_face_status, dim3((unsigned)e->cfg.n_worlds), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), e->D, P,
                       face_tol, goal_xy, active, goal_heading, goal_facing);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

// ---- per-scenario episode records (csrc/cagym_episode_records.h) --------------------------------------------------------------------
int cagym_episode_records_init(void* env, int keep, void* stream) {
    ENTRY_POOL(e, env, "cagym_episode_records_init");
    if (e->streaming)
        return fail(e, CAGYM_E_STATE, "cagym_episode_records_init on a streaming handle: the table has one row per pool slot, which a streamed pool reuses");
    if (keep != CAGYM_EPREC_KEEP_FIRST && keep != CAGYM_EPREC_KEEP_LAST) return fail(e, CAGYM_E_INVALID, "cagym_episode_records_init: unknown keep mode");
    ON_DEVICE(e);
    if (!e->rec.t) {
        const size_t N = e->cfg.n_worlds, M = e->cfg.max_agents, S = e->cfg.n_scenarios;
        EpRec R{};
#define A(call) if (int rc = (call)) return rc;
        A(dalloc(e, &R.extra_t, S * M)); A(dalloc(e, &R.flags, S * M)); A(dalloc(e, &R.ret, S)); A(dalloc(e, &R.steps, S));
        A(dalloc(e, &R.outcome, S)); A(dalloc(e, &R.count, S)); A(dalloc(e, &R.claim, S));
        A(dalloc(e, &R.run.t_run, N * M)); A(dalloc(e, &R.run.ret_run, N)); A(dalloc(e, &R.run.steps_run, N)); A(dalloc(e, &R.run.atgoal_run, N));
        A(dalloc(e, &R.run.cursor, N)); A(dalloc(e, &R.run.desync, 1)); A(dalloc(e, &R.seq, 1));
        A(dalloc(e, &R.t, S * M));  // last: the handle holds the records only when every allocation succeeded
#undef A
        e->rec = R;
    }
    e->rec.keep = keep;
    e->rec_ready = true;
    return eprec_restart(e, nullptr, true, reinterpret_cast<hipStream_t>(stream));
}

int cagym_episode_records_update(void* env, const uint8_t* flags, const float* reward, const uint8_t* game_over, int T, void* stream) {
    ENTRY_POOL(e, env, "cagym_episode_records_update");
    REQUIRE(e, e->rec_ready, "cagym_episode_records_update", "cagym_episode_records_init");
    if (!flags || !reward || !game_over) return fail(e, CAGYM_E_INVALID, "cagym_episode_records_update: flags, reward and game_over are required");
    if (T < 1) return fail(e, CAGYM_E_INVALID, "cagym_episode_records_update: T must be >= 1");
    ON_DEVICE(e);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (e->cfg.n_scenarios % e->cfg.n_worlds == 0) {  // s % N == w: one writer per row
        const int waves_per_wg = EPREC_NT / CAGYM_WAVE;
        hipLaunchKernelGGL(k_episode_records_update, dim3((unsigned)((n_waves(e) + waves_per_wg - 1) / waves_per_wg)), dim3(EPREC_NT), 0, st,
                           e->D, e->rec, flags, reward, game_over, T);
    } else {
        hipLaunchKernelGGL(k_episode_records_update_shared, dim3(1), dim3(EPREC_NT_SHARED), 0, st, e->D, e->rec, flags, reward, game_over, T);
    }
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

int cagym_episode_records_restart(void* env, const uint8_t* world_mask, int clear_table, void* stream) {
    ENTRY_POOL(e, env, "cagym_episode_records_restart");
    REQUIRE(e, e->rec_ready, "cagym_episode_records_restart", "cagym_episode_records_init");
    ON_DEVICE(e);
    return eprec_restart(e, world_mask, clear_table != 0, reinterpret_cast<hipStream_t>(stream));
}

int cagym_episode_records_get(void* env, cagym_episode_record_ptrs* out) {
    ENTRY_POOL(e, env, "cagym_episode_records_get");
    REQUIRE(e, e->rec_ready, "cagym_episode_records_get", "cagym_episode_records_init");
    if (!out) return fail(e, CAGYM_E_INVALID, "null out");
    const EpRec& R = e->rec;
    out->t = R.t; out->extra_t = R.extra_t; out->flags = R.flags; out->ret = R.ret; out->steps = R.steps; out->outcome = R.outcome;
    out->count = R.count; out->t_run = R.run.t_run; out->ret_run = R.run.ret_run; out->steps_run = R.run.steps_run;
    out->atgoal_run = R.run.atgoal_run; out->cursor = R.run.cursor; out->desync = R.run.desync;
    return CAGYM_OK;
}

// ---- append-only episode log (csrc/cagym_episode_log.h) -------------------------------------------------------------------------------
int cagym_episode_log_init(void* env, int capacity, void* stream) {
    ENTRY_POOL(e, env, "cagym_episode_log_init");
    if (capacity < 1) return fail(e, CAGYM_E_INVALID, "cagym_episode_log_init: capacity must be >= 1");
    ON_DEVICE(e);
    if (int rc = eplog_alloc(e, capacity)) return rc;
    e->log_ready = true;
    return eplog_restart(e, nullptr, true, reinterpret_cast<hipStream_t>(stream));
}

int cagym_episode_log_update(void* env, const uint8_t* flags, const float* reward, const uint8_t* game_over, int T, void* stream) {
    ENTRY_POOL(e, env, "cagym_episode_log_update");
    REQUIRE(e, e->log_ready, "cagym_episode_log_update", "cagym_episode_log_init");
    if (!flags || !reward || !game_over) return fail(e, CAGYM_E_INVALID, "cagym_episode_log_update: flags, reward and game_over are required");
    if (T < 1) return fail(e, CAGYM_E_INVALID, "cagym_episode_log_update: T must be >= 1");
    ON_DEVICE(e);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int N = e->cfg.n_worlds, waves_per_wg = EPREC_NT / CAGYM_WAVE;
    if (T > 1)  // (a one-slice update's counts are its game_over bytes: the scan reads them)
        hipLaunchKernelGGL(k_episode_log_count, dim3((unsigned)((N + CAGYM_WAVE - 1) / CAGYM_WAVE)), dim3(CAGYM_WAVE * EPLOG_CNT_WAVES), 0, st, e->elog, N,
                           game_over, T);
    hipLaunchKernelGGL(k_episode_log_scan, dim3(1), dim3(EPLOG_NT_SCAN), 0, st, e->elog, N, T, T > 1 ? nullptr : game_over);
    EpLog G = e->elog;
    G.slot_key = e->replay_on ? e->replay.slot_key : nullptr;  // armed: the key column names the scenario that ran
    hipLaunchKernelGGL(k_episode_log_write, dim3((unsigned)((n_waves(e) + waves_per_wg - 1) / waves_per_wg)), dim3(EPREC_NT), 0, st, e->D, G,
                       flags, reward, game_over, T);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

int cagym_episode_log_restart(void* env, const uint8_t* world_mask, int clear_rows, void* stream) {
    ENTRY_POOL(e, env, "cagym_episode_log_restart");
    REQUIRE(e, e->log_ready, "cagym_episode_log_restart", "cagym_episode_log_init");
    ON_DEVICE(e);
    return eplog_restart(e, world_mask, clear_rows != 0, reinterpret_cast<hipStream_t>(stream));
}

int cagym_episode_log_get(void* env, cagym_episode_log_ptrs* out) {
    ENTRY_POOL(e, env, "cagym_episode_log_get");
    REQUIRE(e, e->log_ready, "cagym_episode_log_get", "cagym_episode_log_init");
    if (!out) return fail(e, CAGYM_E_INVALID, "null out");
    const EpLog& G = e->elog;
    out->key = G.key; out->world = G.world; out->episode = G.episode; out->slice = reinterpret_cast<const int64_t*>(G.slice); out->steps = G.steps;
    out->ret = G.ret; out->outcome = G.outcome; out->n_agents = G.n_agents; out->n_obst = G.n_obst; out->t = G.t; out->extra_t = G.extra_t;
    const EpRunning& Q = G.run;
    out->flags = G.flags; out->t_run = Q.t_run; out->ret_run = Q.ret_run; out->steps_run = Q.steps_run; out->atgoal_run = Q.atgoal_run;
    out->cursor = Q.cursor; out->head = reinterpret_cast<const uint64_t*>(G.head); out->desync = Q.desync; out->capacity = G.capacity;
    return CAGYM_OK;
}

// ---- the IG team's episode log (csrc/cagym_ig_episode_log.h) --------------------------------------------------------------------------
int cagym_ig_episode_log_init(void* env, int capacity, double odds_found, void* stream) {
    ENTRY_IG(e, env, "cagym_ig_episode_log_init");
    if (capacity < 1) return fail(e, CAGYM_E_INVALID, "cagym_ig_episode_log_init: capacity must be >= 1");
    if (!(odds_found > 0.0) || !std::isfinite(odds_found))  // (the negated comparison refuses NaN)
        return fail(e, CAGYM_E_INVALID, "cagym_ig_episode_log_init: odds_found must be finite and positive");
    ON_DEVICE(e);
    if (int rc = iglog_alloc(e, capacity)) return rc;
    e->iglog.odds_found = odds_found;
    e->iglog_ready = true;
    return iglog_restart(e, nullptr, true, reinterpret_cast<hipStream_t>(stream));
}

int cagym_ig_episode_log_update(void* env, const uint8_t* game_over, const double* team_reward, void* stream) {
    ENTRY_IG(e, env, "cagym_ig_episode_log_update");
    REQUIRE(e, e->iglog_ready, "cagym_ig_episode_log_update", "cagym_ig_episode_log_init");
    if (!game_over) return fail(e, CAGYM_E_INVALID, "cagym_ig_episode_log_update: game_over is required");
    ON_DEVICE(e);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int N = e->cfg.n_worlds;
    hipLaunchKernelGGL(k_ig_episode_log_scan, dim3(1), dim3(IGLOG_NT_SCAN), 0, st, e->iglog, N, e->D.episode, game_over);
    hipLaunchKernelGGL(k_ig_episode_log_update, dim3((unsigned)N), dim3(IGLOG_NT), 0, st, e->D, e->G, e->ig_ep, e->iglog, team_reward);
    HIPCHK(e, hipGetLastError());
    return CAGYM_OK;
}

int cagym_ig_episode_log_restart(void* env, const uint8_t* world_mask, int clear_rows, void* stream) {
    ENTRY_IG(e, env, "cagym_ig_episode_log_restart");
    REQUIRE(e, e->iglog_ready, "cagym_ig_episode_log_restart", "cagym_ig_episode_log_init");
    ON_DEVICE(e);
    return iglog_restart(e, world_mask, clear_rows != 0, reinterpret_cast<hipStream_t>(stream));
}

int cagym_ig_episode_log_get(void* env, cagym_ig_episode_log_ptrs* out) {
    ENTRY_IG(e, env, "cagym_ig_episode_log_get");
    REQUIRE(e, e->iglog_ready, "cagym_ig_episode_log_get", "cagym_ig_episode_log_init");
    if (!out) return fail(e, CAGYM_E_INVALID, "null out");
    const IgEpLog& G = e->iglog;
    out->key = G.key; out->world = G.world; out->episode = G.episode; out->slice = reinterpret_cast<const int64_t*>(G.slice); out->steps = G.steps;
    out->ret = G.ret; out->n_targets = G.n_targets; out->n_found = G.n_found; out->found_at = G.found_at; out->entropy = G.entropy;
    out->residual_mi = G.residual_mi; out->n_touched = G.n_touched; out->steps_run = G.steps_run; out->found_run = G.found_run;
    out->cursor = G.cursor; out->head = reinterpret_cast<const uint64_t*>(G.head); out->desync = G.desync; out->capacity = G.capacity;
    return CAGYM_OK;
}

// ---- per-world snapshot, restore and fork (csrc/cagym_snapshot.h) -------------------------------------------------------------------
int cagym_snapshot_layout_of(void* env, cagym_snapshot_layout* out) {
    ENTRY(e, env);
    if (!out) return fail(e, CAGYM_E_INVALID, "null out");
    *out = snap_layout(e);
    return CAGYM_OK;
}

// the argument checks the three calls share
static int snap_check_blob(Env* e, const char* what, const void* blob, int n) {
    if (n < 0 || n > e->cfg.n_worlds) return fail(e, CAGYM_E_INVALID, std::string(what) + ": n must be in [0, n_worlds]");
    if (!blob || (reinterpret_cast<uintptr_t>(blob) & 15)) return fail(e, CAGYM_E_INVALID, std::string(what) + ": the blob must be a 16-byte aligned device buffer");
    return CAGYM_OK;
}

// cagym_restore and cagym_fork move worlds onto another timeline: what cannot follow them there
static int refuse_other_timeline(Env* e, const char* what) {
    const std::string w(what);
    if (e->streaming) return fail(e, CAGYM_E_UNSUPPORTED, w + " on a streaming handle: the ring of scenario slots is not part of a snapshot");
    if (e->rec_ready)
        return fail(e, CAGYM_E_STATE, w + " with episode records initialised: their running rows would describe another timeline; detach the records first");
    if (e->log_ready) return fail(e, CAGYM_E_STATE, w + " with an episode log initialised: its running rows would describe another timeline");
    if (e->traj_ready) return fail(e, CAGYM_E_STATE, w + " with a trajectory ring initialised: its running values would describe another timeline");
    return CAGYM_OK;
}
// ... and, behind every refusal the two calls made before it existed, the IG team's episode log
static int refuse_iglog_timeline(Env* e, const char* what) {
    if (e->iglog_ready)
        return fail(e, CAGYM_E_STATE, std::string(what) + " with an IG episode log initialised: its running values would describe another timeline");
    return CAGYM_OK;
}

int cagym_snapshot(void* env, const int32_t* worlds, int n, void* blob, void* stream) {
    ENTRY_POOL(e, env, "cagym_snapshot");
    if (int rc = snap_check_blob(e, "cagym_snapshot", blob, n)) return rc;
    if (!worlds && n != e->cfg.n_worlds) return fail(e, CAGYM_E_INVALID, "cagym_snapshot: NULL worlds means every world, n must be n_worlds");
    ON_DEVICE(e);  // a pending cagym_step_begin stays valid: nothing moves
    return snap_launch(e, snap_state_table(e, SNAP_GATHER), worlds, nullptr, blob, n, reinterpret_cast<hipStream_t>(stream));
}

int cagym_restore(void* env, const cagym_snapshot_layout* layout, const void* blob, const int32_t* rows, int n, void* stream) {
    ENTRY_POOL(e, env, "cagym_restore");
    if (int rc = snap_check_blob(e, "cagym_restore", blob, n)) return rc;
    if (!layout) return fail(e, CAGYM_E_INVALID, "cagym_restore: null layout");
    const cagym_snapshot_layout own = snap_layout(e);
    if (layout->magic != own.magic || layout->version != own.version || layout->n_worlds != own.n_worlds || layout->max_agents != own.max_agents ||
        layout->n_scenarios != own.n_scenarios || layout->max_obstacles != own.max_obstacles || layout->fields != own.fields ||
        layout->reserved != own.reserved || layout->row_bytes != own.row_bytes)
        return fail(e, CAGYM_E_INVALID, "cagym_restore: the blob's layout is not this handle's (n_worlds, max_agents, n_scenarios, max_obstacles, "
                                        "cagym_ig_init done or not, magic and version must all match)");
    if (int rc = refuse_other_timeline(e, "cagym_restore")) return rc;
    if (int rc = refuse_iglog_timeline(e, "cagym_restore")) return rc;
    ON_DEVICE_VOIDS_BEGUN(e);
    return snap_launch(e, snap_state_table(e, SNAP_SCATTER), rows, nullptr, const_cast<void*>(blob), n, reinterpret_cast<hipStream_t>(stream));
}

int cagym_fork(void* env, const int32_t* src, const int32_t* dst, int n, void* stream) {
    ENTRY_POOL(e, env, "cagym_fork");
    if (n < 0 || n > e->cfg.n_worlds) return fail(e, CAGYM_E_INVALID, "cagym_fork: n must be in [0, n_worlds]");
    if (n > 0 && (!src || !dst)) return fail(e, CAGYM_E_INVALID, "cagym_fork: null src / dst");
    if (int rc = refuse_other_timeline(e, "cagym_fork")) return rc;
    if (e->cfg.n_scenarios % e->cfg.n_worlds != 0)
        return fail(e, CAGYM_E_UNSUPPORTED, "cagym_fork needs n_scenarios to be a multiple of n_worlds: otherwise two worlds can share a scenario "
                                            "slot and the copy of src's slot over dst's could hit a third world");
    // (in front of the refusal after cagym_ig_init, which every handle that holds this log would meet: CAGYM_E_STATE names the log)
    if (int rc = refuse_iglog_timeline(e, "cagym_fork")) return rc;
    if (e->ig_ready) return fail(e, CAGYM_E_UNSUPPORTED, "cagym_fork after cagym_ig_init: the per-slot distance field is not copied");
    ON_DEVICE_VOIDS_BEGUN(e);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (int rc = snap_launch(e, snap_state_table(e, SNAP_FORK, true), src, dst, nullptr, n, st)) return rc;
    return snap_launch(e, snap_pool_table(e), src, dst, nullptr, n, st);
}

// ---- whole-handle checkpoint (csrc/cagym_checkpoint.h) -----------------------------------------------------------------------------------
int cagym_checkpoint_sizes(void* env, uint64_t* sizes) {
    ENTRY_POOL(e, env, "cagym_checkpoint_sizes");
    if (int rc = ckpt_refuse(e, "cagym_checkpoint_sizes")) return rc;
    if (!sizes) return fail(e, CAGYM_E_INVALID, "cagym_checkpoint_sizes: null sizes");
    ckpt_sizes(e, sizes);
    return CAGYM_OK;
}

// the buffer checks save and load share; sizes: what the buffers must hold
static int ckpt_check_buffers(Env* e, const char* what, const void* host_words, uint64_t host_bytes, const void* blob, uint64_t blob_bytes,
                              const uint64_t* sizes) {
    const std::string w(what);
    if (!host_words || host_bytes < sizes[CAGYM_CKPT_HOST]) return fail(e, CAGYM_E_INVALID, w + ": host_words is NULL or shorter than the host header");
    if (!blob || (reinterpret_cast<uintptr_t>(blob) & 15)) return fail(e, CAGYM_E_INVALID, w + ": the blob must be a 16-byte aligned device buffer");
    if (blob_bytes < ckpt_blob_bytes(sizes)) return fail(e, CAGYM_E_INVALID, w + ": blob_bytes is smaller than the sum of the device sections");
    return CAGYM_OK;
}

int cagym_checkpoint_save(void* env, void* host_words, uint64_t host_bytes, void* blob, uint64_t blob_bytes, void* stream) {
    ENTRY_POOL(e, env, "cagym_checkpoint_save");
    if (int rc = ckpt_refuse(e, "cagym_checkpoint_save")) return rc;
    CkptHost H{};
    ckpt_sizes(e, H.sizes);
    if (int rc = ckpt_check_buffers(e, "cagym_checkpoint_save", host_words, host_bytes, blob, blob_bytes, H.sizes)) return rc;
    ON_DEVICE(e);  // a pending cagym_step_begin stays valid: nothing moves
    const cagym_config& c = e->cfg;
    H.magic = CAGYM_CKPT_MAGIC; H.version = CAGYM_CKPT_VERSION;
    H.n_worlds = c.n_worlds; H.max_agents = c.max_agents; H.n_scenarios = c.n_scenarios; H.max_obstacles = c.max_obstacles;
    H.game_over_mode = c.game_over_mode; H.collide_with_static = c.collide_with_static; H.laserscan = c.laserscan;
    H.rvo_max_neighbors = c.rvo_max_neighbors; H.dt = c.dt; H.cfg_reserved = c.reserved;
    H.scenarios_set = 1; H.heading0_set = e->D.sc_heading0 ? 1 : 0; H.any_rvo = e->any_rvo; H.obst_rvo = e->obst_rvo; H.n_ig = e->n_ig;
    H.streaming = e->streaming ? 1 : 0; H.stream_gen = e->stream_gen;
    if (e->streaming) H.stream_P = e->stream_P;
    H.log_ready = e->log_ready ? 1 : 0; H.log_capacity = e->log_ready ? e->elog.capacity : 0;
    H.replay_on = e->replay_on ? 1 : 0; H.replay_capacity = e->replay_on ? e->replay.Q : 0;
    if (e->replay_on) {
        H.replay_mask = e->replay_mask; H.replay_p = e->replay_p; H.replay_seed = e->replay_seed;
    }
    if (int rc = ckpt_copy(e, true, reinterpret_cast<unsigned char*>(blob), e->streaming, H.log_capacity, H.replay_capacity, reinterpret_cast<hipStream_t>(stream)))
        return rc;
    memcpy(host_words, &H, sizeof(H));
    return CAGYM_OK;
}

int cagym_checkpoint_load(void* env, const void* host_words, uint64_t host_bytes, const void* blob, uint64_t blob_bytes, void* stream) {
    ENTRY(e, env);
    if (int rc = ckpt_refuse(e, "cagym_checkpoint_load")) return rc;
    const char* const bad = "cagym_checkpoint_load: ";
    if (!host_words || host_bytes < sizeof(CkptHost)) return fail(e, CAGYM_E_INVALID, std::string(bad) + "host_words is NULL or shorter than the host header");
    CkptHost H;
    memcpy(&H, host_words, sizeof(H));
    if (H.magic != CAGYM_CKPT_MAGIC || H.version != CAGYM_CKPT_VERSION) return fail(e, CAGYM_E_INVALID, std::string(bad) + "not a checkpoint header of this version (magic, version)");
    const cagym_config& c = e->cfg;
    if (H.n_worlds != c.n_worlds || H.max_agents != c.max_agents || H.n_scenarios != c.n_scenarios || H.max_obstacles != c.max_obstacles ||
        H.game_over_mode != c.game_over_mode || H.collide_with_static != c.collide_with_static || H.laserscan != c.laserscan ||
        H.rvo_max_neighbors != c.rvo_max_neighbors || memcmp(&H.dt, &c.dt, sizeof(double)) != 0 || H.cfg_reserved != c.reserved)
        return fail(e, CAGYM_E_INVALID, std::string(bad) + "the checkpoint's configuration is not this handle's (every cagym_config field except device must match)");
    // the members, as the calls that set them check them
    const int K = c.max_obstacles;
    auto flag = [](int32_t v) { return v == 0 || v == 1; };
    const bool flags01 = H.scenarios_set == 1 && flag(H.heading0_set) && flag(H.any_rvo) && flag(H.obst_rvo) && flag(H.streaming) &&
                         flag(H.log_ready) && flag(H.replay_on) && H.reserved == 0;
    if (!flags01 || H.n_ig < N_IG_RANDOM || H.n_ig > c.max_agents || (H.obst_rvo && !(H.any_rvo && K > 0)))
        return fail(e, CAGYM_E_INVALID, std::string(bad) + "the header's pool flags are not ones a pool setter leaves");
    if ((H.log_ready != 0) != (H.log_capacity >= 1) || H.log_capacity < 0 || (H.replay_on != 0) != (H.replay_capacity >= 1) || H.replay_capacity < 0 ||
        (H.replay_on && !H.streaming) || (H.replay_on && (!(H.replay_p >= 0.0 && H.replay_p <= 1.0) || (H.replay_mask & ~7u))) || H.stream_gen < 1)
        return fail(e, CAGYM_E_INVALID, std::string(bad) + "the header's stream, log or replay members contradict each other");
    if (H.obst_rvo && check_obst_rvo_capacity(e) != CAGYM_OK) return fail(e, CAGYM_E_INVALID, std::string(bad) + e->err);
    if (H.streaming) {
        Gen2Flags F;
        if (stream_check(e, "cagym_checkpoint_load", &H.stream_P, F) != CAGYM_OK)
            return fail(e, CAGYM_E_INVALID, std::string(bad) + "the stream's parameter set is refused: " + e->err);
        if ((F.any_rvo && !H.any_rvo) || (F.obst_rvo && !H.obst_rvo))
            return fail(e, CAGYM_E_INVALID, std::string(bad) + "the header's RVO flags do not cover the stream's parameter set");
    }
    uint64_t sizes[CAGYM_CKPT_SECTIONS];
    ckpt_sizes(e, H.streaming != 0, H.log_capacity, H.replay_capacity, sizes);
    if (memcmp(sizes, H.sizes, sizeof(sizes)) != 0)
        return fail(e, CAGYM_E_INVALID, std::string(bad) + "the header's section sizes are not those of its own configuration and capacities");
    if (int rc = ckpt_check_buffers(e, "cagym_checkpoint_load", host_words, host_bytes, blob, blob_bytes, sizes)) return rc;
    ON_DEVICE(e);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // every allocation before the first member changes
    if (H.streaming)
        if (int rc = stream_alloc(e)) return rc;
    if (H.log_ready)
        if (int rc = eplog_alloc(e, H.log_capacity)) return rc;
    if (H.replay_on)
        if (int rc = replay_alloc(e, H.replay_capacity)) return rc;
    e->begun = false;
    if (e->log_ready && !H.log_ready)  // a log the checkpoint lacks: emptied, and it stays initialised
        if (int rc = eplog_restart(e, nullptr, true, st)) return rc;
    e->log_ready = e->log_ready || H.log_ready;
    e->scenarios_set = true;
    e->D.sc_heading0 = H.heading0_set ? e->sc_heading_buf : nullptr;
    e->any_rvo = H.any_rvo; e->obst_rvo = H.obst_rvo; e->n_ig = H.n_ig;
    e->D.ko = H.obst_rvo ? 2 * K : 0;
    e->streaming = H.streaming != 0; e->explore_stream = false;
    if (H.streaming) e->stream_P = H.stream_P;
    e->stream_gen = H.stream_gen;
    e->replay_on = H.replay_on != 0;
    if (H.replay_on) {
        e->replay_p = H.replay_p; e->replay_mask = H.replay_mask; e->replay_seed = H.replay_seed;
    }
    if (int rc = ckpt_copy(e, false, reinterpret_cast<unsigned char*>(const_cast<void*>(blob)), H.streaming != 0, H.log_capacity, H.replay_capacity, st))
        return rc;
    return rasterize_pool(e, st);  // a pure function of the rectangles the pool rows brought
}

}  // extern "C"
