// cw_engine.cpp -- host side of the C ABI in include/craftingworld.h: engine lifetime, device
// buffers, MT19937 state conversion, dense<->slot state conversion, kernel launches.
// No CPU fallback exists: every compute entry point enqueues HIP kernels (cw_kernels.hip).
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <algorithm>
#include <vector>

#include "../../include/craftingworld.h"
#include "cw_layout.h"
#include "cw_host.h"

extern "C" {
hipError_t cwk_launch_step(const CwParams *P, const CwTuning *T, const void *actions, int act_dtype, int obs_mode, int auto_reset, hipStream_t st,
                           hipEvent_t *ev);
hipError_t cwk_launch_refill(const CwParams *P, const CwTuning *T, int all_envs, hipStream_t st);
hipError_t cwk_launch_reset_all(const CwParams *P, const CwTuning *T, int obs_mode, hipStream_t st);
hipError_t cwk_launch_reset_masked(const CwParams *P, const CwTuning *T, const uint8_t *mask, int obs_mode, hipStream_t st);
hipError_t cwk_launch_imagine_masked(const CwParams *P, const CwTuning *T, const uint8_t *mask, const uint16_t *desired, int commit, int obs_mode,
                                     uint8_t *out_frames, uint8_t *out_onehot, hipStream_t st);
hipError_t cwk_launch_sample_state_masked(const CwParams *P, const CwTuning *T, const uint8_t *mask, int pooled, uint16_t *out_cells, hipStream_t st);
hipError_t cwk_launch_snapshot_save(const CwParams *P, const CwTuning *T, const CwBank *B, const int32_t *rows, hipStream_t st);
hipError_t cwk_launch_snapshot_load(const CwParams *P, const CwTuning *T, const CwBank *B, const int32_t *rows, int with_stream, int obs_mode, hipStream_t st);
hipError_t cwk_launch_load_records(const CwParams *P, const CwTuning *T, const int32_t *src, const uint4 *hdr, const uint4 *pos, int n_records, uint8_t *status,
                                   int obs_mode, hipStream_t st);
hipError_t cwk_launch_expand(const CwParams *P, const int32_t *env_of, const uint4 *hdr_in, const uint4 *pos_in, int n_states, const CwExpandOut *O, hipStream_t st);
hipError_t cwk_launch_export_onehot_states(const CwParams *P, const CwTuning *T, const uint4 *hdr, const uint4 *pos, int n_states, uint8_t *out, hipStream_t st);
hipError_t cwk_launch_render_records(const CwParams *P, const CwTuning *T, const uint4 *hdr, const uint4 *pos, const uint8_t *mask, int n_states, uint8_t *out,
                                     hipStream_t st);
hipError_t cwk_launch_pool(const CwParams *P, const CwTuning *T, hipStream_t st);
hipError_t cwk_launch_seed(const CwParams *P, const uint32_t *seeds_dev, hipStream_t st);
hipError_t cwk_launch_resident(const CwParams *P, CwResident *R, uint32_t seq0, int paint_dirty, unsigned long long idle_ticks,
                               unsigned long long life_ticks, hipStream_t st);
hipError_t cwk_launch_render_onehot(const CwParams *P, const uint8_t *onehot, int n_states, uint16_t *out, hipStream_t st);
hipError_t cwk_launch_render_restore(const CwParams *P, const CwTuning *T, hipStream_t st);
hipError_t cwk_launch_plan(const CwParams *P, const int32_t *env_of, const uint4 *hdr_in, const uint4 *pos_in, int n_states, int depth, const CwPlanOut *O,
                           hipStream_t st);
hipError_t cwk_launch_shoot(const CwParams *P, const int32_t *env_of, const uint4 *hdr_in, const uint4 *pos_in, int n_states, int n_steps, int n_samples,
                            unsigned long long seed, const unsigned long long *seed_dev, const uint16_t *weights, const CwShootOut *O, hipStream_t st);
hipError_t cwk_launch_shoot_actions(int n_states, int n_steps, int n_rows, unsigned long long seed, const unsigned long long *seed_dev,
                                    const uint16_t *weights, const int32_t *samples, uint8_t *out, hipStream_t st);
hipError_t cwk_launch_refit(const CwParams *P, const CwTuning *T, const int32_t *env_of, int n_states, int n_steps, int n_samples, int n_elites,
                            unsigned long long seed, const unsigned long long *seed_dev, const uint16_t *weights_in, const int32_t *ret, uint32_t smooth,
                            uint32_t gain, int32_t *elites, uint16_t *weights, int32_t *elite_min, hipStream_t st);
hipError_t cwk_launch_replay_push(const CwParams *P, const CwReplay *R, const void *actions, int act_dtype, hipStream_t st);
hipError_t cwk_launch_replay_clear(const CwParams *P, const CwTuning *T, const CwReplay *R, hipStream_t st);
hipError_t cwk_launch_replay_sample(const CwParams *P, const CwTuning *T, const CwReplay *R, int n_rows, unsigned long long seed,
                                    const unsigned long long *seed_dev, uint32_t her, int strategy, const CwReplayOut *O, hipStream_t st);
hipError_t cwk_launch_seen_insert(const CwParams *P, const CwTuning *T, const CwSeen *S, const int32_t *group, const uint4 *hdr, const uint4 *pos, int n_states,
                                  uint8_t *fresh, int32_t *first, hipStream_t st);
hipError_t cwk_launch_seen_clear(const CwTuning *T, const CwSeen *S, hipStream_t st);
hipError_t cwk_launch_reach(const CwParams *P, const CwTuning *T, const CwSeen *S, const CwReach *R, const int32_t *env_of, const uint4 *hdr, const uint4 *pos,
                            int n_states, int depth, const CwReachOut *O, hipStream_t st);
hipError_t cwk_launch_unroll(const CwParams *P, const int32_t *env_of, const uint4 *hdr, const uint4 *pos, int own, int n_states, const uint8_t *actions,
                             int n_steps, int stop_at_done, const CwUnrollOut *O, hipStream_t st);
hipError_t cwk_launch_simulate(const CwParams *P, const int32_t *env_of, const uint4 *hdr, const uint4 *pos, int own, int n_states, const uint8_t *actions,
                               int n_steps, int stop_at_done, const CwSimulateOut *O, hipStream_t st);
hipError_t cwk_launch_rollout(const CwParams *P, const uint8_t *actions, int T, int32_t *rewards, uint8_t *dones, hipStream_t st);
hipError_t cwk_launch_render_ext(const CwParams *P, const CwTuning *T, uint8_t *out, hipStream_t st);
hipError_t cwk_launch_sweep_calib(const CwParams *P, const CwTuning *T, hipStream_t st);
void cwk_sweep_shape(const CwParams *P, const CwTuning *T, int *n_chunks, int *waves, int *jobs_per_wave);
hipError_t cwk_launch_idle(hipStream_t st);
hipError_t cwk_launch_export(const CwParams *P, const CwTuning *T, uint8_t *out, int onehot, int which, hipStream_t st);
}

#include <time.h>

static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                           \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess)                                                                   \
            return fail(CW_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = (hipSetDevice(dev) == hipSuccess);
    }
    ~DeviceGuard()
    {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// A REGION: one device allocation of the engine's outside every checkpoint blob and snapshot row, cut into sections by a cwh_*_layout of cw_host.cpp -- the
// snapshot bank, the visited set, the reach workspace, the replay buffer.  Its reserve is synchronous: the old region goes first (0 rows / slots / steps:
// that is all), then a NewRegion holds the allocation while it is cleared and frees it again unless the reserve commits it to the engine.
struct Region {
    void *base = nullptr;              // null: none reserved
    size_t bytes = 0;
    explicit operator bool() const { return base != nullptr; }
};
static void region_free(Region &r)
{
    if (r.base) (void)hipFree(r.base);
    r = Region{};
}
struct NewRegion {
    Region r;
    bool alloc(size_t bytes)           // false: no device memory (the error is the caller's to word)
    {
        if (hipMalloc(&r.base, bytes) != hipSuccess) { (void)hipGetLastError(); r.base = nullptr; return false; }
        r.bytes = bytes;
        return true;
    }
    char *at(uint64_t offset) const { return (char *)r.base + offset; }
    Region commit() { const Region out = r; r = Region{}; return out; }
    ~NewRegion() { region_free(r); }
};

struct cw_engine {
    int device = 0;
    int obs_mode = 0;
    int auto_reset = 1;
    bool has_reset = false;
    CwParams P{};
    CwTuning tune{};
    std::vector<void *> allocs;
    std::vector<void *> host_allocs;   // hipHostMalloc'ed (cw_config.host_outputs)
    int32_t *host_actions = nullptr;
    std::vector<CwMenuDev> menus;
    uint32_t *seed_scratch = nullptr;  // [N] device: seeds of cw_seed_int
    Region bank;                       // the snapshot bank (cw_snapshot_reserve), or none reserved
    CwBank B{};                        // ... its sections (cw_host.cpp: cwh_snapshot_section_bytes)
    size_t bank_row_bytes = 0;
    Region seen;                       // the visited set (cw_seen_reserve)
    CwSeen Sn{};                       // ... its arrays (cw_host.cpp: cwh_seen_layout)
    int64_t seen_slots = 0;
    Region reach;                      // cw_reach's workspace (cw_reach_reserve)
    CwReach Rc{};                      // ... its sections (cw_host.cpp: cwh_reach_layout)
    Region replay;                     // the replay buffer (cw_replay_reserve)
    CwReplay Rp{};                     // ... its sections (cw_host.cpp: cwh_replay_layout)
    int n = 0, S = 0, ncell = 0, K = 0;
    // resident stepper of the single-env loop (cw_step_resident; cw_kernels.hip: cw_resident_kernel)
    CwResident *res = nullptr;         // pinned coherent host memory, or null (engine not eligible)
    hipStream_t res_stream = nullptr;
    bool res_running = false;          // a cw_resident_kernel may be on the card
    uint32_t res_seq = 0;              // last sequence number rung
    hipEvent_t last_work = nullptr;    // recorded after the last cw_reset / cw_step / cw_rollout on the caller's stream: a resident kernel starts only after that
    bool last_work_set = false;        //   work (an event of the engine's own: the caller may destroy its stream any time after cw_synchronize)
    unsigned long long res_ticks_per_us = 100;   // the device's constant clock (wall_clock64), hipDeviceAttributeWallClockRate
    std::vector<hipEvent_t> prof_ev;   // 6 per recorded step
    // look-ahead (cw_layout.h): the refill kernel is launched every e->la_period steps, ahead of the step, on the step's stream
    bool la_refill_all = false;        // the next refill covers every env without a record (after cw_reset / a re-seed / a checkpoint load)
    unsigned la_steps = 0;
    unsigned la_period = 16;           // the CURRENT refill period: la_period_max, or shorter while envs finish twice between two refills (la_adapt)
    unsigned la_period_max = 16;       // la_period_for(max_steps), or CW_TUNE_LA_PERIOD
    bool la_adaptive = true;           // (false: a period forced by CW_TUNE_LA_PERIOD)
    int rollout_segment = -1;          // CW_TUNE_ROLLOUT_SEGMENT: steps per persistent launch of cw_rollout, 0: one launch, -1: max_steps
    unsigned long long *la_feedback = nullptr;     // pinned: counters[5] as the last refill kernel saw it
    unsigned long long la_slow_seen = 0;
    int32_t la_quiet = 0;              // refills in a row with (nearly) no slow-path reset
    bool in_step_many = false;         // (cw_step_many decides about the refill of a captured sequence itself)
    bool capturing_now = false;        // ... and asks once whether its stream is capturing, for all of its steps
    // the sweep's clock (calibrate_sweep) and its guard (sweep_guard_tick)
    int sweep_waves = 1024;            // waves of a sweep's launch, jobs (4-KiB pieces) per wave over all of its launches
    double sweep_jobs = 0, sweep_rate = 0, sweep_beside_ms = 0;      // (sweep_rate: cw_create's choice; the live one is guard.rate)
    bool guard_on = false;
    double head_notch = 0.4, busy_notch = 0.75, tune_period_ns = -1, tune_rate_tbs = -1;      // the host's own CW_TUNE_* values (read_tuning; the launch side's are in
    bool tune_guard = true, tune_lookahead = true, verbose = false;                             // tune): the clock's notches (TB/s), a forced period (ns) or starting rate (TB/s; -1: none)
    // the guard's samples in flight: the host runs up to ~1 000 steps ahead of the card, so a sample recorded now is read a dozen samples later
    enum { GUARD_RING = 32 };
    struct GuardSample { hipEvent_t ev[6]; int period16; } guard_ring[GUARD_RING] = {};
    unsigned guard_head = 0, guard_tail = 0;      // next slot to record into / oldest slot not read yet
    unsigned guard_step = 0;
    cwh_guard guard{};                  // its decisions (cw_host.cpp: cwh_guard_step): rate, best rate known, trials, back-off
    int prof_cap = 0, prof_n = 0;
    // the engine's OWN work: the streams it was handed since its last wait (at most 4 are remembered) and a private stream for the synchronous
    // entry points' copies and kernels (cw_seed_*, cw_get_mt, cw_get/set_state, checkpoints): none of them waits for anybody else's work
    hipStream_t aux = nullptr;
    hipStream_t work[4] = {nullptr, nullptr, nullptr, nullptr};
    int n_work = 0;
    bool work_overflow = false;        // more than 4 distinct streams since the last wait: a device-wide wait is the only safe one
    bool captured = false;             // STICKY: a step / rollout of this engine has been captured into a HIP graph.  Replays run on whatever stream the caller
                                       // launches the graph on, which the engine never sees: from then on every synchronous entry point waits for the DEVICE
};
// is `st` recording a graph right now?  (an error counts as no: the launch that follows reports it)
static inline bool stream_capturing(hipStream_t st)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
}
// every entry point that ENQUEUES on a caller's stream notes it (NOT a capturing stream: nothing runs on it, and it may be gone when the graph is replayed) ...
static inline void note_work(cw_engine *e, hipStream_t st)
{
    for (int i = 0; i < e->n_work; i++) if (e->work[i] == st) return;
    if (e->n_work < 4) e->work[e->n_work++] = st; else e->work_overflow = true;
}
// ... and every synchronous one first waits for exactly that: the engine's own work, not the card's (two engines on one device, a learner beside
// them: MultiDeviceVecEnv).  A stream the caller destroyed meanwhile (its work has then been waited for or abandoned by the caller) fails the
// wait: then, and only then, the whole device is waited for.
static hipError_t quiesce(cw_engine *e)
{
    bool all = e->work_overflow || e->captured;
    for (int i = 0; i < e->n_work && !all; i++)
        if (hipStreamSynchronize(e->work[i]) != hipSuccess) { (void)hipGetLastError(); all = true; }
    e->n_work = 0;
    e->work_overflow = false;
    if (all) return hipDeviceSynchronize();
    return e->aux ? hipStreamSynchronize(e->aux) : hipSuccess;
}
static inline hipError_t aux_copy(cw_engine *e, void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
{
    return bytes ? hipMemcpyAsync(dst, src, bytes, kind, e->aux) : hipSuccess;
}
// look-ahead refill: every la_period-th step.  A refill costs one reset's latency (~15 us) whatever the list holds, so rarely is cheap -- but an env
// that finishes twice between two refills is reset the slow way: a quarter of the episode length, 8..64 steps
static int la_period_for(int max_steps) { const int p = max_steps / 4; return p < 8 ? 8 : p > 64 ? 64 : p; }
// THE REFILL PERIOD FOLLOWS THE EPISODES (round 6).  la_period_for() assumes episodes of about max_steps steps -- a random policy's.  A policy that SUCCEEDS ends
// its episodes much earlier: an env then finishes two or three times between two refills, finds no record the second time and is reset the slow way by its
// whole wave -- ~12 us on the step kernel's critical path, and the kernel ends with its slowest wave (a walker on 8x8 grids under max_steps 300, episodes of
// ~140 steps: 98 slow resets per step at the static period of 64, state-only step 21 us instead of 6; profiles/r06_experiments.txt D).  Every refill kernel
// leaves the count of slow resets in a pinned word; the host reads it when it enqueues the next refill -- stale by a period or more, never waited for -- and
// halves the period (8 at least) while a period brings more slow resets than an eighth of its steps (what a refill launch costs), doubles it back after eight
// quiet refills in a row.  Results do not depend on the period; a captured graph keeps the period it was captured with.
static void la_adapt(cw_engine *e)
{
    const unsigned long long slow = __atomic_load_n(e->la_feedback, __ATOMIC_RELAXED);
    const unsigned long long delta = slow >= e->la_slow_seen ? slow - e->la_slow_seen : 0;      // (a loaded checkpoint brings its own counters)
    e->la_slow_seen = slow;
    e->la_period = (unsigned)cwh_la_adapt((int32_t)e->la_period, (int32_t)e->la_period_max, delta, &e->la_quiet);      // (cw_host.cpp: the rule, tested on the CPU)
}

// ------------------------------------------------------------------------------ resident stepper (host side)
// Every entry point that reads or writes the engine's state first makes sure no resident kernel holds it in registers.
static int resident_park(cw_engine *e)
{
    if (!e->res_running) return CW_OK;
    const unsigned long long low = __atomic_load_n(&e->res->bell, __ATOMIC_RELAXED) & 0xFFFFFFFFull;
    __atomic_store_n(&e->res->bell, low | (1ull << 32), __ATOMIC_RELEASE);
    HIP_TRY(hipStreamSynchronize(e->res_stream));        // the kernel leaves within one poll of seeing the flag
    e->res_running = false;
    __atomic_store_n(&e->res->bell, low, __ATOMIC_RELEASE);
    __atomic_store_n(&e->res->exited, 0u, __ATOMIC_RELEASE);
    return CW_OK;
}

// ------------------------------------------------------------------------------ what every entry point does on entry and on exit
// Entry: the engine's device is current until the call returns, and the resident stepper is parked.  `rc` is the call's result if that failed.
struct Entry {
    DeviceGuard guard;
    int rc;
    explicit Entry(cw_engine *e) : guard(e->device), rc(guard.ok ? resident_park(e) : fail(CW_ERR_HIP, "hipSetDevice(%d) failed", e->device)) {}
};
// An entry point that ENQUEUES on the caller's stream: Entry, then the stream is noted for quiesce() (note_work) -- and `return in.done()` records last_work,
// after which a resident kernel starts.  Two properties differ from call to call, and each call keeps the value it was written with:
//   CAPTURE_AWARE  asks whether the stream is recording a graph, and then marks the engine `captured` instead of noting the stream: cw_reset_masked,
//                  cw_imagine_masked, cw_sample_state_masked, cw_snapshot_save / _load, cw_expand, cw_simulate, cw_unroll, cw_plan, cw_shoot, cw_shoot_actions, cw_shoot_refit, cw_seen_clear, cw_seen_insert, cw_reach, cw_load_records, cw_replay_clear, cw_replay_push, cw_replay_sample, cw_export_onehot_states, cw_render_records,
//                  cw_rollout.  ANY_STREAM notes the stream regardless: cw_reset, cw_render, cw_render_onehot, cw_export_grid, cw_export_onehot(_of).
//   LAST_WORK      records the event: cw_reset and every CAPTURE_AWARE call but cw_rollout.  NO_LAST_WORK: cw_rollout and the ANY_STREAM readers.
enum Capture { ANY_STREAM, CAPTURE_AWARE };
enum LastWork { NO_LAST_WORK, LAST_WORK };
static inline void record_last_work(cw_engine *e, hipStream_t st)
{
    if (e->res && hipEventRecord(e->last_work, st) == hipSuccess) e->last_work_set = true;
}
struct EnqueueEntry : Entry {
    cw_engine *const e;
    const hipStream_t st;
    const LastWork last;
    EnqueueEntry(cw_engine *e_, cw_stream_t stream, Capture capture, LastWork last_) : Entry(e_), e(e_), st((hipStream_t)stream), last(last_)
    {
        if (rc != CW_OK) return;
        if (capture == CAPTURE_AWARE && stream_capturing(st)) e->captured = true; else note_work(e, st);
    }
    int done() { if (last == LAST_WORK) record_last_work(e, st); return CW_OK; }
};
// A SYNCHRONOUS entry point: Entry, then quiesce() -- the engine's own work, not the card's.  It copies with hipMemcpyAsync on e->aux into / out of vectors
// and stack buffers of its own (declared AHEAD of this object: they must outlive it): whatever way such a function is left -- an early return on an error
// included -- nothing may still be in flight against storage that dies with its frame, so every exit waits for the private stream; `return in.done()`
// is the exit that reports what that wait brought.
struct SyncEntry : Entry {
    cw_engine *const e;
    bool drain = false;
    explicit SyncEntry(cw_engine *e_) : Entry(e_), e(e_) { if (rc == CW_OK) rc = open(); }
    ~SyncEntry() { if (drain && e->aux) (void)hipStreamSynchronize(e->aux); }
    int open() { HIP_TRY(quiesce(e)); drain = true; return CW_OK; }
    int done() { HIP_TRY(hipStreamSynchronize(e->aux)); return CW_OK; }
};

// (MT19937 state conversion, the DLPack producer, the dense view of a slot record, the checkpoint sections' sizes and the guard's decisions: cw_host.cpp)

// ------------------------------------------------------------------------------ helpers
template <typename T>
static int dev_alloc(cw_engine *e, T **out, size_t count)
{
    void *p = nullptr;
    size_t bytes = count * sizeof(T);
    if (bytes == 0) bytes = 16;
    HIP_TRY(hipMalloc(&p, bytes));
    HIP_TRY(hipMemset(p, 0, bytes));
    e->allocs.push_back(p);
    *out = (T *)p;
    return CW_OK;
}

// pinned host memory mapped into the device's address space: kernels store into it directly (over PCIe), the host
// reads it after a stream sync -- the single-env loop's outputs (cw_config.host_outputs)
template <typename T>
static int host_alloc(cw_engine *e, T **out, size_t count)
{
    void *p = nullptr, *d = nullptr;
    size_t bytes = count * sizeof(T);
    if (bytes == 0) bytes = 16;
    HIP_TRY(hipHostMalloc(&p, bytes, hipHostMallocCoherent));       // (fine-grained: a resident kernel's stores must reach the host while it runs)
    e->host_allocs.push_back(p);
    memset(p, 0, bytes);
    HIP_TRY(hipHostGetDevicePointer(&d, p, 0));
    if (d != p) return fail(CW_ERR_HIP, "cw_create: mapped host memory has a different device address (no unified addressing)");
    *out = (T *)p;
    return CW_OK;
}

static void prof_free(cw_engine *e)
{
    for (hipEvent_t ev : e->prof_ev) (void)hipEventDestroy(ev);
    e->prof_ev.clear();
    e->prof_cap = e->prof_n = 0;
}

// launch time of the per-step render as currently configured (launches queued back to back, one wait: see calibrate_render_pace): the median and the
// 90th percentile of 20 launches -- the write path has a slower regime that a configuration may enter launch by launch (profiles/r03_pieces.txt N-P), and
// a median does not show a configuration that does so one time in three
static int timed_render_stats(cw_engine *e, double *median, double *p90, double *mean = nullptr)
{
    enum { LAUNCHES = 24, SKIP = 4 };
    hipEvent_t evs[2 * LAUNCHES] = {};
    bool ok = true;
    for (hipEvent_t &ev : evs) ok = ok && hipEventCreate(&ev) == hipSuccess;
    for (int rep = 0; rep < LAUNCHES && ok; rep++)
        ok = hipEventRecord(evs[2 * rep], e->aux) == hipSuccess && cwk_launch_sweep_calib(&e->P, &e->tune, e->aux) == hipSuccess &&
             hipEventRecord(evs[2 * rep + 1], e->aux) == hipSuccess && cwk_launch_idle(e->aux) == hipSuccess;
    ok = ok && hipStreamSynchronize(e->aux) == hipSuccess;
    float ms[LAUNCHES];
    for (int rep = 0; rep < LAUNCHES && ok; rep++) ok = hipEventElapsedTime(&ms[rep], evs[2 * rep], evs[2 * rep + 1]) == hipSuccess;
    for (hipEvent_t &ev : evs) if (ev) (void)hipEventDestroy(ev);
    if (!ok) return fail(CW_ERR_HIP, "cw_create: render calibration failed");
    std::sort(ms + SKIP, ms + LAUNCHES);
    const int n = LAUNCHES - SKIP;
    *median = ms[SKIP + n / 2];
    *p90 = ms[SKIP + (9 * n) / 10 - 1];
    if (mean) { double acc = 0; for (int i = SKIP; i < LAUNCHES; i++) acc += ms[i]; *mean = acc / n; }
    return CW_OK;
}

// The sweep's CLOCK (cw_kernels.hip: render_pieces): the period between two jobs of a wave, i.e. the RATE at which a launch writes --
// waves x 4 KiB per period.  In a row of back-to-back launches the memory system of an MI355X takes up to 7.7 TB/s of such a stream (65 536 envs,
// 21x21, 1 024 waves, 545 ns: 0.1988 ms per launch in step, 0.2004 with ~220 envs finishing on every step, 0.89 / 0.88 of the 8 TB/s peak) IF the
// launch's first ~40 us run a notch slower (cw_render_pieces_kernel: the head), and falls into its slower, saturated regime just beyond (525 ns:
// 0.20-0.24 whatever the head) or, box by box, already there (one launch in four 10-15 % late) -- profiles/r04_clock.txt K-M.  So cw_create tries 7.7,
// 7.4, 7.2, 7.0, 6.8, 6.6 TB/s and the unclocked sweep on the engine's own batch (20 launches each, an idle kernel between them like a step's)
// and takes the best 90th percentile -- a rate that is late one time in four loses to the next one -- and a GUARD keeps watching in cw_step
// (sweep_guard_tick): a sweep that does not keep its schedule any more is slowed down a notch.
// CW_TUNE_PERIOD_NS forces a period (0: unclocked, every wave as fast as it can).
static double sweep_period_ns(const cw_engine *e, double tb_per_s) { return (double)e->sweep_waves * 4096.0 / (tb_per_s * 1e12) * 1e9; }
// the clock's three periods from one rate (cwh_sweep_periods): a launch's first CWH_HEAD_JOBS jobs run the engine's head_notch slower, after a step on
// which envs finished its busy_notch slower (cw_render_pieces_kernel; CW_TUNE_HEAD_NOTCH / CW_TUNE_BUSY_NOTCH for experiments: profiles/r05_experiments.txt J)
static void set_sweep_rate(cw_engine *e, double tb_per_s)
{
    cwh_sweep_periods(tb_per_s, e->sweep_waves, e->head_notch, e->busy_notch, &e->tune.period16, &e->tune.period16_head, &e->tune.period16_busy);
}

static int calibrate_sweep(cw_engine *e)
{
    CwTuning &tn = e->tune;
    int n_chunks = 1, jobs_per_wave = 1;
    cwk_sweep_shape(&e->P, &tn, &n_chunks, &e->sweep_waves, &jobs_per_wave);
    e->sweep_jobs = (double)n_chunks * jobs_per_wave;
    if (e->tune_period_ns >= 0) {                                                // (the heads keep their distance: a forced 545 ns is 7.7 TB/s with 7.3 / 6.95 heads)
        const double ns = e->tune_period_ns;
        set_sweep_rate(e, ns > 0 ? (double)e->sweep_waves * 4096.0 / (ns * 1e-9) * 1e-12 : 0.0);
        if (ns > 0) tn.period16 = (int)(ns * 1.6 + 0.5);
        return CW_OK;
    }
    set_sweep_rate(e, 7.0);
    // (small batches are launch-bound: nothing to check; host-mapped frames are PCIe-bound: unclocked)
    if (e->host_actions) { set_sweep_rate(e, 0); return CW_OK; }
    if (e->obs_mode != CW_OBS_PIXELS_FULL || (double)e->n * e->P.frame_bytes < (double)(64ll << 20)) return CW_OK;
    // the candidates, the fastest first; unclocked last (a sweep whose jobs take longer than any useful period -- several small frames per piece --
    // paces itself: the clock then only costs its reads).  The one with the best 90th-percentile launch: in its saturated regime the memory
    // system is slower AND erratic (7.5 TB/s: 0.214-0.235 ms launch by launch where 7.0 reads 0.2112 +- 0.0005), so the slow launches tell.
    static const double rates[] = {7.7, 7.4, 7.2, 7.0, 6.8, 6.6, 0.0};
    char log[1024] = "";
    size_t len = 0;
    int rc = CW_OK;
    double best_p90 = 0, med = 0, p90 = 0, mean = 0;
    rc = timed_render_stats(e, &med, &p90);           // (a card that idled through set-up runs its first launches a few per cent slower: not counted)
    // what a sweep costs beside its jobs (a launch's ramp and tail, the events around it), at a rate the memory system keeps up with easily: the guard's yardstick
    set_sweep_rate(e, 6.4);
    if (rc == CW_OK) rc = timed_render_stats(e, &med, &p90);
    e->sweep_beside_ms = med - e->sweep_jobs * sweep_period_ns(e, 6.4) * 1e-6;
    if (e->tune_rate_tbs >= 0) e->sweep_rate = e->tune_rate_tbs;               // (the starting rate, the guard stays on: the test that it slows a saturated sweep down)
    for (size_t i = 0; i < sizeof(rates) / sizeof(rates[0]) && rc == CW_OK && e->tune_rate_tbs < 0; i++) {
        set_sweep_rate(e, rates[i]);
        rc = timed_render_stats(e, &med, &p90, &mean);
        if (len < sizeof(log) - 56) len += (size_t)snprintf(log + len, sizeof(log) - len, " %.1f TB/s (%.0f ns): %.4f/%.4f/%.4f |", rates[i], tn.period16 / 1.6, med, p90, mean);
        if (rc == CW_OK && (best_p90 == 0 || p90 < 0.995 * best_p90)) { best_p90 = p90; e->sweep_rate = rates[i]; }
    }
    set_sweep_rate(e, e->sweep_rate);
    cwh_guard_init(&e->guard, e->sweep_rate);
    e->guard_on = rc == CW_OK && e->sweep_rate > 0 && e->auto_reset && e->tune_guard;
    if (e->guard_on)
        for (auto &smp : e->guard_ring)
            for (hipEvent_t &ev : smp.ev)
                if (hipEventCreate(&ev) != hipSuccess) e->guard_on = false;
    if (e->verbose)
        fprintf(stderr, "[craftingworld] sweep clock, ms per sweep (median/90th percentile/mean of 20; 0.0 TB/s = unclocked):%s -> %s%.0f ns\n", log,
                tn.period16 ? "" : "unclocked, ", tn.period16 / 1.6);
    return rc;
}

// The GUARD of the sweep's clock, the plumbing: every CW_GUARD_EVERY-th step's sweep is bracketed by two events on the caller's stream; when they have
// completed (read at the next sampled step, however far the host runs ahead) the sweep's time and its schedule go to cwh_guard_step (cw_host.cpp: the
// decisions -- slowdowns, trials one notch up, back-off -- as a pure state machine, tested on synthetic traces in tests/test_host_logic.py), and a
// changed rate is programmed into the clock.  -> the event array for this step's launch, or null.
enum { CW_GUARD_EVERY = 64 };
static hipEvent_t *sweep_guard_tick(cw_engine *e, hipStream_t st)
{
    if (++e->guard_step % CW_GUARD_EVERY) return nullptr;
    // the samples whose sweeps have run by now, oldest first (the host may be a thousand steps ahead of the card: a sample is read long after it was recorded)
    while (e->guard_tail != e->guard_head && hipEventQuery(e->guard_ring[e->guard_tail % cw_engine::GUARD_RING].ev[5]) == hipSuccess) {
        cw_engine::GuardSample &smp = e->guard_ring[e->guard_tail++ % cw_engine::GUARD_RING];
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, smp.ev[4], smp.ev[5]) != hipSuccess || ms <= 0.f || smp.period16 != e->tune.period16) continue;      // (a sample of another rate says nothing)
        const double scheduled = cwh_guard_scheduled_ms(e->sweep_jobs, e->tune.period16, e->tune.period16_busy, e->sweep_beside_ms);
        const double rate_before = e->guard.rate, prev_mean = e->guard.prev_mean;
        const int recovering = e->guard.recovering;
        const int action = cwh_guard_step(&e->guard, ms, scheduled);
        if (e->guard.rate != rate_before) set_sweep_rate(e, e->guard.rate);
        if (e->verbose && action != CWH_GUARD_NONE) {
            static const char *what[] = {"", "three samples in a row late: a notch down", "trying a notch up", "the trial pays: kept", "the trial does not pay: undone"};
            fprintf(stderr, "[craftingworld] sweep clock: %s%s -- %.4f ms against %.4f scheduled (mean at the rate left %.4f): %.1f -> %.1f TB/s (%.0f ns)\n", what[action],
                    recovering ? " (on the way back to the best rate known)" : "", ms, scheduled, prev_mean, rate_before, e->guard.rate, e->tune.period16 / 1.6);
        }
    }
    if (e->guard_head - e->guard_tail >= (unsigned)cw_engine::GUARD_RING) return nullptr;      // (every slot in flight: this step goes unsampled)
    cw_engine::GuardSample &slot = e->guard_ring[e->guard_head++ % cw_engine::GUARD_RING];
    slot.period16 = e->tune.period16;
    return slot.ev;
}

// Every CW_TUNE_* environment variable, read once, by cw_create: the launch side's into e->tune, the host's own into the engine.
// It runs on a fresh engine, whose values are the defaults: a value out of its range keeps the default.  (The default refill period follows P.max_steps.)
static void read_tuning(cw_engine *e)
{
    CwTuning &tn = e->tune;
    cwh_tuning t{};                    // the defaults in, the variables' values out (cw_host.cpp: the parsing and the ranges, tested on the CPU)
    t.render_chunk_rounds = tn.render_chunk_rounds;
    t.step_envs_per_wave = tn.step_envs_per_wave;
    t.gather = tn.gather;
    t.gather_max_size = tn.gather_max_size;
    t.small_frame_bytes = tn.small_frame_bytes;
    t.small_blocks_per_cu = tn.small_blocks_per_cu;
    t.small_launch_mb = (int32_t)(tn.small_launch_bytes >> 20);
    t.reset_blocks_per_cu = tn.reset_blocks_per_cu;
    t.guard = 1;
    t.verbose = 0;
    t.lookahead = 1;
    t.la_period = 0;
    t.rollout_segment = e->rollout_segment;
    t.head_notch = e->head_notch;
    t.busy_notch = e->busy_notch;
    t.period_ns = -1;
    t.rate_tbs = -1;
    cwh_read_tuning([](void *, const char *k) -> const char * { return getenv(k); }, nullptr, &t);
    tn.render_chunk_rounds = t.render_chunk_rounds;
    tn.step_envs_per_wave = t.step_envs_per_wave;
    tn.gather = t.gather;
    tn.gather_max_size = t.gather_max_size;
    tn.small_frame_bytes = t.small_frame_bytes;
    tn.small_blocks_per_cu = t.small_blocks_per_cu;
    tn.small_launch_bytes = (long long)t.small_launch_mb << 20;
    tn.reset_blocks_per_cu = t.reset_blocks_per_cu;
    e->head_notch = t.head_notch;
    e->busy_notch = t.busy_notch;
    e->tune_period_ns = t.period_ns;
    e->tune_rate_tbs = t.rate_tbs;
    e->tune_guard = t.guard != 0;
    e->verbose = t.verbose != 0;
    e->tune_lookahead = t.lookahead != 0;
    e->la_adaptive = t.la_period == 0;
    e->la_period = e->la_period_max = (unsigned)(t.la_period ? t.la_period : la_period_for(e->P.max_steps));
    e->rollout_segment = t.rollout_segment;
}

extern "C" {

const char *cw_last_error(void) { return g_err; }
int cw_abi_version(void) { return CW_ABI_VERSION; }
int cw_num_envs(const cw_engine *e) { return e ? e->n : 0; }

int cw_create(const cw_config *cfg, int device, cw_engine **out)
{
    if (!cfg || !out) return fail(CW_ERR_INVALID, "cw_create: null argument");
    *out = nullptr;
    if (cfg->abi_version != CW_ABI_VERSION)
        return fail(CW_ERR_INVALID, "cw_create: abi_version %d != %d", cfg->abi_version, CW_ABI_VERSION);
    if (cfg->num_envs < 1) return fail(CW_ERR_INVALID, "cw_create: num_envs must be >= 1");
    if (cfg->size < 4 || cfg->size > 255)
        return fail(CW_ERR_INVALID, "cw_create: size must be in 4..255 (square grids only; non-square is a reference defect)");
    if (cfg->max_steps < 1 || cfg->max_steps > 65535) return fail(CW_ERR_INVALID, "cw_create: max_steps must be in 1..65535");
    if (cfg->n_task_list < 9 || cfg->n_task_list > CW_MAX_TASKS)
        return fail(CW_ERR_INVALID, "cw_create: len(task_list) must be in 9..%d", CW_MAX_TASKS);
    if (cfg->fixed_init_state < 0 || cfg->fixed_init_state > 64)
        return fail(CW_ERR_INVALID, "cw_create: fixed_init_state must be in 0..64");
    if (cfg->obs_mode < CW_OBS_STATE || cfg->obs_mode > CW_OBS_PIXELS_DIRTY) return fail(CW_ERR_INVALID, "cw_create: bad obs_mode");
    if (cfg->raster != CW_RASTER_RAY && cfg->raster != CW_RASTER_ALT) return fail(CW_ERR_INVALID, "cw_create: bad raster");
    if (cfg->n_menus < 1 || cfg->n_menus > CW_MAX_MENUS || !cfg->menus) return fail(CW_ERR_INVALID, "cw_create: n_menus must be in 1..%d", CW_MAX_MENUS);
    if ((double)cfg->num_envs * 48.0 * cfg->size * cfg->size > 1.0e12)
        return fail(CW_ERR_INVALID, "cw_create: num_envs x frame size exceeds 1 TB");

    std::vector<CwMenuDev> menus(cfg->n_menus);
    for (int m = 0; m < cfg->n_menus; m++) {
        const cw_task_menu &src = cfg->menus[m];
        if (src.n_selected < 1 || src.n_selected > CW_MAX_TASKS)
            return fail(CW_ERR_INVALID, "cw_create: menu %d: len(selected_tasks) must be in 1..%d", m, CW_MAX_TASKS);
        if (src.number_of_tasks < 1) return fail(CW_ERR_INVALID, "cw_create: menu %d: number_of_tasks must be >= 1", m);
        CwMenuDev d{};
        d.n_selected = src.n_selected;
        d.number_of_tasks = src.number_of_tasks > src.n_selected ? src.n_selected : src.number_of_tasks;  // ray.py:80-81
        d.stacking = src.stacking ? 1 : 0;
        d.reward_subset = src.reward_subset ? 1 : 0;
        for (int i = 0; i < src.n_selected; i++) {
            if (src.selected_bits[i] < 0 || src.selected_bits[i] >= cfg->n_task_list)
                return fail(CW_ERR_INVALID, "cw_create: menu %d: selected task %d is not in task_list", m, i);
            d.sel_bits |= (uint64_t)src.selected_bits[i] << (4 * i);
        }
        menus[m] = d;
    }
    if (cfg->env_menu)
        for (int i = 0; i < cfg->num_envs; i++)
            if (cfg->env_menu[i] >= cfg->n_menus) return fail(CW_ERR_INVALID, "cw_create: env_menu[%d] out of range", i);

    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(CW_ERR_INVALID, "cw_create: device %d not present (%d devices)", device, ndev);
    DeviceGuard guard(device);
    if (!guard.ok) return fail(CW_ERR_HIP, "cw_create: hipSetDevice(%d) failed", device);

    cw_engine *e = new (std::nothrow) cw_engine();
    if (!e) return fail(CW_ERR_INVALID, "cw_create: out of host memory");
    e->device = device;
    e->obs_mode = cfg->obs_mode;
    e->auto_reset = cfg->auto_reset ? 1 : 0;
    e->n = cfg->num_envs;
    e->S = cfg->size;
    e->ncell = cfg->size * cfg->size;
    e->K = cfg->fixed_init_state;
    e->menus = menus;
    CwParams &P = e->P;
    const size_t N = (size_t)e->n;
    P.n_envs = e->n;
    P.size = e->S;
    P.ncell = e->ncell;
    P.max_steps = cfg->max_steps;
    read_tuning(e);                    // (the defaults are the measured best)
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) e->tune.n_cu = prop.multiProcessorCount;
    P.task_mask = (1u << cfg->n_task_list) - 1u;
    P.pool_k = e->K;
    P.div_magic = (uint32_t)((1ull << 32) / (uint64_t)e->S) + 1u;
    P.raster = cfg->raster;
    P.frame_bytes = cfg->raster == CW_RASTER_ALT ? 27u * (uint32_t)e->S * (uint32_t)(e->S + 1) : 48u * (uint32_t)e->ncell;

    int rc = CW_OK;
#define ALLOC(field, count)                                     \
    if (rc == CW_OK) rc = dev_alloc(e, &P.field, (count))
    ALLOC(hdr, N);
    ALLOC(pos, N);
    ALLOC(init_pos, N);
    ALLOC(init_agent, N);
    ALLOC(goal_pos, N);
    ALLOC(goal_codes, N);
    ALLOC(goal_agent, N);
    ALLOC(ep_no, N);
    ALLOC(mt, N * CW_MT_N);
    ALLOC(mt_idx, N);
    ALLOC(pool, N * (size_t)e->K * 9);
    if (rc == CW_OK) rc = dev_alloc(e, &e->seed_scratch, N);
    // step outputs and frames: device memory, or mapped host memory for the single-env loop
#define ALLOC_OUT(field, count)                                 \
    if (rc == CW_OK) rc = cfg->host_outputs ? host_alloc(e, &P.field, (count)) : dev_alloc(e, &P.field, (count))
    ALLOC_OUT(reward, N);
    ALLOC_OUT(done, N);
    ALLOC_OUT(achieved_out, N);
    ALLOC_OUT(desired_out, N);
    ALLOC_OUT(episode_length, N);
    ALLOC_OUT(episode_return, N);
    ALLOC(counters, 8);
    if (rc == CW_OK) {
        // the private stream of the synchronous entry points: at the HIGHEST priority -- the runtime multiplexes streams of one priority onto a handful of
        // hardware queues, and a copy queued behind another engine's thousand pending steps in the same queue waits for them like a device-wide wait
        int pr_least = 0, pr_greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest) != hipSuccess) pr_least = pr_greatest = 0;
        if (hipStreamCreateWithPriority(&e->aux, hipStreamNonBlocking, pr_greatest) != hipSuccess &&
            hipStreamCreateWithFlags(&e->aux, hipStreamNonBlocking) != hipSuccess)
            rc = fail(CW_ERR_HIP, "cw_create: no private stream");
    }
    if (cfg->obs_mode != CW_OBS_STATE) {
        ALLOC_OUT(obs, N * P.frame_bytes);
        ALLOC_OUT(desired_img, N * P.frame_bytes);
        ALLOC_OUT(init_img, N * P.frame_bytes);
        if (cfg->keep_terminal_obs && cfg->auto_reset) ALLOC_OUT(terminal_img, N * P.frame_bytes);
    }
    if (cfg->host_outputs && rc == CW_OK) rc = host_alloc(e, &e->host_actions, N);
    // look-ahead records: every engine that resets by itself and lives in device memory (CW_TUNE_LOOKAHEAD=0: the slow path only, for A/B runs
    // and the test that both give the same results)
    P.lookahead = (cfg->auto_reset && !cfg->host_outputs && e->tune_lookahead) ? 1 : 0;
    ALLOC(nx_init_pos, P.lookahead ? N * CW_LA_DEPTH : 1);      // (a queue of CW_LA_DEPTH records per env, one array per slot: cw_layout.h)
    ALLOC(nx_goal_pos, P.lookahead ? N * CW_LA_DEPTH : 1);
    ALLOC(nx_misc, P.lookahead ? N * CW_LA_DEPTH : 1);
    ALLOC(nx_ctl, P.lookahead ? N : 1);
    if (rc == CW_OK && P.lookahead && e->la_adaptive) {      // (no pinned word: a fixed period)
        void *fb = nullptr;
        if (hipHostMalloc(&fb, 64, hipHostMallocCoherent) == hipSuccess) {
            memset(fb, 0, 64);
            e->host_allocs.push_back(fb);
            e->la_feedback = P.la_feedback = (unsigned long long *)fb;
        }
    }
#undef ALLOC_OUT
#undef ALLOC
    CwMenuDev *dmenus = nullptr;
    if (rc == CW_OK) rc = dev_alloc(e, &dmenus, menus.size());
    if (rc == CW_OK && hipMemcpy(dmenus, menus.data(), menus.size() * sizeof(CwMenuDev), hipMemcpyHostToDevice) != hipSuccess)
        rc = fail(CW_ERR_HIP, "cw_create: menu upload failed");
    P.menus = dmenus;
    if (rc == CW_OK) {
        // header: menu id per env; everything else zero until cw_reset
        std::vector<uint32_t> h(N * 4, 0u);
        for (size_t i = 0; i < N; i++) {
            h[i * 4 + 0] = (uint32_t)(cfg->env_menu ? cfg->env_menu[i] : 0) << 24;
            h[i * 4 + 3] = CW_CODES_INITIAL;
        }
        if (hipMemcpy(P.hdr, h.data(), h.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(CW_ERR_HIP, "cw_create: header upload failed");
    }
    if (rc != CW_OK) {
        if (e->aux) (void)hipStreamDestroy(e->aux);
        for (void *p : e->allocs) (void)hipFree(p);
        for (void *p : e->host_allocs) (void)hipHostFree(p);
        delete e;
        return rc;
    }
    if (cfg->host_outputs && e->n == 1 && !e->auto_reset && e->obs_mode != CW_OBS_PIXELS_FULL) {     // the single-env loop: resident stepper
        void *p = nullptr;
        if (hipHostMalloc(&p, sizeof(CwResident), hipHostMallocCoherent) == hipSuccess &&
            hipStreamCreateWithFlags(&e->res_stream, hipStreamNonBlocking) == hipSuccess) {
            memset(p, 0, sizeof(CwResident));
            e->host_allocs.push_back(p);
            e->res = (CwResident *)p;
            if (host_alloc(e, &e->P.res_onehot, (size_t)e->ncell * 12) != CW_OK) e->P.res_onehot = nullptr;
            int khz = 0;                                 // the kernel's idle-out and time slice are counted on the constant clock
            if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz >= 1000) e->res_ticks_per_us = (unsigned long long)khz / 1000ull;
            if (hipEventCreateWithFlags(&e->last_work, hipEventDisableTiming) != hipSuccess) {       // (no event: no resident stepper)
                e->last_work = nullptr;
                e->res = nullptr;
            }
        } else {
            if (p) (void)hipHostFree(p);
            e->res_stream = nullptr;                 // (no resident stepper: cw_step_resident reports it)
        }
    }
    *out = e;
    // default stream: env i seeded like numpy RandomState(i); callers normally reseed
    std::vector<uint32_t> seeds(N);
    for (size_t i = 0; i < N; i++) seeds[i] = (uint32_t)i;
    rc = cw_seed_int(e, seeds.data());
    if (rc == CW_OK) rc = calibrate_sweep(e);
    if (rc != CW_OK) {
        cw_destroy(e);
        *out = nullptr;
    }
    return rc;
}

int cw_destroy(cw_engine *e)
{
    if (!e) return CW_OK;
    Entry in(e);
    if (in.rc != CW_OK) return in.rc;
    (void)quiesce(e);
    prof_free(e);
    if (e->aux) (void)hipStreamDestroy(e->aux);
    if (e->res_stream) (void)hipStreamDestroy(e->res_stream);
    if (e->last_work) (void)hipEventDestroy(e->last_work);
    for (auto &smp : e->guard_ring) for (hipEvent_t ev : smp.ev) if (ev) (void)hipEventDestroy(ev);
    for (void *p : e->allocs) (void)hipFree(p);
    for (Region *r : {&e->bank, &e->seen, &e->reach, &e->replay}) region_free(*r);
    for (void *p : e->host_allocs) (void)hipHostFree(p);
    delete e;
    return CW_OK;
}

// A new stream makes the records computed from the old one void: drop them all; the next refill covers every env.
static hipError_t lookahead_drop(cw_engine *e)
{
    if (!e->P.lookahead) return hipSuccess;
    hipError_t rc = hipMemsetAsync(e->P.nx_misc, 0, (size_t)e->n * CW_LA_DEPTH * sizeof(uint4), e->aux);
    if (rc == hipSuccess) rc = hipMemsetAsync(e->P.nx_ctl, 0, (size_t)e->n * sizeof(uint32_t), e->aux);
    e->la_refill_all = true;
    return rc;
}

// Both seeders run on the device (cw_seed_kernel, one lane per env): the host only copies what the caller handed over.
// (A host-side conversion built an N x 624-word vector serially: 2.6 GB and seconds at 2^20 envs per GPU.)
int cw_seed_mt(cw_engine *e, const uint32_t *keys, const int32_t *pos)
{
    if (!e || !keys || !pos) return fail(CW_ERR_INVALID, "cw_seed_mt: null argument");
    const size_t N = (size_t)e->n;
    for (size_t i = 0; i < N; i++)
        if (pos[i] < 0 || pos[i] > CW_MT_N) return fail(CW_ERR_INVALID, "cw_seed_mt: pos[%zu]=%d outside 0..624", i, pos[i]);
    SyncEntry in(e);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(aux_copy(e, e->P.mt, keys, N * CW_MT_N * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(aux_copy(e, e->P.mt_idx, pos, N * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(cwk_launch_seed(&e->P, nullptr, e->aux));
    HIP_TRY(lookahead_drop(e));
    return in.done();
}

int cw_seed_int(cw_engine *e, const uint32_t *seeds)
{
    if (!e || !seeds) return fail(CW_ERR_INVALID, "cw_seed_int: null argument");
    SyncEntry in(e);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(aux_copy(e, e->seed_scratch, seeds, (size_t)e->n * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(cwk_launch_seed(&e->P, e->seed_scratch, e->aux));
    HIP_TRY(lookahead_drop(e));
    return in.done();
}

int cw_get_mt(cw_engine *e, uint32_t *keys, int32_t *pos)
{
    if (!e || !keys || !pos) return fail(CW_ERR_INVALID, "cw_get_mt: null argument");
    const size_t N = (size_t)e->n;
    std::vector<uint32_t> words(N * CW_MT_N);
    std::vector<uint32_t> misc(e->P.lookahead ? N * 4 * CW_LA_DEPTH : 0);
    SyncEntry in(e);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(aux_copy(e, words.data(), e->P.mt, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(aux_copy(e, pos, e->P.mt_idx, N * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (e->P.lookahead) HIP_TRY(aux_copy(e, misc.data(), e->P.nx_misc, N * 16 * CW_LA_DEPTH, hipMemcpyDeviceToHost));
    HIP_TRY(hipStreamSynchronize(e->aux));
    for (size_t i = 0; i < N; i++) cwh_mt_to_numpy(&words[i * CW_MT_N], pos[i], keys + i * CW_MT_N);
    if (e->P.lookahead) {                            // the engine's streams are as many resets ahead as records wait: report the position BEFORE the first of them
        for (size_t i = 0; i < N; i++) {
            uint32_t ahead = 0;
            for (size_t d = 0; d < CW_LA_DEPTH; d++)
                if (misc[(d * N + i) * 4 + 2] >> 31) ahead += misc[(d * N + i) * 4 + 3];
            if (ahead) cwh_mt_rewind(keys + i * CW_MT_N, &pos[i], ahead);
        }
    }
    // numpy's own form of a stream that stands at a generation's end: it regenerates lazily, so after the 624th draw RandomState.get_state() shows
    // (the generation just used up, 624), never (the next one, 0) -- the engine's consume-and-replace form holds the next one already
    for (size_t i = 0; i < N; i++)
        if (pos[i] == 0) { cwh_mt_untwist(keys + i * CW_MT_N); pos[i] = CW_MT_N; }
    return CW_OK;
}

// imagine_obs() / sample_state() draw from the envs' streams at their LOGICAL position.  An engine that keeps look-ahead records has run its streams ahead of
// that: rewind them and drop the records, as cw_generate_fixed_states does before its pool draws (synchronous; the next refill covers the whole batch).
static int rewind_streams(cw_engine *e, hipStream_t st, const char *who)
{
    if (!e->P.lookahead) return CW_OK;
    Entry in(e);      // (an entry of its own: cw_imagine_masked / cw_sample_state_masked come here AHEAD of theirs -- the quiesce() below forgets every noted stream)
    if (in.rc != CW_OK) return in.rc;
    if (stream_capturing(st)) return fail(CW_ERR_STATE, "%s: an engine that keeps look-ahead records rewinds its streams through the host and cannot be captured", who);
    std::vector<uint32_t> keys((size_t)e->n * CW_MT_N);
    std::vector<int32_t> pos((size_t)e->n);
    int rc = cw_get_mt(e, keys.data(), pos.data());
    if (rc == CW_OK) rc = cw_seed_mt(e, keys.data(), pos.data());
    return rc;
}

int cw_generate_fixed_states(cw_engine *e, cw_stream_t stream)
{
    if (!e) return fail(CW_ERR_INVALID, "cw_generate_fixed_states: null engine");
    if (e->K == 0) return CW_OK;
    Entry in(e);
    if (in.rc != CW_OK) return in.rc;
    if (e->has_reset) {                              // records wait, computed from the stream the pool is about to draw from: rewind and drop them
        const int rc = rewind_streams(e, (hipStream_t)stream, "cw_generate_fixed_states");      // (never capturing: the call synchronises below)
        if (rc != CW_OK) return rc;
    }
    HIP_TRY(cwk_launch_pool(&e->P, &e->tune, (hipStream_t)stream));
    // one-time, off the hot path: the pool and the advanced RNG streams are complete before any other stream can reset from them
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return CW_OK;
}

int cw_reset(cw_engine *e, cw_stream_t stream)
{
    if (!e) return fail(CW_ERR_INVALID, "cw_reset: null engine");
    EnqueueEntry in(e, stream, ANY_STREAM, LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(cwk_launch_reset_all(&e->P, &e->tune, e->obs_mode, (hipStream_t)stream));
    if (e->P.lookahead) {                            // every env's NEXT episode, ahead of time (cw_refill_kernel)
        HIP_TRY(cwk_launch_refill(&e->P, &e->tune, 1, (hipStream_t)stream));
        e->la_refill_all = false;
        e->la_steps = 0;
    }
    e->has_reset = true;
    return in.done();
}

// reset() of the envs the caller selects: ONE kernel (cw_reset_masked_kernel) and nothing else.  No refill of its own -- an env that took a record is QUEUED,
// and the refill that rides on cw_step serves it; la_steps / la_refill_all stay as they are -- so the call is the same whether it is enqueued or captured.
int cw_reset_masked(cw_engine *e, const uint8_t *mask, cw_stream_t stream)
{
    if (!e || !mask) return fail(CW_ERR_INVALID, "cw_reset_masked: null %s", !e ? "engine" : "mask");
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_reset_masked called before cw_reset");
    EnqueueEntry in(e, stream, CAPTURE_AWARE, LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(cwk_launch_reset_masked(&e->P, &e->tune, mask, e->obs_mode, (hipStream_t)stream));
    return in.done();
}

int cw_imagine_masked(cw_engine *e, const uint8_t *mask, const uint16_t *desired, int32_t commit, uint8_t *out_frames, uint8_t *out_onehot,
                      cw_stream_t stream)
{
    if (!e) return fail(CW_ERR_INVALID, "cw_imagine_masked: null engine");
    if (!commit && !out_frames && !out_onehot) return fail(CW_ERR_INVALID, "cw_imagine_masked: commit == 0 and no output pointer: nothing to do");
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_imagine_masked called before cw_reset");
    const int rc = rewind_streams(e, (hipStream_t)stream, "cw_imagine_masked");
    if (rc != CW_OK) return rc;
    EnqueueEntry in(e, stream, CAPTURE_AWARE, LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(cwk_launch_imagine_masked(&e->P, &e->tune, mask, desired, commit != 0, e->obs_mode, out_frames, out_onehot, (hipStream_t)stream));
    return in.done();
}

int cw_sample_state_masked(cw_engine *e, const uint8_t *mask, int32_t pooled, uint16_t *out_cells, cw_stream_t stream)
{
    if (!e || !out_cells) return fail(CW_ERR_INVALID, "cw_sample_state_masked: null %s", !e ? "engine" : "out_cells");
    if (pooled && e->K == 0) return fail(CW_ERR_INVALID, "cw_sample_state_masked: pooled with fixed_init_state == 0");
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_sample_state_masked called before cw_reset");
    const int rc = rewind_streams(e, (hipStream_t)stream, "cw_sample_state_masked");
    if (rc != CW_OK) return rc;
    EnqueueEntry in(e, stream, CAPTURE_AWARE, LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(cwk_launch_sample_state_masked(&e->P, &e->tune, mask, pooled != 0, out_cells, (hipStream_t)stream));
    return in.done();
}

// ------------------------------------------------------------------------------ snapshot bank
// The bank is a Region of the engine's, outside every checkpoint blob; cw_checkpoint_load, cw_seed_* and cw_generate_fixed_states leave it alone (a row
// is self-contained: it carries its own stream, ring and pool row).  Re-allocating drops every saved row: the new bank's valid bytes are zero.
int cw_snapshot_reserve(cw_engine *e, int32_t rows)
{
    if (!e) return fail(CW_ERR_INVALID, "cw_snapshot_reserve: null engine");
    if (rows < 0) return fail(CW_ERR_INVALID, "cw_snapshot_reserve: rows = %d must be >= 0", rows);
    SyncEntry in(e);                                 // (the engine's own work: a save or load in flight uses the bank about to go)
    if (in.rc != CW_OK) return in.rc;
    region_free(e->bank);
    e->B = CwBank{};
    e->bank_row_bytes = 0;
    if (rows == 0) return CW_OK;
    size_t bytes[CWH_SNAP_SECTIONS], at[CWH_SNAP_SECTIONS];
    uint64_t total = 0, row_bytes = 0;
    cwh_snapshot_section_bytes(rows, e->K, e->P.lookahead ? CW_LA_DEPTH : 0, bytes, at, &total, &row_bytes);
    NewRegion nr;
    if (!nr.alloc((size_t)total))
        return fail(CW_ERR_HIP, "cw_snapshot_reserve: no device memory for %d rows of %llu bytes", rows, (unsigned long long)row_bytes);
    if (hipMemsetAsync(nr.at(at[CWH_SNAP_VALID]), 0, bytes[CWH_SNAP_VALID], e->aux) != hipSuccess || hipStreamSynchronize(e->aux) != hipSuccess) {
        (void)hipGetLastError();
        return fail(CW_ERR_HIP, "cw_snapshot_reserve: clearing the valid bytes failed");
    }
    CwBank &B = e->B;
    B.hdr = (uint4 *)nr.at(at[CWH_SNAP_HDR]); B.pos = (uint4 *)nr.at(at[CWH_SNAP_POS]);
    B.init_pos = (uint4 *)nr.at(at[CWH_SNAP_INIT_POS]); B.goal_pos = (uint4 *)nr.at(at[CWH_SNAP_GOAL_POS]);
    B.goal_codes = (uint32_t *)nr.at(at[CWH_SNAP_GOAL_CODES]); B.ep_no = (int32_t *)nr.at(at[CWH_SNAP_EP_NO]);
    B.init_agent = (uint16_t *)nr.at(at[CWH_SNAP_INIT_AGENT]); B.goal_agent = (uint16_t *)nr.at(at[CWH_SNAP_GOAL_AGENT]);
    B.mt = (uint32_t *)nr.at(at[CWH_SNAP_MT]); B.mt_idx = (int32_t *)nr.at(at[CWH_SNAP_MT_IDX]);
    B.nx_init_pos = (uint4 *)nr.at(at[CWH_SNAP_NX_INIT_POS]); B.nx_goal_pos = (uint4 *)nr.at(at[CWH_SNAP_NX_GOAL_POS]);
    B.nx_misc = (uint4 *)nr.at(at[CWH_SNAP_NX_MISC]); B.nx_ctl = (uint32_t *)nr.at(at[CWH_SNAP_NX_CTL]);
    B.pool = (uint16_t *)nr.at(at[CWH_SNAP_POOL]); B.valid = (uint8_t *)nr.at(at[CWH_SNAP_VALID]);
    B.rows = rows;
    e->bank = nr.commit();
    e->bank_row_bytes = (size_t)row_bytes;
    return CW_OK;
}

size_t cw_snapshot_row_bytes(const cw_engine *e)
{
    if (!e) { (void)fail(CW_ERR_INVALID, "cw_snapshot_row_bytes: null engine"); return 0; }
    return e->bank ? e->bank_row_bytes : 0;
}

// Both only enqueue ONE kernel: no wait, no allocation, the same call whether it runs or is captured.
int cw_snapshot_save(cw_engine *e, const int32_t *rows, cw_stream_t stream)
{
    if (!e || !rows) return fail(CW_ERR_INVALID, "cw_snapshot_save: null %s", !e ? "engine" : "rows");
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_snapshot_save called before cw_reset");
    if (!e->bank) return fail(CW_ERR_STATE, "cw_snapshot_save: no bank reserved (cw_snapshot_reserve)");
    EnqueueEntry in(e, stream, CAPTURE_AWARE, LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(cwk_launch_snapshot_save(&e->P, &e->tune, &e->B, rows, (hipStream_t)stream));
    return in.done();
}

int cw_snapshot_load(cw_engine *e, const int32_t *rows, int32_t with_stream, cw_stream_t stream)
{
    if (!e || !rows) return fail(CW_ERR_INVALID, "cw_snapshot_load: null %s", !e ? "engine" : "rows");
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_snapshot_load called before cw_reset");
    if (!e->bank) return fail(CW_ERR_STATE, "cw_snapshot_load: no bank reserved (cw_snapshot_reserve)");
    EnqueueEntry in(e, stream, CAPTURE_AWARE, LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(cwk_launch_snapshot_load(&e->P, &e->tune, &e->B, rows, with_stream != 0, e->obs_mode, (hipStream_t)stream));
    return in.done();
}

// ------------------------------------------------------------------------------ expand: the six successors of every state
// a pointer as the integer the HIP-free rules of cw_host.cpp take (0: null)
static uint64_t addr(const void *p) { return (uint64_t)(uintptr_t)p; }
// a record array is read and written 16 bytes at a time (null: not given)
static int aligned16(const void *p, const char *what, const char *who)
{
    return (addr(p) & 15u) == 0 ? CW_OK : fail(CW_ERR_INVALID, "%s: %s is not 16-byte aligned", who, what);
}
// What cw_expand (max_steps 0: no steps, its own states once), cw_plan (the same, depth already checked) and cw_simulate (its own states broadcast) check alike: the HIP-free rules of cw_host.cpp
// (cwh_records_args, tested on the CPU) as the caller's error text, then the alignment of the records in and out.
static int records_args(const char *who, const cw_engine *e, const void *env_of, const void *hdr_in, const void *pos_in, int32_t n_states, int32_t n_steps,
                        int32_t max_steps, bool broadcast, int n_fields, const void *out_hdr, const void *out_pos)
{
    switch (cwh_records_args(e->n, env_of != nullptr, hdr_in != nullptr, pos_in != nullptr, n_states, n_steps, n_fields, max_steps, broadcast)) {
    case CWH_REC_OK: break;
    case CWH_REC_NO_FIELD: return fail(CW_ERR_INVALID, "%s: every field of out is null", who);
    case CWH_REC_N_STATES: return fail(CW_ERR_INVALID, "%s: n_states = %d must be 0 .. %d", who, n_states, CWH_MAX_STATES);
    case CWH_REC_N_STEPS: return fail(CW_ERR_INVALID, "%s: n_steps = %d must be 1 .. %d", who, n_steps, max_steps);
    case CWH_REC_PAIR: return fail(CW_ERR_INVALID, "%s: %s given without %s", who, hdr_in ? "hdr_in" : "slot_pos_in", hdr_in ? "slot_pos_in" : "hdr_in");
    case CWH_REC_ENV_OF: return fail(CW_ERR_INVALID, "%s: env_of given without hdr_in", who);
    default:
        return fail(CW_ERR_INVALID, "%s: n_states = %d must be %snum_envs = %d without hdr_in", who, n_states, broadcast ? "a positive multiple of " : "", e->n);
    }
    int rc = aligned16(hdr_in, "hdr_in", who);
    if (rc == CW_OK) rc = aligned16(pos_in, "slot_pos_in", who);
    if (rc == CW_OK) rc = aligned16(out_hdr, "out->hdr", who);
    if (rc == CW_OK) rc = aligned16(out_pos, "out->slot_pos", who);
    return rc;
}

// ... and what cw_export_onehot_states and cw_render_records, which require their records, check alike: the cap and the two arrays' alignment
static int states_args(const char *who, const void *hdr, const void *pos, int32_t n_states)
{
    if (n_states < 0 || n_states > CWH_MAX_STATES) return fail(CW_ERR_INVALID, "%s: n_states = %d must be 0 .. %d", who, n_states, CWH_MAX_STATES);
    const int rc = aligned16(hdr, "hdr", who);
    return rc == CW_OK ? aligned16(pos, "slot_pos", who) : rc;
}

// Only enqueues ONE kernel: no wait, no allocation, the same call whether it runs or is captured.  Writes nothing of the engine but counters[7].
int cw_expand(cw_engine *e, const int32_t *env_of, const uint8_t *hdr_in, const uint16_t *slot_pos_in, int32_t n_states, const cw_expand_out *out,
              cw_stream_t stream)
{
    if (!e || !out) return fail(CW_ERR_INVALID, "cw_expand: null %s", !e ? "engine" : "out");
    const int n_fields = !!out->reward + !!out->done + !!out->changed + !!out->achieved + !!out->hdr + !!out->slot_pos;
    const int bad = records_args("cw_expand", e, env_of, hdr_in, slot_pos_in, n_states, 0, 0, false, n_fields, out->hdr, out->slot_pos);
    if (bad != CW_OK) return bad;
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_expand called before cw_reset");
    if (n_states == 0) return CW_OK;
    EnqueueEntry in(e, stream, CAPTURE_AWARE, LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    CwExpandOut O;
    O.reward = out->reward; O.done = out->done; O.changed = out->changed; O.achieved = out->achieved;
    O.hdr = (uint4 *)out->hdr; O.pos = (uint4 *)out->slot_pos;
    const uint4 *const h = hdr_in ? (const uint4 *)hdr_in : e->P.hdr, *const p = hdr_in ? (const uint4 *)slot_pos_in : e->P.pos;
    HIP_TRY(cwk_launch_expand(&e->P, env_of, h, p, n_states, &O, (hipStream_t)stream));
    return in.done();
}

// ------------------------------------------------------------------------------ simulate: T steps of M states along the caller's action sequences
// cw_expand's shape: checks (records_args; its outputs may not overlap the records it reads), then ONE kernel.  Writes nothing of the engine but counters[7].
int cw_simulate(cw_engine *e, const int32_t *env_of, const uint8_t *hdr_in, const uint16_t *slot_pos_in, int32_t n_states, const uint8_t *actions,
                int32_t n_steps, int32_t stop_at_done, const cw_simulate_out *out, cw_stream_t stream)
{
    if (!e || !out || !actions) return fail(CW_ERR_INVALID, "cw_simulate: null %s", !e ? "engine" : !out ? "out" : "actions");
    const int n_fields = !!out->ret + !!out->length + !!out->done + !!out->achieved + !!out->hdr + !!out->slot_pos + !!out->rewards + !!out->dones;
    const int bad = records_args("cw_simulate", e, env_of, hdr_in, slot_pos_in, n_states, n_steps, CWH_SIM_MAX_STEPS, true, n_fields, out->hdr, out->slot_pos);
    if (bad != CW_OK) return bad;
    // the records the kernel reads: the caller's n_states, or the engine's own num_envs
    const uint4 *const h = hdr_in ? (const uint4 *)hdr_in : e->P.hdr, *const p = hdr_in ? (const uint4 *)slot_pos_in : e->P.pos;
    const uint64_t in_bytes = 16ull * (uint64_t)(hdr_in ? n_states : e->n), out_bytes = 16ull * (uint64_t)n_states;
    const cwh_span outs[2] = {{addr(out->hdr), out_bytes, 16}, {addr(out->slot_pos), out_bytes, 16}}, ins[2] = {{addr(h), in_bytes, 16}, {addr(p), in_bytes, 16}};
    const int clash = cwh_spans_clash(outs, 2, ins, 2, 0, nullptr);
    if (clash >= 0) return fail(CW_ERR_INVALID, "cw_simulate: out->%s overlaps the records read", clash ? "slot_pos" : "hdr");
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_simulate called before cw_reset");
    if (n_states == 0) return CW_OK;
    EnqueueEntry in(e, stream, CAPTURE_AWARE, LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    CwSimulateOut O;
    O.ret = out->ret; O.length = out->length; O.done = out->done; O.achieved = out->achieved;
    O.hdr = (uint4 *)out->hdr; O.pos = (uint4 *)out->slot_pos; O.rewards = out->rewards; O.dones = out->dones;
    HIP_TRY(cwk_launch_simulate(&e->P, env_of, h, p, hdr_in ? 0 : 1, n_states, actions, n_steps, stop_at_done ? 1 : 0, &O, (hipStream_t)stream));
    return in.done();
}

// ------------------------------------------------------------------------------ unroll: cw_simulate with every record along the way written out
// cw_simulate's shape: checks (cwh_unroll_args: cw_simulate's rules and the cap on one launch's rows; alignment; no output may share a byte with the records
// read, the actions, env_of or another output), then ONE kernel.  Writes nothing of the engine but counters[7].
int cw_unroll(cw_engine *e, const int32_t *env_of, const uint8_t *hdr_in, const uint16_t *slot_pos_in, int32_t n_states, const uint8_t *actions,
              int32_t n_steps, int32_t stop_at_done, const cw_unroll_out *out, cw_stream_t stream)
{
    if (!e || !out || !actions) return fail(CW_ERR_INVALID, "cw_unroll: null %s", !e ? "engine" : !out ? "out" : "actions");
    const int n_fields = !!out->hdr + !!out->slot_pos + !!out->reward + !!out->done + !!out->changed + !!out->taken + !!out->length;
    if (cwh_unroll_args(e->n, env_of != nullptr, hdr_in != nullptr, slot_pos_in != nullptr, n_states, n_steps, n_fields) == CWH_REC_UNROLL_ROWS)
        return fail(CW_ERR_INVALID, "cw_unroll: (n_steps + 1) = %d times n_states = %d is above %d records in one call", n_steps + 1, n_states, CWH_MAX_STATES);
    const int bad = records_args("cw_unroll", e, env_of, hdr_in, slot_pos_in, n_states, n_steps, CWH_SIM_MAX_STEPS, true, n_fields, out->hdr, out->slot_pos);
    if (bad != CW_OK) return bad;
    // the records the kernel reads: the caller's n_states, or the engine's own num_envs
    const uint4 *const h = hdr_in ? (const uint4 *)hdr_in : e->P.hdr, *const p = hdr_in ? (const uint4 *)slot_pos_in : e->P.pos;
    const uint64_t m = (uint64_t)n_states, in_bytes = 16ull * (uint64_t)(hdr_in ? n_states : e->n), steps = (uint64_t)n_steps * m, rows = steps + m;
    static const char *const out_names[7] = {"hdr", "slot_pos", "reward", "done", "changed", "taken", "length"};
    static const char *const in_names[4] = {"the records read", "the records read", "actions", "env_of"};
    const cwh_span outs[7] = {{addr(out->hdr), 16 * rows, 16}, {addr(out->slot_pos), 16 * rows, 16}, {addr(out->reward), 4 * steps, 4}, {addr(out->done), steps, 1},
                              {addr(out->changed), steps, 1}, {addr(out->taken), steps, 1}, {addr(out->length), 4 * m, 4}};
    const cwh_span ins[4] = {{addr(h), in_bytes, 16}, {addr(p), in_bytes, 16}, {addr(actions), steps, 1}, {addr(env_of), 4 * m, 4}};
    int at = cwh_spans_misaligned(outs, 7);
    if (at >= 0) return fail(CW_ERR_INVALID, "cw_unroll: out->%s is not %d-byte aligned", out_names[at], (int)outs[at].align);
    if (cwh_spans_misaligned(ins, 4) >= 0) return fail(CW_ERR_INVALID, "cw_unroll: env_of is not 4-byte aligned");      // (the records: records_args)
    int other = 0;
    at = cwh_spans_clash(outs, 7, ins, 4, 1, &other);
    if (at >= 0) return fail(CW_ERR_INVALID, "cw_unroll: out->%s overlaps %s%s", out_names[at], other < 4 ? "" : "out->", other < 4 ? in_names[other] : out_names[other - 4]);
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_unroll called before cw_reset");
    if (n_states == 0) return CW_OK;
    EnqueueEntry in(e, stream, CAPTURE_AWARE, LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    CwUnrollOut O;
    O.hdr = (uint4 *)out->hdr; O.pos = (uint4 *)out->slot_pos; O.reward = out->reward; O.done = out->done; O.changed = out->changed; O.taken = out->taken;
    O.length = out->length;
    HIP_TRY(cwk_launch_unroll(&e->P, env_of, h, p, hdr_in ? 0 : 1, n_states, actions, n_steps, stop_at_done ? 1 : 0, &O, (hipStream_t)stream));
    return in.done();
}

// ------------------------------------------------------------------------------ plan: the best return within `depth` steps after each first action
// cw_expand's shape: checks (cwh_plan_args: cw_expand's rules, the depth and the cap on one launch's work), then ONE kernel.  Writes nothing of the engine
// but counters[7].
int cw_plan(cw_engine *e, const int32_t *env_of, const uint8_t *hdr_in, const uint16_t *slot_pos_in, int32_t n_states, int32_t depth, const cw_plan_out *out,
            cw_stream_t stream)
{
    if (!e || !out) return fail(CW_ERR_INVALID, "cw_plan: null %s", !e ? "engine" : "out");
    const int n_fields = !!out->q + !!out->length + !!out->done + !!out->achieved + !!out->hdr + !!out->slot_pos + !!out->plan;
    switch (cwh_plan_args(e->n, env_of != nullptr, hdr_in != nullptr, slot_pos_in != nullptr, n_states, depth, n_fields)) {
    case CWH_REC_N_STEPS: return fail(CW_ERR_INVALID, "cw_plan: depth = %d must be 1 .. %d", depth, CWH_PLAN_MAX_DEPTH);
    case CWH_REC_PLAN_WORK: return fail(CW_ERR_INVALID, "cw_plan: n_states = %d times 6^depth = 6^%d is above 2^32 plans in one call", n_states, depth);
    default: break;
    }
    const int bad = records_args("cw_plan", e, env_of, hdr_in, slot_pos_in, n_states, depth, CWH_PLAN_MAX_DEPTH, false, n_fields, out->hdr, out->slot_pos);
    if (bad != CW_OK) return bad;
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_plan called before cw_reset");
    if (n_states == 0) return CW_OK;
    EnqueueEntry in(e, stream, CAPTURE_AWARE, LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    CwPlanOut O;
    O.q = out->q; O.length = out->length; O.done = out->done; O.achieved = out->achieved;
    O.hdr = (uint4 *)out->hdr; O.pos = (uint4 *)out->slot_pos; O.plan = out->plan;
    const uint4 *const h = hdr_in ? (const uint4 *)hdr_in : e->P.hdr, *const p = hdr_in ? (const uint4 *)slot_pos_in : e->P.pos;
    HIP_TRY(cwk_launch_plan(&e->P, env_of, h, p, n_states, depth, &O, (hipStream_t)stream));
    return in.done();
}

// ------------------------------------------------------------------------------ shoot: the best of n_samples drawn plans of n_steps steps per state
// cw_plan's shape: checks (cwh_shoot_args: cw_plan's rules on the records, the steps, the samples and the cap on one launch's work; the large outputs may
// overlap neither the records read nor the weights), then ONE kernel.  Writes nothing of the engine but counters[7].
int cw_shoot(cw_engine *e, const int32_t *env_of, const uint8_t *hdr_in, const uint16_t *slot_pos_in, int32_t n_states, int32_t n_steps, int32_t n_samples,
             uint64_t seed, const uint64_t *seed_dev, const uint16_t *weights, const cw_shoot_out *out, cw_stream_t stream)
{
    if (!e || !out) return fail(CW_ERR_INVALID, "cw_shoot: null %s", !e ? "engine" : "out");
    const int n_fields = !!out->best_ret + !!out->best_sample + !!out->best_action + !!out->length + !!out->done + !!out->achieved + !!out->hdr +
                         !!out->slot_pos + !!out->plan + !!out->ret;
    switch (cwh_shoot_args(e->n, env_of != nullptr, hdr_in != nullptr, slot_pos_in != nullptr, n_states, n_steps, n_samples, n_fields)) {
    case CWH_REC_SHOOT_SAMPLES: return fail(CW_ERR_INVALID, "cw_shoot: n_samples = %d must be 1 .. %d", n_samples, CWH_SHOOT_MAX_SAMPLES);
    case CWH_REC_SHOOT_WORK:
        return fail(CW_ERR_INVALID, "cw_shoot: n_states = %d times n_samples = %d times n_steps = %d is above 2^32 steps in one call", n_states, n_samples, n_steps);
    default: break;
    }
    const int bad = records_args("cw_shoot", e, env_of, hdr_in, slot_pos_in, n_states, n_steps, CWH_SIM_MAX_STEPS, false, n_fields, out->hdr, out->slot_pos);
    if (bad != CW_OK) return bad;
    const uint4 *const h = hdr_in ? (const uint4 *)hdr_in : e->P.hdr, *const p = hdr_in ? (const uint4 *)slot_pos_in : e->P.pos;
    const uint64_t m = (uint64_t)n_states, rec_bytes = 16ull * m, w_bytes = weights ? 12ull * (uint64_t)n_steps * m : 0;
    static const char *const names[4] = {"hdr", "slot_pos", "plan", "ret"};
    const cwh_span outs[4] = {{addr(out->hdr), rec_bytes, 16}, {addr(out->slot_pos), rec_bytes, 16}, {addr(out->plan), (uint64_t)n_steps * m, 1},
                              {addr(out->ret), 4ull * (uint64_t)n_samples * m, 4}};
    const cwh_span ins[3] = {{addr(h), rec_bytes, 16}, {addr(p), rec_bytes, 16}, {addr(weights), w_bytes, 2}};
    int other = 0;
    const int clash = cwh_spans_clash(outs, 4, ins, 3, 0, &other);
    if (clash >= 0) return fail(CW_ERR_INVALID, "cw_shoot: out->%s overlaps the %s", names[clash], other < 2 ? "records read" : "weights");
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_shoot called before cw_reset");
    if (n_states == 0) return CW_OK;
    EnqueueEntry in(e, stream, CAPTURE_AWARE, LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    CwShootOut O;
    O.best_ret = out->best_ret; O.best_sample = out->best_sample; O.best_action = out->best_action; O.length = out->length; O.done = out->done;
    O.achieved = out->achieved; O.hdr = (uint4 *)out->hdr; O.pos = (uint4 *)out->slot_pos; O.plan = out->plan; O.ret = out->ret;
    HIP_TRY(cwk_launch_shoot(&e->P, env_of, h, p, n_states, n_steps, n_samples, (unsigned long long)seed, (const unsigned long long *)seed_dev, weights, &O,
                             (hipStream_t)stream));
    return in.done();
}

// ... and the draws themselves: the engine contributes its stream bookkeeping and the has_reset rule, nothing of it is read by the kernel
int cw_shoot_actions(cw_engine *e, int32_t n_states, int32_t n_steps, uint64_t seed, const uint64_t *seed_dev, const uint16_t *weights, const int32_t *samples,
                     int32_t n_rows, uint8_t *out, cw_stream_t stream)
{
    if (!e || !out) return fail(CW_ERR_INVALID, "cw_shoot_actions: null %s", !e ? "engine" : "out");
    switch (cwh_shoot_actions_args(n_states, n_steps, n_rows)) {
    case CWH_REC_OK: break;
    case CWH_REC_N_STATES: return fail(CW_ERR_INVALID, "cw_shoot_actions: n_states = %d must be 0 .. %d", n_states, CWH_MAX_STATES);
    case CWH_REC_SHOOT_SAMPLES: return fail(CW_ERR_INVALID, "cw_shoot_actions: n_rows = %d must be 0 .. %d", n_rows, CWH_MAX_STATES);
    case CWH_REC_N_STEPS: return fail(CW_ERR_INVALID, "cw_shoot_actions: n_steps = %d must be 1 .. %d", n_steps, CWH_SIM_MAX_STEPS);
    default:
        return fail(CW_ERR_INVALID, "cw_shoot_actions: n_rows = %d times n_states = %d times n_steps = %d is above 2^32 actions in one call", n_rows, n_states, n_steps);
    }
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_shoot_actions called before cw_reset");
    if (n_states == 0 || n_rows == 0) return CW_OK;
    EnqueueEntry in(e, stream, CAPTURE_AWARE, LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(cwk_launch_shoot_actions(n_states, n_steps, n_rows, (unsigned long long)seed, (const unsigned long long *)seed_dev, weights, samples, out,
                                     (hipStream_t)stream));
    return in.done();
}

// ... and the refit, the other half of a CEM iteration: checks (cwh_refit_args), then the selection kernel and -- when weights are asked for -- the count
// kernel.  The engine contributes its stream bookkeeping and the has_reset rule; the kernels read num_envs for the env_of test and nothing else of it.
int cw_shoot_refit(cw_engine *e, const int32_t *env_of, int32_t n_states, int32_t n_steps, int32_t n_samples, int32_t n_elites, uint64_t seed,
                   const uint64_t *seed_dev, const uint16_t *weights_in, const int32_t *ret, uint32_t smooth, uint32_t gain, const cw_refit_out *out,
                   cw_stream_t stream)
{
    if (!e || !out) return fail(CW_ERR_INVALID, "cw_shoot_refit: null %s", !e ? "engine" : "out");
    switch (cwh_refit_args(addr(env_of), n_states, n_steps, n_samples, n_elites, addr(weights_in), addr(ret), smooth, gain, addr(out->elites), addr(out->weights),
                           addr(out->elite_min))) {
    case CWH_REFIT_OK: break;
    case CWH_REFIT_NULL: return fail(CW_ERR_INVALID, "cw_shoot_refit: null %s", !ret ? "ret" : "out->elites");
    case CWH_REFIT_N_STATES: return fail(CW_ERR_INVALID, "cw_shoot_refit: n_states = %d must be 0 .. %d", n_states, CWH_MAX_STATES);
    case CWH_REFIT_N_STEPS: return fail(CW_ERR_INVALID, "cw_shoot_refit: n_steps = %d must be 1 .. %d", n_steps, CWH_SIM_MAX_STEPS);
    case CWH_REFIT_N_SAMPLES: return fail(CW_ERR_INVALID, "cw_shoot_refit: n_samples = %d must be 1 .. %d", n_samples, CWH_SHOOT_MAX_SAMPLES);
    case CWH_REFIT_N_ELITES: return fail(CW_ERR_INVALID, "cw_shoot_refit: n_elites = %d must be 1 .. n_samples = %d", n_elites, n_samples);
    case CWH_REFIT_WORK:
        return fail(CW_ERR_INVALID, "cw_shoot_refit: n_states = %d times n_samples = %d times n_steps = %d is above 2^32 steps in one call", n_states, n_samples,
                    n_steps);
    case CWH_REFIT_SMOOTH: return fail(CW_ERR_INVALID, "cw_shoot_refit: smooth = %u must be 0 .. 65535", smooth);
    case CWH_REFIT_GAIN: return fail(CW_ERR_INVALID, "cw_shoot_refit: gain = %u must be 1 .. 65535", gain);
    case CWH_REFIT_ALIGN: return fail(CW_ERR_INVALID, "cw_shoot_refit: env_of, ret, out->elites and out->elite_min must be 4-byte, the weights 2-byte aligned");
    default:
        return fail(CW_ERR_INVALID, "cw_shoot_refit: an output overlaps ret, env_of, another output or weights_in (out->weights == weights_in, in place, is legal)");
    }
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_shoot_refit called before cw_reset");
    if (n_states == 0) return CW_OK;
    EnqueueEntry in(e, stream, CAPTURE_AWARE, LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(cwk_launch_refit(&e->P, &e->tune, env_of, n_states, n_steps, n_samples, n_elites, (unsigned long long)seed, (const unsigned long long *)seed_dev,
                             weights_in, ret, smooth, gain, out->elites, out->weights, out->elite_min, (hipStream_t)stream));
    return in.done();
}

// ------------------------------------------------------------------------------ replay: transitions as packed records, relabelled minibatches
// A Region of the engine's, as far from every checkpoint blob and snapshot row as the others; its sections are cw_host.cpp's (cwh_replay_layout).
// A reserve drops everything stored: the new buffer is zero-filled and cleared before the call returns.
int cw_replay_reserve(cw_engine *e, int32_t steps)
{
    if (!e) return fail(CW_ERR_INVALID, "cw_replay_reserve: null engine");
    uint64_t at[CWH_REPLAY_SECTIONS];
    const int64_t bytes = steps == 0 ? 0 : cwh_replay_layout(steps, e->n, at);
    if (bytes < 0)
        return fail(CW_ERR_INVALID, "cw_replay_reserve: steps = %d must be 0 .. %d with steps * num_envs (%d) below 2^31", steps, CWH_REPLAY_MAX_STEPS, e->n);
    SyncEntry in(e);                                 // (the engine's own work: a push or a sample in flight uses the buffer about to go)
    if (in.rc != CW_OK) return in.rc;
    region_free(e->replay);
    e->Rp = CwReplay{};
    if (steps == 0) return CW_OK;
    NewRegion nr;
    if (!nr.alloc((size_t)bytes))
        return fail(CW_ERR_HIP, "cw_replay_reserve: no device memory for %d steps of %d envs (%lld bytes)", steps, e->n, (long long)bytes);
    CwReplay R{};
    R.ctl = (unsigned long long *)nr.at(at[CWH_REPLAY_S_CTL]);
    R.env_episode = (uint32_t *)nr.at(at[CWH_REPLAY_S_ENV_EPISODE]);
    R.hdr = (uint4 *)nr.at(at[CWH_REPLAY_S_HDR]);
    R.pos = (uint4 *)nr.at(at[CWH_REPLAY_S_POS]);
    R.next_hdr = (uint4 *)nr.at(at[CWH_REPLAY_S_NEXT_HDR]);
    R.next_pos = (uint4 *)nr.at(at[CWH_REPLAY_S_NEXT_POS]);
    R.goal_hdr = (uint4 *)nr.at(at[CWH_REPLAY_S_GOAL_HDR]);
    R.goal_pos = (uint4 *)nr.at(at[CWH_REPLAY_S_GOAL_POS]);
    R.reward = (int32_t *)nr.at(at[CWH_REPLAY_S_REWARD]);
    R.episode = (uint32_t *)nr.at(at[CWH_REPLAY_S_EPISODE]);
    R.action = (uint8_t *)nr.at(at[CWH_REPLAY_S_ACTION]);
    R.flags = (uint8_t *)nr.at(at[CWH_REPLAY_S_FLAGS]);
    R.steps = steps;
    if (hipMemsetAsync(nr.r.base, 0, nr.r.bytes, e->aux) != hipSuccess || cwk_launch_replay_clear(&e->P, &e->tune, &R, e->aux) != hipSuccess ||
        hipStreamSynchronize(e->aux) != hipSuccess) {
        (void)hipGetLastError();
        return fail(CW_ERR_HIP, "cw_replay_reserve: clearing the buffer failed");
    }
    e->replay = nr.commit();
    e->Rp = R;
    return CW_OK;
}

size_t cw_replay_bytes(const cw_engine *e)
{
    if (!e) { (void)fail(CW_ERR_INVALID, "cw_replay_bytes: null engine"); return 0; }
    return e->replay.bytes;
}

int cw_replay_buffers(cw_engine *e, cw_replay_table *out)
{
    if (!e || !out) return fail(CW_ERR_INVALID, "cw_replay_buffers: null %s", !e ? "engine" : "out");
    if (!e->replay) return fail(CW_ERR_STATE, "cw_replay_buffers: no buffer reserved (cw_replay_reserve)");
    const CwReplay &R = e->Rp;
    out->hdr = (const uint8_t *)R.hdr;
    out->slot_pos = (const uint16_t *)R.pos;
    out->next_hdr = (const uint8_t *)R.next_hdr;
    out->next_slot_pos = (const uint16_t *)R.next_pos;
    out->goal_hdr = (const uint8_t *)R.goal_hdr;
    out->goal_slot_pos = (const uint16_t *)R.goal_pos;
    out->action = R.action;
    out->flags = R.flags;
    out->reward = R.reward;
    out->episode = R.episode;
    out->env_episode = R.env_episode;
    out->n = (const uint64_t *)R.ctl;
    out->steps = R.steps;
    out->num_envs = e->n;
    return CW_OK;
}

// Only enqueues ONE kernel: no wait, no allocation, the same call whether it runs or is captured.
int cw_replay_clear(cw_engine *e, cw_stream_t stream)
{
    if (!e) return fail(CW_ERR_INVALID, "cw_replay_clear: null engine");
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_replay_clear called before cw_reset");
    if (!e->replay) return fail(CW_ERR_STATE, "cw_replay_clear: no buffer reserved (cw_replay_reserve)");
    EnqueueEntry in(e, stream, CAPTURE_AWARE, LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(cwk_launch_replay_clear(&e->P, &e->tune, &e->Rp, (hipStream_t)stream));
    return in.done();
}

// cw_step's argument rules, then the push and the one-lane launch that advances n.  Of the engine only the buffer is written.
int cw_replay_push(cw_engine *e, const void *actions, int action_dtype, cw_stream_t stream)
{
    if (!e || !actions) return fail(CW_ERR_INVALID, "cw_replay_push: null argument");
    if (action_dtype < CW_ACT_I32 || action_dtype > CW_ACT_U8) return fail(CW_ERR_INVALID, "cw_replay_push: bad action dtype %d", action_dtype);
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_replay_push called before cw_reset");
    if (!e->replay) return fail(CW_ERR_STATE, "cw_replay_push: no buffer reserved (cw_replay_reserve)");
    EnqueueEntry in(e, stream, CAPTURE_AWARE, LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(cwk_launch_replay_push(&e->P, &e->Rp, actions, action_dtype, (hipStream_t)stream));
    return in.done();
}

// Checks (cwh_replay_sample_args, tested on the CPU), then ONE kernel.  Nothing of the engine is written.
int cw_replay_sample(cw_engine *e, int32_t n_rows, uint64_t seed, const uint64_t *seed_dev, uint32_t her, int32_t strategy, const cw_replay_out *out,
                     cw_stream_t stream)
{
    if (!e || !out) return fail(CW_ERR_INVALID, "cw_replay_sample: null %s", !e ? "engine" : "out");
    const uint64_t fields[CWH_REPLAY_FIELDS] = {addr(out->hdr), addr(out->slot_pos), addr(out->next_hdr), addr(out->next_slot_pos), addr(out->goal_hdr),
                                                addr(out->goal_slot_pos), addr(out->action), addr(out->reward), addr(out->done), addr(out->desired), addr(out->env),
                                                addr(out->slot), addr(out->future)};
    switch (cwh_replay_sample_args(n_rows, her, strategy, fields)) {
    case CWH_REPLAY_OK: break;
    case CWH_REPLAY_N_ROWS: return fail(CW_ERR_INVALID, "cw_replay_sample: n_rows = %d must be 0 .. %d", n_rows, CWH_MAX_STATES);
    case CWH_REPLAY_HER: return fail(CW_ERR_INVALID, "cw_replay_sample: her = %u must be 0 .. 65536", her);
    case CWH_REPLAY_STRATEGY: return fail(CW_ERR_INVALID, "cw_replay_sample: strategy = %d must be 0 (future) or 1 (final)", strategy);
    case CWH_REPLAY_NO_FIELD: return fail(CW_ERR_INVALID, "cw_replay_sample: every field of out is null");
    case CWH_REPLAY_ALIGN:
        return fail(CW_ERR_INVALID, "cw_replay_sample: the record fields must be 16-byte, reward / env / slot / future 4-byte and desired 2-byte aligned");
    default: return fail(CW_ERR_INVALID, "cw_replay_sample: two fields of out overlap");
    }
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_replay_sample called before cw_reset");
    if (!e->replay) return fail(CW_ERR_STATE, "cw_replay_sample: no buffer reserved (cw_replay_reserve)");
    if (n_rows == 0) return CW_OK;
    EnqueueEntry in(e, stream, CAPTURE_AWARE, LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    CwReplayOut O{};
    O.hdr = (uint4 *)out->hdr; O.pos = (uint4 *)out->slot_pos; O.next_hdr = (uint4 *)out->next_hdr; O.next_pos = (uint4 *)out->next_slot_pos;
    O.goal_hdr = (uint4 *)out->goal_hdr; O.goal_pos = (uint4 *)out->goal_slot_pos; O.action = out->action; O.reward = out->reward; O.done = out->done;
    O.desired = out->desired; O.env = out->env; O.slot = out->slot; O.future = out->future;
    HIP_TRY(cwk_launch_replay_sample(&e->P, &e->tune, &e->Rp, n_rows, (unsigned long long)seed, (const unsigned long long *)seed_dev, her, strategy, &O,
                                     (hipStream_t)stream));
    return in.done();
}

// ------------------------------------------------------------------------------ seen: the visited set of packed records
// A Region of the engine's, as far from every checkpoint blob and snapshot row as the others; its sections are cw_host.cpp's (cwh_seen_layout: the control
// block, then the tags, the owners and the two halves of the stored keys, 48 bytes a slot).  A reserve drops everything seen: the new set is cleared before the call returns.
int cw_seen_reserve(cw_engine *e, int64_t capacity, int32_t tag_bits)
{
    if (!e) return fail(CW_ERR_INVALID, "cw_seen_reserve: null engine");
    const int64_t slots = cwh_seen_slots_of(capacity);
    if (slots < 0) return fail(CW_ERR_INVALID, "cw_seen_reserve: capacity = %lld must be 0 .. %lld", (long long)capacity, (long long)CWH_SEEN_MAX_CAPACITY);
    if (tag_bits < 0 || tag_bits > 63) return fail(CW_ERR_INVALID, "cw_seen_reserve: tag_bits = %d must be 0 (the full hash) .. 63", tag_bits);
    SyncEntry in(e);                                 // (the engine's own work: an insert in flight uses the set about to go)
    if (in.rc != CW_OK) return in.rc;
    region_free(e->seen);
    e->Sn = CwSeen{};
    e->seen_slots = 0;
    if (slots == 0) return CW_OK;
    uint64_t at[CWH_SEEN_SECTIONS];
    const int64_t bytes = cwh_seen_layout(slots, at);
    NewRegion nr;
    if (!nr.alloc((size_t)bytes)) return fail(CW_ERR_HIP, "cw_seen_reserve: no device memory for %lld slots of 48 bytes", (long long)slots);
    CwSeen S{};
    S.ctl = (unsigned long long *)nr.at(at[CWH_SEEN_S_CTL]);
    S.tag = (unsigned long long *)nr.at(at[CWH_SEEN_S_TAG]);
    S.owner = (unsigned long long *)nr.at(at[CWH_SEEN_S_OWNER]);
    S.key_a = (uint4 *)nr.at(at[CWH_SEEN_S_KEY_A]);
    S.key_b = (uint4 *)nr.at(at[CWH_SEEN_S_KEY_B]);
    S.mask = (uint32_t)(slots - 1);
    S.probes = slots < CWH_SEEN_PROBES ? (int32_t)slots : CWH_SEEN_PROBES;
    S.tag_bits = tag_bits;
    if (cwk_launch_seen_clear(&e->tune, &S, e->aux) != hipSuccess || hipStreamSynchronize(e->aux) != hipSuccess) {
        (void)hipGetLastError();
        return fail(CW_ERR_HIP, "cw_seen_reserve: clearing the set failed");
    }
    e->seen = nr.commit();
    e->Sn = S;
    e->seen_slots = slots;
    return CW_OK;
}

size_t cw_seen_slots(const cw_engine *e)
{
    if (!e) { (void)fail(CW_ERR_INVALID, "cw_seen_slots: null engine"); return 0; }
    return e->seen ? (size_t)e->seen_slots : 0;
}

int cw_seen_counters(const cw_engine *e, const uint64_t **counters)
{
    if (!e || !counters) return fail(CW_ERR_INVALID, "cw_seen_counters: null %s", !e ? "engine" : "counters");
    *counters = e->seen ? (const uint64_t *)e->Sn.ctl : nullptr;
    return e->seen ? CW_OK : fail(CW_ERR_STATE, "cw_seen_counters: no set reserved (cw_seen_reserve)");
}

// Only enqueues ONE kernel: no wait, no allocation, the same call whether it runs or is captured.
int cw_seen_clear(cw_engine *e, cw_stream_t stream)
{
    if (!e) return fail(CW_ERR_INVALID, "cw_seen_clear: null engine");
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_seen_clear called before cw_reset");
    if (!e->seen) return fail(CW_ERR_STATE, "cw_seen_clear: no set reserved (cw_seen_reserve)");
    EnqueueEntry in(e, stream, CAPTURE_AWARE, LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(cwk_launch_seen_clear(&e->tune, &e->Sn, (hipStream_t)stream));
    return in.done();
}

// Checks (cwh_seen_args, tested on the CPU), then TWO kernels.  Of the engine only the set is written.
int cw_seen_insert(cw_engine *e, const int32_t *group, const uint8_t *hdr, const uint16_t *slot_pos, int32_t n_states, const cw_seen_out *out, cw_stream_t stream)
{
    if (!e || !out) return fail(CW_ERR_INVALID, "cw_seen_insert: null %s", !e ? "engine" : "out");
    switch (cwh_seen_args(addr(group), addr(hdr), addr(slot_pos), n_states, addr(out->fresh), addr(out->first))) {
    case CWH_SEEN_OK: break;
    case CWH_SEEN_NO_RECORDS: return fail(CW_ERR_INVALID, "cw_seen_insert: null %s", !hdr ? "hdr" : "slot_pos");
    case CWH_SEEN_NO_FIELD: return fail(CW_ERR_INVALID, "cw_seen_insert: every field of out is null");
    case CWH_SEEN_N_STATES: return fail(CW_ERR_INVALID, "cw_seen_insert: n_states = %d must be 0 .. %d", n_states, CWH_MAX_STATES);
    case CWH_SEEN_ALIGN: return fail(CW_ERR_INVALID, "cw_seen_insert: hdr / slot_pos must be 16-byte aligned, group / out->first 4-byte aligned");
    default: return fail(CW_ERR_INVALID, "cw_seen_insert: an output overlaps the records, group or the other output");
    }
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_seen_insert called before cw_reset");
    if (!e->seen) return fail(CW_ERR_STATE, "cw_seen_insert: no set reserved (cw_seen_reserve)");
    if (n_states == 0) return CW_OK;
    EnqueueEntry in(e, stream, CAPTURE_AWARE, LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(cwk_launch_seen_insert(&e->P, &e->tune, &e->Sn, group, (const uint4 *)hdr, (const uint4 *)slot_pos, n_states, out->fresh, out->first,
                                   (hipStream_t)stream));
    return in.done();
}

// ------------------------------------------------------------------------------ load records: packed records into envs
// Checks (cwh_load_records_args, tested on the CPU), then ONE kernel: no wait, no allocation, the same call whether it runs or is captured.
int cw_load_records(cw_engine *e, const int32_t *src, const uint8_t *hdr, const uint16_t *slot_pos, int32_t n_records, uint8_t *status, cw_stream_t stream)
{
    if (!e) return fail(CW_ERR_INVALID, "cw_load_records: null engine");
    switch (cwh_load_records_args(e->n, addr(src), addr(hdr), addr(slot_pos), n_records, addr(status), addr(e->P.hdr), addr(e->P.pos))) {
    case CWH_LOAD_OK: break;
    case CWH_LOAD_NO_RECORDS: return fail(CW_ERR_INVALID, "cw_load_records: null %s", !hdr ? "hdr" : "slot_pos");
    case CWH_LOAD_N_RECORDS: return fail(CW_ERR_INVALID, "cw_load_records: n_records = %d must be 0 .. %d", n_records, CWH_MAX_STATES);
    case CWH_LOAD_OWN_ORDER: return fail(CW_ERR_INVALID, "cw_load_records: n_records = %d must be num_envs = %d without src", n_records, e->n);
    case CWH_LOAD_ALIGN: return fail(CW_ERR_INVALID, "cw_load_records: hdr / slot_pos must be 16-byte aligned, src 4-byte aligned");
    case CWH_LOAD_ENGINE_OVERLAP: return fail(CW_ERR_INVALID, "cw_load_records: the records overlap the engine's own hdr / slot_pos buffers (clone them first)");
    default: return fail(CW_ERR_INVALID, "cw_load_records: status overlaps the records or src");
    }
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_load_records called before cw_reset");
    if (n_records == 0) return CW_OK;
    EnqueueEntry in(e, stream, CAPTURE_AWARE, LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(cwk_launch_load_records(&e->P, &e->tune, src, (const uint4 *)hdr, (const uint4 *)slot_pos, n_records, status, e->obs_mode, (hipStream_t)stream));
    return in.done();
}

// ------------------------------------------------------------------------------ reach: breadth-first search without a host round trip
// The workspace is a Region of the engine's, as far from every checkpoint blob and snapshot row as the others; its sections are cw_host.cpp's
// (cwh_reach_layout).  Nothing of it needs an initial value: every call writes what it reads.
int cw_reach_reserve(cw_engine *e, int64_t max_rows, int32_t max_depth)
{
    if (!e) return fail(CW_ERR_INVALID, "cw_reach_reserve: null engine");
    uint64_t at[CWH_REACH_SECTIONS];
    const int64_t bytes = max_rows == 0 ? 0 : cwh_reach_layout(max_rows, max_depth, at);
    if (bytes < 0)
        return fail(CW_ERR_INVALID, "cw_reach_reserve: max_rows = %lld must be 0 .. %lld and max_depth = %d 1 .. %d", (long long)max_rows,
                    (long long)CWH_REACH_MAX_ROWS, max_depth, CWH_REACH_MAX_DEPTH);
    SyncEntry in(e);                                 // (the engine's own work: a search in flight uses the workspace about to go)
    if (in.rc != CW_OK) return in.rc;
    region_free(e->reach);
    e->Rc = CwReach{};
    if (bytes == 0) return CW_OK;
    NewRegion nr;
    if (!nr.alloc((size_t)bytes))
        return fail(CW_ERR_HIP, "cw_reach_reserve: no device memory for %lld bytes (%lld rows, %d levels)", (long long)bytes, (long long)max_rows, max_depth);
    CwReach R{};
    R.ctl = (int32_t *)nr.at(at[CWH_REACH_S_CTL]);
    R.sizes = R.ctl + CWH_REACH_CTL_WORDS;
    R.chunk = R.sizes + max_depth + 1;
    for (int k = 0; k < 2; k++) {
        R.f_hdr[k] = (uint4 *)nr.at(at[CWH_REACH_S_F_HDR0 + 4 * k]);
        R.f_pos[k] = (uint4 *)nr.at(at[CWH_REACH_S_F_POS0 + 4 * k]);
        R.f_env[k] = (int32_t *)nr.at(at[CWH_REACH_S_F_ENV0 + 4 * k]);
        R.f_start[k] = (int32_t *)nr.at(at[CWH_REACH_S_F_START0 + 4 * k]);
    }
    R.s_hdr = (uint4 *)nr.at(at[CWH_REACH_S_HDR]);
    R.s_pos = (uint4 *)nr.at(at[CWH_REACH_S_POS]);
    R.s_grp = (int32_t *)nr.at(at[CWH_REACH_S_GRP]);
    R.s_fresh = (uint8_t *)nr.at(at[CWH_REACH_S_FRESH]);
    R.links = (int32_t *)nr.at(at[CWH_REACH_S_LINKS]);
    R.dist = (int32_t *)nr.at(at[CWH_REACH_S_DIST]);
    R.sol = (int32_t *)nr.at(at[CWH_REACH_S_SOL]);
    R.bid = (int32_t *)nr.at(at[CWH_REACH_S_BID]);
    R.active = (uint8_t *)nr.at(at[CWH_REACH_S_ACTIVE]);
    R.max_rows = (int32_t)max_rows;
    R.max_depth = max_depth;
    e->reach = nr.commit();
    e->Rc = R;
    return CW_OK;
}

size_t cw_reach_bytes(const cw_engine *e)
{
    if (!e) { (void)fail(CW_ERR_INVALID, "cw_reach_bytes: null engine"); return 0; }
    return e->reach.bytes;
}

// Checks (cwh_reach_args, tested on the CPU), then kernels only: no wait, no allocation, the same call whether it runs or is captured.  Of the engine the
// set and the workspace are written, nothing else: a start row whose env index is outside the batch takes no part and is NOT counted in counters[7].
int cw_reach(cw_engine *e, const int32_t *env_of, const uint8_t *hdr_in, const uint16_t *slot_pos_in, int32_t n_states, int32_t max_depth, const cw_reach_out *out,
             cw_stream_t stream)
{
    if (!e || !out) return fail(CW_ERR_INVALID, "cw_reach: null %s", !e ? "engine" : "out");
    switch (cwh_reach_args(e->n, addr(env_of), addr(hdr_in), addr(slot_pos_in), n_states, max_depth, addr(out->distance), addr(out->plan),
                           addr(out->first_action), addr(out->frontier), addr(out->searched_depth))) {
    case CWH_REACH_OK: break;
    case CWH_REACH_NO_FIELD: return fail(CW_ERR_INVALID, "cw_reach: every field of out is null");
    case CWH_REACH_N_STATES: return fail(CW_ERR_INVALID, "cw_reach: n_states = %d must be 0 .. %lld", n_states, (long long)CWH_REACH_MAX_ROWS);
    case CWH_REACH_DEPTH: return fail(CW_ERR_INVALID, "cw_reach: max_depth = %d must be 1 .. %d", max_depth, CWH_REACH_MAX_DEPTH);
    case CWH_REACH_PAIR: return fail(CW_ERR_INVALID, "cw_reach: hdr_in and slot_pos_in go together");
    case CWH_REACH_ENV_OF: return fail(CW_ERR_INVALID, "cw_reach: env_of needs hdr_in and slot_pos_in");
    case CWH_REACH_OWN_STATES: return fail(CW_ERR_INVALID, "cw_reach: n_states = %d must be num_envs = %d without records", n_states, e->n);
    case CWH_REACH_ALIGN:
        return fail(CW_ERR_INVALID, "cw_reach: hdr_in / slot_pos_in must be 16-byte aligned, env_of / out->distance / frontier / searched_depth 4-byte aligned");
    default: return fail(CW_ERR_INVALID, "cw_reach: an output overlaps the records, env_of or another output");
    }
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_reach called before cw_reset");
    if (!e->seen) return fail(CW_ERR_STATE, "cw_reach: no set reserved (cw_seen_reserve)");
    if (!e->reach) return fail(CW_ERR_STATE, "cw_reach: no workspace reserved (cw_reach_reserve)");
    if (n_states > e->Rc.max_rows || max_depth > e->Rc.max_depth)
        return fail(CW_ERR_STATE, "cw_reach: n_states = %d, max_depth = %d, the workspace holds %d rows and %d levels (cw_reach_reserve)", n_states, max_depth,
                    e->Rc.max_rows, e->Rc.max_depth);
    EnqueueEntry in(e, stream, CAPTURE_AWARE, LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    CwReachOut O;
    O.distance = out->distance; O.plan = out->plan; O.first_action = out->first_action; O.frontier = out->frontier; O.searched_depth = out->searched_depth;
    const uint4 *const h = hdr_in ? (const uint4 *)hdr_in : e->P.hdr, *const p = hdr_in ? (const uint4 *)slot_pos_in : e->P.pos;
    HIP_TRY(cwk_launch_reach(&e->P, &e->tune, &e->Sn, &e->Rc, env_of, h, p, n_states, max_depth, &O, (hipStream_t)stream));
    return in.done();
}

int cw_export_onehot_states(cw_engine *e, const uint8_t *hdr, const uint16_t *slot_pos, int32_t n_states, uint8_t *out, cw_stream_t stream)
{
    if (!e || !hdr || !slot_pos || !out)
        return fail(CW_ERR_INVALID, "cw_export_onehot_states: null %s", !e ? "engine" : !hdr ? "hdr" : !slot_pos ? "slot_pos" : "out");
    const int bad = states_args("cw_export_onehot_states", hdr, slot_pos, n_states);
    if (bad != CW_OK) return bad;
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_export_onehot_states called before cw_reset");
    if (n_states == 0) return CW_OK;
    EnqueueEntry in(e, stream, CAPTURE_AWARE, LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(cwk_launch_export_onehot_states(&e->P, &e->tune, (const uint4 *)hdr, (const uint4 *)slot_pos, n_states, out, (hipStream_t)stream));
    return in.done();
}

// ------------------------------------------------------------------------------ render_records: the frames of packed records, straight from the records
// cw_export_onehot_states' shape: checks, then ONE kernel.  PURE: of the engine only size and raster are read, nothing of it is written (no counter either).
int cw_render_records(cw_engine *e, const uint8_t *hdr, const uint16_t *slot_pos, const uint8_t *mask, int32_t n_states, uint8_t *out_frames,
                      cw_stream_t stream)
{
    if (!e || !hdr || !slot_pos || !out_frames)
        return fail(CW_ERR_INVALID, "cw_render_records: null %s", !e ? "engine" : !hdr ? "hdr" : !slot_pos ? "slot_pos" : "out_frames");
    const int bad = states_args("cw_render_records", hdr, slot_pos, n_states);
    if (bad != CW_OK) return bad;
    const uint64_t m = (uint64_t)n_states;
    // (4-byte aligned for the Ray painter's 12-byte stores; AltObs frames start at every alignment anyway)
    const cwh_span frames = {addr(out_frames), m * e->P.frame_bytes, e->P.raster != CW_RASTER_ALT ? 4u : 1u};
    const cwh_span ins[3] = {{addr(hdr), 16 * m, 16}, {addr(slot_pos), 16 * m, 16}, {addr(mask), m, 1}};
    if (cwh_spans_misaligned(&frames, 1) >= 0) return fail(CW_ERR_INVALID, "cw_render_records: out_frames is not 4-byte aligned");
    int other = 0;
    if (cwh_spans_clash(&frames, 1, ins, 3, 0, &other) >= 0)
        return fail(CW_ERR_INVALID, "cw_render_records: out_frames overlaps the %s", other < 2 ? "records read" : "mask");
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_render_records called before cw_reset");
    if (n_states == 0) return CW_OK;
    EnqueueEntry in(e, stream, CAPTURE_AWARE, LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(cwk_launch_render_records(&e->P, &e->tune, (const uint4 *)hdr, (const uint4 *)slot_pos, mask, n_states, out_frames, (hipStream_t)stream));
    return in.done();
}

int cw_step(cw_engine *e, const void *actions, int action_dtype, cw_stream_t stream)
{
    if (!e || !actions) return fail(CW_ERR_INVALID, "cw_step: null argument");
    if (action_dtype < CW_ACT_I32 || action_dtype > CW_ACT_U8) return fail(CW_ERR_INVALID, "cw_step: bad action dtype %d", action_dtype);
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_step called before cw_reset");
    Entry in(e);      // (not EnqueueEntry: cw_step_many asked once for all of its steps whether the stream captures, and the usual stream is found without note_work)
    if (in.rc != CW_OK) return in.rc;
    const bool capturing = e->in_step_many ? e->capturing_now : stream_capturing((hipStream_t)stream);
    if (capturing) e->captured = true;
    else if (e->n_work != 1 || e->work[0] != (hipStream_t)stream) note_work(e, (hipStream_t)stream);
    hipEvent_t *ev = (e->prof_n < e->prof_cap) ? &e->prof_ev[(size_t)e->prof_n * 6] : nullptr;
    const bool profiled = ev != nullptr;
    if (e->guard_on && !ev && !capturing) ev = sweep_guard_tick(e, (hipStream_t)stream);       // (a captured graph keeps the rate it was captured with)
    // a step captured into a HIP graph on its own carries the refill with it: a replayed graph would otherwise never refill
    if (capturing && e->P.lookahead && !e->la_refill_all && e->la_steps + 1 < e->la_period && !e->in_step_many) e->la_steps = e->la_period;
    if (e->P.lookahead && (e->la_refill_all || ++e->la_steps >= e->la_period)) {      // look-ahead refill, between two steps
        if (e->la_feedback && !capturing) la_adapt(e);
        HIP_TRY(cwk_launch_refill(&e->P, &e->tune, e->la_refill_all ? 1 : 0, (hipStream_t)stream));
        e->la_refill_all = false;
        e->la_steps = 0;
    }
    HIP_TRY(cwk_launch_step(&e->P, &e->tune, actions, action_dtype, e->obs_mode, e->auto_reset, (hipStream_t)stream, ev));
    if (profiled) e->prof_n++;
    record_last_work(e, (hipStream_t)stream);
    return CW_OK;
}

// n_steps consecutive steps from an action array [n_steps][N]: what a loop over cw_step enqueues, without the caller's per-step cost (a Python
// loop spends more per step than a state-only step takes on the card).  Capturable into a HIP graph as one piece; inside a capture the
// look-ahead refill rides at the head of the sequence too, so that a replayed graph of fewer than e->la_period steps still refills.
int cw_step_many(cw_engine *e, const void *actions, int action_dtype, int32_t n_steps, cw_stream_t stream)
{
    if (!e || !actions) return fail(CW_ERR_INVALID, "cw_step_many: null argument");
    if (n_steps < 1) return fail(CW_ERR_INVALID, "cw_step_many: n_steps must be >= 1");
    if (action_dtype < CW_ACT_I32 || action_dtype > CW_ACT_U8) return fail(CW_ERR_INVALID, "cw_step_many: bad action dtype %d", action_dtype);
    e->capturing_now = stream_capturing((hipStream_t)stream);
    if (e->P.lookahead && e->capturing_now) e->la_steps = e->la_period;
    const size_t row = (size_t)e->n * (action_dtype == CW_ACT_I32 ? 4 : action_dtype == CW_ACT_I64 ? 8 : 1);
    e->in_step_many = true;
    int rc = CW_OK;
    for (int32_t t = 0; t < n_steps && rc == CW_OK; t++) rc = cw_step(e, (const unsigned char *)actions + (size_t)t * row, action_dtype, stream);
    e->in_step_many = false;
    return rc;
}

// One step of the single-env loop WITHOUT a kernel launch: ring the resident kernel's doorbell, spin on its answer (cw_kernels.hip:
// cw_resident_kernel).  The kernel is (re)launched on demand -- the first call, after it idled out (0.5 ms without a request), after its
// time slice (200 ms), after any other entry point parked it -- and a request that raced with its exit is served by the next instance:
// `ack` says which sequence number was served last, and a new instance starts from there.
int cw_step_resident(cw_engine *e, int32_t action, int32_t want_onehot)
{
    if (!e) return fail(CW_ERR_INVALID, "cw_step_resident: null engine");
    if (!e->res) return fail(CW_ERR_INVALID, "cw_step_resident needs num_envs == 1, host_outputs, auto_reset == 0 and obs_mode state or pixels_dirty");
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_step_resident called before cw_reset");
    if (action < 0 || action > 127) return fail(CW_ERR_INVALID, "cw_step_resident: action %d outside 0..127", action);
    if (want_onehot && !e->P.res_onehot) return fail(CW_ERR_INVALID, "cw_step_resident: no host one-hot buffer on this engine");
    CwResident *R = e->res;
    const uint32_t seq = (++e->res_seq) & 0xFFFFFFu;
    __atomic_store_n(&R->bell, (unsigned long long)((seq << 8) | (want_onehot ? 0x80u : 0u) | (uint32_t)action), __ATOMIC_RELEASE);
    struct timespec t0;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (unsigned spins = 0;; spins++) {
        if (e->res_running && __atomic_load_n(&R->ack, __ATOMIC_ACQUIRE) == seq) return CW_OK;
        if (!e->res_running || __atomic_load_n(&R->exited, __ATOMIC_ACQUIRE) != 0) {
            // no kernel on the card, or it has left (idle, time slice): wait for it to be gone, then start one that continues after `ack`
            DeviceGuard guard(e->device);
            if (!guard.ok) return fail(CW_ERR_HIP, "hipSetDevice(%d) failed", e->device);
            if (e->res_running) HIP_TRY(hipStreamSynchronize(e->res_stream));
            e->res_running = false;
            if (__atomic_load_n(&R->ack, __ATOMIC_ACQUIRE) == seq) {            // it answered on its way out
                __atomic_store_n(&R->exited, 0u, __ATOMIC_RELEASE);
                return CW_OK;
            }
            // (the new instance reads the env's records: whatever cw_reset / cw_step enqueued last comes first -- an event of the engine's own,
            // recorded when that work was enqueued: the caller's stream may be gone by now)
            if (e->last_work_set) { HIP_TRY(hipStreamWaitEvent(e->res_stream, e->last_work, 0)); e->last_work_set = false; }
            __atomic_store_n(&R->exited, 0u, __ATOMIC_RELEASE);
            __atomic_store_n(&R->ack, (seq - 1u) & 0xFFFFFFu, __ATOMIC_RELEASE);
            HIP_TRY(cwk_launch_resident(&e->P, R, (seq - 1u) & 0xFFFFFFu, e->obs_mode == CW_OBS_PIXELS_DIRTY ? 1 : 0,
                                        500ull * e->res_ticks_per_us /* 0.5 ms idle */, 200000ull * e->res_ticks_per_us /* 200 ms slice */, e->res_stream));
            e->res_running = true;
            continue;
        }
        __builtin_ia32_pause();
        if ((spins & 1023u) == 1023u) {
            struct timespec t1;
            clock_gettime(CLOCK_MONOTONIC, &t1);
            if ((t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec) > 5.0) {
                // WITHDRAW the request before parking: the kernel serves a pending sequence number before it honours the stop bit, so the doorbell
                // goes back to the last number it answered, with the stop bit -- and if it did serve the step meanwhile, that is the answer
                const uint32_t acked = __atomic_load_n(&R->ack, __ATOMIC_ACQUIRE);
                __atomic_store_n(&R->bell, (1ull << 32) | ((unsigned long long)acked << 8), __ATOMIC_RELEASE);
                const hipError_t he = hipStreamSynchronize(e->res_stream);
                e->res_running = false;
                const uint32_t now_acked = __atomic_load_n(&R->ack, __ATOMIC_ACQUIRE);
                __atomic_store_n(&R->bell, (unsigned long long)now_acked << 8, __ATOMIC_RELEASE);
                __atomic_store_n(&R->exited, 0u, __ATOMIC_RELEASE);
                e->res_seq = now_acked;
                if (he == hipSuccess && now_acked == seq) return CW_OK;
                return fail(CW_ERR_HIP, "cw_step_resident: no answer from the resident kernel within 5 s (request withdrawn, kernel parked: the step was not taken)");
            }
        }
    }
}

int cw_resident_stop(cw_engine *e)
{
    if (!e) return fail(CW_ERR_INVALID, "cw_resident_stop: null engine");
    return Entry(e).rc;
}

int cw_rollout(cw_engine *e, const uint8_t *actions, int32_t n_steps, int32_t *rewards, uint8_t *dones, cw_stream_t stream)
{
    if (!e || !actions) return fail(CW_ERR_INVALID, "cw_rollout: null argument");
    if (n_steps < 1) return fail(CW_ERR_INVALID, "cw_rollout: n_steps must be >= 1");
    if (e->obs_mode != CW_OBS_STATE || !e->auto_reset)
        return fail(CW_ERR_INVALID, "cw_rollout needs obs_mode CW_OBS_STATE and auto_reset (frames are not painted by the persistent kernel)");
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_rollout called before cw_reset");
    EnqueueEntry in(e, stream, CAPTURE_AWARE, NO_LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    // Engines with look-ahead records: the n_steps go out in SEGMENTS of max_steps steps (64 at least), a refill kernel ahead of each -- a persistent launch
    // cannot refill, and an env that finishes a second time inside it finds no record and is reset the slow way by its whole wave (~12 us per env: the second
    // all-env time-out of a 600-step launch cost 64 envs x 12 us per wave, as much as the 600 steps themselves).  An episode lasts max_steps steps at most, so
    // with one segment per max_steps steps every time-out finds its record; shorter segments cost more in launches than they save (a segment start is ~20 us:
    // the refill, the launch, the state's round trip): 65 536 envs, T = 600: one launch 2.2e10 env-steps/s, segments of 64 / 128 / 300 steps 2.0 / 2.7 / 2.9e10
    // (2^20 envs: 4.1 -> 6.0e10; profiles/r06_experiments.txt C).  Same results, the same stream order.  CW_TUNE_ROLLOUT_SEGMENT=n: segments of n steps, 0: one launch.
    const int32_t seg = !e->P.lookahead || e->rollout_segment == 0 ? n_steps : e->rollout_segment > 0 ? e->rollout_segment : (e->P.max_steps > 64 ? e->P.max_steps : 64);
    const size_t N = (size_t)e->n;
    for (int32_t t0 = 0; t0 < n_steps; t0 += seg) {
        if (e->P.lookahead) {
            HIP_TRY(cwk_launch_refill(&e->P, &e->tune, e->la_refill_all ? 1 : 0, (hipStream_t)stream));
            e->la_refill_all = false;
            e->la_steps = 0;
        }
        const int32_t n = n_steps - t0 < seg ? n_steps - t0 : seg;
        HIP_TRY(cwk_launch_rollout(&e->P, actions + (size_t)t0 * N, n, rewards ? rewards + (size_t)t0 * N : nullptr, dones ? dones + (size_t)t0 * N : nullptr,
                                   (hipStream_t)stream));
    }
    return in.done();
}

int cw_render(cw_engine *e, uint8_t *out_frames, cw_stream_t stream)
{
    if (!e || !out_frames) return fail(CW_ERR_INVALID, "cw_render: null argument");
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_render called before cw_reset");
    EnqueueEntry in(e, stream, ANY_STREAM, NO_LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(cwk_launch_render_ext(&e->P, &e->tune, out_frames, (hipStream_t)stream));
    return in.done();
}

int cw_render_onehot(cw_engine *e, const uint8_t *onehot, int32_t n_states, uint16_t *out_frames, cw_stream_t stream)
{
    if (!e || !onehot || !out_frames) return fail(CW_ERR_INVALID, "cw_render_onehot: null argument");
    if (n_states < 1) return fail(CW_ERR_INVALID, "cw_render_onehot: n_states must be >= 1");
    EnqueueEntry in(e, stream, ANY_STREAM, NO_LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(cwk_launch_render_onehot(&e->P, onehot, n_states, out_frames, (hipStream_t)stream));
    return in.done();
}

int cw_export_grid(cw_engine *e, uint8_t *out, cw_stream_t stream)
{
    if (!e || !out) return fail(CW_ERR_INVALID, "cw_export_grid: null argument");
    EnqueueEntry in(e, stream, ANY_STREAM, NO_LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(cwk_launch_export(&e->P, &e->tune, out, 0, 0, (hipStream_t)stream));
    return in.done();
}

int cw_export_onehot(cw_engine *e, uint8_t *out, cw_stream_t stream)
{
    if (!e || !out) return fail(CW_ERR_INVALID, "cw_export_onehot: null argument");
    EnqueueEntry in(e, stream, ANY_STREAM, NO_LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(cwk_launch_export(&e->P, &e->tune, out, 1, 0, (hipStream_t)stream));
    return in.done();
}

int cw_export_onehot_of(cw_engine *e, int which, uint8_t *out, cw_stream_t stream)
{
    if (!e || !out) return fail(CW_ERR_INVALID, "cw_export_onehot_of: null argument");
    if (which < CW_STATE_CURRENT || which > CW_STATE_INIT) return fail(CW_ERR_INVALID, "cw_export_onehot_of: which must be CW_STATE_*");
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_export_onehot_of called before cw_reset");
    EnqueueEntry in(e, stream, ANY_STREAM, NO_LAST_WORK);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(cwk_launch_export(&e->P, &e->tune, out, 1, which, (hipStream_t)stream));
    return in.done();
}

int cw_profile_begin(cw_engine *e, int max_steps)
{
    if (!e || max_steps < 1 || max_steps > 100000) return fail(CW_ERR_INVALID, "cw_profile_begin: bad argument");
    Entry in(e);
    if (in.rc != CW_OK) return in.rc;
    prof_free(e);
    e->prof_ev.resize((size_t)max_steps * 6);
    for (auto &ev : e->prof_ev) HIP_TRY(hipEventCreate(&ev));
    e->prof_cap = max_steps;
    return CW_OK;
}

int cw_profile_end(cw_engine *e, cw_profile *out)
{
    if (!e || !out) return fail(CW_ERR_INVALID, "cw_profile_end: null argument");
    Entry in(e);
    if (in.rc != CW_OK) return in.rc;
    memset(out, 0, sizeof(*out));
    const int n = e->prof_n;
    if (n > 0) {
        const bool side_recorded = e->obs_mode != CW_OBS_PIXELS_FULL;      // (full-frame mode: only the sweep is bracketed)
        for (int k = 0; k < 6; k++)
            if (side_recorded || k >= 4) HIP_TRY(hipEventSynchronize(e->prof_ev[(size_t)(n - 1) * 6 + k]));
        double acc[3] = {0, 0, 0};
        float rmax = 0.f, rmin = 1e30f;
        std::vector<float> render_ms;
        render_ms.reserve((size_t)n);
        for (int i = 0; i < n; i++)
            for (int k = 0; k < 3; k++) {
                if (k != 2 && !side_recorded) continue;      // overlapped full-pixel step: only the render kernel is bracketed
                float ms = 0.f;
                HIP_TRY(hipEventElapsedTime(&ms, e->prof_ev[(size_t)i * 6 + 2 * k], e->prof_ev[(size_t)i * 6 + 2 * k + 1]));
                acc[k] += ms;
                if (k == 2) { rmax = ms > rmax ? ms : rmax; rmin = ms < rmin ? ms : rmin; render_ms.push_back(ms); }
            }
        out->steps = n;
        out->ms_step_kernel = (float)(acc[0] / n);
        out->ms_reset_kernel = (float)(acc[1] / n);
        out->ms_render_kernel = (float)(acc[2] / n);
        out->ms_render_kernel_max = rmax;
        out->ms_render_kernel_min = rmin;
        std::sort(render_ms.begin(), render_ms.end());
        out->ms_render_kernel_median = render_ms.empty() ? 0.f : render_ms[render_ms.size() / 2];
    }
    prof_free(e);
    return CW_OK;
}

const char *cw_render_kernel_name(const cw_engine *e)
{
    if (!e || e->obs_mode == CW_OBS_STATE) return "";
    if (e->obs_mode == CW_OBS_PIXELS_DIRTY) return e->auto_reset ? "cw_step_fused_kernel" : "cw_step_kernel";
    if (e->tune.gather && e->P.raster == CW_RASTER_RAY && e->S <= e->tune.gather_max_size) return "cw_render_gather_kernel";
    return "cw_render_pieces_kernel";
}

int cw_tuner(const cw_engine *e, cw_tuner_state *out)
{
    if (!e || !out) return fail(CW_ERR_INVALID, "cw_tuner: null argument");
    out->period16 = e->tune.period16;
    out->period16_head = e->tune.period16_head;
    out->period16_busy = e->tune.period16_busy;
    out->lookahead = e->P.lookahead;
    out->resident = e->res ? 1 : 0;
    out->guard_slowdowns = e->guard_on ? e->guard.slowdowns : -1;
    return CW_OK;
}

int cw_buffers(cw_engine *e, cw_buffer_table *out)
{
    if (!e || !out) return fail(CW_ERR_INVALID, "cw_buffers: null argument");
    const CwParams &P = e->P;
    out->obs = P.obs;
    out->desired_goal = P.desired_img;
    out->init_obs = P.init_img;
    out->terminal_obs = P.terminal_img;
    out->reward = P.reward;
    out->done = P.done;
    out->achieved = P.achieved_out;
    out->desired = P.desired_out;
    out->episode_length = P.episode_length;
    out->episode_return = P.episode_return;
    out->hdr = (uint8_t *)P.hdr;
    out->slot_pos = (uint16_t *)P.pos;
    out->counters = (uint64_t *)P.counters;
    out->frame_bytes = P.frame_bytes;
    out->host_actions = e->host_actions;
    out->host_onehot = P.res_onehot;
    return CW_OK;
}

int cw_synchronize(cw_engine *e, cw_stream_t stream)
{
    if (!e) return fail(CW_ERR_INVALID, "cw_synchronize: null engine");
    Entry in(e);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    for (int i = 0; i < e->n_work; i++)               // (that stream's share of the engine's work is done: the caller may destroy it now)
        if (e->work[i] == (hipStream_t)stream) { e->work[i] = e->work[--e->n_work]; break; }
    return CW_OK;
}

// generate_fixed_states' result (ray.py:116-118: fixed_state_list): the K pooled placements of every env as cell indices, [N][K][9] uint16 =
// objects 0..7 (OBJECTS order, ray.py:21) then the agent.  Synchronous host call.
int cw_get_fixed_states(cw_engine *e, uint16_t *out)
{
    if (!e || !out) return fail(CW_ERR_INVALID, "cw_get_fixed_states: null argument");
    if (e->K == 0) return fail(CW_ERR_INVALID, "cw_get_fixed_states: the engine was created with fixed_init_state = 0");
    SyncEntry in(e);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(aux_copy(e, out, e->P.pool, (size_t)e->n * e->K * 9 * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return in.done();
}

// ------------------------------------------------------------------------------ state get/set
int cw_get_state(cw_engine *e, cw_state_view *v)
{
    if (!e || !v) return fail(CW_ERR_INVALID, "cw_get_state: null argument");
    const size_t N = (size_t)e->n;
    const int S = e->S, nc = e->ncell;
    std::vector<uint32_t> hdr(N * 4), goal_codes(N);
    std::vector<uint16_t> pos(N * 8), ipos(N * 8), gpos(N * 8), iagent(N), gagent(N);
    std::vector<int32_t> epno(N);
    SyncEntry in(e);
    if (in.rc != CW_OK) return in.rc;
    HIP_TRY(aux_copy(e, hdr.data(), e->P.hdr, N * 16, hipMemcpyDeviceToHost));
    HIP_TRY(aux_copy(e, pos.data(), e->P.pos, N * 16, hipMemcpyDeviceToHost));
    HIP_TRY(aux_copy(e, ipos.data(), e->P.init_pos, N * 16, hipMemcpyDeviceToHost));
    HIP_TRY(aux_copy(e, gpos.data(), e->P.goal_pos, N * 16, hipMemcpyDeviceToHost));
    HIP_TRY(aux_copy(e, goal_codes.data(), e->P.goal_codes, N * 4, hipMemcpyDeviceToHost));
    HIP_TRY(aux_copy(e, iagent.data(), e->P.init_agent, N * 2, hipMemcpyDeviceToHost));
    HIP_TRY(aux_copy(e, gagent.data(), e->P.goal_agent, N * 2, hipMemcpyDeviceToHost));
    HIP_TRY(aux_copy(e, epno.data(), e->P.ep_no, N * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipStreamSynchronize(e->aux));
    for (size_t i = 0; i < N; i++) {
        const uint32_t *h = &hdr[i * 4];
        if (v->grid) cwh_slots_to_grid(&pos[i * 8], h[3], nc, v->grid + i * nc);
        if (v->init_grid) cwh_slots_to_grid(&ipos[i * 8], CW_CODES_INITIAL, nc, v->init_grid + i * nc);
        if (v->goal_grid) cwh_slots_to_grid(&gpos[i * 8], goal_codes[i], nc, v->goal_grid + i * nc);
        if (v->agent_rc) { v->agent_rc[i * 2] = h[0] & 0xFF; v->agent_rc[i * 2 + 1] = (h[0] >> 8) & 0xFF; }
        if (v->init_agent_rc) { v->init_agent_rc[i * 2] = (uint8_t)(iagent[i] / S); v->init_agent_rc[i * 2 + 1] = (uint8_t)(iagent[i] % S); }
        if (v->goal_agent_rc) { v->goal_agent_rc[i * 2] = (uint8_t)(gagent[i] / S); v->goal_agent_rc[i * 2 + 1] = (uint8_t)(gagent[i] % S); }
        if (v->hold) v->hold[i] = (h[0] >> 16) & 0xFF;
        if (v->achieved) v->achieved[i] = (uint16_t)(h[1] & 0xFFFF);
        if (v->desired) v->desired[i] = (uint16_t)(h[1] >> 16);
        if (v->step_num) v->step_num[i] = (int32_t)(h[2] & 0xFFFF);
        if (v->ep_no) v->ep_no[i] = epno[i];
    }
    return CW_OK;
}

int cw_set_state(cw_engine *e, const cw_state_view *v)
{
    if (!e || !v) return fail(CW_ERR_INVALID, "cw_set_state: null argument");
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_set_state called before cw_reset");
    const size_t N = (size_t)e->n;
    const int S = e->S, nc = e->ncell;
    std::vector<uint32_t> hdr(N * 4);
    std::vector<uint16_t> pos(N * 8), ipos(N * 8), gpos, gagent, iagent;
    std::vector<uint32_t> gcodes;
    std::vector<int32_t> epno(N);
    const bool restore_episode = v->goal_grid || v->goal_agent_rc || v->init_agent_rc;
    SyncEntry in(e);
    if (in.rc != CW_OK) return in.rc;
    if (restore_episode) {                           // the episode records: goal state (imagine_obs' result) and the agent's start cell
        gpos.resize(N * 8); gagent.resize(N); iagent.resize(N); gcodes.resize(N);
        HIP_TRY(aux_copy(e, gpos.data(), e->P.goal_pos, N * 16, hipMemcpyDeviceToHost));
        HIP_TRY(aux_copy(e, gcodes.data(), e->P.goal_codes, N * 4, hipMemcpyDeviceToHost));
        HIP_TRY(aux_copy(e, gagent.data(), e->P.goal_agent, N * 2, hipMemcpyDeviceToHost));
        HIP_TRY(aux_copy(e, iagent.data(), e->P.init_agent, N * 2, hipMemcpyDeviceToHost));
    }
    HIP_TRY(aux_copy(e, hdr.data(), e->P.hdr, N * 16, hipMemcpyDeviceToHost));
    HIP_TRY(aux_copy(e, pos.data(), e->P.pos, N * 16, hipMemcpyDeviceToHost));
    HIP_TRY(aux_copy(e, ipos.data(), e->P.init_pos, N * 16, hipMemcpyDeviceToHost));
    HIP_TRY(aux_copy(e, epno.data(), e->P.ep_no, N * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipStreamSynchronize(e->aux));
    for (size_t i = 0; i < N; i++) {
        uint32_t *h = &hdr[i * 4];
        uint32_t hold = (h[0] >> 16) & 0xFF;
        if (v->hold) {
            if (v->hold[i] > 3) return fail(CW_ERR_INVALID, "cw_set_state: hold[%zu]=%d outside 0..3", i, v->hold[i]);
            hold = v->hold[i];
        }
        if (v->agent_rc) {
            if (v->agent_rc[i * 2] >= S || v->agent_rc[i * 2 + 1] >= S) return fail(CW_ERR_INVALID, "cw_set_state: agent of env %zu off the grid", i);
            h[0] = (h[0] & 0xFFFF0000u) | v->agent_rc[i * 2] | ((uint32_t)v->agent_rc[i * 2 + 1] << 8);
        }
        if (v->grid) {
            // every object on the grid takes a slot; the held object (if any) takes one more
            uint32_t codes = 0;
            int k = 0;
            const uint8_t *g = v->grid + i * nc;
            for (int c = 0; c < nc; c++) {
                if (g[c] == 0) continue;
                if (g[c] > 8) return fail(CW_ERR_INVALID, "cw_set_state: env %zu cell %d has code %d > 8", i, c, g[c]);
                if (k >= 8) return fail(CW_ERR_INVALID, "cw_set_state: env %zu has more than 8 objects (outside the reference's reachable states)", i);
                pos[i * 8 + k] = (uint16_t)c;
                codes |= (uint32_t)g[c] << (4 * k);
                k++;
            }
            if (hold) {
                if (k >= 8) return fail(CW_ERR_INVALID, "cw_set_state: env %zu: 8 objects on the grid plus a held one", i);
                pos[i * 8 + k] = CW_POS_HELD;
                codes |= hold << (4 * k);
                k++;
            }
            for (; k < 8; k++) pos[i * 8 + k] = CW_POS_GONE;
            h[3] = codes;
        } else if (v->hold) {
            return fail(CW_ERR_INVALID, "cw_set_state: hold given without grid");
        }
        h[0] = (h[0] & 0xFF00FFFFu) | (hold << 16);
        if (v->init_grid) {
            const uint8_t *g = v->init_grid + i * nc;
            for (int k = 0; k < 8; k++) ipos[i * 8 + k] = CW_POS_GONE;
            for (int c = 0; c < nc; c++) {
                if (g[c] == 0) continue;
                if (g[c] > 8) return fail(CW_ERR_INVALID, "cw_set_state: env %zu init cell %d has code %d > 8", i, c, g[c]);
                if (ipos[i * 8 + g[c] - 1] != CW_POS_GONE)
                    return fail(CW_ERR_INVALID, "cw_set_state: env %zu init grid holds object %d twice (sample_state places one of each, ray.py:605-608)", i, g[c]);
                ipos[i * 8 + g[c] - 1] = (uint16_t)c;
            }
        }
        if (v->goal_grid) {                          // any slot order paints the same goal frame
            const uint8_t *g = v->goal_grid + i * nc;
            uint32_t codes = 0;
            int k = 0;
            for (int c = 0; c < nc; c++) {
                if (g[c] == 0) continue;
                if (g[c] > 8 || k >= 8) return fail(CW_ERR_INVALID, "cw_set_state: env %zu goal grid: code > 8 or more than 8 objects", i);
                gpos[i * 8 + k] = (uint16_t)c;
                codes |= (uint32_t)g[c] << (4 * k);
                k++;
            }
            for (; k < 8; k++) gpos[i * 8 + k] = CW_POS_GONE;
            gcodes[i] = codes;
        }
        if (v->goal_agent_rc) {
            if (v->goal_agent_rc[i * 2] >= S || v->goal_agent_rc[i * 2 + 1] >= S) return fail(CW_ERR_INVALID, "cw_set_state: goal agent of env %zu off the grid", i);
            gagent[i] = (uint16_t)(v->goal_agent_rc[i * 2] * S + v->goal_agent_rc[i * 2 + 1]);
        }
        if (v->init_agent_rc) {
            if (v->init_agent_rc[i * 2] >= S || v->init_agent_rc[i * 2 + 1] >= S) return fail(CW_ERR_INVALID, "cw_set_state: init agent of env %zu off the grid", i);
            iagent[i] = (uint16_t)(v->init_agent_rc[i * 2] * S + v->init_agent_rc[i * 2 + 1]);
        }
        if (v->achieved) h[1] = (h[1] & 0xFFFF0000u) | v->achieved[i];
        if (v->desired) h[1] = (h[1] & 0x0000FFFFu) | ((uint32_t)v->desired[i] << 16);
        if (v->step_num) {
            if (v->step_num[i] < 0 || v->step_num[i] > 65535) return fail(CW_ERR_INVALID, "cw_set_state: step_num[%zu] outside 0..65535", i);
            h[2] = (h[2] & 0xFFFF0000u) | (uint32_t)v->step_num[i];
        }
        if (v->ep_no) epno[i] = v->ep_no[i];
    }
    HIP_TRY(aux_copy(e, e->P.hdr, hdr.data(), N * 16, hipMemcpyHostToDevice));
    HIP_TRY(aux_copy(e, e->P.pos, pos.data(), N * 16, hipMemcpyHostToDevice));
    HIP_TRY(aux_copy(e, e->P.init_pos, ipos.data(), N * 16, hipMemcpyHostToDevice));
    HIP_TRY(aux_copy(e, e->P.ep_no, epno.data(), N * 4, hipMemcpyHostToDevice));
    if (restore_episode) {
        HIP_TRY(aux_copy(e, e->P.goal_pos, gpos.data(), N * 16, hipMemcpyHostToDevice));
        HIP_TRY(aux_copy(e, e->P.goal_codes, gcodes.data(), N * 4, hipMemcpyHostToDevice));
        HIP_TRY(aux_copy(e, e->P.goal_agent, gagent.data(), N * 2, hipMemcpyHostToDevice));
        HIP_TRY(aux_copy(e, e->P.init_agent, iagent.data(), N * 2, hipMemcpyHostToDevice));
    }
    if (e->obs_mode != CW_OBS_STATE) {   // the persistent frames must follow the injected state
        if (restore_episode) HIP_TRY(cwk_launch_render_restore(&e->P, &e->tune, e->aux));
        else HIP_TRY(cwk_launch_render_ext(&e->P, &e->tune, e->P.obs, e->aux));
    }
    return in.done();
}

}  // extern "C"

// ------------------------------------------------------------------------------ checkpoint blob
// The engine's complete resumable state as one opaque host blob: the RAW device records (header, slots, episode
// records, RNG streams in engine form, fixed_init_state pool, last step outputs, counters), restored verbatim -- so a
// resumed engine returns the same tensors as the run that never stopped, slot order included -- plus a header that
// pins the configuration the records only make sense under (batch, grid, episode length, task_list width, pool size,
// and a hash of the task menus; each env's menu id and reward rule travel inside its header record).
struct CwCkptHeader {
    char magic[8];
    uint32_t version, header_bytes;
    int32_t n_envs, size, max_steps, pool_k;
    uint32_t task_mask, n_menus, lookahead, reserved;
    uint64_t menus_hash, total_bytes;
};
static const char CW_CKPT_MAGIC[8] = {'C', 'W', 'C', 'K', 'P', 'T', 0, 1};
enum { CW_CKPT_VERSION = 4 };      // 2: look-ahead records; 3: episode_return, the sweep's private counter word, the QUEUED bit of nx_misc; 4: a queue of CW_LA_DEPTH records per env

struct CkptSection { void *dev; size_t bytes; };
static std::vector<CkptSection> ckpt_sections(cw_engine *e)
{
    const CwParams &P = e->P;
    // (file order; the sizes are cw_host.cpp's: cwh_ckpt_section_bytes -- the RNG streams are one reset ahead wherever a look-ahead record waits)
    void *dev[CWH_CKPT_SECTIONS] = {P.hdr, P.pos, P.init_pos, P.goal_pos, P.goal_codes, P.init_agent, P.goal_agent, P.ep_no, P.mt, P.mt_idx, P.pool, P.reward, P.done,
                                    P.achieved_out, P.desired_out, P.episode_length, P.episode_return, P.counters, P.nx_init_pos, P.nx_goal_pos, P.nx_misc,
                                    P.nx_ctl};
    size_t bytes[CWH_CKPT_SECTIONS];
    const int n = cwh_ckpt_section_bytes(e->n, e->K, e->P.lookahead ? CW_LA_DEPTH : 0, bytes, nullptr);
    std::vector<CkptSection> out;
    for (int i = 0; i < n; i++) out.push_back({dev[i], bytes[i]});
    return out;
}
static uint64_t menus_hash(const cw_engine *e)
{
    uint64_t h = 1469598103934665603ull;                 // FNV-1a over the device-form menus
    const unsigned char *b = (const unsigned char *)e->menus.data();
    for (size_t i = 0; i < e->menus.size() * sizeof(CwMenuDev); i++) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}
static CwCkptHeader ckpt_header(cw_engine *e)
{
    CwCkptHeader h{};
    memcpy(h.magic, CW_CKPT_MAGIC, 8);
    h.version = CW_CKPT_VERSION;
    h.header_bytes = (uint32_t)sizeof(CwCkptHeader);
    h.n_envs = e->n; h.size = e->S; h.max_steps = e->P.max_steps; h.pool_k = e->K;
    h.task_mask = e->P.task_mask; h.n_menus = (uint32_t)e->menus.size();
    h.lookahead = (uint32_t)e->P.lookahead;
    h.menus_hash = menus_hash(e);
    h.total_bytes = sizeof(CwCkptHeader);
    for (const CkptSection &sec : ckpt_sections(e)) h.total_bytes += sec.bytes;
    return h;
}

extern "C" {

size_t cw_checkpoint_bytes(cw_engine *e) { return e ? (size_t)ckpt_header(e).total_bytes : 0; }

int cw_checkpoint_save(cw_engine *e, void *buf, size_t capacity)
{
    if (!e || !buf) return fail(CW_ERR_INVALID, "cw_checkpoint_save: null argument");
    if (!e->has_reset) return fail(CW_ERR_STATE, "cw_checkpoint_save called before cw_reset");
    const CwCkptHeader h = ckpt_header(e);
    if (capacity < h.total_bytes) return fail(CW_ERR_INVALID, "cw_checkpoint_save: buffer of %zu bytes, %llu needed", capacity, (unsigned long long)h.total_bytes);
    SyncEntry in(e);
    if (in.rc != CW_OK) return in.rc;
    unsigned char *p = (unsigned char *)buf;
    memcpy(p, &h, sizeof(h));
    p += sizeof(h);
    for (const CkptSection &sec : ckpt_sections(e)) {
        if (sec.bytes) HIP_TRY(aux_copy(e, p, sec.dev, sec.bytes, hipMemcpyDefault));
        p += sec.bytes;
    }
    return in.done();
}

int cw_checkpoint_load(cw_engine *e, const void *buf, size_t length)
{
    if (!e || !buf) return fail(CW_ERR_INVALID, "cw_checkpoint_load: null argument");
    CwCkptHeader h;
    if (length < sizeof(h)) return fail(CW_ERR_INVALID, "cw_checkpoint_load: %zu bytes is not a checkpoint", length);
    memcpy(&h, buf, sizeof(h));
    const CwCkptHeader mine = ckpt_header(e);
    if (memcmp(h.magic, CW_CKPT_MAGIC, 8) != 0) return fail(CW_ERR_INVALID, "cw_checkpoint_load: not a CraftingWorld checkpoint");
    if (h.version != CW_CKPT_VERSION || h.header_bytes != sizeof(CwCkptHeader))
        return fail(CW_ERR_INVALID, "cw_checkpoint_load: checkpoint version %u, this library reads version %d", h.version, (int)CW_CKPT_VERSION);
    if (h.n_envs != mine.n_envs || h.size != mine.size || h.max_steps != mine.max_steps || h.pool_k != mine.pool_k ||
        h.task_mask != mine.task_mask)
        return fail(CW_ERR_INVALID, "cw_checkpoint_load: checkpoint of %d envs, size %d, max_steps %d, fixed_init_state %d, task mask %#x; "
                    "this engine: %d, %d, %d, %d, %#x", h.n_envs, h.size, h.max_steps, h.pool_k, h.task_mask, mine.n_envs, mine.size,
                    mine.max_steps, mine.pool_k, mine.task_mask);
    if (h.n_menus != mine.n_menus || h.menus_hash != mine.menus_hash)
        return fail(CW_ERR_INVALID, "cw_checkpoint_load: the checkpoint was written with different task menus (selected_tasks / "
                    "number_of_tasks / stacking / reward_style)");
    // A checkpoint written WITH look-ahead records can be resumed by an engine that keeps none (CW_TUNE_LOOKAHEAD=0, host-mapped outputs) and the
    // other way round: the records are not state, only work done ahead -- where one waits, the env's stream is rewound by the draws it took
    // (cwh_mt_rewind) and the record dropped; an engine that keeps records recomputes them at its next refill.
    const size_t N = (size_t)e->n;
    std::vector<uint32_t> key(CW_MT_N), words(CW_MT_N);      // (scratch of the rewind below; declared ahead of the entry: it outlives every copy)
    const size_t la_bytes = N * 16 * 3 * CW_LA_DEPTH + N * 4;
    const unsigned long long expect = mine.total_bytes + (h.lookahead && !mine.lookahead ? la_bytes : 0) - (!h.lookahead && mine.lookahead ? la_bytes : 0);
    if (h.total_bytes != expect || length < h.total_bytes)
        return fail(CW_ERR_INVALID, "cw_checkpoint_load: truncated checkpoint (%zu of %llu bytes)", length, (unsigned long long)h.total_bytes);
    SyncEntry in(e);
    if (in.rc != CW_OK) return in.rc;
    const unsigned char *p = (const unsigned char *)buf + sizeof(h);
    const unsigned char *blob_mt = nullptr, *blob_idx = nullptr;
    for (const CkptSection &sec : ckpt_sections(e)) {
        if (sec.dev == (void *)e->P.mt) blob_mt = p;
        if (sec.dev == (void *)e->P.mt_idx) blob_idx = p;
        const bool la_section = sec.dev == (void *)e->P.nx_init_pos || sec.dev == (void *)e->P.nx_goal_pos || sec.dev == (void *)e->P.nx_misc || sec.dev == (void *)e->P.nx_ctl;
        if (la_section && h.lookahead != mine.lookahead) continue;           // (handled below)
        if (sec.bytes) HIP_TRY(aux_copy(e, sec.dev, p, sec.bytes, hipMemcpyDefault));
        p += sec.bytes;
    }
    if (h.lookahead && !mine.lookahead) {            // p: the file's look-ahead sections (nx_init_pos, nx_goal_pos, nx_misc, list, count)
        const unsigned char *misc_bytes = p + N * 32 * CW_LA_DEPTH;     // (nx_misc of the file: 4 words per record at an offset that need not be 4-byte aligned -- the 'done' section is N bytes)
        HIP_TRY(hipStreamSynchronize(e->aux));
        for (size_t i = 0; i < N; i++) {
            uint32_t misc[4] = {0, 0, 0, 0};         // [3]: the draws of every record that waited, summed
            for (size_t d = 0; d < CW_LA_DEPTH; d++) {
                uint32_t md[4];
                memcpy(md, misc_bytes + (d * N + i) * 16, 16);
                if (md[2] >> 31) { misc[2] = md[2]; misc[3] += md[3]; }
            }
            if (!(misc[2] >> 31)) continue;
            int32_t pos = 0;
            memcpy(&pos, blob_idx + i * 4, 4);
            memcpy(words.data(), blob_mt + i * CW_MT_N * 4, CW_MT_N * 4);
            cwh_mt_to_numpy(words.data(), pos, key.data());
            cwh_mt_rewind(key.data(), &pos, misc[3]);
            const int32_t idx = cwh_mt_from_numpy(key.data(), pos);
            HIP_TRY(aux_copy(e, e->P.mt + i * CW_MT_N, key.data(), CW_MT_N * 4, hipMemcpyHostToDevice));
            HIP_TRY(aux_copy(e, e->P.mt_idx + i, &idx, 4, hipMemcpyHostToDevice));
            HIP_TRY(hipStreamSynchronize(e->aux));                           // (key / idx are reused by the next env)
        }
    } else if (!h.lookahead && mine.lookahead) {
        HIP_TRY(lookahead_drop(e));                  // no record anywhere: the next refill computes every env's
    }
    e->has_reset = true;
    e->la_refill_all = e->P.lookahead != 0;          // (harmless: envs that hold a record are skipped)
    if (e->obs_mode != CW_OBS_STATE) HIP_TRY(cwk_launch_render_restore(&e->P, &e->tune, e->aux));   // frames follow the records
    return in.done();
}

}  // extern "C"
