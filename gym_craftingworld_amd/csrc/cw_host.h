// cw_host.h -- the HIP-FREE host logic of the engine: MT19937 state conversion between numpy's form and the engine's, the dense view of a slot
// record, the checkpoint blob's section sizes, the DLPack producer, and the DECISIONS of the sweep clock's guard.  Plain C++ with a C ABI
// (cwh_*): compiled into libcraftingworld.so by hipcc, and on its own by g++ under -fsanitize=address,undefined for the CPU test tier
// (make -C gym_craftingworld_amd/csrc host_asan -> libcw_host_asan.so; tests/test_host_logic.py, tests/test_sanitizers.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#define CWH_MT_N 624

#ifdef __cplusplus
extern "C" {
#endif

// ---- MT19937: numpy RandomState (key, pos)  <->  the engine's consume-and-replace form (cw_mt.h)
int cwh_mt_from_numpy(uint32_t *s, int pos);                       // in place; returns the engine index (pos mod 624)
void cwh_mt_to_numpy(const uint32_t *s, int idx, uint32_t *key);   // engine (s, idx) -> a numpy key whose stream from position idx is identical
void cwh_mt_untwist(uint32_t *key);                                // one generation back (the twist's inverse)
void cwh_mt_rewind(uint32_t *key, int32_t *pos, uint32_t n);       // numpy state -> the state n raw draws earlier
void cwh_mt_init_genrand(uint32_t *s, uint32_t seed);              // numpy RandomState(int)

// ---- DLPack producer (a malloc'ed, non-owning DLManagedTensor over engine memory; device_type 10 = kDLROCM)
void *cwh_dlpack_make(void *data, int device_id, int code, int bits, int ndim, const int64_t *shape);

// ---- a slot record (8 cell indices u16 + 8 4-bit codes) as the dense grid of cw_state_view: grid[ncell] cell codes (0 empty)
void cwh_slots_to_grid(const uint16_t *pos, uint32_t codes, int ncell, uint8_t *grid);

// ---- checkpoint blob: byte sizes of its sections, in file order, for n envs / fixed_init_state pool k / la_depth look-ahead records per env (0: none kept).
// Writes at most CWH_CKPT_SECTIONS sizes, returns how many; *total (may be null) = their sum (the blob is header + total).
#define CWH_CKPT_SECTIONS 22
int cwh_ckpt_section_bytes(int64_t n, int32_t k, int32_t la_depth, size_t *sizes, uint64_t *total);

// ---- snapshot bank (cw_snapshot_reserve / _save / _load): `rows` rows in device memory, each of which holds one env completely, laid out like the engine --
// one array per field, a row's MT words contiguous, the look-ahead ring as [la_depth][rows].  The sections in bank order: hdr, pos, init_pos, goal_pos (16 B a
// row), goal_codes, ep_no (4), init_agent, goal_agent (2), mt (624 x 4), mt_idx (4), nx_init_pos, nx_goal_pos, nx_misc (la_depth x 16), nx_ctl (4 with a ring,
// else 0), pool (k x 9 x 2), valid (1: the row has been saved since the last reserve).  Every section starts on a CWH_SNAP_ALIGN boundary.
// Writes CWH_SNAP_SECTIONS sizes and offsets (either may be null), returns how many; *total = the allocation, *row_bytes = what one row holds.
#define CWH_SNAP_SECTIONS 16
#define CWH_SNAP_ALIGN 256
enum { CWH_SNAP_HDR = 0, CWH_SNAP_POS, CWH_SNAP_INIT_POS, CWH_SNAP_GOAL_POS, CWH_SNAP_GOAL_CODES, CWH_SNAP_EP_NO, CWH_SNAP_INIT_AGENT, CWH_SNAP_GOAL_AGENT,
       CWH_SNAP_MT, CWH_SNAP_MT_IDX, CWH_SNAP_NX_INIT_POS, CWH_SNAP_NX_GOAL_POS, CWH_SNAP_NX_MISC, CWH_SNAP_NX_CTL, CWH_SNAP_POOL, CWH_SNAP_VALID };
int cwh_snapshot_section_bytes(int64_t rows, int32_t k, int32_t la_depth, size_t *sizes, size_t *offsets, uint64_t *total, uint64_t *row_bytes);
// THE row check of the snapshot kernels, shared by host and device: a row number from the caller's array may index the bank only if this says so
#if defined(__HIP__) || defined(__HIPCC__)
#define CWH_HOST_DEVICE __host__ __device__
#else
#define CWH_HOST_DEVICE
#endif
static inline CWH_HOST_DEVICE int cwh_snapshot_row_ok(int32_t row, int32_t capacity) { return row >= 0 && row < capacity; }
int cwh_snapshot_row_in_bank(int32_t row, int32_t capacity);       // (the same, exported for the CPU tests)
// THE env check of cw_expand_kernel, shared by host and device: an entry of the caller's env_of array may index the engine's per-env arrays only if this says so
static inline CWH_HOST_DEVICE int cwh_expand_env_ok(int32_t env, int32_t num_envs) { return env >= 0 && env < num_envs; }
int cwh_expand_env_in_batch(int32_t env, int32_t num_envs);        // (the same, exported for the CPU tests)
// THE pixel offset of cw_render_records_kernel's AltObs painter, shared by host and device: where in a frame of 27 * S * (S + 1) bytes the three bytes of
// item 1..9 (object code 1..8, 9 = the agent) in cell `pos` of an S x S grid go -- pixel item - 1 of the cell's 3x3 tile (craftingworld_altobs.py:527-543) --
// or CWH_ALT_NO_PIXEL for every other item and every position at or above S * S (the two markers of a slot, gone and held, included).  A record's bytes
// become a store address only through this: an offset it returns satisfies offset + 3 <= 27 * S * S, inside the grid part of the frame.
#define CWH_ALT_NO_PIXEL 0xFFFFFFFFu
static inline CWH_HOST_DEVICE uint32_t cwh_alt_pixel_offset(uint32_t size, uint32_t pos, uint32_t item)
{
    if (size - 1u >= 255u || item - 1u >= 9u || pos >= size * size) return CWH_ALT_NO_PIXEL;
    const uint32_t r = pos / size, c = pos - r * size, k = item - 1u, k3 = k / 3u;
    return (3u * r + k3) * (9u * size) + 9u * c + 3u * (k - 3u * k3);
}
uint32_t cwh_alt_pixel_offset_of(uint32_t size, uint32_t pos, uint32_t item);     // (the same, exported for the CPU tests)

// ---- launch shapes shared by the launchers (cw_kernels.hip) and the CPU tests: the code the launchers run, no copy of it
#define CW_WAVE 64          // lanes of a wavefront
#define CW_RESET_WAVES 4    // waves (= envs in flight) per workgroup of the kernels that reset
// workgroups of CW_RESET_WAVES waves for `jobs` waves' worth of work -- persistent: one wave per env in flight, n_cu * reset_blocks_per_cu workgroups at most
static inline int cwh_reset_grid(int jobs, int n_cu, int reset_blocks_per_cu)
{
    int blocks = (jobs + CW_RESET_WAVES - 1) / CW_RESET_WAVES;
    if (blocks > n_cu * reset_blocks_per_cu) blocks = n_cu * reset_blocks_per_cu;
    return blocks < 1 ? 1 : blocks;
}
int cwh_reset_grid_of(int jobs, int n_cu, int reset_blocks_per_cu);        // (the same, exported for the CPU tests)
// THE shape of the masked kernels (reset, imagine, sample) and the snapshot kernels: a workgroup scans `epb` mask bytes (row numbers) per round and deals the
// selected envs out to its four waves: 64, halved down to 4 (one env per wave, cw_reset_kernel's shape) while the ceil(N / epb) chunks would not fill
// most = n_cu * reset_blocks_per_cu workgroups; min(chunks, most) workgroups, each taking chunks blockIdx.x, blockIdx.x + gridDim.x, ...  With
// CW_TUNE_RESET_BLOCKS=4 on 256 CUs: 4 below 8 185 envs, 64 from 65 473 (tests/test_masked_shapes.py runs every width with the value 1).  -> epb; *blocks
static inline int cwh_masked_launch(int n_envs, int n_cu, int reset_blocks_per_cu, int *blocks)
{
    const int most = n_cu * reset_blocks_per_cu;
    int epb = CW_WAVE;
    while (epb > CW_RESET_WAVES && (n_envs + epb - 1) / epb < most) epb >>= 1;
    *blocks = cwh_reset_grid(((n_envs + epb - 1) / epb) * CW_RESET_WAVES, n_cu, reset_blocks_per_cu);
    return epb;
}
int cwh_masked_launch_of(int n_envs, int n_cu, int reset_blocks_per_cu, int *blocks);      // (the same, exported for the CPU tests)
// envs per wavefront of the kernels that reset inline (an inline reset occupies the whole wave, one finished env at a time -- rare now that
// finished envs take their look-ahead records): aim for ~1024 waves (one per SIMD) -- `most` (64) envs per wave for large batches, down to 8 for small ones
static inline int cwh_envs_per_wave(int n, int most)
{
    int epw = most;
    while (epw > 8 && (n + epw - 1) / epw < 1024) epw >>= 1;
    return epw;
}
int cwh_envs_per_wave_of(int n, int most);         // (the same, exported for the CPU tests)
// THE CHUNKS of the sweep over one frame array [n_envs][frame_bytes] (cw_launch_sweep).  The sweep's waves are in step only at the start of a
// launch; over thousands of rounds they drift apart (0.62-0.74 of the HBM peak at 2^20 envs in one launch against 0.86 in eight,
// profiles/history/r03_other_configs.txt).  So a large batch is swept in chunks of consecutive envs, back-to-back launches on one stream of at most
// render_chunk_rounds rounds of 3 KB per wave (~2.8 GB; 0: no limit of its own).  The kernels index a chunk with 32-bit offsets and round its bytes up to whole
// 4-KiB pieces, so a chunk holds at most CWH_CHUNK_MAX_BYTES = 2^32 - 4096 bytes; and every chunk starts on a 4-KiB boundary of the array, so that every
// wave of a chunk paints whole aligned pieces.  Chunks are whole multiples of 4 096 envs wherever that many frames fit a chunk -- every frame up to 147x147
// (Ray, 48 S^2 bytes) or 196x196 (AltObs, 27 S (S + 1) bytes).  Larger frames take the smallest count of envs whose frames end on a 4-KiB boundary instead,
// 4096 / gcd(frame_bytes, 4096): at most 256 envs (Ray frames are multiples of 16 bytes) or 2 048 (AltObs: of 2), under 2^32 bytes at every size up to 255.
// A batch that needs no split -- one launch within the rounds, at most CWH_CHUNK_MAX_BYTES -- is one chunk of n_envs.
// -> number of chunks; *per = envs per chunk (the last one may be shorter): chunk c covers envs [c * per, min(n_envs, (c + 1) * per))
#define CWH_CHUNK_MAX_BYTES ((1ll << 32) - 4096)
static inline int cwh_piece_chunks(int n_envs, uint32_t frame_bytes, int n_cu, int render_chunk_rounds, int *per)
{
    const long long waves = (long long)n_cu * (256 / CW_WAVE), fb = (long long)frame_bytes;
    const long long cap = (long long)(render_chunk_rounds > 0 ? render_chunk_rounds : 1 << 20) * waves * 3072;
    const long long bytes = (long long)n_envs * fb;
    long long n = (bytes + cap - 1) / cap;
    if (n < 1) n = 1;
    long long p = (n_envs + n - 1) / n;
    if (n > 1 || bytes > CWH_CHUNK_MAX_BYTES) {
        p = (p + 4095) / 4096 * 4096;
        while (p * fb > CWH_CHUNK_MAX_BYTES && p > 4096) p = (p / 2 + 4095) / 4096 * 4096;
        if ((p < n_envs ? p : n_envs) * fb > CWH_CHUNK_MAX_BYTES) {      // 4 096 frames do not fit: as few equal chunks of whole granules as the limit allows
            long long d = 4096;
            while (fb % d) d >>= 1;                                      // gcd(frame_bytes, 4096)
            const long long g = 4096 / d;
            const long long most = CWH_CHUNK_MAX_BYTES / fb / g * g;     // (>= g for every frame the engine accepts; a frame beyond them goes one to a chunk)
            long long k = most > 0 ? (n_envs + most - 1) / most : n_envs;
            if (k < n) k = n;                                            // (... and no fewer than the rounds ask for)
            p = most > 0 ? ((n_envs + k - 1) / k + g - 1) / g * g : 1;
        }
    }
    *per = (int)p;
    return (int)((n_envs + p - 1) / p);
}
int cwh_piece_chunks_of(int n_envs, uint32_t frame_bytes, int n_cu, int render_chunk_rounds, int *per);      // (the same, exported for the CPU tests)

// ---- the argument rules of an entry point that reads PACKED RECORDS and needs no HIP to check them (cw_engine.cpp: cw_expand and cw_simulate turn the code
// into their error texts), in the order they are tested: some output field, 0 <= n_states <= CWH_MAX_STATES (cw_export_onehot_states and cw_render_records,
// which require their records, share only this cap), 1 <= n_steps <= max_steps (max_steps 0: a call without steps, cw_expand), hdr_in and slot_pos_in
// together, env_of only with them, and without them (the engine's own states) n_states = num_envs -- or, broadcast (cw_simulate), a positive multiple of it.
// has_*: the pointer is not null; n_out_fields: how many fields of out are not.
#define CWH_MAX_STATES (1 << 27)
#define CWH_SIM_MAX_STEPS 32767     // with max_steps <= 65 535 the int32 sum of n_steps rewards cannot overflow
enum { CWH_REC_OK = 0, CWH_REC_NO_FIELD = 1, CWH_REC_N_STATES = 2, CWH_REC_N_STEPS = 3, CWH_REC_PAIR = 4, CWH_REC_ENV_OF = 5, CWH_REC_OWN_STATES = 6 };
int cwh_records_args(int32_t num_envs, int has_env_of, int has_hdr_in, int has_slot_pos_in, int32_t n_states, int32_t n_steps, int n_out_fields,
                     int32_t max_steps, int broadcast);
// ... and of cw_plan: cwh_records_args as cw_expand calls it (its own states once, no broadcast) with 1 <= depth <= CWH_PLAN_MAX_DEPTH in the place of n_steps
// (CWH_REC_N_STEPS), and behind that check and before the pointer rules the cap on the work of ONE launch: n_states * 6^depth <= CWH_PLAN_MAX_LEAVES
// (CWH_REC_PLAN_WORK) -- 65 536 states at depth 6, 2 048 at depth 8.
#define CWH_PLAN_MAX_DEPTH 8
#define CWH_PLAN_MAX_LEAVES (1ull << 32)
enum { CWH_REC_PLAN_WORK = 7 };
int cwh_plan_args(int32_t num_envs, int has_env_of, int has_hdr_in, int has_slot_pos_in, int32_t n_states, int32_t depth, int n_out_fields);
// ... and of cw_unroll: cwh_records_args as cw_simulate calls it (1 <= n_steps <= CWH_SIM_MAX_STEPS, its own states broadcast), and behind the step check and
// before the pointer rules the cap on the rows of ONE launch: (n_steps + 1) * n_states <= CWH_MAX_STATES (CWH_REC_UNROLL_ROWS) -- the whole [T + 1][M] record
// array is then a legal input, flattened, to every call that reads records, and each record array stays at or below 2 GiB.
enum { CWH_REC_UNROLL_ROWS = 8 };
int cwh_unroll_args(int32_t num_envs, int has_env_of, int has_hdr_in, int has_slot_pos_in, int32_t n_states, int32_t n_steps, int n_out_fields);
// the byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte (an empty range shares none; a range that would wrap ends at the top of the address space)
int cwh_ranges_overlap(uint64_t a, uint64_t a_bytes, uint64_t b, uint64_t b_bytes);

// ---- THE SPAN CHECKER: every "is this pointer aligned, does this output share a byte with what it must not" of the entry points goes through these two.
// A span is what a call reads or writes through one pointer: the address as an integer (0: not given), its bytes, the alignment the kernels need of it
// (0 or 1: any address).
typedef struct cwh_span { uint64_t at, bytes, align; } cwh_span;
// the index of the first given span whose address is no multiple of its alignment, -1: none
int cwh_spans_misaligned(const cwh_span *spans, int n);
// The first output that shares a byte (cwh_ranges_overlap) with something it must not: the outputs in order, each against the inputs in order and then, with
// among_outs, against the outputs behind it in order.  A span not given, or of no bytes, shares none.  -> the output's index and in *other (may be null) the
// other side's -- i for ins[i], n_ins + q for outs[q] --, or -1: no clash.
int cwh_spans_clash(const cwh_span *outs, int n_outs, const cwh_span *ins, int n_ins, int among_outs, int *other);
// ---- THE SECTION LAYOUT of a region, one allocation cut into n sections in order (snapshot bank, visited set, reach workspace, replay buffer): section i
// starts at offsets[i] (may be null), the sum of the sections before it, each rounded up to a multiple of align (>= 1).  -> the bytes of the region
uint64_t cwh_sections_layout(const uint64_t *bytes, int n, uint64_t align, uint64_t *offsets);

// ---- cw_shoot / cw_shoot_actions: THE DRAW (include/craftingworld.h states it), shared by the kernels and the host -- integers only, so a CPU model is exact.
// cwh_shoot_prefix is the part that does not depend on the step: the kernels compute it once per sample, outside the step loop.
static inline CWH_HOST_DEVICE uint32_t cwh_shoot_mix(uint32_t x)
{
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}
static inline CWH_HOST_DEVICE uint32_t cwh_shoot_prefix(uint64_t seed, uint32_t state, uint32_t sample)
{
    const uint32_t x = cwh_shoot_mix((uint32_t)seed ^ state * 0x9E3779B1u);
    return cwh_shoot_mix(x ^ ((uint32_t)(seed >> 32) + sample * 0x85EBCA77u));
}
static inline CWH_HOST_DEVICE uint32_t cwh_shoot_step(uint32_t prefix, uint32_t step) { return cwh_shoot_mix(prefix ^ step * 0xC2B2AE3Du); }
static inline CWH_HOST_DEVICE uint32_t cwh_shoot_draw(uint64_t seed, uint32_t state, uint32_t sample, uint32_t step)
{
    return cwh_shoot_step(cwh_shoot_prefix(seed, state, sample), step);
}
static inline CWH_HOST_DEVICE uint32_t cwh_shoot_mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }
// the action of a draw under six weights (all 0: uniform, like no weights at all): how many of the first five partial sums lie at or below mulhi32(r, W)
static inline CWH_HOST_DEVICE uint32_t cwh_shoot_action_w(uint32_t r, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4, uint32_t w5)
{
    const uint32_t c0 = w0, c1 = c0 + w1, c2 = c1 + w2, c3 = c2 + w3, c4 = c3 + w4, W = c4 + w5;
    if (W == 0u) return cwh_shoot_mulhi(r, 6u);
    const uint32_t x = cwh_shoot_mulhi(r, W);
    return (uint32_t)(c0 <= x) + (uint32_t)(c1 <= x) + (uint32_t)(c2 <= x) + (uint32_t)(c3 <= x) + (uint32_t)(c4 <= x);
}
static inline CWH_HOST_DEVICE uint32_t cwh_shoot_action(uint32_t r, const uint16_t *w, size_t stride)
{
    if (!w) return cwh_shoot_mulhi(r, 6u);
    return cwh_shoot_action_w(r, w[0], w[stride], w[2 * stride], w[3 * stride], w[4 * stride], w[5 * stride]);
}
// (the draw and its action, exported for the CPU tests: weights null or six uint16, contiguous)
uint32_t cwh_shoot_draw_of(uint64_t seed, uint32_t state, uint32_t sample, uint32_t step);
uint32_t cwh_shoot_action_of(uint64_t seed, uint32_t state, uint32_t sample, uint32_t step, const uint16_t *weights);
// THE lanes cw_shoot_kernel gives one state (they play its samples g, g + G, ...): the smallest power of two G with n_states * G >= 65 536 -- a small batch
// spreads its samples over the wave --, at most 64 and at most the largest power of two <= n_samples (so one sample is one lane).  n_states * G < 2^28.
#ifndef CWH_SHOOT_FILL
#define CWH_SHOOT_FILL 65536     // (one wave on each SIMD of 256 CUs; an experimental build may set another target: make exp EXP='-DCWH_SHOOT_FILL=...')
#endif
static inline int cwh_shoot_lanes(int32_t n_states, int32_t n_samples)
{
    int g = 1;
    while (g < CW_WAVE && 2 * g <= n_samples && (int64_t)n_states * g < CWH_SHOOT_FILL) g <<= 1;
    return g;
}
int cwh_shoot_lanes_of(int32_t n_states, int32_t n_samples);       // (the same, exported for the CPU tests)
// the argument rules of cw_shoot: cwh_records_args as cw_plan calls it (its own states once) with 1 <= n_steps <= CWH_SIM_MAX_STEPS, then
// 1 <= n_samples <= CWH_SHOOT_MAX_SAMPLES (CWH_REC_SHOOT_SAMPLES) and the cap on the work of ONE launch, n_states * n_samples * n_steps <=
// CWH_SHOOT_MAX_WORK (CWH_REC_SHOOT_WORK: 65 536 states x 1 024 samples x 64 steps), both behind the step check and before the pointer rules.
#define CWH_SHOOT_MAX_SAMPLES 65536
#define CWH_SHOOT_MAX_WORK (1ull << 32)
enum { CWH_REC_SHOOT_WORK = 8, CWH_REC_SHOOT_SAMPLES = 9 };
int cwh_shoot_args(int32_t num_envs, int has_env_of, int has_hdr_in, int has_slot_pos_in, int32_t n_states, int32_t n_steps, int32_t n_samples,
                   int n_out_fields);
// ... and of cw_shoot_actions, in order: 0 <= n_states <= CWH_MAX_STATES (CWH_REC_N_STATES), 0 <= n_rows <= CWH_MAX_STATES (CWH_REC_SHOOT_SAMPLES),
// 1 <= n_steps <= CWH_SIM_MAX_STEPS (CWH_REC_N_STEPS), n_rows * n_states * n_steps <= CWH_SHOOT_MAX_WORK (CWH_REC_SHOOT_WORK)
int cwh_shoot_actions_args(int32_t n_states, int32_t n_steps, int32_t n_rows);

// ---- cw_shoot_refit: the other half of a CEM iteration (include/craftingworld.h states it).  THE WEIGHT an action gets that `count` of the elites drew:
// min(65 535, smooth + gain * count) in uint32 arithmetic -- smooth and gain <= 65 535 and count <= 65 536 (CWH_SHOOT_MAX_SAMPLES), so the sum is at most
// 2^32 - 1 and never wraps.  Shared by the kernel and the host.
static inline CWH_HOST_DEVICE uint32_t cwh_refit_weight(uint32_t smooth, uint32_t gain, uint32_t count)
{
    const uint32_t w = smooth + gain * count;
    return w < 65535u ? w : 65535u;
}
uint32_t cwh_refit_weight_of(uint32_t smooth, uint32_t gain, uint32_t count);       // (the same, exported for the CPU tests)
// workgroups of 256 lanes of the two refit kernels, grid-stride over `items` lanes: ceil(items / 256), 1 at least, n_cu * CWH_REFIT_BLOCKS_PER_CU at most
#define CWH_REFIT_BLOCKS_PER_CU 8
static inline int64_t cwh_refit_grid(int64_t items, int32_t n_cu)
{
    const int64_t want = (items + 255) / 256, most = (int64_t)n_cu * CWH_REFIT_BLOCKS_PER_CU;
    return want < most ? (want < 1 ? 1 : want) : most;
}
int64_t cwh_refit_grid_of(int64_t items, int32_t n_cu);                             // (the same, exported for the CPU tests)
// the argument rules of cw_shoot_refit, in the order they are tested; addresses as integers (0: null), so the rules need no HIP: ret and elites given
// (CWH_REFIT_NULL), 0 <= n_states <= CWH_MAX_STATES (CWH_REFIT_N_STATES), 1 <= n_steps <= CWH_SIM_MAX_STEPS (CWH_REFIT_N_STEPS), 1 <= n_samples <=
// CWH_SHOOT_MAX_SAMPLES (CWH_REFIT_N_SAMPLES), 1 <= n_elites <= n_samples (CWH_REFIT_N_ELITES), n_states * n_samples * n_steps <= CWH_SHOOT_MAX_WORK
// (CWH_REFIT_WORK: cw_shoot's cap; the refit draws n_states * n_elites * n_steps times at most), smooth <= 65 535 (CWH_REFIT_SMOOTH), 1 <= gain <= 65 535
// (CWH_REFIT_GAIN), env_of, ret, elites, elite_min 4-byte and weights_in, weights 2-byte aligned (CWH_REFIT_ALIGN: cwh_spans_misaligned), no output
// sharing a byte with ret, env_of, another output or weights_in (CWH_REFIT_OVERLAP: cwh_spans_clash) -- except weights == weights_in, the SAME address, the
// refit in place: weights_in then is no input of its own, its bytes are exactly those of weights, which is tested against every other span.
enum { CWH_REFIT_OK = 0, CWH_REFIT_NULL = 1, CWH_REFIT_N_STATES = 2, CWH_REFIT_N_STEPS = 3, CWH_REFIT_N_SAMPLES = 4, CWH_REFIT_N_ELITES = 5, CWH_REFIT_WORK = 6,
       CWH_REFIT_SMOOTH = 7, CWH_REFIT_GAIN = 8, CWH_REFIT_ALIGN = 9, CWH_REFIT_OVERLAP = 10 };
int cwh_refit_args(uint64_t env_of, int32_t n_states, int32_t n_steps, int32_t n_samples, int32_t n_elites, uint64_t weights_in, uint64_t ret, uint32_t smooth,
                   uint32_t gain, uint64_t elites, uint64_t weights, uint64_t elite_min);

// ---- cw_seen_*: the visited set of packed records.  THE KEY of a record (include/craftingworld.h states it): everything step_env reads of a state but the two
// step counters, and the group that says which records may be merged at all -- group, hdr bytes 0-2, 4-7, bit 1 of byte 10, 12-15 and the 16 bytes of slot_pos:
// 36 bytes as nine dwords.  hdr and slot_pos as the four little-endian dwords of a record each (the uint4 the kernels load).  Shared by the kernels and the host.
#define CWH_SEEN_KEY_WORDS 9
static inline CWH_HOST_DEVICE void cwh_seen_key(int32_t group, const uint32_t hdr[4], const uint32_t pos[4], uint32_t key[CWH_SEEN_KEY_WORDS])
{
    key[0] = (uint32_t)group;
    key[1] = hdr[0] & 0x00FFFFFFu;              // agent row, agent col, hold; not the menu id
    key[2] = hdr[1];                            // achieved | desired << 16
    key[3] = (hdr[2] >> 17) & 1u;               // the subset reward rule; not step_num, flag bit 0 or the success count
    key[4] = hdr[3];                            // the eight slot codes
    key[5] = pos[0]; key[6] = pos[1]; key[7] = pos[2]; key[8] = pos[3];
}
// its 64-bit hash: splitmix64's finaliser folded over the nine dwords (any value, 0 included; the slot tag is made from it by cwh_seen_tag)
static inline CWH_HOST_DEVICE uint64_t cwh_seen_mix(uint64_t x)
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return x;
}
static inline CWH_HOST_DEVICE uint64_t cwh_seen_hash(const uint32_t key[CWH_SEEN_KEY_WORDS])
{
    uint64_t h = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < CWH_SEEN_KEY_WORDS - 1; i += 2) h = cwh_seen_mix(h ^ ((uint64_t)key[i] | (uint64_t)key[i + 1] << 32));
    return cwh_seen_mix(h ^ (uint64_t)key[CWH_SEEN_KEY_WORDS - 1]);
}
// the tag a slot holds for that hash: all 64 bits, or the low tag_bits of them (1 .. 63: tests and tools/measure_seen.py drive the same-tag-different-key path
// with it); never 0, which marks an empty slot
static inline CWH_HOST_DEVICE uint64_t cwh_seen_tag(uint64_t hash, int32_t tag_bits)
{
    const uint64_t t = tag_bits > 0 && tag_bits < 64 ? hash & ((1ull << tag_bits) - 1ull) : hash;
    return t ? t : 1ull;
}
void cwh_seen_key_of(int32_t group, const uint8_t *hdr /* [16] */, const uint16_t *slot_pos /* [8] */, uint32_t *key /* [9] */);   // (exported for the CPU tests;
uint64_t cwh_seen_hash_of(const uint32_t *key /* [9] */);                                                                         //  any alignment, little-endian)
// slots of a set meant to hold `capacity` distinct keys: the next power of two >= 2 * capacity (2 at least); 0 for capacity 0 (no set), -1 outside 0 .. 2^28
#define CWH_SEEN_MAX_CAPACITY (1ll << 28)
#define CWH_SEEN_PROBES 128         // slots a row looks at, linearly from hash & (slots - 1), before it gives up and is counted as overflow (fewer in a smaller set)
#define CWH_SEEN_ROW_BITS 28        // an owner word is epoch << 28 | row: rows below 2^27, 36 bits of epoch
#define CWH_SEEN_MAX_EPOCH ((1ull << 36) - 2ull)
int64_t cwh_seen_slots_of(int64_t capacity);
// the set of `slots` slots: CWH_SEEN_SECTIONS sections in this order -- the control block (CWH_SEEN_CTL_BYTES), tag and owner (8 bytes a slot each), key_a and
// key_b (16 each) --, packed: every one a multiple of 16 bytes, the alignment the key halves need, 48 bytes a slot in all.  Writes the sections' offsets (may
// be null); -> the bytes, -1 unless slots is a count cwh_seen_slots_of gives a set: a power of two, 2 .. 2 * CWH_SEEN_MAX_CAPACITY.
#define CWH_SEEN_CTL_BYTES 256
enum { CWH_SEEN_S_CTL = 0, CWH_SEEN_S_TAG, CWH_SEEN_S_OWNER, CWH_SEEN_S_KEY_A, CWH_SEEN_S_KEY_B, CWH_SEEN_SECTIONS };
int64_t cwh_seen_layout(int64_t slots, uint64_t *offsets);
// the argument rules of cw_seen_insert, in the order they are tested; addresses as integers (0: null), so the rules need no HIP: records given
// (CWH_SEEN_NO_RECORDS), some output (CWH_SEEN_NO_FIELD), 0 <= n_states <= CWH_MAX_STATES (CWH_SEEN_N_STATES), hdr and slot_pos 16-byte aligned and group,
// first 4-byte aligned (CWH_SEEN_ALIGN: cwh_spans_misaligned), neither output sharing a byte with hdr, slot_pos, group or the other output
// (CWH_SEEN_OVERLAP: cwh_spans_clash)
enum { CWH_SEEN_OK = 0, CWH_SEEN_NO_RECORDS = 1, CWH_SEEN_NO_FIELD = 2, CWH_SEEN_N_STATES = 3, CWH_SEEN_ALIGN = 4, CWH_SEEN_OVERLAP = 5 };
int cwh_seen_args(uint64_t group, uint64_t hdr, uint64_t slot_pos, int32_t n_states, uint64_t fresh, uint64_t first);

// ---- cw_load_records: packed records INTO envs.  The pure calls above only compare a record's cells; a loaded record becomes engine state -- the dirty-cell
// painter turns the agent's cell into an address, the colour tables are indexed by code -- so an env takes a record only after THE RULE, shared by the kernel
// and the host.  hdr and slot_pos as the four little-endian dwords of a record each (the uint4 the kernels load), S the grid size.  A record passes iff the
// agent's row and column are below S, hold <= 3, every slot code <= 8, every slot is one of gone (0xFFFF) with code 0 / held (0xFFFE) with code == hold != 0 /
// on the grid (below S * S) with a code -- any other position or pairing fails --, exactly one slot is held if hold != 0 and none otherwise, and the
// on-grid positions are pairwise different (the sparse layout's "one object per cell").  The masks, step_num, the flag word and the menu byte are free.
static inline CWH_HOST_DEVICE int cwh_record_ok(uint32_t size, const uint32_t hdr[4], const uint32_t pos[4])
{
    const uint32_t hold = (hdr[0] >> 16) & 0xFFu, ncell = size * size;
    int ok = (hdr[0] & 0xFFu) < size && ((hdr[0] >> 8) & 0xFFu) < size && hold <= 3u;
    uint32_t p[8], held = 0;
    for (int k = 0; k < 8; k++) {
        const uint32_t code = (hdr[3] >> (4 * k)) & 15u;
        p[k] = (pos[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
        const int gone = p[k] == 0xFFFFu && code == 0u, in_hand = p[k] == 0xFFFEu && code == hold && hold != 0u, on_grid = p[k] < ncell && code != 0u;
        ok &= code <= 8u && (gone || in_hand || on_grid);
        held += p[k] == 0xFFFEu;
    }
    ok &= held == (hold != 0u ? 1u : 0u);
    for (int k = 1; k < 8; k++)
        for (int j = 0; j < k; j++) ok &= p[k] >= 0xFFFEu || p[k] != p[j];
    return ok;
}
int cwh_record_ok_of(uint32_t size, const uint8_t *hdr /* [16] */, const uint16_t *slot_pos /* [8] */);       // (exported for the CPU tests; any alignment)
// THE index check of cw_load_records_kernel, shared by host and device: an entry of the caller's src array may index the records only if this says so
static inline CWH_HOST_DEVICE int cwh_load_record_index_ok(int32_t index, int32_t n_records) { return index >= 0 && index < n_records; }
int cwh_load_record_index_in_range(int32_t index, int32_t n_records);      // (the same, exported for the CPU tests)
// what cw_load_records_kernel leaves in status[env]
enum { CWH_LOAD_NO_PART = 0, CWH_LOAD_LOADED = 1, CWH_LOAD_BAD_INDEX = 2, CWH_LOAD_REFUSED = 3 };
// the argument rules of cw_load_records, in the order they are tested; addresses as integers (0: null): records given (CWH_LOAD_NO_RECORDS), 0 <= n_records <=
// CWH_MAX_STATES (CWH_LOAD_N_RECORDS), without src n_records = num_envs (CWH_LOAD_OWN_ORDER), hdr and slot_pos 16-byte aligned and src 4-byte aligned
// (CWH_LOAD_ALIGN), the records sharing no byte with the engine's own hdr / slot_pos arrays -- engine_hdr, engine_slot_pos: 16 * num_envs bytes each; env i
// would be written while env j reads it -- (CWH_LOAD_ENGINE_OVERLAP), status sharing no byte with the records or src (CWH_LOAD_STATUS_OVERLAP)
enum { CWH_LOAD_OK = 0, CWH_LOAD_NO_RECORDS = 1, CWH_LOAD_N_RECORDS = 2, CWH_LOAD_OWN_ORDER = 3, CWH_LOAD_ALIGN = 4, CWH_LOAD_ENGINE_OVERLAP = 5,
       CWH_LOAD_STATUS_OVERLAP = 6 };
int cwh_load_records_args(int32_t num_envs, uint64_t src, uint64_t hdr, uint64_t slot_pos, int32_t n_records, uint64_t status, uint64_t engine_hdr,
                          uint64_t engine_slot_pos);

// ---- cw_replay_*: the replay buffer of packed records (include/craftingworld.h states it).  THE REWARD of a relabelled row, shared by the sample kernel and
// the host: -1 unless the stored transition changed the state; then max_steps iff the goal g holds of the successor's achieved mask a under the task mask --
// subset == 0: a == g; else (g & ~a) == 0 and some position equal -- the expressions of step_env and of compute_reward_batch.
static inline CWH_HOST_DEVICE int32_t cwh_replay_reward(uint32_t achieved, uint32_t goal, uint32_t task_mask, int subset, int changed, int32_t max_steps)
{
    if (!changed) return -1;
    const uint32_t am = achieved & task_mask, dm = goal & task_mask;
    const int hit = subset ? ((dm & ~am) == 0u && ((~(dm ^ am)) & task_mask) != 0u) : am == dm;
    return hit ? max_steps : -1;
}
int32_t cwh_replay_reward_of(uint32_t achieved, uint32_t goal, uint32_t task_mask, int subset, int changed, int32_t max_steps);   // (exported for the CPU tests)
// the buffer of `steps` slots of `num_envs` transitions: CWH_REPLAY_SECTIONS sections, each a multiple of CWH_SNAP_ALIGN bytes, in this order -- the control
// block (CWH_REPLAY_CTL_BYTES), env_episode (4 bytes an env), the six record arrays (16 bytes a transition each), reward and episode (4 each), action and
// flags (1 each): 106 bytes a transition.  Writes the sections' offsets (may be null); -> the bytes, -1 outside the limits: steps 1 .. CWH_REPLAY_MAX_STEPS,
// num_envs >= 1, steps * num_envs < 2^31 (the total then stays below 2^38).
#define CWH_REPLAY_MAX_STEPS (1 << 24)
#define CWH_REPLAY_CTL_BYTES 256
enum { CWH_REPLAY_S_CTL = 0, CWH_REPLAY_S_ENV_EPISODE, CWH_REPLAY_S_HDR, CWH_REPLAY_S_POS, CWH_REPLAY_S_NEXT_HDR, CWH_REPLAY_S_NEXT_POS, CWH_REPLAY_S_GOAL_HDR,
       CWH_REPLAY_S_GOAL_POS, CWH_REPLAY_S_REWARD, CWH_REPLAY_S_EPISODE, CWH_REPLAY_S_ACTION, CWH_REPLAY_S_FLAGS, CWH_REPLAY_SECTIONS };
int64_t cwh_replay_layout(int32_t steps, int32_t num_envs, uint64_t *offsets);
int64_t cwh_replay_bytes_of(int32_t steps, int32_t num_envs);
// the argument rules of cw_replay_sample, in the order they are tested; fields: the CWH_REPLAY_FIELDS addresses of cw_replay_out in its order, as integers
// (0: null): 0 <= n_rows <= CWH_MAX_STATES (CWH_REPLAY_N_ROWS), her <= 65 536 (CWH_REPLAY_HER), strategy 0 or 1 (CWH_REPLAY_STRATEGY), some field given
// (CWH_REPLAY_NO_FIELD), the six record fields 16-byte, reward / env / slot / future 4-byte and desired 2-byte aligned (CWH_REPLAY_ALIGN), no two fields
// sharing a byte of their n_rows rows (CWH_REPLAY_OVERLAP).
#define CWH_REPLAY_FIELDS 13
enum { CWH_REPLAY_OK = 0, CWH_REPLAY_N_ROWS = 1, CWH_REPLAY_HER = 2, CWH_REPLAY_STRATEGY = 3, CWH_REPLAY_NO_FIELD = 4, CWH_REPLAY_ALIGN = 5,
       CWH_REPLAY_OVERLAP = 6 };
int cwh_replay_sample_args(int32_t n_rows, uint32_t her, int32_t strategy, const uint64_t *fields);
int cwh_replay_field_bytes_of(int field);          // bytes a row of field 0 .. CWH_REPLAY_FIELDS - 1 takes (16, 1, 4 or 2); 0 for any other number

// ---- cw_reach: breadth-first search on the device (cw_reach_reserve / cw_reach).  THE ROWS of a level over a frontier of F states: row a * Fp + j is action a
// on frontier state j, Fp = F rounded up to a wavefront, so that no wave straddles two actions; rows j >= F of an action take no part.  The order is the one
// a * F + j gives.  The row is the row field of the visited set's bids: 6 * (max_rows + 63) < 2^CWH_SEEN_ROW_BITS is the cap on max_rows.
// max_depth: 1 .. CWH_REACH_MAX_DEPTH = CWH_SIM_MAX_STEPS (a plan feeds cw_simulate); the workspace then stays below 2^43 bytes, far inside int64.
#define CWH_REACH_CHUNK 4096        // rows a workgroup of 256 lanes compacts at a time: 16 flag bytes (one 16-byte load) a lane
#define CWH_REACH_MAX_ROWS (((1ll << CWH_SEEN_ROW_BITS) - 1) / 6 - 63)
#define CWH_REACH_MAX_DEPTH CWH_SIM_MAX_STEPS
#define CWH_REACH_BLOCKS_PER_CU 8   // workgroups of 256 per CU at most: the grid-stride kernels of a level (the visited set's own shape)
static inline CWH_HOST_DEVICE int64_t cwh_reach_padded(int64_t f) { return (f + CW_WAVE - 1) / CW_WAVE * CW_WAVE; }
static inline CWH_HOST_DEVICE int64_t cwh_reach_rows(int64_t f) { return 6 * cwh_reach_padded(f); }                       // rows of a level over F states
static inline CWH_HOST_DEVICE int64_t cwh_reach_chunks(int64_t rows) { return (rows + CWH_REACH_CHUNK - 1) / CWH_REACH_CHUNK; }
// workgroups of 256 lanes for `items` items, one lane each, grid-stride: ceil(items / 256), 1 at least, n_cu * CWH_REACH_BLOCKS_PER_CU at most
static inline int64_t cwh_reach_grid(int64_t items, int32_t n_cu)
{
    const int64_t want = (items + 255) / 256, most = (int64_t)n_cu * CWH_REACH_BLOCKS_PER_CU;
    return want < most ? (want < 1 ? 1 : want) : most;
}
int64_t cwh_reach_rows_of(int64_t f);                  // (the same, exported for the CPU tests)
int64_t cwh_reach_chunks_of(int64_t rows);
int64_t cwh_reach_grid_of(int64_t items, int32_t n_cu);
// THE WORKSPACE: one allocation, its sections in this order, each starting on a CWH_SNAP_ALIGN boundary.  ctl: CWH_REACH_CTL_WORDS int32 (the stop flag, the
// searched depth), then the frontier's size per level [max_depth + 1] and the scan's scratch, one int32 per chunk of the largest level.  Two frontiers (record,
// env, start row: 40 bytes a row), the successors of one level (record, group, fresh flag: 37 bytes for each of the 6 * padded(max_rows) rows, the flags padded
// to whole chunks), the links of every level but the last (parent << 3 | action: 4 bytes a row and level), and per start row dist, the solving link, the bid
// (the smallest solving row of the level in hand) and active: 13 bytes.  Writes CWH_REACH_SECTIONS offsets (may be null); -> the bytes, -1 outside the limits
// (max_rows 1 .. CWH_REACH_MAX_ROWS, max_depth 1 .. CWH_REACH_MAX_DEPTH).
#define CWH_REACH_CTL_WORDS 64
enum { CWH_REACH_STOP = 0, CWH_REACH_SEARCHED = 1 };
enum { CWH_REACH_S_CTL = 0, CWH_REACH_S_F_HDR0, CWH_REACH_S_F_POS0, CWH_REACH_S_F_ENV0, CWH_REACH_S_F_START0, CWH_REACH_S_F_HDR1, CWH_REACH_S_F_POS1,
       CWH_REACH_S_F_ENV1, CWH_REACH_S_F_START1, CWH_REACH_S_HDR, CWH_REACH_S_POS, CWH_REACH_S_GRP, CWH_REACH_S_FRESH, CWH_REACH_S_LINKS, CWH_REACH_S_DIST,
       CWH_REACH_S_SOL, CWH_REACH_S_BID, CWH_REACH_S_ACTIVE, CWH_REACH_SECTIONS };
int64_t cwh_reach_layout(int64_t max_rows, int32_t max_depth, uint64_t *offsets);
int64_t cwh_reach_bytes_of(int64_t max_rows, int32_t max_depth);
// the argument rules of cw_reach, in the order they are tested; addresses as integers (0: null): some output (CWH_REACH_NO_FIELD), 0 <= n_states <=
// CWH_REACH_MAX_ROWS (CWH_REACH_N_STATES), 1 <= max_depth <= CWH_REACH_MAX_DEPTH (CWH_REACH_DEPTH), hdr_in and slot_pos_in together (CWH_REACH_PAIR), env_of
// only with them (CWH_REACH_ENV_OF), without them n_states = num_envs (CWH_REACH_OWN_STATES), hdr_in and slot_pos_in 16-byte aligned and env_of, distance,
// frontier, searched_depth 4-byte aligned (CWH_REACH_ALIGN), no output sharing a byte with hdr_in, slot_pos_in, env_of or another output (CWH_REACH_OVERLAP)
enum { CWH_REACH_OK = 0, CWH_REACH_NO_FIELD = 1, CWH_REACH_N_STATES = 2, CWH_REACH_DEPTH = 3, CWH_REACH_PAIR = 4, CWH_REACH_ENV_OF = 5, CWH_REACH_OWN_STATES = 6,
       CWH_REACH_ALIGN = 7, CWH_REACH_OVERLAP = 8 };
int cwh_reach_args(int32_t num_envs, uint64_t env_of, uint64_t hdr_in, uint64_t slot_pos_in, int32_t n_states, int32_t max_depth, uint64_t distance,
                   uint64_t plan, uint64_t first_action, uint64_t frontier, uint64_t searched_depth);

// ---- the GUARD of the sweep's clock as a pure state machine (cw_engine.cpp: sweep_guard_tick feeds it one timed sweep at a time; nothing here
// touches HIP).  Rates in TB/s, times in ms.  DESIGN.md 4.3; the constants are the ones round 4/5 measured (profiles/r04_clock.txt, r05_experiments.txt).
typedef struct cwh_guard {
    double rate;            // the clock's current rate
    double rate_top;        // the best rate known to hold: cw_create's choice, raised by a probe that paid
    double ms_sum;          // sweep times sampled at the current rate (decayed: the last ~100)
    double prev_mean;       // their mean at the rate a running trial left
    double ref_ms;          // what the current rate delivered when a trial ACCEPTED it (its yardstick if that is more than its schedule)
    double ref_prev;        // ... the one of the rate a running trial left
    int32_t ms_n;
    int32_t late;           // samples late in a row
    int32_t good;           // samples on time, "mostly in a row" (a late one costs 8)
    int32_t slowdowns;      // moves down that were not the end of a trial
    int32_t probes;         // trials beyond rate_top started
    int32_t probe_need;     // samples on time before the next probe (doubles after one that did not pay, capped)
    int32_t recover_need;   // ... before the next step back towards rate_top after a slowdown
    int32_t probing;        // a TRIAL is running: one notch up, verdict after CWH_GUARD_PROBE_SAMPLES samples
    int32_t recovering;     // ... and it is a step back towards rate_top, not beyond it
} cwh_guard;

enum { CWH_GUARD_NONE = 0, CWH_GUARD_SLOWDOWN = 1, CWH_GUARD_TRIAL_UP = 2, CWH_GUARD_TRIAL_KEPT = 3, CWH_GUARD_TRIAL_UNDONE = 4 };
#define CWH_GUARD_RECOVER 64
#define CWH_GUARD_PROBE_SAMPLES 32
#define CWH_GUARD_NEED_MAX 2048
#define CWH_GUARD_RATE_FLOOR 5.0
#define CWH_GUARD_RATE_CEILING 7.7
#define CWH_GUARD_NOTCH 0.2

void cwh_guard_init(cwh_guard *g, double rate);
// One timed sweep at the CURRENT rate: `ms` measured, `scheduled_ms` what its clock promises (cwh_guard_scheduled_ms).  Returns what the guard
// does about it (CWH_GUARD_*); on every action but NONE and TRIAL_KEPT g->rate has changed and the caller re-programs the clock.
int cwh_guard_step(cwh_guard *g, double ms, double scheduled_ms);
// The three periods of the clock at a rate, in 1/16 of a 10-ns tick (0 at rate 0 = unclocked): a wave starts a 4-KiB piece every period; a launch's
// first CWH_HEAD_JOBS jobs run head_notch TB/s slower, those after a step on which envs finished busy_notch slower (never under the floor).
#define CWH_HEAD_JOBS 64
void cwh_sweep_periods(double rate, int32_t sweep_waves, double head_notch, double busy_notch, int32_t *period16, int32_t *period16_head, int32_t *period16_busy);
// What a sweep of `sweep_jobs` jobs per wave should take with those periods, after a busy step, plus what a launch costs beside its jobs
double cwh_guard_scheduled_ms(double sweep_jobs, int32_t period16, int32_t period16_busy, double beside_ms);

// ---- the look-ahead refill period follows the episodes (cw_engine.cpp: la_adapt).  `slow_delta` slow-path resets were counted since the last refill was
// enqueued (read from a pinned word the refill kernels write; stale by a period, never waited for): more than an eighth of the period's steps -> half the
// period (CWH_LA_PERIOD_MIN at least); at most a 32nd of them for CWH_LA_QUIET refills in a row -> twice the period (period_max at most).  -> the new period.
#define CWH_LA_PERIOD_MIN 8
#define CWH_LA_QUIET 8
int32_t cwh_la_adapt(int32_t period, int32_t period_max, uint64_t slow_delta, int32_t *quiet);

// ---- the CW_TUNE_* variables (cw_engine.cpp: read_tuning, once at cw_create).  `t` holds the defaults on entry; a variable whose text is
// a number in its range replaces its field.  Text that is empty, not a number, has trailing characters, does not fit, or is nan / inf keeps the default,
// like a value out of range; whitespace around the number is accepted.  `lookup` maps a variable's name to its text (null: unset) -- getenv, or a test's dict.
typedef struct cwh_tuning {
    int32_t render_chunk_rounds;    // CW_TUNE_RENDER_CHUNK_ROUNDS >= 0
    int32_t step_envs_per_wave;     // CW_TUNE_STEP_ENVS_PER_WAVE 8 / 16 / 32 / 64
    int32_t gather;                 // CW_TUNE_GATHER any int (0: off)
    int32_t gather_max_size;        // CW_TUNE_GATHER_MAX_SIZE 0 .. 9
    int32_t small_frame_bytes;      // CW_TUNE_SMALL_FRAME_BYTES >= 0
    int32_t small_blocks_per_cu;    // CW_TUNE_SMALL_BLOCKS 1 .. 8
    int32_t small_launch_mb;        // CW_TUNE_SMALL_LAUNCH_MB >= 0
    int32_t reset_blocks_per_cu;    // CW_TUNE_RESET_BLOCKS 1 .. 16
    int32_t guard;                  // CW_TUNE_GUARD any int -> 0 / 1
    int32_t verbose;                // CW_TUNE_VERBOSE: 1 when set at all, whatever its text ("0" included)
    int32_t lookahead;              // CW_TUNE_LOOKAHEAD any int -> 0 / 1
    int32_t la_period;              // CW_TUNE_LA_PERIOD >= 1 (the default 0: adaptive)
    int32_t rollout_segment;        // CW_TUNE_ROLLOUT_SEGMENT >= -1
    int32_t pad;
    double head_notch;              // CW_TUNE_HEAD_NOTCH >= 0
    double busy_notch;              // CW_TUNE_BUSY_NOTCH >= 0
    double period_ns;               // CW_TUNE_PERIOD_NS >= 0 (the default -1: none)
    double rate_tbs;                // CW_TUNE_RATE_TBS >= 0 (the default -1: none)
} cwh_tuning;
typedef const char *(*cwh_lookup)(void *ctx, const char *name);
void cwh_read_tuning(cwh_lookup lookup, void *ctx, cwh_tuning *t);

#ifdef __cplusplus
}
#endif
