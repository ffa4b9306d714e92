// cw_host.cpp -- the engine's HIP-free host logic (cw_host.h): no HIP header, no engine struct.  Built into libcraftingworld.so, and alone under
// ASAN/UBSAN for the CPU test tier (make host_asan).
#include "cw_host.h"

#include <algorithm>
#include <cerrno>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>

// ------------------------------------------------------------------------------ MT19937 (host)
// numpy RandomState (key, pos)  <->  the engine's consume-and-replace form (cw_mt.h).
static inline uint32_t mt_twist(uint32_t cur, uint32_t nxt, uint32_t far)
{
    const uint32_t y = (cur & 0x80000000u) | (nxt & 0x7fffffffu);
    return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

extern "C" {

// in place: words < pos become next-generation (numpy's twist loop, first `pos` iterations);
// returns the engine index (pos mod 624)
int cwh_mt_from_numpy(uint32_t *s, int pos)
{
    if (pos < 0) pos = 0;
    if (pos > CWH_MT_N) pos = CWH_MT_N;
    for (int k = 0; k < pos; k++)
        s[k] = mt_twist(s[k], s[(k + 1) % CWH_MT_N], s[(k + 397) % CWH_MT_N]);
    return pos % CWH_MT_N;
}

// inverse: from engine form (s, idx) recover a numpy key whose stream from position idx is
// identical.  Words < idx are un-twisted; key[0]'s low 31 bits are not part of the MT19937 state and
// cannot be un-twisted ...
void cwh_mt_to_numpy(const uint32_t *s, int idx, uint32_t *key)
{
    for (int j = idx; j < CWH_MT_N; j++) key[j] = s[j];
    for (int j = 0; j < idx; j++) key[j] = 0;
    for (int j = idx - 1; j >= 0; j--) {
        const uint32_t m = (j < CWH_MT_N - 397) ? key[j + 397] : s[j - (CWH_MT_N - 397)];
        uint32_t t = s[j] ^ m;
        const uint32_t odd = t >> 31;
        if (odd) t ^= 0x9908b0dfu;
        const uint32_t y = (t << 1) | odd;     // (G[j] & UPPER) | (G[j+1] & LOWER)
        key[j] |= y & 0x80000000u;
        if (j + 1 < idx) key[j + 1] |= y & 0x7fffffffu;
    }
    if (idx > 0) {     // ... but they are what the generation's word 623 was made with: key[623] = key[396] ^ T(previous[623].hi, key[0].lo)
        uint32_t t = key[CWH_MT_N - 1] ^ key[396];
        const uint32_t odd = t >> 31;
        if (odd) t ^= 0x9908b0dfu;
        key[0] |= ((t << 1) | odd) & 0x7fffffffu;      // (exact for every key a twist produced; a rewind to position 0 reads this word again)
    }
}

// One generation back: key = all 624 words of a generation as numpy holds them after its twist -> the generation before (whose twist
// produced it).  The twist is a bijection on the 19 937 state bits (word 0 counts with its top bit only): word k >= 227 of the new
// generation is new[k-227] ^ T(old[k].hi, old[k+1].lo), word 623 new[396] ^ T(old[623].hi, new[0].lo), word k < 227 old[k+397] ^ T(...);
// T(y) = (y >> 1) ^ (y odd ? 0x9908b0df : 0) is undone through its top bit.  The low 31 bits of key[0] (not part of the state; the export
// above restores them from words 623 and 396) are REPAIRED on the way in -- the step for word 227 needs them -- and restored in the result.
void cwh_mt_untwist(uint32_t *key)
{
    uint32_t prev[CWH_MT_N];
    memset(prev, 0, sizeof(prev));
    for (int k = CWH_MT_N - 1; k >= 0; k--) {
        uint32_t t = key[k] ^ (k == CWH_MT_N - 1 ? key[396] : k >= CWH_MT_N - 397 ? key[k - (CWH_MT_N - 397)] : prev[k + 397]);
        const uint32_t odd = t >> 31;
        if (odd) t ^= 0x9908b0dfu;
        const uint32_t y = (t << 1) | odd;
        prev[k] |= y & 0x80000000u;
        if (k == CWH_MT_N - 1) key[0] = (key[0] & 0x80000000u) | (y & 0x7fffffffu);
        else prev[k + 1] |= y & 0x7fffffffu;
    }
    uint32_t t = prev[CWH_MT_N - 1] ^ prev[396];          // prev[0]'s own low bits, the same way (cwh_mt_to_numpy): a rewind may stop at position 0
    const uint32_t odd = t >> 31;
    if (odd) t ^= 0x9908b0dfu;
    prev[0] |= ((t << 1) | odd) & 0x7fffffffu;
    memcpy(key, prev, sizeof(prev));
}
// numpy state (key, pos) -> the state n raw draws earlier (a look-ahead record's draws, cw_get_mt); pos stays in 0..623 like the export's
void cwh_mt_rewind(uint32_t *key, int32_t *pos, uint32_t n)
{
    while (n > 0) {
        if ((uint32_t)*pos >= n) { *pos -= (int32_t)n; n = 0; }
        else { n -= (uint32_t)*pos; cwh_mt_untwist(key); *pos = CWH_MT_N; }
    }
}

// ------------------------------------------------------------------------------ DLPack producer
// Non-owning DLManagedTensor over engine memory (DLPack ABI v0: the struct layout below is the
// published one).  Produced and freed in C so that no Python callback is involved when a consumer
// (torch) drops its last view -- possibly during interpreter shutdown.
struct CwDLDevice { int32_t device_type, device_id; };
struct CwDLDataType { uint8_t code, bits; uint16_t lanes; };
struct CwDLTensor { void *data; CwDLDevice device; int32_t ndim; CwDLDataType dtype; int64_t *shape, *strides; uint64_t byte_offset; };
struct CwDLManagedTensor { CwDLTensor dl_tensor; void *manager_ctx; void (*deleter)(CwDLManagedTensor *); };

static void cw_dl_deleter(CwDLManagedTensor *m)
{
    if (!m) return;
    free(m->dl_tensor.shape);
    free(m);
}

// device_type 10 = kDLROCM; code 0 int / 1 uint; returns a malloc'ed DLManagedTensor* (or NULL)
void *cwh_dlpack_make(void *data, int device_id, int code, int bits, int ndim, const int64_t *shape)
{
    CwDLManagedTensor *m = (CwDLManagedTensor *)calloc(1, sizeof(CwDLManagedTensor));
    int64_t *shp = (int64_t *)malloc(sizeof(int64_t) * (size_t)(ndim > 0 ? ndim : 1));
    if (!m || !shp) { free(m); free(shp); return nullptr; }
    for (int i = 0; i < ndim; i++) shp[i] = shape[i];
    m->dl_tensor.data = data;
    m->dl_tensor.device = CwDLDevice{10, device_id};
    m->dl_tensor.ndim = ndim;
    m->dl_tensor.dtype = CwDLDataType{(uint8_t)code, (uint8_t)bits, 1};
    m->dl_tensor.shape = shp;
    m->dl_tensor.strides = nullptr;
    m->dl_tensor.byte_offset = 0;
    m->deleter = cw_dl_deleter;
    return m;
}

void cwh_mt_init_genrand(uint32_t *s, uint32_t seed)   // numpy RandomState(int): init_genrand
{
    s[0] = seed;
    for (int i = 1; i < CWH_MT_N; i++) s[i] = 1812433253u * (s[i - 1] ^ (s[i - 1] >> 30)) + (uint32_t)i;
}

}  // extern "C"


extern "C" {

// ------------------------------------------------------------------------------ dense view of a slot record
void cwh_slots_to_grid(const uint16_t *pos, uint32_t codes, int ncell, uint8_t *grid)
{
    memset(grid, 0, (size_t)ncell);
    for (int k = 0; k < 8; k++)
        if (pos[k] < (uint32_t)ncell) grid[pos[k]] = (uint8_t)((codes >> (4 * k)) & 15u);
}

// ------------------------------------------------------------------------------ checkpoint blob sections (cw_engine.cpp: ckpt_sections pairs them with device pointers)
// hdr, pos, init_pos, goal_pos (16 B / env), goal_codes (4), init_agent, goal_agent (2), ep_no (4), mt (624 x 4), mt_idx (4), pool (k x 9 x 2),
// reward (4), done (1), achieved_out, desired_out (2), episode_length, episode_return (4), counters (5 x 8: the four public ones + the sweep's
// private word), then the look-ahead records verbatim -- la_depth of them per env (0: the engine keeps none): nx_init_pos, nx_goal_pos, nx_misc (16 each per
// record), nx_ctl (4: the ring's head and the QUEUED bit)
int cwh_ckpt_section_bytes(int64_t n, int32_t k, int32_t la_depth, size_t *sizes, uint64_t *total)
{
    const size_t N = n > 0 ? (size_t)n : 0, K = k > 0 ? (size_t)k : 0, D = la_depth > 0 ? (size_t)la_depth : 0, la = D ? 1 : 0;
    const size_t sz[CWH_CKPT_SECTIONS] = {N * 16, N * 16, N * 16, N * 16, N * 4, N * 2, N * 2, N * 4, N * CWH_MT_N * 4, N * 4, N * K * 9 * 2,
                                          N * 4, N, N * 2, N * 2, N * 4, N * 4, 5 * 8,
                                          D * N * 16, D * N * 16, D * N * 16, la * N * 4};
    uint64_t sum = 0;
    for (int i = 0; i < CWH_CKPT_SECTIONS; i++) { if (sizes) sizes[i] = sz[i]; sum += sz[i]; }
    if (total) *total = sum;
    return CWH_CKPT_SECTIONS;
}

// ------------------------------------------------------------------------------ snapshot bank sections (cw_engine.cpp: cw_snapshot_reserve pairs them with pointers)
int cwh_snapshot_section_bytes(int64_t rows, int32_t k, int32_t la_depth, size_t *sizes, size_t *offsets, uint64_t *total, uint64_t *row_bytes)
{
    const size_t R = rows > 0 ? (size_t)rows : 0, K = k > 0 ? (size_t)k : 0, D = la_depth > 0 ? (size_t)la_depth : 0, la = D ? 1 : 0;
    const size_t per_row[CWH_SNAP_SECTIONS] = {16, 16, 16, 16, 4, 4, 2, 2, CWH_MT_N * 4, 4, D * 16, D * 16, D * 16, la * 4, K * 9 * 2, 1};
    uint64_t bytes[CWH_SNAP_SECTIONS], at[CWH_SNAP_SECTIONS], row = 0;
    for (int i = 0; i < CWH_SNAP_SECTIONS; i++) { bytes[i] = per_row[i] * R; row += per_row[i]; }
    const uint64_t all = cwh_sections_layout(bytes, CWH_SNAP_SECTIONS, CWH_SNAP_ALIGN, at);
    for (int i = 0; i < CWH_SNAP_SECTIONS; i++) { if (sizes) sizes[i] = (size_t)bytes[i]; if (offsets) offsets[i] = (size_t)at[i]; }
    if (total) *total = all;
    if (row_bytes) *row_bytes = row;
    return CWH_SNAP_SECTIONS;
}
int cwh_snapshot_row_in_bank(int32_t row, int32_t capacity) { return cwh_snapshot_row_ok(row, capacity); }
int cwh_expand_env_in_batch(int32_t env, int32_t num_envs) { return cwh_expand_env_ok(env, num_envs); }
uint32_t cwh_alt_pixel_offset_of(uint32_t size, uint32_t pos, uint32_t item) { return cwh_alt_pixel_offset(size, pos, item); }
int cwh_reset_grid_of(int jobs, int n_cu, int reset_blocks_per_cu) { return cwh_reset_grid(jobs, n_cu, reset_blocks_per_cu); }
int cwh_masked_launch_of(int n_envs, int n_cu, int reset_blocks_per_cu, int *blocks) { return cwh_masked_launch(n_envs, n_cu, reset_blocks_per_cu, blocks); }
int cwh_envs_per_wave_of(int n, int most) { return cwh_envs_per_wave(n, most); }
int cwh_piece_chunks_of(int n_envs, uint32_t frame_bytes, int n_cu, int render_chunk_rounds, int *per)
{
    return cwh_piece_chunks(n_envs, frame_bytes, n_cu, render_chunk_rounds, per);
}

// ------------------------------------------------------------------------------ the argument rules of a call that reads packed records
int cwh_records_args(int32_t num_envs, int has_env_of, int has_hdr_in, int has_slot_pos_in, int32_t n_states, int32_t n_steps, int n_out_fields,
                     int32_t max_steps, int broadcast)
{
    if (n_out_fields <= 0) return CWH_REC_NO_FIELD;
    if (n_states < 0 || n_states > CWH_MAX_STATES) return CWH_REC_N_STATES;
    if (max_steps > 0 && (n_steps < 1 || n_steps > max_steps)) return CWH_REC_N_STEPS;
    if (!has_hdr_in != !has_slot_pos_in) return CWH_REC_PAIR;
    if (has_env_of && !has_hdr_in) return CWH_REC_ENV_OF;
    if (!has_hdr_in && (broadcast ? num_envs <= 0 || n_states <= 0 || n_states % num_envs != 0 : n_states != num_envs)) return CWH_REC_OWN_STATES;
    return CWH_REC_OK;
}

int cwh_plan_args(int32_t num_envs, int has_env_of, int has_hdr_in, int has_slot_pos_in, int32_t n_states, int32_t depth, int n_out_fields)
{
    const int rc = cwh_records_args(num_envs, has_env_of, has_hdr_in, has_slot_pos_in, n_states, depth, n_out_fields, CWH_PLAN_MAX_DEPTH, 0);
    if (rc == CWH_REC_NO_FIELD || rc == CWH_REC_N_STATES || rc == CWH_REC_N_STEPS) return rc;
    uint64_t leaves = (uint64_t)n_states;                             // (<= 2^27, times 6^8 < 2^21: no overflow)
    for (int32_t d = 0; d < depth; d++) leaves *= 6u;
    if (leaves > CWH_PLAN_MAX_LEAVES) return CWH_REC_PLAN_WORK;
    return rc;
}

int cwh_unroll_args(int32_t num_envs, int has_env_of, int has_hdr_in, int has_slot_pos_in, int32_t n_states, int32_t n_steps, int n_out_fields)
{
    const int rc = cwh_records_args(num_envs, has_env_of, has_hdr_in, has_slot_pos_in, n_states, n_steps, n_out_fields, CWH_SIM_MAX_STEPS, 1);
    if (rc == CWH_REC_NO_FIELD || rc == CWH_REC_N_STATES || rc == CWH_REC_N_STEPS) return rc;
    if (((uint64_t)n_steps + 1u) * (uint64_t)n_states > (uint64_t)CWH_MAX_STATES) return CWH_REC_UNROLL_ROWS;      // (<= 2^15 * 2^27)
    return rc;
}

int cwh_shoot_args(int32_t num_envs, int has_env_of, int has_hdr_in, int has_slot_pos_in, int32_t n_states, int32_t n_steps, int32_t n_samples,
                   int n_out_fields)
{
    const int rc = cwh_records_args(num_envs, has_env_of, has_hdr_in, has_slot_pos_in, n_states, n_steps, n_out_fields, CWH_SIM_MAX_STEPS, 0);
    if (rc == CWH_REC_NO_FIELD || rc == CWH_REC_N_STATES || rc == CWH_REC_N_STEPS) return rc;
    if (n_samples < 1 || n_samples > CWH_SHOOT_MAX_SAMPLES) return CWH_REC_SHOOT_SAMPLES;
    if ((uint64_t)n_states * (uint64_t)n_samples * (uint64_t)n_steps > CWH_SHOOT_MAX_WORK) return CWH_REC_SHOOT_WORK;      // (<= 2^27 * 2^16 * 2^15)
    return rc;
}

int cwh_shoot_actions_args(int32_t n_states, int32_t n_steps, int32_t n_rows)
{
    if (n_states < 0 || n_states > CWH_MAX_STATES) return CWH_REC_N_STATES;
    if (n_rows < 0 || n_rows > CWH_MAX_STATES) return CWH_REC_SHOOT_SAMPLES;
    if (n_steps < 1 || n_steps > CWH_SIM_MAX_STEPS) return CWH_REC_N_STEPS;
    const uint64_t columns = (uint64_t)n_rows * (uint64_t)n_states;   // (<= 2^54)
    if (columns > CWH_SHOOT_MAX_WORK || columns * (uint64_t)n_steps > CWH_SHOOT_MAX_WORK) return CWH_REC_SHOOT_WORK;
    return CWH_REC_OK;
}

uint32_t cwh_shoot_draw_of(uint64_t seed, uint32_t state, uint32_t sample, uint32_t step) { return cwh_shoot_draw(seed, state, sample, step); }
uint32_t cwh_shoot_action_of(uint64_t seed, uint32_t state, uint32_t sample, uint32_t step, const uint16_t *weights)
{
    return cwh_shoot_action(cwh_shoot_draw(seed, state, sample, step), weights, 1);
}
int cwh_shoot_lanes_of(int32_t n_states, int32_t n_samples) { return cwh_shoot_lanes(n_states, n_samples); }

int cwh_ranges_overlap(uint64_t a, uint64_t a_bytes, uint64_t b, uint64_t b_bytes)
{
    if (!a_bytes || !b_bytes) return 0;
    const uint64_t a_end = a + a_bytes < a ? UINT64_MAX : a + a_bytes, b_end = b + b_bytes < b ? UINT64_MAX : b + b_bytes;
    return a < b_end && b < a_end;
}

// ------------------------------------------------------------------------------ the span checker and the section layout
int cwh_spans_misaligned(const cwh_span *spans, int n)
{
    for (int i = 0; i < n; i++)
        if (spans[i].at && spans[i].align && spans[i].at % spans[i].align) return i;
    return -1;
}

static bool spans_share(const cwh_span &a, const cwh_span &b) { return a.at && b.at && cwh_ranges_overlap(a.at, a.bytes, b.at, b.bytes); }
int cwh_spans_clash(const cwh_span *outs, int n_outs, const cwh_span *ins, int n_ins, int among_outs, int *other)
{
    for (int o = 0; o < n_outs; o++) {
        int hit = -1;
        for (int i = 0; i < n_ins && hit < 0; i++)
            if (spans_share(outs[o], ins[i])) hit = i;
        for (int q = o + 1; among_outs && q < n_outs && hit < 0; q++)
            if (spans_share(outs[o], outs[q])) hit = n_ins + q;
        if (hit < 0) continue;
        if (other) *other = hit;
        return o;
    }
    return -1;
}

uint64_t cwh_sections_layout(const uint64_t *bytes, int n, uint64_t align, uint64_t *offsets)
{
    uint64_t at = 0;
    if (!align) align = 1;
    for (int i = 0; i < n; i++) {
        if (offsets) offsets[i] = at;
        at += (bytes[i] + align - 1) / align * align;
    }
    return at;
}

// ------------------------------------------------------------------------------ cw_shoot_refit: the weight, the grid, the argument rules
uint32_t cwh_refit_weight_of(uint32_t smooth, uint32_t gain, uint32_t count) { return cwh_refit_weight(smooth, gain, count); }
int64_t cwh_refit_grid_of(int64_t items, int32_t n_cu) { return cwh_refit_grid(items, n_cu); }

int cwh_refit_args(uint64_t env_of, int32_t n_states, int32_t n_steps, int32_t n_samples, int32_t n_elites, uint64_t weights_in, uint64_t ret, uint32_t smooth,
                   uint32_t gain, uint64_t elites, uint64_t weights, uint64_t elite_min)
{
    if (!ret || !elites) return CWH_REFIT_NULL;
    if (n_states < 0 || n_states > CWH_MAX_STATES) return CWH_REFIT_N_STATES;
    if (n_steps < 1 || n_steps > CWH_SIM_MAX_STEPS) return CWH_REFIT_N_STEPS;
    if (n_samples < 1 || n_samples > CWH_SHOOT_MAX_SAMPLES) return CWH_REFIT_N_SAMPLES;
    if (n_elites < 1 || n_elites > n_samples) return CWH_REFIT_N_ELITES;
    if ((uint64_t)n_states * (uint64_t)n_samples * (uint64_t)n_steps > CWH_SHOOT_MAX_WORK) return CWH_REFIT_WORK;       // (<= 2^27 * 2^16 * 2^15)
    if (smooth > 65535u) return CWH_REFIT_SMOOTH;
    if (gain < 1u || gain > 65535u) return CWH_REFIT_GAIN;
    const uint64_t m = (uint64_t)n_states, w_bytes = 12 * (uint64_t)n_steps * m;
    const cwh_span outs[3] = {{elites, 4 * (uint64_t)n_elites * m, 4}, {weights, w_bytes, 2}, {elite_min, 4 * m, 4}};
    const cwh_span ins[3] = {{ret, 4 * (uint64_t)n_samples * m, 4}, {env_of, 4 * m, 4}, {weights_in, w_bytes, 2}};
    if (cwh_spans_misaligned(outs, 3) >= 0 || cwh_spans_misaligned(ins, 3) >= 0) return CWH_REFIT_ALIGN;
    // (in place, the one overlap allowed: weights_in at the address of weights is the same bytes, and weights is tested against everything else)
    return cwh_spans_clash(outs, 3, ins, weights == weights_in ? 2 : 3, 1, nullptr) >= 0 ? CWH_REFIT_OVERLAP : CWH_REFIT_OK;
}

// ------------------------------------------------------------------------------ the visited set's key, size and argument rules
void cwh_seen_key_of(int32_t group, const uint8_t *hdr, const uint16_t *slot_pos, uint32_t *key)
{
    uint32_t h[4], p[4];
    for (int i = 0; i < 4; i++) {
        h[i] = (uint32_t)hdr[4 * i] | (uint32_t)hdr[4 * i + 1] << 8 | (uint32_t)hdr[4 * i + 2] << 16 | (uint32_t)hdr[4 * i + 3] << 24;
        uint16_t lo, hi;
        memcpy(&lo, (const char *)slot_pos + 4 * i, 2);
        memcpy(&hi, (const char *)slot_pos + 4 * i + 2, 2);
        p[i] = (uint32_t)lo | (uint32_t)hi << 16;
    }
    cwh_seen_key(group, h, p, key);
}
uint64_t cwh_seen_hash_of(const uint32_t *key) { return cwh_seen_hash(key); }

int64_t cwh_seen_slots_of(int64_t capacity)
{
    if (capacity < 0 || capacity > CWH_SEEN_MAX_CAPACITY) return -1;
    if (capacity == 0) return 0;
    int64_t slots = 2;
    while (slots < 2 * capacity) slots <<= 1;
    return slots;
}

int cwh_seen_args(uint64_t group, uint64_t hdr, uint64_t slot_pos, int32_t n_states, uint64_t fresh, uint64_t first)
{
    if (!hdr || !slot_pos) return CWH_SEEN_NO_RECORDS;
    if (!fresh && !first) return CWH_SEEN_NO_FIELD;
    if (n_states < 0 || n_states > CWH_MAX_STATES) return CWH_SEEN_N_STATES;
    const uint64_t m = (uint64_t)n_states;
    const cwh_span outs[2] = {{fresh, m, 1}, {first, 4 * m, 4}}, ins[3] = {{hdr, 16 * m, 16}, {slot_pos, 16 * m, 16}, {group, 4 * m, 4}};
    if (cwh_spans_misaligned(outs, 2) >= 0 || cwh_spans_misaligned(ins, 3) >= 0) return CWH_SEEN_ALIGN;
    return cwh_spans_clash(outs, 2, ins, 3, 1, nullptr) >= 0 ? CWH_SEEN_OVERLAP : CWH_SEEN_OK;
}

int64_t cwh_seen_layout(int64_t slots, uint64_t *offsets)
{
    if (slots < 2 || slots > 2 * CWH_SEEN_MAX_CAPACITY || (slots & (slots - 1))) return -1;
    const uint64_t n = (uint64_t)slots, bytes[CWH_SEEN_SECTIONS] = {CWH_SEEN_CTL_BYTES, 8 * n, 8 * n, 16 * n, 16 * n};
    return (int64_t)cwh_sections_layout(bytes, CWH_SEEN_SECTIONS, 16, offsets);
}

// ------------------------------------------------------------------------------ cw_load_records: the rule a record passes, the index check, the argument rules
int cwh_record_ok_of(uint32_t size, const uint8_t *hdr, const uint16_t *slot_pos)
{
    uint32_t h[4], p[4];
    for (int i = 0; i < 4; i++) {
        h[i] = (uint32_t)hdr[4 * i] | (uint32_t)hdr[4 * i + 1] << 8 | (uint32_t)hdr[4 * i + 2] << 16 | (uint32_t)hdr[4 * i + 3] << 24;
        uint16_t lo, hi;
        memcpy(&lo, (const char *)slot_pos + 4 * i, 2);
        memcpy(&hi, (const char *)slot_pos + 4 * i + 2, 2);
        p[i] = (uint32_t)lo | (uint32_t)hi << 16;
    }
    return cwh_record_ok(size, h, p);
}
int cwh_load_record_index_in_range(int32_t index, int32_t n_records) { return cwh_load_record_index_ok(index, n_records); }

int cwh_load_records_args(int32_t num_envs, uint64_t src, uint64_t hdr, uint64_t slot_pos, int32_t n_records, uint64_t status, uint64_t engine_hdr,
                          uint64_t engine_slot_pos)
{
    if (!hdr || !slot_pos) return CWH_LOAD_NO_RECORDS;
    if (n_records < 0 || n_records > CWH_MAX_STATES) return CWH_LOAD_N_RECORDS;
    if (!src && n_records != num_envs) return CWH_LOAD_OWN_ORDER;
    const uint64_t r = 16ull * (uint64_t)n_records, n = num_envs > 0 ? (uint64_t)num_envs : 0;
    const cwh_span read[3] = {{hdr, r, 16}, {slot_pos, r, 16}, {src, 4 * n, 4}}, own[2] = {{engine_hdr, 16 * n, 16}, {engine_slot_pos, 16 * n, 16}};
    const cwh_span status_span = {status, n, 1};
    if (cwh_spans_misaligned(read, 3) >= 0) return CWH_LOAD_ALIGN;
    if (cwh_spans_clash(read, 2, own, 2, 0, nullptr) >= 0) return CWH_LOAD_ENGINE_OVERLAP;
    return cwh_spans_clash(&status_span, 1, read, 3, 0, nullptr) >= 0 ? CWH_LOAD_STATUS_OVERLAP : CWH_LOAD_OK;
}

// ------------------------------------------------------------------------------ cw_replay_*: the relabelled reward, the buffer's sections, the argument rules
int32_t cwh_replay_reward_of(uint32_t achieved, uint32_t goal, uint32_t task_mask, int subset, int changed, int32_t max_steps)
{
    return cwh_replay_reward(achieved, goal, task_mask, subset, changed, max_steps);
}

int64_t cwh_replay_layout(int32_t steps, int32_t num_envs, uint64_t *offsets)
{
    if (steps < 1 || steps > CWH_REPLAY_MAX_STEPS || num_envs < 1 || (int64_t)steps * (int64_t)num_envs >= (1ll << 31)) return -1;
    const uint64_t N = (uint64_t)num_envs, T = (uint64_t)steps * N;
    const uint64_t bytes[CWH_REPLAY_SECTIONS] = {CWH_REPLAY_CTL_BYTES, 4 * N, 16 * T, 16 * T, 16 * T, 16 * T, 16 * T, 16 * T, 4 * T, 4 * T, T, T};
    return (int64_t)cwh_sections_layout(bytes, CWH_REPLAY_SECTIONS, CWH_SNAP_ALIGN, offsets);
}
int64_t cwh_replay_bytes_of(int32_t steps, int32_t num_envs) { return cwh_replay_layout(steps, num_envs, nullptr); }

// cw_replay_out's fields in its order: hdr, slot_pos, next_hdr, next_slot_pos, goal_hdr, goal_slot_pos, action, reward, done, desired, env, slot, future
static const int kReplayFieldBytes[CWH_REPLAY_FIELDS] = {16, 16, 16, 16, 16, 16, 1, 4, 1, 2, 4, 4, 4};
int cwh_replay_field_bytes_of(int field) { return field >= 0 && field < CWH_REPLAY_FIELDS ? kReplayFieldBytes[field] : 0; }

int cwh_replay_sample_args(int32_t n_rows, uint32_t her, int32_t strategy, const uint64_t *fields)
{
    if (n_rows < 0 || n_rows > CWH_MAX_STATES) return CWH_REPLAY_N_ROWS;
    if (her > 65536u) return CWH_REPLAY_HER;
    if (strategy != 0 && strategy != 1) return CWH_REPLAY_STRATEGY;
    int any = 0;
    cwh_span outs[CWH_REPLAY_FIELDS];
    for (int f = 0; f < CWH_REPLAY_FIELDS; f++) {
        any |= fields[f] != 0;
        outs[f] = cwh_span{fields[f], (uint64_t)kReplayFieldBytes[f] * (uint64_t)n_rows, (uint64_t)kReplayFieldBytes[f]};
    }
    if (!any) return CWH_REPLAY_NO_FIELD;
    if (cwh_spans_misaligned(outs, CWH_REPLAY_FIELDS) >= 0) return CWH_REPLAY_ALIGN;
    return cwh_spans_clash(outs, CWH_REPLAY_FIELDS, nullptr, 0, 1, nullptr) >= 0 ? CWH_REPLAY_OVERLAP : CWH_REPLAY_OK;
}

// ------------------------------------------------------------------------------ cw_reach: the rows of a level, the workspace's sections, the argument rules
int64_t cwh_reach_rows_of(int64_t f) { return cwh_reach_rows(f); }
int64_t cwh_reach_chunks_of(int64_t rows) { return cwh_reach_chunks(rows); }
int64_t cwh_reach_grid_of(int64_t items, int32_t n_cu) { return cwh_reach_grid(items, n_cu); }

int64_t cwh_reach_layout(int64_t max_rows, int32_t max_depth, uint64_t *offsets)
{
    if (max_rows < 1 || max_rows > CWH_REACH_MAX_ROWS || max_depth < 1 || max_depth > CWH_REACH_MAX_DEPTH) return -1;
    const uint64_t R = (uint64_t)max_rows, D = (uint64_t)max_depth, rows = (uint64_t)cwh_reach_rows(max_rows), chunks = (uint64_t)cwh_reach_chunks((int64_t)rows);
    const uint64_t bytes[CWH_REACH_SECTIONS] = {4 * (CWH_REACH_CTL_WORDS + D + 1 + chunks), 16 * R, 16 * R, 4 * R, 4 * R, 16 * R, 16 * R, 4 * R, 4 * R,
                                                16 * rows, 16 * rows, 4 * rows, chunks * CWH_REACH_CHUNK, 4 * R * (D - 1), 4 * R, 4 * R, 4 * R, R};
    return (int64_t)cwh_sections_layout(bytes, CWH_REACH_SECTIONS, CWH_SNAP_ALIGN, offsets);
}
int64_t cwh_reach_bytes_of(int64_t max_rows, int32_t max_depth) { return cwh_reach_layout(max_rows, max_depth, nullptr); }

int cwh_reach_args(int32_t num_envs, uint64_t env_of, uint64_t hdr_in, uint64_t slot_pos_in, int32_t n_states, int32_t max_depth, uint64_t distance,
                   uint64_t plan, uint64_t first_action, uint64_t frontier, uint64_t searched_depth)
{
    if (!distance && !plan && !first_action && !frontier && !searched_depth) return CWH_REACH_NO_FIELD;
    if (n_states < 0 || n_states > CWH_REACH_MAX_ROWS) return CWH_REACH_N_STATES;
    if (max_depth < 1 || max_depth > CWH_REACH_MAX_DEPTH) return CWH_REACH_DEPTH;
    if (!hdr_in != !slot_pos_in) return CWH_REACH_PAIR;
    if (env_of && !hdr_in) return CWH_REACH_ENV_OF;
    if (!hdr_in && n_states != num_envs) return CWH_REACH_OWN_STATES;
    const uint64_t m = (uint64_t)n_states, d = (uint64_t)max_depth;
    const cwh_span outs[5] = {{distance, 4 * m, 4}, {plan, d * m, 1}, {first_action, m, 1}, {frontier, 4 * d, 4}, {searched_depth, 4, 4}};
    const cwh_span ins[3] = {{hdr_in, 16 * m, 16}, {slot_pos_in, 16 * m, 16}, {env_of, 4 * m, 4}};
    if (cwh_spans_misaligned(outs, 5) >= 0 || cwh_spans_misaligned(ins, 3) >= 0) return CWH_REACH_ALIGN;
    return cwh_spans_clash(outs, 5, ins, 3, 1, nullptr) >= 0 ? CWH_REACH_OVERLAP : CWH_REACH_OK;
}

// ------------------------------------------------------------------------------ the sweep clock's periods and schedule
static double period_ns(int32_t sweep_waves, double tb_per_s) { return (double)sweep_waves * 4096.0 / (tb_per_s * 1e12) * 1e9; }
void cwh_sweep_periods(double rate, int32_t sweep_waves, double head_notch, double busy_notch, int32_t *period16, int32_t *period16_head, int32_t *period16_busy)
{
    const double head = rate - head_notch > CWH_GUARD_RATE_FLOOR ? rate - head_notch : CWH_GUARD_RATE_FLOOR;
    const double busy = rate - busy_notch > CWH_GUARD_RATE_FLOOR ? rate - busy_notch : CWH_GUARD_RATE_FLOOR;
    *period16 = rate > 0 ? (int32_t)(period_ns(sweep_waves, rate) * 1.6 + 0.5) : 0;
    *period16_head = rate > 0 ? (int32_t)(period_ns(sweep_waves, head) * 1.6 + 0.5) : 0;
    *period16_busy = rate > 0 ? (int32_t)(period_ns(sweep_waves, busy) * 1.6 + 0.5) : 0;
}
double cwh_guard_scheduled_ms(double sweep_jobs, int32_t period16, int32_t period16_busy, double beside_ms)
{   // (as after a step on which envs finished: a quiet step is 4 us early)
    return (sweep_jobs * (period16 / 1.6) + CWH_HEAD_JOBS * ((period16_busy - period16) / 1.6)) * 1e-6 + beside_ms;
}

// ------------------------------------------------------------------------------ the guard's decisions
// Every CW_GUARD_EVERY-th step's sweep is timed (cw_engine.cpp) and held against its schedule -- jobs x period + the busy head + what a launch costs
// beside its jobs (measured at cw_create).  A sweep in the memory system's saturated regime misses that by 10-16 % launch after launch; at the edge
// (7.7 TB/s) one launch in ten is 7-12 % late and the rest on time.  Three samples in a row more than 6 % late: the rate goes down by a notch (a
// SLOWDOWN: the only move that is not a trial).
// TRIALS (round 5).  cw_create's choice is a measurement of one moment: an engine created while the card was in a worse state settles a notch or two
// under what the card takes an hour later, and round 4's guard only ever went down.  Every move UP is a trial: after enough samples on time
// (recover_need below the best rate known, probe_need at it: a PROBE, never beyond the ceiling, the write path's edge) the guard tries ONE notch more
// and keeps it only if it PAYS -- the mean of CWH_GUARD_PROBE_SAMPLES sweeps at the new rate must be under the mean at the old one; "on time" is
// not enough (a clock a little too fast is on time and slower) and not needed either: with something else between the sweeps (another engine's step
// kernel) every sweep is a constant late, a rate judged by its schedule alone comes to rest a notch or two under the one with the shortest sweeps, and
// so a rate a trial has accepted is from then on measured against what it delivered then (ref_ms).  A trial that does not pay is undone and the next
// one of its kind waits twice as long: a disturbance that has passed does not slow the engine for the rest of its life, and a clock that moves once
// in thousands of steps does not hunt.
static void guard_set_rate(cwh_guard *g, double rate)
{
    g->rate = rate;
    g->ms_sum = 0;
    g->ms_n = 0;
    g->good = g->late = 0;
    g->ref_ms = 0;
}
void cwh_guard_init(cwh_guard *g, double rate)
{
    memset(g, 0, sizeof(*g));
    g->rate = g->rate_top = rate;
    g->probe_need = CWH_GUARD_RECOVER;
    g->recover_need = CWH_GUARD_RECOVER;
}
int cwh_guard_step(cwh_guard *g, double ms, double scheduled)
{
    // the yardstick: the schedule, or what this rate delivered when a trial accepted it.  While a trial runs only sweeps FAR off -- 15 % over the
    // schedule AND over what the rate it left delivered -- end it early: its verdict is the mean.
    const double ref = std::max(scheduled, g->probing ? g->prev_mean : g->ref_ms);
    const bool late = ms > (g->probing ? 1.15 : 1.06) * ref;
    g->late = late ? g->late + 1 : 0;
    // ("in a row" for the way up means MOSTLY: at the edge one launch in ten is late by itself, and 64 strictly in a row would never come)
    g->good = late ? std::max(0, g->good - 8) : g->good + 1;
    if (g->ms_n >= 128) { g->ms_sum *= 0.5; g->ms_n /= 2; }              // (the mean is of the last ~100 samples, not of the rate's whole past)
    g->ms_sum += ms;
    g->ms_n++;
    const bool verdict_due = g->probing && g->ms_n >= CWH_GUARD_PROBE_SAMPLES;
    const double mean = g->ms_sum / g->ms_n;
    if (g->probing && (g->late >= 3 || (verdict_due && mean >= 0.998 * g->prev_mean))) {      // ---- a trial that does not pay: undone
        const double ref_prev = g->ref_prev;
        guard_set_rate(g, g->rate - CWH_GUARD_NOTCH);
        g->ref_ms = ref_prev;
        int32_t &need = g->recovering ? g->recover_need : g->probe_need;  // the next attempt of its kind waits twice as long (no see-saw between two notches)
        need = std::min(2 * need, (int32_t)CWH_GUARD_NEED_MAX);
        g->probing = g->recovering = 0;
        return CWH_GUARD_TRIAL_UNDONE;
    }
    if (verdict_due) {                                                   // ---- a trial that PAYS: kept, and its mean is this rate's yardstick
        if (g->recovering) g->recover_need = CWH_GUARD_RECOVER;
        else { g->rate_top = g->rate; g->probe_need = CWH_GUARD_RECOVER / 4; }      // (the next notch is tried sooner)
        g->ref_ms = mean;
        g->probing = g->recovering = 0;
        return CWH_GUARD_TRIAL_KEPT;
    }
    if (!g->probing && g->late >= 3 && g->rate > CWH_GUARD_RATE_FLOOR + 0.1) {          // ---- not keeping its schedule: a notch down
        guard_set_rate(g, g->rate - CWH_GUARD_NOTCH);
        g->slowdowns++;
        return CWH_GUARD_SLOWDOWN;
    }
    if (!g->probing && g->ms_n >= CWH_GUARD_PROBE_SAMPLES && g->rate + 0.05 < CWH_GUARD_RATE_CEILING &&
        g->good >= (g->rate + 0.1 < g->rate_top ? g->recover_need : g->probe_need)) {
        // ---- a trial: one notch up -- back towards the best rate known after a slowdown, or beyond it (a probe)
        g->recovering = g->rate + 0.1 < g->rate_top;
        g->prev_mean = mean;
        g->ref_prev = g->ref_ms;
        guard_set_rate(g, std::min(g->rate + CWH_GUARD_NOTCH, CWH_GUARD_RATE_CEILING));
        g->probing = 1;
        if (!g->recovering) g->probes++;
        return CWH_GUARD_TRIAL_UP;
    }
    return CWH_GUARD_NONE;
}

// ------------------------------------------------------------------------------ the look-ahead refill period
int32_t cwh_la_adapt(int32_t period, int32_t period_max, uint64_t slow_delta, int32_t *quiet)
{
    if (slow_delta * 8ull > (uint64_t)period) {          // (what a refill launch costs: ~2 us per step at a period of 8 against 12 us per slow reset)
        *quiet = 0;
        if (period > CWH_LA_PERIOD_MIN) period = period / 2 < CWH_LA_PERIOD_MIN ? CWH_LA_PERIOD_MIN : period / 2;
    } else if (slow_delta * 32ull <= (uint64_t)period && ++*quiet >= CWH_LA_QUIET) {
        *quiet = 0;
        if (period < period_max) period = period * 2 > period_max ? period_max : period * 2;
    }
    return period;
}

}  // extern "C"

// ------------------------------------------------------------------------------ the CW_TUNE_* variables
// Whole-text parses: strtol / strtod must consume everything but surrounding whitespace, and the value must be in range (an int that overflows a long,
// or a double that overflows, sets ERANGE; nan and inf are no tuning values).  On any failure the field keeps what it held.
static bool tail_is_blank(const char *end)
{
    while (*end == ' ' || (*end >= '\t' && *end <= '\r')) end++;
    return *end == '\0';
}
static void tune_int(cwh_lookup lookup, void *ctx, const char *name, int32_t *field, long lo, long hi)
{
    const char *s = lookup(ctx, name);
    if (!s) return;
    char *end = nullptr;
    errno = 0;
    const long v = strtol(s, &end, 10);
    if (end == s || errno == ERANGE || !tail_is_blank(end) || v < lo || v > hi) return;
    *field = (int32_t)v;
}
static void tune_real(cwh_lookup lookup, void *ctx, const char *name, double *field, double lo)
{
    const char *s = lookup(ctx, name);
    if (!s) return;
    char *end = nullptr;
    errno = 0;
    const double v = strtod(s, &end);
    if (end == s || errno == ERANGE || !tail_is_blank(end) || !std::isfinite(v) || v < lo) return;
    *field = v;
}

extern "C" void cwh_read_tuning(cwh_lookup lookup, void *ctx, cwh_tuning *t)
{
    tune_int(lookup, ctx, "CW_TUNE_RENDER_CHUNK_ROUNDS", &t->render_chunk_rounds, 0, INT32_MAX);
    int32_t epw = t->step_envs_per_wave;
    tune_int(lookup, ctx, "CW_TUNE_STEP_ENVS_PER_WAVE", &epw, 8, 64);
    if (epw == 8 || epw == 16 || epw == 32 || epw == 64) t->step_envs_per_wave = epw;
    tune_int(lookup, ctx, "CW_TUNE_GATHER", &t->gather, INT32_MIN, INT32_MAX);
    tune_int(lookup, ctx, "CW_TUNE_GATHER_MAX_SIZE", &t->gather_max_size, 0, 9);          // (cw_render_gather_kernel's tables: frames under 4 KiB)
    tune_int(lookup, ctx, "CW_TUNE_SMALL_FRAME_BYTES", &t->small_frame_bytes, 0, INT32_MAX);
    tune_int(lookup, ctx, "CW_TUNE_SMALL_BLOCKS", &t->small_blocks_per_cu, 1, 8);
    tune_int(lookup, ctx, "CW_TUNE_SMALL_LAUNCH_MB", &t->small_launch_mb, 0, INT32_MAX);
    tune_int(lookup, ctx, "CW_TUNE_RESET_BLOCKS", &t->reset_blocks_per_cu, 1, 16);
    tune_real(lookup, ctx, "CW_TUNE_HEAD_NOTCH", &t->head_notch, 0);
    tune_real(lookup, ctx, "CW_TUNE_BUSY_NOTCH", &t->busy_notch, 0);
    tune_real(lookup, ctx, "CW_TUNE_PERIOD_NS", &t->period_ns, 0);
    tune_real(lookup, ctx, "CW_TUNE_RATE_TBS", &t->rate_tbs, 0);
    tune_int(lookup, ctx, "CW_TUNE_GUARD", &t->guard, INT32_MIN, INT32_MAX);
    t->guard = t->guard != 0;
    if (lookup(ctx, "CW_TUNE_VERBOSE")) t->verbose = 1;
    tune_int(lookup, ctx, "CW_TUNE_LOOKAHEAD", &t->lookahead, INT32_MIN, INT32_MAX);
    t->lookahead = t->lookahead != 0;
    tune_int(lookup, ctx, "CW_TUNE_LA_PERIOD", &t->la_period, 1, INT32_MAX);            // (a forced refill period, no adaptation: profiles/r06_experiments.txt D)
    tune_int(lookup, ctx, "CW_TUNE_ROLLOUT_SEGMENT", &t->rollout_segment, -1, INT32_MAX);
}
