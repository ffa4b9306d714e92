// cw_layout.h -- HBM data layout of the batched CraftingWorld engine (host + device).
//
// State is SPARSE, not a dense grid: the reference world always holds exactly the 8 objects
// sample_state() placed (ray.py:599-628) -- they transform in place (tree->sticks, sticks->house,
// wheat->bread), vanish (rock, bread) or are carried, but never multiply -- so an env is
//   header (16 B) + 8 object slots (cell index u16 each, 4-bit code each).
// Every per-env array is a structure-of-arrays of 16-byte records, so one wavefront reads
// 64 x 16 B = 1 KiB contiguous per load (env i handled by lane i): fully coalesced, and the
// step kernel never makes a data-dependent (gather) access to HBM.  "What is in cell p" is 8
// register compares.  Dense views (grid codes, one-hot, pixels) are materialised by the
// render/export kernels from the slots.
#pragma once
#include <stdint.h>

#define CW_POS_GONE 0xFFFFu   // slot's object no longer exists
#define CW_POS_HELD 0xFFFEu   // slot's object is in the agent's hand

// hdr.flags
#define CW_FLAG_RESET 0x1u    // env was (re)set by the last cw_reset / auto-reset (render: also write desired/init frames)
#define CW_FLAG_SUBSET 0x2u   // reward_style is not None (compute_reward_subset, ray.py:763-767)
//   flags bits 2-15: steps of the running episode that returned MAX_STEPS (saturating at 16 383): the episode's return so far is a closed form of this count
//   and step_num (episode_return_of) -- exact also where an env WITHOUT auto-reset is stepped on after its first done, as the reference allows (ray.py:367)

// Packed header, one uint4 per env:
//   x = agent_r | agent_c << 8 | hold << 16 | menu << 24
//   y = achieved | desired << 16
//   z = step_num | flags << 16
//   w = slot codes, 4 bits each (slot k = bits 4k..4k+3); code 0 = gone
// Slot positions, one uint4 per env: 8 x u16, slot k = (word[k>>1] >> 16*(k&1)) & 0xFFFF.
// Slot k initially holds object k (code k+1) -- OBJECTS order, ray.py:21.

#define CW_CODES_INITIAL 0x87654321u  // slot k has code k+1
#define CW_CTL_QUEUED 0x100u          // nx_ctl: the env's ring wants a refill (a record was taken, or it was reset the slow way): the refill kernel scans for this bit; bits 0-7: the queue's head slot
#define CW_LA_DEPTH 4                 // look-ahead records kept per env (round 6: a QUEUE -- an env that finishes two, three, four times between two refills
                                      // still finds a record; rounds 4-5 kept one, and every further finish was reset the slow way on the step's critical path)

// One ordered selected_tasks list, device form (cw_task_menu packed): selected_bits as nibbles.
struct CwMenuDev {
    uint64_t sel_bits;       // nibble i = task_list.index(selected_tasks[i])
    int32_t n_selected;
    int32_t number_of_tasks;
    int32_t stacking;
    int32_t reward_subset;
};

// Host-side launch tuning of one engine (defaults = the measured best; the CW_TUNE_* environment variables, read once by
// cw_create (cw_engine.cpp: read_tuning), override them for experiments; a value out of range keeps the default).
struct CwTuning {
    int n_cu = 256;                 // compute units of the engine's device (hipDeviceProp_t::multiProcessorCount, set by cw_create)
    int period16 = 0;               // the sweep's CLOCK: a wave's jobs (4-KiB pieces) start one period apart; in 1/16 of a 10-ns tick of the 100-MHz clock (0: unclocked)
    int period16_head = 0;          // ... of a launch's first 64 jobs (the write path takes a notch less from a launch's first ~40 us) ...
    int period16_busy = 0;          // ... and of those after a step on which envs finished (their frames were written just before the sweep)
    int render_chunk_rounds = 896;  // a large batch is swept in launches of at most this many rounds of 3 KB per wave over consecutive env ranges:
                                    // 131 072 envs at 21x21 (0: one launch whatever the batch)
    int gather = 1;                 // the smallest Ray frames (grids up to gather_max_size) by cw_render_gather_kernel; 0: by the piece sweep like all others (CW_TUNE_GATHER)
    int gather_max_size = 7;        // (measured: the gather painter wins up to 7x7, the piece sweep from 8x8 on; profiles/r05_small_frames.txt)
    int small_frame_bytes = 4096;   // frames under this many bytes are swept with small_blocks_per_cu workgroups per CU instead of one (CW_TUNE_SMALL_FRAME_BYTES)
    int small_blocks_per_cu = 4;    // (CW_TUNE_SMALL_BLOCKS)
    long long small_launch_bytes = 320ll << 20;   // ... the piece sweep only while a launch writes less than this (the gather painter always); CW_TUNE_SMALL_LAUNCH_MB
    int step_envs_per_wave = 64;    // most envs a wave of cw_step_fused_kernel steps (64: one wave per SIMD at 65 536 envs; CW_TUNE_STEP_ENVS_PER_WAVE: 8 / 16 / 32 / 64)
    int reset_blocks_per_cu = 4;    // resetting workgroups (4 waves = 4 envs in flight each) per CU at most: the reset, refill and pool kernels (round 6: 2 -> 4;
                                    // nothing runs beside the sweep any more, the refill's scan wants the waves: CW_TUNE_RESET_BLOCKS, profiles/r06_experiments.txt D)
};

// Control block of the RESIDENT stepper (cw_step_resident: the single-env loop, a step without a kernel launch): pinned, coherent host memory
// the device polls.  One 128-byte line per direction so that the host's doorbell stores and the device's answers never share a line.
struct CwResident {
    unsigned long long bell; // host -> device, ONE word so that a poll is one PCIe read: low half (seq << 8) | action, seq = 1, 2, ... (a new seq is a
                             // new step request); high half 1 = leave now (cw_resident_stop and every entry point that touches the engine's state)
    uint32_t pad0[30];
    uint32_t ack;            // device -> host: the last seq whose outputs (reward, done, masks, repainted cells, state) are visible
    uint32_t exited;         // device -> host: 0 while resident; else reason (1 stop, 2 idle, 3 time slice used up) | last seq served << 8
    uint32_t pad1[30];
};

// The SNAPSHOT BANK of an engine (cw_snapshot_reserve): `rows` rows in device memory, each of which can hold one env completely -- the arrays of CwParams
// that make up an env, with `rows` in the place of n_envs (the ring as [CW_LA_DEPTH][rows], the pool as [rows][K][9]), plus one byte per row: the row has
// been saved since the last reserve.  One allocation; the sections' sizes and offsets are cw_host.cpp's (cwh_snapshot_section_bytes).  The snapshot kernels
// also describe the ENGINE's own arrays with this struct (rows = n_envs, valid = null), so that one device function copies either way.
struct CwBank {
    uint4 *hdr, *pos, *init_pos, *goal_pos;
    uint32_t *goal_codes;
    int32_t *ep_no;
    uint16_t *init_agent, *goal_agent;
    uint32_t *mt;            // [rows][624]
    int32_t *mt_idx;
    uint4 *nx_init_pos, *nx_goal_pos, *nx_misc;      // [CW_LA_DEPTH][rows] (engines that keep look-ahead records)
    uint32_t *nx_ctl;
    uint16_t *pool;          // [rows][K][9]
    uint8_t *valid;          // [rows]
    int32_t rows;            // the capacity: a row number is an index only after cwh_snapshot_row_ok(row, rows) (cw_host.h)
};

// The VISITED SET of an engine (cw_seen_reserve): an open-addressed table of `mask + 1` slots (a power of two) in device memory, one array per field, and a
// control block.  A slot: tag (0: empty, else cwh_seen_tag of the key's hash), owner (all ones: empty, else epoch << CWH_SEEN_ROW_BITS | row of the smallest
// row that claimed it in the call that filled it) and the key in its stored form, two uint4: a = (group, hdr.x & 0xFFFFFF | subset << 24, hdr.y, hdr.w),
// b = slot_pos.  48 bytes a slot.  ctl: [0] keys held, [1] overflow, [2] collisions (the three public counters), [3] epoch: the number of inserts since the
// last clear, advanced ON THE DEVICE by the last workgroup of every insert, [4] the ticket that finds that workgroup.
#define CW_SEEN_CTL_WORDS 8
enum { CW_SEEN_SIZE = 0, CW_SEEN_OVERFLOW = 1, CW_SEEN_COLLISIONS = 2, CW_SEEN_EPOCH = 3, CW_SEEN_TICKET = 4 };
struct CwSeen {
    unsigned long long *tag;     // [slots]
    unsigned long long *owner;   // [slots]
    uint4 *key_a, *key_b;        // [slots]
    unsigned long long *ctl;     // [CW_SEEN_CTL_WORDS]
    uint32_t mask;               // slots - 1: a hash becomes a slot index only through `& mask`
    int32_t probes;              // min(CWH_SEEN_PROBES, slots)
    int32_t tag_bits;            // 0: the full hash
};

// The WORKSPACE of cw_reach (cw_reach_reserve): one allocation in device memory, its sections cw_host.cpp's (cwh_reach_layout).  Frontier k -- the states
// level k + 1 expands, k = 0 the participating start rows -- lives in buffer k & 1; sizes[k] is its size, written ON THE DEVICE by the scan that closes
// level k, and every kernel of a level reads it from there.  s_*: the successors of the level in hand, row a * Fp + j (cw_host.h: THE ROWS).  links: level k's
// scatter leaves parent << 3 | action for every state of frontier k at links[(k - 1) * max_rows + i].  Per start row: dist (-1: unsolved), sol (the link of its
// solving row), bid (the smallest solving row of the level in hand, CW_REACH_NONE: none) and active.
#define CW_REACH_NONE 0x7FFFFFFF
struct CwReach {
    int32_t *ctl;                // [CWH_REACH_CTL_WORDS]: CWH_REACH_STOP, CWH_REACH_SEARCHED
    int32_t *sizes;              // [max_depth + 1]
    int32_t *chunk;              // [chunks of the largest level]: the count of every chunk, then (the scan) what lies ahead of it
    uint4 *f_hdr[2], *f_pos[2];  // [max_rows]
    int32_t *f_env[2], *f_start[2];
    uint4 *s_hdr, *s_pos;        // [6 * padded(max_rows)]
    int32_t *s_grp;              // ... the start row, -1 for a done successor and for a row that takes no part
    uint8_t *s_fresh;            // ... 1: the row brings its key into the set (whole chunks: read 16 bytes at a time)
    int32_t *links;              // [max_depth - 1][max_rows]
    int32_t *dist, *sol, *bid;   // [max_rows]
    uint8_t *active;             // [max_rows]
    int32_t max_rows, max_depth;
};

// Where cw_reach leaves its results (the public cw_reach_out).  A null field is not written.
struct CwReachOut {
    int32_t *distance;           // [M]
    uint8_t *plan;               // [D][M] step-major
    uint8_t *first_action;       // [M]
    int32_t *frontier;           // [D]
    int32_t *searched_depth;     // [1]
};

// The REPLAY BUFFER of an engine (cw_replay_reserve): `steps` slots of n_envs transitions each in device memory, TIME-MAJOR -- slot t of env i at [t * n_envs + i],
// so a push is one coalesced run per array -- one array per field, and a control block.  One allocation, its sections cw_host.cpp's (cwh_replay_layout).  A
// transition is three packed records (the state s, its successor s', the episode's goal as a record), the action (255: outside 0..5), flags (bit 0 changed,
// bit 1 done), the reward and the env's episode number: 106 bytes.  ctl[0] = n, the pushes since the last clear, advanced ON THE DEVICE by a one-lane kernel
// behind every push; env_episode[i]: the episode number of env i's newest transition.
#define CW_REPLAY_CHANGED 0x1u
#define CW_REPLAY_DONE 0x2u
struct CwReplay {
    uint4 *hdr, *pos;                // [steps][n_envs] s
    uint4 *next_hdr, *next_pos;      // [steps][n_envs] s'
    uint4 *goal_hdr, *goal_pos;      // [steps][n_envs] the goal record
    int32_t *reward;                 // [steps][n_envs]
    uint32_t *episode;               // [steps][n_envs]
    uint8_t *action, *flags;         // [steps][n_envs]
    uint32_t *env_episode;           // [n_envs]
    unsigned long long *ctl;         // [CW_REPLAY_CTL_WORDS]: [0] n
    int32_t steps;                   // L: a position becomes a slot only through `% steps`
};
#define CW_REPLAY_CTL_WORDS 32

// Where cw_replay_sample_kernel leaves a minibatch of B rows (the public cw_replay_out with the records typed).  A null field is not written.
struct CwReplayOut {
    uint4 *hdr, *pos, *next_hdr, *next_pos, *goal_hdr, *goal_pos;     // [B]
    uint8_t *action;
    int32_t *reward;
    uint8_t *done;
    uint16_t *desired;
    int32_t *env, *slot, *future;
};

// Where cw_expand_kernel leaves the six successors of M states (the public cw_expand_out with the records typed): every array ACTION-MAJOR, row a * M + j =
// action a on input state j.  A null field is not written.
struct CwExpandOut {
    int32_t *reward;         // [6][M]
    uint8_t *done;           // [6][M]
    uint8_t *changed;        // [6][M]
    uint16_t *achieved;      // [6][M]
    uint4 *hdr;              // [6][M] successor headers
    uint4 *pos;              // [6][M] successor slot positions
};

// Where cw_simulate_kernel leaves the outcome of T steps of M states (the public cw_simulate_out with the records typed).  A null field is not written.
struct CwSimulateOut {
    int32_t *ret;            // [M] sum of the rewards of the steps taken
    int32_t *length;         // [M] 1 + index of the first done step, T if none
    uint8_t *done;           // [M]
    uint16_t *achieved;      // [M]
    uint4 *hdr;              // [M] record after the last step taken
    uint4 *pos;              // [M]
    int32_t *rewards;        // [T][M] step-major trace
    uint8_t *dones;          // [T][M]
};

// Where cw_unroll_kernel leaves EVERY record along T steps of M states (the public cw_unroll_out with the records typed), step-major.  A null field is not
// written.
struct CwUnrollOut {
    uint4 *hdr;              // [T + 1][M] row 0: the record as read, row t + 1: the record after step t (a step not taken repeats the row before it)
    uint4 *pos;              // [T + 1][M]
    int32_t *reward;         // [T][M] 0 for a step not taken
    uint8_t *done;           // [T][M]
    uint8_t *changed;        // [T][M] the step changed the state
    uint8_t *taken;          // [T][M] 1: the step was taken
    int32_t *length;         // [M] 1 + index of the first done step, T if none
};

// Where cw_plan_kernel leaves the best plan of each (first action, state) pair (the public cw_plan_out with the records typed): ACTION-MAJOR like CwExpandOut,
// row a * M + j.  A null field is not written.
struct CwPlanOut {
    int32_t *q;              // [6][M] the best return within the horizon after first action a
    int32_t *length;         // [6][M] steps the best plan takes
    uint8_t *done;           // [6][M] it ends inside the horizon
    uint16_t *achieved;      // [6][M]
    uint4 *hdr;              // [6][M] record after its last step
    uint4 *pos;              // [6][M]
    uint8_t *plan;           // [6][D][M] its actions, step-major; 0 behind its end
};

// Where cw_shoot_kernel leaves the best of each state's K sampled plans (the public cw_shoot_out with the records typed).  A null field is not written.
struct CwShootOut {
    int32_t *best_ret;       // [M] the largest return of any sample
    int32_t *best_sample;    // [M] the smallest sample that reaches it
    uint8_t *best_action;    // [M] its first action
    int32_t *length;         // [M] steps it takes
    uint8_t *done;           // [M] it ends inside the horizon
    uint16_t *achieved;      // [M]
    uint4 *hdr;              // [M] record after its last step
    uint4 *pos;              // [M]
    uint8_t *plan;           // [T][M] all T drawn actions of it, step-major
    int32_t *ret;            // [K][M] the return of every sample
};

// Everything the kernels need, passed by value.
struct CwParams {
    // per-env state (SoA of 16-byte records unless noted)
    uint4 *hdr;              // [N]
    uint4 *pos;              // [N] current slot positions
    uint4 *init_pos;         // [N] positions at reset of objects 0..7 (INIT_OBS_VECTOR, ray.py:183)
    uint16_t *init_agent;    // [N] agent cell at reset
    uint4 *goal_pos;         // [N] imagine_obs final_state slot positions (ray.py:220-299)
    uint32_t *goal_codes;    // [N]
    uint16_t *goal_agent;    // [N]
    int32_t *ep_no;          // [N]
    // MT19937 per env, env-contiguous [N][624], "consume-and-replace" convention (cw_mt.h)
    uint32_t *mt;
    int32_t *mt_idx;         // [N] next word index 0..623
    // fixed_init_state pool: [N][K][9] u16 (objects 0..7 + agent cell)
    uint16_t *pool;
    // outputs
    int32_t *reward;         // [N]
    uint8_t *done;           // [N]
    uint16_t *achieved_out;  // [N]
    uint16_t *desired_out;   // [N]
    int32_t *episode_length; // [N]
    int32_t *episode_return; // [N] sum of the finished episode's rewards (ray.py:361-367), written where done
    uint8_t *obs;            // [N][P][P][3] or null
    uint8_t *desired_img;
    uint8_t *init_img;
    uint8_t *terminal_img;   // or null
    // LOOK-AHEAD: the outcome of every env's NEXT reset(), computed ahead of time.  Only reset() draws from an env's RNG stream, so the next
    // episode's placement, goal state and task set are known as soon as the previous reset has been taken: the refill kernel runs them ahead in
    // bulk, off the per-step path, and a finished env just takes the record over inside the step kernel (a POP: three 16-byte loads).  An env
    // that finishes again before the next refill finds no record and is reset the slow way, on the spot, from the same stream position.
    // The records of an env form a RING of CW_LA_DEPTH slots, slot d of env e at [d * N + e] (one coalesced array per slot): nx_ctl[e] names the head slot --
    // the NEXT episode --, the valid records follow it in stream order, a pop invalidates the head and advances it (one round trip: the three 16-byte loads of
    // the head slot, as with the single record of rounds 4-5), the refill computes the missing ones behind the last valid one.
    uint4 *nx_init_pos;      // [D][N] sample_state placement of the episode
    uint4 *nx_goal_pos;      // [D][N] its imagine_obs final state
    uint4 *nx_misc;          // [D][N] x = init_agent | goal_agent << 16, y = goal_codes, z = desired | subset << 16 | VALID << 31, w = raw 32-bit draws the
                             //     record consumed (cw_get_mt rewinds the exported stream by the draws of every waiting record)
    uint32_t *nx_ctl;        // [N] head slot (bits 0-7) | CW_CTL_QUEUED; read with the env's state when a step begins
    int32_t lookahead;       // 0: no records are kept (engines without auto-reset, host-mapped engines, CW_TUNE_LOOKAHEAD=0)
    unsigned long long *la_feedback;   // pinned host word or null: every refill kernel leaves counters[5] (resets taken the slow way so far) here -- the host
                                       // adapts its refill period to it without ever waiting for the card (cw_engine.cpp: cw_step)
    unsigned long long *counters; // [4] public: steps, finished, successes, invalid actions; [4] PRIVATE: the finished count the last sweep of the
                                  // observation array saw (cw_render_pieces_kernel: what kind of step does it follow?), [5] PRIVATE: resets of
                                  // look-ahead engines that found no record and were taken the slow way; [6] public: envs a snapshot or record load
                                  // skipped (cw_snapshot_save_kernel, cw_snapshot_load_kernel: a bad row number; cw_load_records_kernel: an index out of range, a refused record); [7] public: states cw_expand_kernel,
                                  // cw_simulate_kernel or cw_plan_kernel skipped for an env index at or above n_envs; 8 words allocated
    const CwMenuDev *menus;
    // constants
    int32_t n_envs;
    int32_t size;            // S
    int32_t ncell;           // S*S
    int32_t max_steps;
    uint32_t task_mask;      // (1 << n_task_list) - 1
    int32_t pool_k;          // fixed_init_state
    uint32_t div_magic;      // floor(2^32 / S) + 1 : x / S == mulhi(x, magic) for x < 2^18
    uint32_t frame_bytes;    // 48 * S * S, or 27 * S * (S+1) for the AltObs rasteriser
    int32_t raster;          // CW_RASTER_*
    uint8_t *res_onehot;     // resident stepper only (else null): host-mapped [S][S][12] one-hot state, rewritten after every resident step
};
