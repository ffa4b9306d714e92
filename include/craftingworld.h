/*
 * craftingworld.h -- C ABI of the MI355X-native batched CraftingWorld step/reset engine.
 *
 * The reference (lauradarcy/gym-craftingworld) has no FFI/plugin interface: its boundary is the
 * gym Python API of CraftingWorldEnvRay (gym_craftingworld/envs/craftingworld_ray.py, "ray.py").
 * This header is the boundary a binding for that API calls into; every entry point cites the
 * reference interface it replaces.  Plain C: pointers, sizes, integer status codes.  No torch or
 * HIP types appear in the signatures (cw_stream_t is a hipStream_t passed as void*).
 *
 * Threading: one engine per device; calls on one engine are serialized by the caller.  Every
 * call that takes a stream only ENQUEUES work on it (no host synchronisation) unless stated.
 * Ownership: the engine owns all device buffers for its lifetime; cw_buffers() exposes them for
 * zero-copy wrapping (valid until cw_destroy; contents valid until the next cw_step/cw_reset --
 * the same live-alias contract as the reference, whose step() returns obs_image itself).
 */
#ifndef CRAFTINGWORLD_H
#define CRAFTINGWORLD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CW_ABI_VERSION 5   /* 5: cw_buffer_table.episode_return, cw_get_fixed_states (and, added since without a new number: cw_reset_masked, cw_imagine_masked, cw_sample_state_masked, cw_snapshot_reserve, cw_snapshot_save,
                            * cw_snapshot_load, cw_snapshot_row_bytes, cw_expand, cw_export_onehot_states, cw_simulate_out, cw_simulate), then cw_render_records, then cw_plan_out, cw_plan; then cw_shoot_out, cw_shoot, cw_shoot_actions; then cw_seen_out, cw_seen_reserve, cw_seen_clear, cw_seen_insert, cw_seen_counters, cw_seen_slots; then cw_reach_out, cw_reach_reserve, cw_reach_bytes, cw_reach; then cw_load_records; then cw_refit_out, cw_shoot_refit; then cw_replay_table, cw_replay_out, cw_replay_reserve, cw_replay_bytes, cw_replay_buffers, cw_replay_clear, cw_replay_push, cw_replay_sample; then cw_unroll_out, cw_unroll; 4: cw_tuner_state, one painter, look-ahead records.  Round 6 changed no
                            * signature or struct: cw_get_mt reports numpy's own (key, pos) form, cw_rollout issues one launch per max_steps steps, checkpoint blobs
                            * are version 4 (a ring of look-ahead records per env; older blobs are refused with CW_ERR_INVALID), hdr flags bits 2-15 count successes */
#define CW_MT_N 624        /* MT19937 words per env (numpy RandomState key)        */
#define CW_MAX_TASKS 16    /* len(task_list) upper bound (bits of the goal masks)  */
#define CW_MAX_MENUS 256   /* distinct ordered selected_tasks lists per engine     */
#define CW_NUM_OBJECTS 8   /* OBJECTS, ray.py:21                                   */
#define CW_NUM_ACTIONS 6   /* ACTIONS, ray.py:130-131: Up, Right, Down, Left, PickUp, Drop */

/* status codes */
#define CW_OK 0
#define CW_ERR_INVALID (-1)   /* bad argument / config (cw_last_error() has the text) */
#define CW_ERR_HIP (-2)       /* a HIP runtime call failed                             */
#define CW_ERR_STATE (-3)     /* call order (e.g. cw_step before cw_reset)             */

/* cell codes of the dense views: 0 empty, k+1 = OBJECTS[k] (ray.py:21) */
enum { CW_EMPTY = 0, CW_STICKS = 1, CW_AXE = 2, CW_HAMMER = 3, CW_ROCK = 4, CW_TREE = 5,
       CW_BREAD = 6, CW_HOUSE = 7, CW_WHEAT = 8 };

/* observation modes (cw_config.obs_mode) */
enum {
    CW_OBS_STATE = 0,        /* no pixel buffers; state tensors only (BASELINE config 2)            */
    CW_OBS_PIXELS_FULL = 1,  /* render(): whole (4S,4S,3) uint8 frame rewritten every step, ray.py:442-520 */
    CW_OBS_PIXELS_DIRTY = 2  /* render_edit(): persistent frame, <=2 changed cells repainted, ray.py:522-557 */
};

/* rasterisers (cw_config.raster) */
enum {
    CW_RASTER_RAY = 0,  /* CraftingWorldEnvRay: 4x4 px per cell in the object's colour, frames [4S][4S][3]   (ray.py:442-557) */
    CW_RASTER_ALT = 1   /* CraftingWorldEnvAltObs: 3x3 px per cell, pixel k lit with CPV_COLORS[k] iff item k is in the
                         * cell, + a 3-px strip with a "holding" flag: frames [3S+3][3S][3] (craftingworld_altobs.py:489-642);
                         * values are the reference's int image modulo 256 */
};

/* action dtypes accepted by cw_step */
enum { CW_ACT_I32 = 0, CW_ACT_I64 = 1, CW_ACT_U8 = 2 };

/* One ordered selected_tasks list with its draw rules -- the ctor kwargs selected_tasks,
 * number_of_tasks, stacking, reward_style of ray.py:59-83.  Kept as an ORDERED list because
 * reset() shuffles indices into it (ray.py:171-174). */
typedef struct cw_task_menu {
    int32_t n_selected;                  /* len(selected_tasks), 1..CW_MAX_TASKS                   */
    int32_t number_of_tasks;             /* ray.py:79-81 (clamped to n_selected by cw_create)      */
    int32_t stacking;                    /* `stacking is True`, ray.py:169                         */
    int32_t reward_subset;               /* reward_style is not None -> compute_reward_subset      */
    int32_t selected_bits[CW_MAX_TASKS]; /* task_list.index(selected_tasks[i]), ray.py:174         */
} cw_task_menu;

/* CraftingWorldEnvRay.__init__ kwargs (ray.py:59-60) for a batch of num_envs envs */
typedef struct cw_config {
    int32_t abi_version;        /* CW_ABI_VERSION */
    int32_t num_envs;           /* N */
    int32_t size;               /* STATE_W == STATE_H, 4..255 (non-square rejected: reference defect) */
    int32_t max_steps;          /* MAX_STEPS, 1..65535 */
    int32_t n_task_list;        /* len(task_list), 9..CW_MAX_TASKS */
    int32_t fixed_init_state;   /* 0, or pool size K per env (ray.py:116-118), K <= 64 */
    int32_t obs_mode;           /* CW_OBS_* */
    int32_t auto_reset;         /* 1: cw_step resets finished envs itself (gym.vector semantics);
                                 * 0: finished envs keep stepping until cw_reset / cw_reset_masked (single gym.Env semantics, ray.py:367) */
    int32_t keep_terminal_obs;  /* 1 (pixel modes + auto_reset): before a finished env is reset, its last frame is
                                 * painted into cw_buffer_table.terminal_obs (gym.vector's info["terminal_observation"]) */
    int32_t raster;             /* CW_RASTER_* (pixel modes) */
    int32_t host_outputs;       /* 1: the step outputs and the frames (every cw_buffer_table pointer down to episode_length) live in
                                 * pinned, GPU-mapped HOST memory and are valid on the host too; cw_buffer_table.host_actions is a
                                 * mapped int32[N] to write actions into.  For the single-env gym loop (ray.py step()/reset() called
                                 * from host code, docs/source/envs/gen_info.rst:62-82): a step is one launch + cw_synchronize, no
                                 * copies.  Kernel stores then cross PCIe -- not for large batches. */
    int32_t n_menus;            /* 1..CW_MAX_MENUS */
    const cw_task_menu *menus;  /* host array [n_menus] */
    const uint8_t *env_menu;    /* host array [num_envs] of menu ids, or NULL (= all envs use menu 0) */
} cw_config;

typedef struct cw_engine cw_engine;
typedef void *cw_stream_t;      /* hipStream_t */

/* Device buffers owned by the engine (cw_buffers).  N = num_envs, S = size, P = 4*S.
 * Pixel buffers are NULL in CW_OBS_STATE. */
typedef struct cw_buffer_table {
    uint8_t *obs;            /* [N][P][P][3]  observation == achieved_goal image (ray.py:194-196) */
    uint8_t *desired_goal;   /* [N][P][P][3]  imagine_obs() image, rewritten at reset (ray.py:191) */
    uint8_t *init_obs;       /* [N][P][P][3]  INIT_OBS, rewritten at reset (ray.py:193)            */
    uint8_t *terminal_obs;   /* [N][P][P][3]  last frame of the episode that just ended, valid where done==1 (NULL unless keep_terminal_obs) */
    int32_t *reward;         /* [N]  -1 or max_steps (ray.py:361-363)                              */
    uint8_t *done;           /* [N]  0/1 (ray.py:367); done envs have already been auto-reset      */
    uint16_t *achieved;      /* [N]  achieved_goal_vector as a bit mask AFTER the step, BEFORE auto-reset */
    uint16_t *desired;       /* [N]  desired_goal_vector of the episode the step belonged to       */
    int32_t *episode_length; /* [N]  step_num at done (valid where done==1)                        */
    int32_t *episode_return; /* [N]  sum of the episode's rewards up to a step that returned done==1 (valid where done==1), as the reference's
                              *      loop sums them (ray.py:361-367: -1 per step, MAX_STEPS on a step that leaves the goal satisfied).  With
                              *      auto_reset the episode ends there: max_steps - (length - 1) after a success, -length after a time-out.
                              *      WITHOUT auto_reset a finished env keeps stepping until cw_reset (ray.py:367) and every later done step
                              *      rewrites episode_length / episode_return with the sums up to that step, repeated success rewards included.
                              *      cw_rollout writes both at EVERY done step of its n_steps, like n_steps calls of cw_step. */
    uint8_t *hdr;            /* [N][16] packed per-env header of the CURRENT state (after auto-reset):
                              *   byte 0 agent row, 1 agent col, 2 hold (0 none,1 sticks,2 axe,3 hammer), 3 menu id,
                              *   bytes 4-5 achieved mask (LE u16), 6-7 desired mask, 8-9 step_num, 10-11 flags (bit 0: no step
                              *   taken yet in this episode, bit 1: subset reward rule, bits 2-15: steps of this episode that returned max_steps),
                              *   bytes 12-15 the 8 object slots' codes, 4 bits each (slot k in bits 4k..4k+3)      */
    uint16_t *slot_pos;      /* [N][8] cell index (row*S+col) of object slot k; 0xFFFF gone, 0xFFFE held          */
    uint64_t *counters;      /* [4]  {env-steps, episodes finished, successes (reward==max_steps), invalid actions}; the allocation holds
                              *      8 words: [4] is the engine's own (the finished count the last sweep of the observation array saw --
                              *      the sweep paces its first jobs by what the step before it did), [5] counts resets of a look-ahead engine that
                              *      found no record waiting (performance diagnostics), [6] counts the envs a snapshot or record load skipped
                              *      (cw_snapshot_save / cw_snapshot_load: a bad row number; cw_load_records: an index out of range or a refused record), [7] counts the states skipped by cw_expand, cw_simulate, cw_unroll, cw_plan or cw_shoot for an env index at or above num_envs.
                              *      Read-only for callers. */
    size_t frame_bytes;      /* P*P*3 (CW_RASTER_RAY) or (3S+3)*3S*3 (CW_RASTER_ALT) */
    int32_t *host_actions;   /* [N]  cw_config.host_outputs only (else NULL): mapped host buffer usable as cw_step's actions (CW_ACT_I32) */
    uint8_t *host_onehot;    /* [S][S][12] engines that can run cw_step_resident only (else NULL): obs_one_hot (ray.py:119) of the env in pinned host
                              * memory, rewritten by every cw_step_resident (CraftingWorldEnvOneHot returns it as the observation, onehot.py:369-371) */
} cw_buffer_table;

/* Host-side dense snapshot for parity injection / checkpointing (cw_get_state, cw_set_state).
 * All pointers are HOST arrays supplied by the caller; a NULL pointer skips that field. */
typedef struct cw_state_view {
    uint8_t *grid;        /* [N][S][S] cell codes            (obs_one_hot[:,:,:8], ray.py:119)   */
    uint8_t *init_grid;   /* [N][S][S] codes at reset        (INIT_OBS_VECTOR, ray.py:183)       */
    uint8_t *goal_grid;   /* [N][S][S] imagine_obs final_state codes (set: restores a checkpoint's goal)  */
    uint8_t *agent_rc;    /* [N][2]                          (agent_pos)                          */
    uint8_t *init_agent_rc; /* [N][2] agent cell at reset (channel 8 of INIT_OBS_VECTOR)              */
    uint8_t *goal_agent_rc; /* [N][2] agent cell of the goal state                                    */
    uint8_t *hold;        /* [N]                                                                   */
    uint16_t *achieved;   /* [N]                             (achieved_goal_vector)               */
    uint16_t *desired;    /* [N]                             (desired_goal_vector)                */
    int32_t *step_num;    /* [N]                                                                   */
    int32_t *ep_no;       /* [N]                                                                   */
} cw_state_view;

/* --- lifetime: replaces CraftingWorldEnvRay.__init__ (ray.py:59-143) for N envs ------------- */
int cw_create(const cw_config *cfg, int device, cw_engine **out);
int cw_destroy(cw_engine *e);

/* --- RNG: replaces seed() (ray.py:145-147) ----------------------------------------------------
 * cw_seed_mt injects numpy RandomState states: keys[N][624], pos[N] (RandomState.get_state()[1:3]).
 * cw_seed_int seeds env i like numpy RandomState(seeds[i]) (init_genrand).  Both are synchronous
 * host calls; the conversion itself runs on the device, one lane per env.  cw_get_mt returns states a numpy RandomState accepts via set_state and that
 * continue the identical stream, in numpy's own form: pos in 1..624 (a stream at a generation's end is reported as (that generation, 624), as
 * RandomState.get_state() does, not as (the next generation, 0)) -- after at least one draw the (key, pos) pair EQUALS the reference generator's.
 * These and the other synchronous entry points (cw_get_state, cw_set_state, cw_get_fixed_states, cw_checkpoint_*) wait for THIS ENGINE'S
 * work only -- whatever it enqueued on the streams it was handed since the last wait -- and do their copies on a stream of the engine's
 * own: another engine on the same device, or a learner, is not stalled (no device-wide synchronisation).  A stream handed to an enqueueing
 * call should stay alive until cw_synchronize on it (or one of these calls) has returned; if it was destroyed earlier the engine falls
 * back to one device-wide wait.  Work the engine cannot know of -- replays of a HIP graph its calls were captured into run on whatever
 * stream the graph is launched on -- is the caller's to wait for (cw_synchronize on that stream) before a synchronous call. */
int cw_seed_mt(cw_engine *e, const uint32_t *keys, const int32_t *pos);
int cw_seed_int(cw_engine *e, const uint32_t *seeds);
int cw_get_mt(cw_engine *e, uint32_t *keys, int32_t *pos);

/* generate_fixed_states (ray.py:149-154): draw fixed_init_state placements per env from the
 * env's current RNG stream.  No-op when fixed_init_state == 0.  Returns after the pool is complete (one-time cost). */
int cw_generate_fixed_states(cw_engine *e, cw_stream_t stream);
/* fixed_state_list (ray.py:116-118): the pool as cell indices, HOST array out[N][K][9] uint16 = the cells (row*S+col) of objects 0..7
 * (OBJECTS order, ray.py:21) and of the agent in each of the K placements of every env.  Synchronous; CW_ERR_INVALID when K == 0. */
int cw_get_fixed_states(cw_engine *e, uint16_t *out);

/* --- reset() for every env (ray.py:156-218): task draw, placement, imagine_obs, render ------ */
int cw_reset(cw_engine *e, cw_stream_t stream);

/* --- reset() (ray.py:156-218) for the envs i with mask[i] != 0; every other env is left exactly as it is.  The reference has no counterpart (there it
 * is one reset() call per env object).  mask: DEVICE pointer (with cw_config.host_outputs: or GPU-mapped host memory) to num_envs bytes, only read;
 * it may be cw_buffer_table.done itself -- `cw_step(e, a, t, s); cw_reset_masked(e, tab.done, s);` is the manual-reset loop of an engine without
 * auto_reset, which then computes what an auto_reset engine computes.  Works on auto_reset engines too (an episode cut short by the caller).
 * A selected row is left as cw_reset leaves it: new state, achieved = 0, desired = the new episode's mask, in the pixel modes its obs, init_obs and
 * desired_goal frames; reward, done, episode_length, episode_return, terminal_obs and counters[0..3] are NOT written -- a forced reset is not a finished
 * episode.  Engines that keep look-ahead records hand the env the record at the head of its ring (the refill that rides on cw_step tops the ring up);
 * an env without one is reset from its stream on the spot and counted in counters[5].
 * Only enqueues ONE kernel (cw_reset_masked_kernel) on `stream` -- no host synchronisation, no allocation -- so it can be captured into a HIP graph together
 * with cw_step / cw_step_many.  CW_ERR_STATE before the first cw_reset / cw_checkpoint_load. */
int cw_reset_masked(cw_engine *e, const uint8_t *mask, cw_stream_t stream);

/* --- imagine_obs() (ray.py:220-299) for the envs i with mask[i] != 0 (mask == NULL: every env), against each env's RUNNING episode: a new goal state drawn
 * from the episode's start state (INIT_OBS_VECTOR), the task bits in `desired` and -- in the GoToHouse branch, ray.py:274-276 -- the agent's CURRENT cell:
 * the goal's agent stands on the drawn house only while the agent stands on its start cell, else it stays on the start cell; the house is drawn either way.
 * Each selected env's stream advances by the draws its goal took.
 * mask, desired, out_frames, out_onehot: DEVICE pointers (with cw_config.host_outputs: or GPU-mapped host memory).
 * desired: uint16[num_envs] task bits (bit t = task_list[t]; bits at or above len(task_list) are ignored), or NULL: each env's own desired mask.  0 is
 *   legal: the goal is the start state and nothing is drawn.  (The start state holds one of each object, a bread and a house among them: every branch finds
 *   its object whatever the mask.)
 * commit != 0: the goal state becomes the episode's (cw_get_state goal_*, cw_export_onehot_of CW_STATE_GOAL, in the pixel modes the env's desired_goal
 *   frame is repainted); when `desired` was given the env's desired mask (hdr bytes 6-7, cw_buffer_table.desired) takes it too.  achieved, step_num, the
 *   flags, reward, done, the episode outputs and counters[0..3] are not written: a new goal is not a new episode.
 * out_frames (or NULL): the goal frame of env i at out_frames + i * frame_bytes, in the engine's raster and in every obs_mode (as cw_render);
 * out_onehot (or NULL): the goal state at out_onehot[i][S][S][12] (the OneHot variant's return, onehot.py:310).  Rows of unselected envs are not touched.
 * commit == 0 with neither output is CW_ERR_INVALID (nothing to do).  CW_ERR_STATE before the first cw_reset / cw_checkpoint_load.
 * Engines WITHOUT look-ahead records (auto_reset == 0, or host_outputs): enqueues ONE kernel (cw_imagine_masked_kernel) on `stream` -- no host synchronisation,
 * no allocation -- and can be captured into a HIP graph with cw_step / cw_reset_masked.
 * Engines that KEEP look-ahead records: their streams stand ahead of the envs' logical position, so the call first rewinds them as cw_generate_fixed_states
 * does (cw_get_mt + cw_seed_mt: every record is dropped, the next refill covers the whole batch), then launches.  That is synchronous, moves every env's
 * 2.5 KB of stream through the host and cannot be captured (CW_ERR_STATE while `stream` is capturing): it is OFF THE HOT PATH
 * (not timed yet: tools/measure_imagine.py).  A relabelling loop belongs on an auto_reset == 0 engine with cw_step + cw_reset_masked(done), which computes the same episodes. */
int cw_imagine_masked(cw_engine *e, const uint8_t *mask, const uint16_t *desired, int32_t commit,
                      uint8_t *out_frames, uint8_t *out_onehot, cw_stream_t stream);

/* --- sample_state() (ray.py:599-628; pooled != 0: generate_fixed_initial_state(), ray.py:630-644) for the envs i with mask[i] != 0 (NULL: every env), from
 * each env's stream: one shuffle of S*S tokens (pooled: one randint(K) and that row of the env's pool).  out_cells: DEVICE uint16[num_envs][9] = the cells
 * (row*S+col) of objects 0..7 and of the agent, the format of cw_get_fixed_states; rows of unselected envs are not touched, and nothing of an env but its
 * stream moves.  pooled with fixed_init_state == 0 is CW_ERR_INVALID (the reference's randint(0) raises before any draw).  Look-ahead records, capture and
 * call order as for cw_imagine_masked. */
int cw_sample_state_masked(cw_engine *e, const uint8_t *mask, int32_t pooled, uint16_t *out_cells, cw_stream_t stream);

/* --- device-resident snapshots: put an env back where it was, or let many envs continue from one env's state (tree search, "return, then explore",
 * branching rollouts, curriculum restarts).  The reference has no counterpart but copy.deepcopy of an env object.  Every engine can hold one snapshot
 * BANK in device memory: `rows` rows, each of which holds one env completely.
 * cw_snapshot_reserve allocates the bank, or re-allocates it: every saved row is dropped (a row loads only after it has been saved since the last reserve);
 *   rows == 0 frees it.  Synchronous; waits for this engine's own work only, as the other synchronous calls do (replays of a captured graph that uses the
 *   bank are the caller's to wait for).  CW_ERR_INVALID for rows < 0, CW_ERR_HIP when the allocation fails -- the engine is then left WITHOUT a bank.
 *   cw_snapshot_row_bytes: what one row holds (0 without a bank): 2 577 bytes + 196 on engines that keep look-ahead records + 18 per fixed_init_state.
 * rows (save and load): DEVICE int32[num_envs] (with cw_config.host_outputs: or GPU-mapped host memory), only read: the bank row of env i; rows[i] < 0:
 *   env i takes no part.  A row number at or above the capacity -- and on load a row never saved since the last reserve -- is SKIPPED: the env is left
 *   exactly as it is and counters[6] is incremented once.  No row number becomes an address without that check.
 * cw_snapshot_save: bank row rows[i] receives env i.  Writes nothing of the engine but the bank (and counters[6] for a skipped env).  Two envs naming the
 *   same row are the caller's error: the row then holds an unspecified mix of the two, nothing else is harmed.
 * cw_snapshot_load: env i receives bank row rows[i]; any number of envs may name the same row -- the fork.
 *   A row holds the EPISODE (current state and header, the start and goal states, ep_no) and the env's SOURCE OF FUTURE EPISODES (its MT19937 stream, on
 *   engines that keep look-ahead records its whole ring of them, its menu id -- hdr byte 3 -- and with fixed_init_state > 0 its pool row).
 *   with_stream != 0 restores both: the env becomes an exact twin of the saved one, and all its later resets are the saved env's.
 *   with_stream == 0 restores the episode only: the env keeps its own stream, ring, pool and menu id (everything else in hdr is the row's, the subset-reward
 *   flag and the success count among it), plays the saved episode to its end and goes on with episodes of its own -- what a caller wants who forks one
 *   state into 64 envs and does not want 64 identical next episodes.
 *   cw_buffer_table.achieved / .desired take the restored masks, as after cw_reset_masked; in the pixel modes the env's obs (held item included), init_obs and
 *   desired_goal frames are repainted.  reward, done, episode_length, episode_return, terminal_obs and counters[0..5] are NOT written: a restore is not
 *   a step and not a finished episode.
 * Both enqueue ONE kernel (cw_snapshot_save_kernel / cw_snapshot_load_kernel) on `stream` -- no host synchronisation, no allocation -- and can be captured
 * into a HIP graph with cw_step / cw_step_many / cw_reset_masked.  CW_ERR_STATE before the first cw_reset / cw_checkpoint_load and without a bank.
 * The bank is not part of a checkpoint blob; cw_checkpoint_load, cw_seed_* and cw_generate_fixed_states leave it alone.  (Not timed: tools/measure_snapshot.py.) */
int cw_snapshot_reserve(cw_engine *e, int32_t rows);
size_t cw_snapshot_row_bytes(const cw_engine *e);
int cw_snapshot_save(cw_engine *e, const int32_t *rows, cw_stream_t stream);
int cw_snapshot_load(cw_engine *e, const int32_t *rows, int32_t with_stream, cw_stream_t stream);

/* --- looking one step ahead: the successors of ALL SIX actions, of the engine's current states or of any states the caller hands in as packed records
 * (planners, greedy and one-step-lookahead policies, action masks, Q-bootstraps, tree search of any depth on the device).  The reference has no counterpart
 * but copy.deepcopy of an env object and six step() calls.  step() is a pure function of an env's header, its eight slot positions and its episode's
 * start positions (eval_task_edit, ray.py:672-702); it draws nothing from the RNG stream.  cw_expand is that function, with no env touched.
 * M = n_states.  Every output is ACTION-MAJOR: row a * M + j is action a (0..5 = Up, Right, Down, Left, PickUp, Drop) applied to input state j. */
typedef struct cw_expand_out {   /* DEVICE pointers (cw_config.host_outputs engines: or GPU-mapped host memory); a NULL field is not written; all NULL: CW_ERR_INVALID */
    int32_t  *reward;    /* [6][M]      what cw_step would return: -1 or max_steps                                  */
    uint8_t  *done;      /* [6][M]      step_num reached max_steps, or success (ray.py:367)                         */
    uint8_t  *changed;   /* [6][M]      the action changed the state (the reference's reward gate, ray.py:348-363)  */
    uint16_t *achieved;  /* [6][M]      achieved mask after the step                                                */
    uint8_t  *hdr;       /* [6][M][16]  successor header, the format of cw_buffer_table.hdr; 16-byte aligned        */
    uint16_t *slot_pos;  /* [6][M][8]   successor slots, the format of cw_buffer_table.slot_pos; 16-byte aligned    */
} cw_expand_out;
/* hdr_in == NULL: the engine's CURRENT states.  slot_pos_in and env_of must be NULL too and n_states must equal num_envs; input state j is env j.
 * hdr_in != NULL: n_states records of the caller's in the public packed formats, hdr_in [M][16] and slot_pos_in [M][8] (both required, both 16-byte
 *   aligned, device memory, only read): the engine's own hdr / slot_pos buffers, an earlier call's out->hdr / out->slot_pos, a pruned frontier.  The header
 *   supplies agent, hold, achieved, desired, step_num and the subset-reward flag; the ENV a record belongs to supplies what a record does not hold: its
 *   episode's start positions, and the engine its max_steps, size and task mask.
 *   env_of == NULL: state j belongs to env j % num_envs -- the action-major output of an engine-state call feeds back as n_states = 6 * num_envs with no
 *   index array, and again at 36 x and beyond.
 *   env_of != NULL: DEVICE int32[n_states], only read.  A negative entry: the state takes no part, its output rows are not written.  An entry >= num_envs
 *   is SKIPPED: its output rows are not written either and counters[7] is incremented once (not once per action).  No entry becomes an address
 *   without that check.
 * Records are never used as addresses: the step only compares cells.  An impossible record (an agent outside the grid, a hold above 3, a slot position
 * outside the grid) gives unspecified successor VALUES and never an out-of-bounds access.  out->hdr / out->slot_pos must not overlap the inputs.
 * Successor (a, j) is byte for byte what cw_step leaves in hdr / slot_pos for that env and action on an auto_reset == 0 engine: step_num + 1 (saturating),
 *   flag bit 0 cleared, the success count in flag bits 2-15 updated, the menu byte kept.  On auto-reset engines it is therefore the state BEFORE the reset --
 *   the terminal state the caller otherwise never sees.  A done state can be expanded again: like the reference (ray.py:367) it just keeps stepping.
 * PURE: nothing of the engine is written except counters[7], and that only for a skipped state -- no state, stream, look-ahead record, pool, bank, reward /
 *   done / mask / episode output, frame, or counters[0..6].
 * Enqueues ONE kernel (cw_expand_kernel: one lane per (action, state) pair, the action uniform across a wave) on `stream` -- no host synchronisation, no
 *   allocation -- and can be captured into a HIP graph with cw_step / cw_reset_masked / cw_snapshot_*.  Every obs_mode, with and without auto_reset,
 *   host_outputs engines included.  n_states == 0: CW_OK, nothing enqueued.  CW_ERR_STATE before the first cw_reset / cw_checkpoint_load.  CW_ERR_INVALID:
 *   a null engine or out, all six fields NULL, n_states < 0 or above 2^27, n_states != num_envs without hdr_in, hdr_in without slot_pos_in or the reverse,
 *   env_of without hdr_in, a misaligned hdr_in / slot_pos_in / out->hdr / out->slot_pos.  (13 us per call at 4 096 and at 65 536 states, launch included: tools/measure_expand.py, profiles/r07_expand.txt.) */
int cw_expand(cw_engine *e, const int32_t *env_of, const uint8_t *hdr_in, const uint16_t *slot_pos_in,
              int32_t n_states, const cw_expand_out *out, cw_stream_t stream);
/* cw_export_onehot for caller-supplied packed records instead of the engine's arrays: hdr [n_states][16], slot_pos [n_states][8] (16-byte aligned, device)
 * -> out [n_states][S][S][12], hold channels 9-11 at the agent's cell.  With cw_render_onehot it gives the reference's exact INT image of any successor
 * (int16, render(state=...)); the frame a pixel policy would see -- uint8, the engine's own raster, the bytes of `obs` -- is cw_render_records, one kernel
 * straight from the records.  One kernel (cw_export_onehot_states_kernel); the engine contributes only S.  n_states == 0: CW_OK, nothing enqueued; CW_ERR_INVALID for a null
 * argument, n_states < 0 or above 2^27, a misaligned hdr / slot_pos; CW_ERR_STATE before the first cw_reset / cw_checkpoint_load. */
int cw_export_onehot_states(cw_engine *e, const uint8_t *hdr, const uint16_t *slot_pos, int32_t n_states,
                            uint8_t *out /* [n_states][S][S][12] */, cw_stream_t stream);

/* --- what a pixel policy would SEE of packed records: frame j = the frame of record j (hdr [M][16], slot_pos [M][8], taken exactly as cw_expand and
 * cw_export_onehot_states take them: device memory, 16-byte aligned, only read), at out_frames + (size_t)j * frame_bytes.  uint8, in the engine's raster, in
 * every obs_mode (CW_OBS_STATE included, as cw_render does): byte for byte what cw_render or the obs array shows for an env in that state, the AltObs
 * modulo-256 pixel (sticks held over sticks) included.  Q(s') for the six successors of cw_expand, the value of the leaf of a cw_simulate plan: no one-hot
 * scratch tensor, no int16 image, no conversion.
 * Of a record only the agent's cell (hdr bytes 0-1), the hold (byte 2), the eight slot codes (bytes 12-15) and the slot positions matter; 0xFFFF and 0xFFFE
 *   (gone, held) are not drawn.  The engine contributes only its size and raster.  PURE: no env, stream, counter or buffer of the engine is read or written
 *   (unlike cw_expand not even counters[7]).
 * mask == NULL: every state.  Otherwise DEVICE uint8[M], only read: where mask[j] == 0 no byte of frame j is written, and the state costs one byte load.
 *   cw_expand's out->changed goes in as it is: an unchanged successor's frame is its parent's, which the caller already has.
 * Alignment as cw_render's: CW_RASTER_RAY needs a 4-byte aligned out_frames; CW_RASTER_ALT takes any (its frames start at every alignment anyway).  Offsets
 *   are 64-bit throughout (6 x 65 536 successors at 21x21 are 8.3 GB).  out_frames must not overlap the records or the mask.
 * An impossible record (an agent off the grid, a hold above 3, a slot code of 9..15, a slot position at or above S*S that is not one of the two markers) gives
 *   unspecified pixel VALUES inside that state's own frame and never a load or store outside the frame_bytes of frame j: the Ray painter only compares cells
 *   and selects colours, the AltObs painter turns (position, item) into a byte offset through one checked function (cw_host.h: cwh_alt_pixel_offset).
 * Enqueues ONE kernel (cw_render_records_kernel: one wave per state, grid-stride) on `stream` -- no host synchronisation, no allocation -- and can be
 *   captured into a HIP graph together with cw_expand / cw_simulate / cw_step.  host_outputs engines included.  n_states == 0: CW_OK, nothing enqueued.
 *   CW_ERR_STATE before the first cw_reset / cw_checkpoint_load.  CW_ERR_INVALID: a null engine, hdr, slot_pos or out_frames, n_states < 0 or above 2^27, a
 *   misaligned hdr / slot_pos, a Ray out_frames that is not 4-byte aligned, out_frames overlapping the records or the mask.
 *   (6 x 65 536 successors at 21x21, launch included: 1.69 ms for the 8.3 GB of Ray frames (4.9 TB/s), 1.16 ms for the 4.9 GB of AltObs frames; with mask = changed, 63 % of the rows: 1.13 / 0.78 ms; the one-hot route on the same records: 18.7 / 12.0 ms: tools/measure_render_records.py, profiles/r09_render_records.txt.) */
int cw_render_records(cw_engine *e, const uint8_t *hdr, const uint16_t *slot_pos, const uint8_t *mask /* DEVICE uint8 [n_states] or NULL */,
                      int32_t n_states, uint8_t *out_frames /* [n_states][frame_bytes] */, cw_stream_t stream);

/* --- trying plans: T steps of M states along M action sequences of the caller's, with no env touched (random shooting, CEM, MPC, MCTS leaf rollouts, beam
 * search).  The multi-step companion of cw_expand: the same pure step function, each state kept in registers for the whole sequence, ONE kernel.
 * M = n_states, T = n_steps.  State j steps through actions[t * M + j] for t = 0 .. T-1 (DEVICE uint8, step-major like cw_rollout's, only read).  An action
 * id above 5 is the state-preserving no-op of cw_step (step_num + 1, reward -1); it is not counted anywhere. */
typedef struct cw_simulate_out {  /* DEVICE pointers (host_outputs engines: or GPU-mapped host memory); NULL = not written; all NULL: CW_ERR_INVALID */
    int32_t  *ret;       /* [M]      sum of the rewards of the steps TAKEN                                   */
    int32_t  *length;    /* [M]      1 + index of the first step that returned done; n_steps if none did     */
    uint8_t  *done;      /* [M]      some step returned done                                                 */
    uint16_t *achieved;  /* [M]      achieved mask after the last step taken                                 */
    uint8_t  *hdr;       /* [M][16]  record after the last step taken; 16-byte aligned                       */
    uint16_t *slot_pos;  /* [M][8]   16-byte aligned                                                         */
    int32_t  *rewards;   /* [T][M]   per-step trace, step-major like cw_rollout's                            */
    uint8_t  *dones;     /* [T][M]                                                                           */
} cw_simulate_out;
/* hdr_in != NULL: n_states records of the caller's, exactly as cw_expand takes them: hdr_in [M][16] and slot_pos_in [M][8] (both required, both 16-byte
 *   aligned, device memory, only read); env_of == NULL: state j belongs to env j % num_envs; env_of != NULL: DEVICE int32[n_states] -- a negative entry:
 *   the state takes no part and NO output row of it is written, its trace rows [t][j] included; an entry >= num_envs is SKIPPED: its rows are not written
 *   either and counters[7] is incremented once.  No entry becomes an address without that check.
 * hdr_in == NULL: the engine's CURRENT states, BROADCAST: slot_pos_in and env_of must be NULL, n_states must be a positive multiple of num_envs, and state
 *   j is env j % num_envs -- K candidate plans per env are n_states = K * num_envs, plan k of env i in row k * num_envs + i, with no copy of the records.
 * stop_at_done != 0: a state's first done step is its last -- the episode ends there, as on an auto-reset engine, minus the reset.  hdr, slot_pos,
 *   achieved, ret and length are those of that step; the trace row of the ending step holds its reward and done 1, the rows after it reward 0 and done 0.
 * stop_at_done == 0: every state takes all T steps, as the reference keeps stepping a finished env (ray.py:367): ret sums all T rewards, length is still
 *   1 + the first done step (T if none), done: some step returned done.
 * The final record is byte for byte what the same number of cw_step calls leave in hdr / slot_pos on an auto_reset == 0 engine (step_num saturating, flag
 *   bit 0 cleared, the success count in flag bits 2-15, the menu byte kept), and what chaining cw_expand and picking the action's row each time gives.
 *   out->hdr / out->slot_pos must not overlap the records read.  Records are never used as addresses (cw_expand's rule for impossible records holds).
 * PURE: nothing of the engine is written except counters[7], and that only for a skipped state; nothing is drawn from any RNG stream.
 * Enqueues ONE kernel (cw_simulate_kernel: one lane per state) on `stream` -- no host synchronisation, no allocation -- and can be captured into a HIP graph
 *   with cw_step / cw_expand / cw_snapshot_*.  Every obs_mode, with and without auto_reset, host_outputs engines included.  n_states == 0 (with hdr_in):
 *   CW_OK, nothing enqueued.  CW_ERR_STATE before the first cw_reset / cw_checkpoint_load.  CW_ERR_INVALID: a null engine, out or actions, all eight fields
 *   NULL, n_states < 0 or above 2^27, n_steps < 1 or above 32 767 (with max_steps <= 65 535 the int32 sum then cannot overflow), n_states not a positive
 *   multiple of num_envs without hdr_in, hdr_in without slot_pos_in or the reverse, env_of without hdr_in, a misaligned hdr_in / slot_pos_in / out->hdr /
 *   out->slot_pos, out->hdr or out->slot_pos overlapping the records read.  (65 536 envs, 21x21, launch included: 22 us for 8 steps, 83 us for 64; 16 plans per env: 62 / 359 us: tools/measure_simulate.py, profiles/r08_simulate.txt.) */
int cw_simulate(cw_engine *e, const int32_t *env_of, const uint8_t *hdr_in, const uint16_t *slot_pos_in, int32_t n_states,
                const uint8_t *actions /* DEVICE uint8 [n_steps][n_states] */, int32_t n_steps, int32_t stop_at_done,
                const cw_simulate_out *out, cw_stream_t stream);

/* --- whole trajectories: cw_simulate with EVERY record along the way written out -- the states of a plan, not only its end (imitation data from the planners,
 * value targets along a plan, the frames of a whole trajectory through cw_render_records, any step of a plan as a start state through cw_load_records).
 * M = n_states, T = n_steps; the records are step-major, row t of state j at [t * M + j]. */
typedef struct cw_unroll_out {   /* DEVICE pointers (host_outputs engines: or GPU-mapped host memory); NULL = not written; all NULL: CW_ERR_INVALID */
    uint8_t  *hdr;       /* [T+1][M][16]  row 0: the record as read; row t+1: the record after step t; 16-byte aligned */
    uint16_t *slot_pos;  /* [T+1][M][8]   16-byte aligned */
    int32_t  *reward;    /* [T][M]  */
    uint8_t  *done;      /* [T][M]  */
    uint8_t  *changed;   /* [T][M]  the step changed the state (cw_expand's `changed`) */
    uint8_t  *taken;     /* [T][M]  1: step t was taken; goes into cw_render_records as a mask for rows 1..T */
    int32_t  *length;    /* [M]     cw_simulate's length */
} cw_unroll_out;
/* The inputs are cw_simulate's, rule for rule: hdr_in == NULL broadcasts the engine's own states (n_states a positive multiple of num_envs, state j is env
 *   j % num_envs); otherwise the caller's records with env_of NULL or DEVICE int32[M] -- a negative entry: the state takes no part and NO row of it is
 *   written at any t; an entry >= num_envs is skipped the same way and counted once in counters[7].  An action id above 5 is the no-op: step_num + 1,
 *   reward -1, changed 0.
 * The outputs, by equalities with the calls that exist:
 *   reward, done and length equal cw_simulate's rewards, dones and length for the same arguments.
 *   Row T of hdr / slot_pos equals cw_simulate's hdr / slot_pos byte for byte.  Row 0 is the record read, byte for byte -- with broadcast states the
 *     engine's records tiled.
 *   For a TAKEN step t with action a <= 5, row t+1 is byte for byte cw_expand's successor (a, .) of row t, and changed[t] is its `changed`.
 *   stop_at_done != 0: step t is taken iff no earlier step of that state returned done.  For a step NOT taken reward, done, changed and taken are all 0 and
 *     row t+1 equals row t, so the final record repeats to row T.  stop_at_done == 0: every step is taken.
 *   The achieved mask after step t is bytes 4-5 of hdr[t+1]; there is no separate field.
 * ONE LAUNCH STAYS BOUNDED: (n_steps + 1) * n_states <= 2^27.  The whole [T+1][M] record array is then a legal input, flattened, to cw_render_records,
 *   cw_export_onehot_states, cw_seen_insert and cw_load_records, and each record array stays at or below 2 GiB.
 * PURE: nothing of the engine is written except counters[7], and that only for a skipped state; nothing is drawn from any RNG stream.
 * Enqueues ONE kernel (cw_unroll_kernel: one lane per state, the state in registers for all T steps, two 16-byte stores a lane and step) on `stream` -- no
 *   host synchronisation, no allocation -- and can be captured into a HIP graph.  Every obs_mode, with and without auto_reset, host_outputs engines included.
 *   n_states == 0 (with hdr_in): CW_OK, nothing enqueued.  Errors, tested in this order -- CW_ERR_INVALID: a null engine, out or actions; all seven fields
 *   NULL, n_states < 0 or above 2^27, n_steps < 1 or above 32 767, (n_steps + 1) * n_states above 2^27, hdr_in without slot_pos_in or the reverse, env_of
 *   without hdr_in, n_states not a positive multiple of num_envs without hdr_in; a misaligned hdr_in / slot_pos_in / out->hdr / out->slot_pos (16 bytes),
 *   out->reward / out->length / env_of (4 bytes); an output sharing a byte with the records read, actions, env_of or another output.  Then CW_ERR_STATE
 *   before the first cw_reset / cw_checkpoint_load.  (Not timed yet: tools/measure_unroll.py.) */
int cw_unroll(cw_engine *e, const int32_t *env_of, const uint8_t *hdr_in, const uint16_t *slot_pos_in, int32_t n_states,
              const uint8_t *actions /* DEVICE uint8 [n_steps][n_states] */, int32_t n_steps, int32_t stop_at_done,
              const cw_unroll_out *out, cw_stream_t stream);

/* --- searching every plan: the best that can be done from a state within D steps, and which action starts it (the exhaustive receding-horizon controller:
 * an expert for imitation, an optimal-within-horizon baseline, an exact ranking of the six actions, the "goal reachable within D steps" label).
 * M = n_states, D = depth.  For input state j and first action a in 0..5 take every action string p in {0..5}^D with p[0] = a, and let R(p) be cw_simulate's
 * `ret` for that state with n_steps = D and stop_at_done = 1.  q[a][j] = max R(p).  The BEST PLAN p* is the lexicographically smallest maximiser in canonical
 * form: its entries at t >= length are 0 (those steps are never taken: all strings that share the taken prefix tie, and the smallest of them ends in zeros) --
 * the first strict maximum of a depth-first pre-order walk that does not descend below a done step.  length, done, achieved, hdr and slot_pos are what
 * cw_simulate returns for p*, hdr and slot_pos byte for byte. */
typedef struct cw_plan_out {   /* DEVICE pointers (host_outputs engines: or GPU-mapped host memory); NULL = not written; all NULL: CW_ERR_INVALID; ACTION-MAJOR like cw_expand_out */
    int32_t  *q;         /* [6][M]      the best return within D steps after first action a                            */
    int32_t  *length;    /* [6][M]      steps p* takes: 1 + its done step, D if it has none                            */
    uint8_t  *done;      /* [6][M]      p* ends inside the horizon                                                     */
    uint16_t *achieved;  /* [6][M]      achieved mask after p*'s last step                                             */
    uint8_t  *hdr;       /* [6][M][16]  record after p*'s last step; 16-byte aligned                                   */
    uint16_t *slot_pos;  /* [6][M][8]   16-byte aligned                                                                */
    uint8_t  *plan;      /* [6][D][M]   p*; plan[a] is step-major: it feeds cw_simulate's `actions` as it is; plan[a][0][j] == a */
} cw_plan_out;
/* The inputs follow cw_expand's rules.  hdr_in == NULL: the engine's CURRENT states, n_states == num_envs, slot_pos_in and env_of NULL.  Otherwise n_states
 *   records of the caller's (hdr_in [M][16], slot_pos_in [M][8], both required, 16-byte aligned, only read); the env of state j is j % num_envs, or
 *   env_of[j] (DEVICE int32 [M]): a negative entry takes no part and NO row of it is written; an entry >= num_envs is SKIPPED: no row is written either and
 *   counters[7] is incremented once.  No entry becomes an address without that check.
 * 1 <= depth <= 8, and n_states * 6^depth <= 2^32: one launch on a shared card must stay short (65 536 states at depth 6, 2 048 at depth 8).
 * PURE: nothing of the engine is written except counters[7]; nothing is drawn from any RNG stream.
 * Enqueues ONE kernel (cw_plan_kernel: one lane per (first action, state) pair, a depth-first search whose stack is in registers and whose action is uniform
 *   across a wave at every level; no memory access inside the search) on `stream` -- no host synchronisation, no allocation -- and can be captured into a HIP
 *   graph with cw_step / cw_expand / cw_simulate.  Every obs_mode, with and without auto_reset, host_outputs engines included.  n_states == 0 (with hdr_in):
 *   CW_OK, nothing enqueued.  CW_ERR_STATE before the first cw_reset / cw_checkpoint_load.  CW_ERR_INVALID: a null engine or out, all seven fields NULL,
 *   n_states < 0 or above 2^27, depth < 1 or above 8, n_states * 6^depth above 2^32, hdr_in without slot_pos_in or the reverse, env_of without hdr_in,
 *   n_states != num_envs without hdr_in, a misaligned hdr_in / slot_pos_in / out->hdr / out->slot_pos.
 *   (21x21, launch included: 65 536 envs 23 us at depth 1, 1.08 ms at 4, 5.9 ms at 5, 33.5 ms at 6 with no goal in reach -- the whole tree; the enumeration through cw_simulate: 311 us / 2.47 ms at depths 1 / 4, over its cap from 5 on: tools/measure_plan.py, profiles/r10_plan.txt.) */
int cw_plan(cw_engine *e, const int32_t *env_of, const uint8_t *hdr_in, const uint16_t *slot_pos_in, int32_t n_states, int32_t depth,
            const cw_plan_out *out, cw_stream_t stream);

/* --- shooting plans: the best of K SAMPLED plans of T steps per state, at horizons cw_plan cannot reach (random shooting; with `weights` and `ret` the two halves
 * of a CEM iteration) -- the actions are drawn where they are used, so no [T][K][M] action tensor exists.  M = n_states, T = n_steps, K = n_samples.
 * THE DRAW is a public, exact, integer function of (seed, state, sample, step); callers reproduce it (uint32 arithmetic wraps; mulhi32(a, b) = (a * b) >> 32 in 64 bits):
 *   mix(x):   x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16        (uint32, wrapping)
 *   draw(seed, state, sample, step):                                                            (seed uint64, the rest uint32)
 *             x = mix((uint32)seed ^ state * 0x9E3779B1)
 *             x = mix(x ^ ((uint32)(seed >> 32) + sample * 0x85EBCA77))
 *             return mix(x ^ step * 0xC2B2AE3D)
 *   action(r, w == NULL)   = mulhi32(r, 6)                                                      (uniform over 0..5)
 *   action(r, w[0..5] u16) = W = w0 + .. + w5;  W == 0: as w == NULL;
 *                            else x = mulhi32(r, W);  the number of a in 0..4 with w0 + .. + wa <= x
 * `state` is the input row j (not its env), `sample` is k, `step` is t.  No float appears anywhere.  The effective seed is s = seed + (seed_dev ? *seed_dev : 0)
 * mod 2^64; seed_dev is a DEVICE word the kernel reads, so a captured graph draws new plans on every replay once the caller bumps the word.
 * Sample k of state j plays the actions a(k, t) = action(draw(s, j, k, t), weights ? the six uint16 weights[(t * 6 + a) * M + j], a = 0..5 : NULL); weights is
 * DEVICE uint16 [T][6][M], only read (a zero weight forbids its action at that step of that state; all six zero: uniform).  R(k) is cw_simulate's `ret` for
 * state j along those actions with n_steps = T and stop_at_done = 1.  k* is the SMALLEST k with R(k) = max R; length, done, achieved, hdr and slot_pos are what
 * cw_simulate returns for sample k*, hdr and slot_pos byte for byte. */
typedef struct cw_shoot_out {   /* DEVICE pointers (host_outputs engines: or mapped host memory); NULL = not written; all NULL: CW_ERR_INVALID */
    int32_t  *best_ret;     /* [M]     max over k of R(k)                                                   */
    int32_t  *best_sample;  /* [M]     k*: the SMALLEST k that reaches it                                   */
    uint8_t  *best_action;  /* [M]     the first action of sample k*                                        */
    int32_t  *length;       /* [M]     of sample k*, as cw_simulate (stop_at_done = 1)                      */
    uint8_t  *done;         /* [M]                                                                          */
    uint16_t *achieved;     /* [M]                                                                          */
    uint8_t  *hdr;          /* [M][16] record after k*'s last step taken, byte for byte cw_simulate's; 16-byte aligned */
    uint16_t *slot_pos;     /* [M][8]  16-byte aligned                                                      */
    uint8_t  *plan;         /* [T][M]  ALL T drawn actions of sample k*, step-major: feeds cw_simulate as it is */
    int32_t  *ret;          /* [K][M]  R(k) of every sample (CEM's elite selection)                         */
} cw_shoot_out;
/* The inputs follow cw_plan's rules exactly.  hdr_in == NULL: the engine's CURRENT states, n_states == num_envs, slot_pos_in and env_of NULL.  Otherwise n_states
 *   records of the caller's (hdr_in [M][16], slot_pos_in [M][8], both required, 16-byte aligned, only read); the env of state j is j % num_envs, or env_of[j]
 *   (DEVICE int32 [M]): a negative entry takes no part and NO row of it is written, ret[k][j] and plan[t][j] included; an entry >= num_envs is SKIPPED: no row is
 *   written either and counters[7] is incremented once per state.  No entry becomes an address without that check.
 * 1 <= n_steps <= 32 767, 1 <= n_samples <= 65 536, and n_states * n_samples * n_steps <= 2^32: one launch on a shared card must stay short (65 536 states x
 *   1 024 samples x 64 steps).  out->hdr / slot_pos / plan / ret must overlap neither the records read nor weights.
 * PURE: nothing of the engine is written except counters[7]; nothing is drawn from any RNG stream of the engine.
 * Enqueues ONE kernel (cw_shoot_kernel: G lanes per state, G a power of two <= 64 chosen so that a small batch spreads its samples over the wave, each lane
 *   playing samples g, g + G, ... with the state in registers; the lanes reduce by shuffles and the winning lane writes its own record; no memory access inside
 *   the step loop but the six weights a step, fetched a block ahead) on `stream` -- no host synchronisation, no allocation -- and can be captured into a HIP graph
 *   with cw_step / cw_expand / cw_simulate / cw_plan.  Every obs_mode, with and without auto_reset, host_outputs engines included.  n_states == 0 (with hdr_in):
 *   CW_OK, nothing enqueued.  CW_ERR_STATE before the first cw_reset / cw_checkpoint_load.  CW_ERR_INVALID: a null engine or out, all ten fields NULL, n_states < 0
 *   or above 2^27, n_steps < 1 or above 32 767, n_samples < 1 or above 65 536, the product above 2^32, hdr_in without slot_pos_in or the reverse, env_of without
 *   hdr_in, n_states != num_envs without hdr_in, a misaligned hdr_in / slot_pos_in / out->hdr / out->slot_pos, an overlap as above.
 *   (21x21, launch included, no goal in reach: 4 096 envs x 16 samples 23 us at 8 steps and 81 us at 64, against 114 / 131 us for torch.randint + cw_simulate + the reduction in torch; NOT faster than that route from 4 096 x 64 x 32 on and at 65 536 envs -- 63.8 against 25.5 ms at 65 536 x 1 024 x 64 -- because the lane rule fills the card with one wave per SIMD: tools/measure_shoot.py, profiles/r11_shoot.txt.) */
int cw_shoot(cw_engine *e, const int32_t *env_of, const uint8_t *hdr_in, const uint16_t *slot_pos_in, int32_t n_states, int32_t n_steps, int32_t n_samples,
             uint64_t seed, const uint64_t *seed_dev, const uint16_t *weights, const cw_shoot_out *out, cw_stream_t stream);
/* THE DECODER: out[t][r][j] = action(draw(s, j, samples ? samples[r * M + j] : r, t), weights as above), uint8 [T][n_rows][M] in device memory.  samples: DEVICE
 * int32 [n_rows][M], only read; a NEGATIVE entry leaves that column of that row unwritten (cw_shoot's best_sample of a state that took no part, once the caller
 * has filled it with -1).  samples == NULL with n_rows = K materialises the whole action tensor in cw_simulate's broadcast layout (the bridge to cw_simulate);
 * samples = the elites' indices gives a CEM refit its elites' actions.  One grid-stride kernel (cw_shoot_actions_kernel), pure: the engine contributes only its
 * stream bookkeeping and CW_ERR_STATE before the first cw_reset.  0 <= n_rows, n_states <= 2^27, 1 <= n_steps <= 32 767, n_rows * n_states * n_steps <= 2^32, else
 * CW_ERR_INVALID, as for a null engine or out; n_states == 0 or n_rows == 0: CW_OK, nothing enqueued. */
int cw_shoot_actions(cw_engine *e, int32_t n_states, int32_t n_steps, uint64_t seed, const uint64_t *seed_dev, const uint16_t *weights,
                     const int32_t *samples, int32_t n_rows, uint8_t *out /* [T][n_rows][M] */, cw_stream_t stream);
/* THE REFIT: the other half of a CEM iteration -- from cw_shoot's ret [K][M] to the next weights [T][6][M], exact, integer and deterministic, with no [T][E][M]
 * action tensor: the elites' actions are regenerated from THE DRAW.  M = n_states, T = n_steps, K = n_samples, E = n_elites.
 * ret is DEVICE int32 [K][M], only read: cw_shoot's, or any int32 values at all (INT32_MIN and INT32_MAX order as integers do).
 * THE ELITES of state j: order its K samples by (ret[k][j] DESCENDING, k ASCENDING) and take the first E -- a tie goes to the smaller sample, best_sample's
 *   rule.  Equivalently: v = the E-th largest value of the column, counted with multiplicity; the elites are every sample above v and the smallest-indexed samples
 *   equal to v until E is reached.  elites[0..E-1][j] holds them in ASCENDING sample order; elite_min[j] = v.  A function of the inputs alone, never of scheduling.
 * THE COUNTS: c[t][a][j] = how many elites k of state j have action(draw(s, j, k, t), weights_in ? the six uint16 weights_in[(t * 6 + a') * M + j], a' = 0..5 : NULL)
 *   == a, with s = seed + (seed_dev ? *seed_dev : 0) mod 2^64 -- cw_shoot's draw with cw_shoot's seed and weights.  ALL T drawn actions of an elite count, as
 *   cw_shoot's `plan` holds all T: the steps BEHIND a sample's done step, which cw_shoot never played, are included.  The six counts of a (t, j) sum to E.
 * THE NEW WEIGHTS: weights[(t * 6 + a) * M + j] = min(65535, smooth + gain * c[t][a][j]) in uint32 arithmetic (no wrap: at most 65535 + 65535 * 65536).  smooth,
 *   0 .. 65 535, is a pseudo-count: 0 lets an action no elite drew become FORBIDDEN at that step of that state.  gain is 1 .. 65 535.  The six new weights are
 *   never all zero (E >= 1 and gain >= 1).
 * IN PLACE: out->weights == weights_in, the same address, is legal -- the six weights of a (t, j) are read by the one lane that writes them, before it writes;
 *   a CEM loop keeps one weights buffer.  Any other overlap of the two is CW_ERR_INVALID.
 * STATES THAT TAKE NO PART: env_of is NULL (every state takes part) or DEVICE int32 [M], cw_shoot's; a negative entry or an entry >= num_envs takes no part --
 *   exactly the states whose ret column cw_shoot did not write -- and NOTHING of such a state is written in any output.  It is not counted in counters[7]:
 *   cw_shoot counted it already.  No entry becomes an address. */
typedef struct cw_refit_out {      /* DEVICE pointers; elites is REQUIRED, the others may be NULL */
    int32_t  *elites;     /* [E][M]     the E elite samples of state j, in ASCENDING sample order; 4-byte aligned */
    uint16_t *weights;    /* [T][6][M]  the refitted weights, cw_shoot's layout; NULL: selection only              */
    int32_t  *elite_min;  /* [M]        the smallest return among the elites (the E-th largest of the column)      */
} cw_refit_out;
/* PURE: nothing of the engine is read but num_envs (the env_of test) and nothing written; the engine contributes its stream bookkeeping and the has_reset rule.
 * Enqueues TWO kernels on `stream` (cw_refit_select_kernel: cw_shoot's G lanes per state, the column's min and max, a binary search on the value for v -- at most
 *   32 passes over the column, 17 for cw_shoot's returns -- and one pass that compacts in sample order by ballots; cw_refit_count_kernel: one lane per (t, j), E
 *   regenerated draws, six coalesced stores; not enqueued when out->weights is NULL) -- no atomics, no host synchronisation, no allocation -- and can be captured
 *   into a HIP graph with cw_shoot / cw_step.  Every obs_mode, host_outputs engines included.  n_states == 0: CW_OK, nothing enqueued.  CW_ERR_STATE before the
 *   first cw_reset / cw_checkpoint_load.  CW_ERR_INVALID, tested in this order: a null engine or out; a null ret or out->elites; n_states < 0 or above 2^27;
 *   n_steps outside 1 .. 32 767; n_samples outside 1 .. 65 536; n_elites outside 1 .. n_samples; n_states * n_samples * n_steps above 2^32 (cw_shoot's cap: the
 *   refit does at most that many draws); smooth above 65 535; gain outside 1 .. 65 535; env_of, ret, out->elites or out->elite_min not 4-byte or weights_in,
 *   out->weights not 2-byte aligned; an output sharing a byte with ret, env_of, another output, or weights_in other than the exact in-place case.
 *   (21x21, launch included, (K, T, E) = (16, 8, 4) / (1 024, 64, 64): 4 096 envs 20 / 131 us, 65 536 envs 32 us / 2.69 ms, against 70 / 622 us and 439 us / 8.77 ms for torch.topk + cw_shoot_actions + a scatter_add histogram + clamp and cast in torch; a whole iteration behind cw_shoot 42 us / 4.38 ms and 176 us / 66.5 ms against 92 us / 4.89 ms and 584 us / 72.6 ms: tools/measure_refit.py, profiles/r14_refit.txt.) */
int cw_shoot_refit(cw_engine *e, const int32_t *env_of, int32_t n_states, int32_t n_steps, int32_t n_samples, int32_t n_elites,
                   uint64_t seed, const uint64_t *seed_dev, const uint16_t *weights_in, const int32_t *ret,
                   uint32_t smooth, uint32_t gain, const cw_refit_out *out, cw_stream_t stream);

/* --- searching deep: "have I seen this state before?" -- a device-resident VISITED SET of packed records, filled by kernels (breadth-first search with duplicate
 * detection, distance-to-goal labels, the "solvable within D steps" filter of a curriculum).  6^D action strings reach far fewer than 6^D states; cw_expand plus
 * this set walk the states, not the strings.  The reference has no counterpart.
 * THE KEY.  Two records of one GROUP are the same state if they agree in everything a step reads except the two step counters.  The 36-byte key is: group
 *   (int32); hdr bytes 0-2 (agent row, agent col, hold); hdr bytes 4-7 (achieved mask, desired mask); bit 1 of hdr byte 10 (the subset reward rule); hdr bytes
 *   12-15 (the eight slot codes); the 16 bytes of slot_pos.  NOT in the key: hdr byte 3 (the menu id: kept by a step, never read), hdr bytes 8-9 (step_num),
 *   flags bit 0 and bits 2-15 (no step taken yet, the success count).  (csrc/cw_host.h: cwh_seen_key, shared by the kernels and the CPU tests.)
 *   CONSEQUENCE: records with equal keys (the group being the env, or finer) have successors with equal keys under every action, and equal reward, changed and
 *   achieved; done is equal except for its time-out term step_num >= max_steps.
 *   The group says which records may be merged at all: by default the env index j % num_envs -- an episode's start positions decide its Move tasks --, or any
 *   non-negative int32 of the caller's (a search from several start states of one env with different step budgets passes the start row).
 * cw_seen_reserve: one set per engine, or a new one: everything seen is dropped.  `capacity` is the number of distinct keys the caller means to hold; the table
 *   gets the next power of two >= 2 * capacity slots of 48 bytes (cw_seen_slots; 0 without a set); capacity == 0 frees it.  Synchronous; waits for this engine's
 *   own work only, as cw_snapshot_reserve does.  CW_ERR_INVALID for capacity < 0 or above 2^28 or tag_bits outside 0 .. 63; CW_ERR_HIP when the allocation fails --
 *   the engine is then left WITHOUT a set.  tag_bits: 0, a slot's tag is the full 64-bit hash of the key; 1 .. 63 truncates it to that many bits -- only speed
 *   and the collisions counter depend on it (it lets tests and tools/measure_seen.py drive the same-tag-different-key path, which 64 bits never take in practice).
 *   The set is not part of a checkpoint blob or of a snapshot row; cw_reset, cw_checkpoint_load and cw_seed_* leave it alone.
 * cw_seen_clear: empties the set and resets its counters by ONE kernel (cw_seen_clear_kernel) on `stream`; capturable.
 * cw_seen_counters: where the set's three counters live -- DEVICE uint64[3], read-only for callers, valid until the next cw_seen_reserve: [0] keys held,
 *   [1] overflow, [2] collisions (below). */
typedef struct cw_seen_out {   /* DEVICE pointers; a NULL field is not written; both NULL: CW_ERR_INVALID */
    uint8_t *fresh;   /* [M]  1: this row brings its key into the set */
    int32_t *first;   /* [M]  -1: the key was in the set BEFORE this call; else the smallest participating row of this call with the same key; 4-byte aligned */
} cw_seen_out;
/* cw_seen_insert: hdr [M][16] and slot_pos [M][8] are taken exactly as cw_expand takes records: device memory, 16-byte aligned, only read.  group: DEVICE
 *   int32[M], only read, or NULL: row j is of group j % num_envs.  A NEGATIVE group entry: the row takes no part -- nothing of it is written, it is not inserted.
 *   For a participating row j: first[j] = -1 if its key was in the set before this call; otherwise the smallest participating row of this call with the same
 *   key -- j itself for the one row that brings the key in; fresh[j] = (first[j] == j).  After the call every participating key is in the set.
 * The outputs are a function of the inputs and of the calls since the last clear, NOT of scheduling: the smallest row wins, whatever order the waves arrive in.
 *   Two exceptions, both in the SAFE direction and both counted: counters[1] OVERFLOW -- a row found no slot within the probe bound (128 slots from its hash;
 *   a set filled beyond its capacity) --, counters[2] COLLISIONS -- a row met a slot whose tag equals its own but whose key differs.  Such a row is reported
 *   first = j, fresh = 1 and may not be remembered.  The opposite error is impossible by construction -- a key is reported as seen, or as a duplicate of row i,
 *   only after a byte comparison with the stored key, or with record i --: a search on top of the set stays exact and at worst expands a state again.
 *   counters[0] is the number of keys held.
 * "Before this call" is told from "in this call" by an epoch word that lives in the set and advances ON THE DEVICE with every insert: a replayed graph behaves
 *   like a repeated call.  2^36 - 1 inserts after a clear the epochs are used up: from then on every participating row is reported fresh and counted as
 *   overflow, and nothing is inserted, until the next cw_seen_clear.
 * PURE with respect to the engine: no env, stream, record, bank, frame or counters[0..7] of cw_buffer_table is read or written; the engine contributes its set,
 *   num_envs for the default group and its stream bookkeeping.
 * Enqueues TWO kernels (cw_seen_claim_kernel, cw_seen_resolve_kernel: one lane per row, grid-stride, atomics on the slot words, no lane ever waits for another)
 *   on `stream` -- no host synchronisation, no allocation -- and can be captured into a HIP graph with cw_expand.  n_states == 0: CW_OK, nothing enqueued.
 *   CW_ERR_STATE before the first cw_reset / cw_checkpoint_load and without a set.  CW_ERR_INVALID: a null engine, out, hdr or slot_pos, both fields NULL,
 *   n_states < 0 or above 2^27, misaligned records (group and first: 4 bytes), an output overlapping the records, group or the other output.
 *   (21x21, the 6 N successors of cw_expand, launch included: 31 us for 24 576 rows and 151 us for 393 216 into an empty set, 23 / 106 us for the same rows again; torch.unique over the same keys: 225 / 390 us, and it has no memory of earlier calls: tools/measure_seen.py, profiles/r12_seen.txt.) */
int cw_seen_reserve(cw_engine *e, int64_t capacity, int32_t tag_bits);
int cw_seen_clear(cw_engine *e, cw_stream_t stream);
int cw_seen_insert(cw_engine *e, const int32_t *group, const uint8_t *hdr, const uint16_t *slot_pos, int32_t n_states, const cw_seen_out *out, cw_stream_t stream);
int cw_seen_counters(const cw_engine *e, const uint64_t **counters);   /* *counters = the DEVICE uint64[3]; CW_ERR_STATE (and NULL) without a set */
size_t cw_seen_slots(const cw_engine *e);

/* --- breadth-first search without a host round trip: the SHORTEST plan that ends in success from each of M start states, or "none within max_depth steps" --
 * cw_expand's step, the visited set above and a stable compaction, level after level, in ONE call that only enqueues kernels: the frontier's size lives in
 * device memory.  Capturable with the steps ("step, then label every env with its distance to the goal").  The reference has no counterpart.
 * cw_reach_reserve: the WORKSPACE, one allocation per engine, or a new one; max_rows == 0 frees it.  max_rows is the cap on a frontier AND on the start rows of a
 *   call; 1 <= max_rows with 6 * (max_rows + 63) < 2^28 (the row field of the set's bids), 1 <= max_depth <= 32 767, else CW_ERR_INVALID; CW_ERR_HIP when the
 *   allocation fails -- the engine is then left WITHOUT a workspace.  Synchronous; waits for this engine's own work only, as cw_seen_reserve does.  It holds two
 *   frontiers (record, env, start row: 80 bytes a row), the successors of one level (6 x 37 bytes a row), the links of every level but the last (parent and
 *   action, 4 bytes a row and level), 13 bytes per start row and a control block (the frontier's size per level, a stop flag, the scan's scratch):
 *   cw_reach_bytes (0 without one); about 315 + 4 * (max_depth - 1) bytes a row.  Not part of a checkpoint blob or of a snapshot row; freed by cw_destroy.
 * cw_reach: the start states are cw_expand's: hdr_in / slot_pos_in NULL: the engine's own records (n_states = num_envs), else the caller's, only read; env_of
 *   NULL: start row j belongs to env j % num_envs, else to env_of[j].  A start row whose entry is outside 0 .. num_envs - 1 takes no part: it reports -1 and is
 *   NOT counted in counters[7].  Needs a visited set (cw_seen_reserve) and a workspace with max_rows >= n_states and max_depth >= the one asked for.
 *   START: the set is CLEARED; the participating start rows are inserted with group = their row number -- two start rows are searched apart whatever they
 *     share -- and form frontier 0 in row order.
 *   LEVEL d = 1 .. max_depth over a frontier of F states: a successor row belongs to action a and parent j, in the order of a * F + j.  A successor whose
 *     reward is max_steps bids for its start row; the smallest such row wins and sets distance = d.  A solved start row leaves the search at once: in the same
 *     level its successors are not inserted.  A done successor is not inserted.  The rest go into the set with group = start row, and the fresh ones, in row
 *     order, are the next frontier.  More than max_rows (the workspace's) of them: searched_depth = d and every later level is a no-op.  At d = max_depth
 *     nothing is inserted.  An empty frontier ends the search with searched_depth = max_depth.
 *   With a set that neither overflows nor collides (cw_seen_counters) the outputs are a function of the inputs alone -- which of several equally short plans
 *     is returned included: the smallest solving row of the level, and behind it the smallest row of each key.  An overflow or a collision expands a state
 *     again: the distances stay exact while the frontier stays within max_rows.  The set is left filled: its keys are the states searched.
 * Enqueues the set's clear, 6 kernels for frontier 0, 7 per level (cw_reach_expand_kernel, cw_reach_claim_kernel, cw_reach_resolve_kernel, cw_reach_count_kernel,
 *   cw_reach_scan_kernel, cw_reach_scatter_kernel, cw_reach_settle_kernel; the last level: expand and settle) and cw_reach_walk_kernel, which follows the links
 *   back, one lane per start row.  Their launch shapes depend on the workspace's max_rows and the card alone; every kernel reads the frontier's size from the
 *   workspace, so a level over an empty or stopped frontier costs its launches and nothing else.  No lane or workgroup waits for another anywhere: a kernel
 *   boundary is the only grid-wide ordering.  No host synchronisation, no allocation.
 *   CW_ERR_STATE before the first cw_reset / cw_checkpoint_load, without a set, without a workspace, for n_states above its max_rows or max_depth above its
 *   max_depth.  CW_ERR_INVALID: a null engine or out, every field NULL, n_states < 0 or above the cap of max_rows, max_depth outside 1 .. 32 767, hdr_in without
 *   slot_pos_in or the reverse, env_of without them, n_states != num_envs without records, misaligned records (env_of, distance, frontier, searched_depth:
 *   4 bytes), an output overlapping the records, env_of or another output.  n_states == 0: frontier zeros, searched_depth = max_depth. */
typedef struct cw_reach_out {          /* DEVICE pointers; a NULL field is not written; all NULL: CW_ERR_INVALID */
    int32_t *distance;                 /* [n_states]  steps of a shortest plan that ends in success; -1: none within the searched depth, or no part */
    uint8_t *plan;                     /* [max_depth][n_states]  that plan, step-major like cw_simulate's actions; 0 behind its end and for -1 rows */
    uint8_t *first_action;             /* [n_states]  plan[0] */
    int32_t *frontier;                 /* [max_depth]  states expanded per level, 0 for levels not run */
    int32_t *searched_depth;           /* [1]  every plan of at most this many steps has been considered */
} cw_reach_out;
int cw_reach_reserve(cw_engine *e, int64_t max_rows, int32_t max_depth);
size_t cw_reach_bytes(const cw_engine *e);
int cw_reach(cw_engine *e, const int32_t *env_of, const uint8_t *hdr_in, const uint16_t *slot_pos_in, int32_t n_states, int32_t max_depth,
             const cw_reach_out *out, cw_stream_t stream);

/* --- packed records INTO envs: the other direction of the record family.  cw_expand, cw_simulate, cw_plan, cw_shoot, cw_seen_insert, cw_reach and
 * cw_render_records read records and write records; this call puts one back into an env, which then goes on stepping from it: an archive of 32-byte cells
 * ("return, then explore"), committing the chosen child of a tree search -- the terminal successor cw_expand exposes included --, starting episodes k steps
 * from the goal out of cw_reach's states, restarting from demonstration states.
 * hdr [R][16] and slot_pos [R][8], R = n_records: taken exactly as cw_expand takes records (device memory, 16-byte aligned, only read -- and not written by
 *   anyone while the call runs).  They must NOT overlap the engine's own hdr / slot_pos buffers (CW_ERR_INVALID): env i would be written while env j reads
 *   it; a caller who wants that clones them first.
 * src: DEVICE int32[num_envs], only read: env i takes record src[i].  A negative entry: env i takes no part.  An entry >= n_records is SKIPPED.  No entry
 *   becomes an address without that check (cw_host.h: cwh_load_record_index_ok).  Any number of envs may name the same record.  src == NULL: n_records must
 *   equal num_envs, and env i takes record i.
 * THE RULE (cw_host.h: cwh_record_ok, written once for the kernel and the host).  Unlike the pure calls, which only compare a record's cells, a loaded
 *   record becomes engine state: the dirty-cell painter turns the agent's cell into an address, the colour tables are indexed by code.  A record is loaded
 *   iff agent row < S and agent col < S; hold <= 3; every slot code <= 8; every slot is gone (0xFFFF) with code 0, or held (0xFFFE) with code == hold and
 *   hold != 0, or on the grid (position < S*S) with code != 0 -- any other position value or pairing fails --; exactly one slot is held if hold != 0 and
 *   none otherwise; the on-grid positions are pairwise different (one object per cell: what cw_export_grid can show).  Everything else in hdr is free: the
 *   masks, step_num, the flag word, the menu byte.  Every record cw_step, cw_expand, cw_simulate, cw_plan, cw_shoot or cw_reach produced from a state of the
 *   engine passes.  A REFUSED record is skipped like an index out of range.
 * status (or NULL): DEVICE uint8[num_envs], written once for EVERY env: 0 no part, 1 loaded, 2 index out of range, 3 record refused.  It must not overlap
 *   the records or src.
 * A LOADED env receives the record's hdr except byte 3 (it keeps its own menu id) and the record's slot_pos; cw_buffer_table.achieved / .desired take the
 *   record's masks, as after cw_snapshot_load; in the pixel modes its obs frame is repainted at once, held item included.
 *   NOT written: the episode's start and goal states and their two frames (init_obs, desired_goal), ep_no, the RNG stream, the look-ahead ring, the pool,
 *   reward, done, episode_length, episode_return, terminal_obs, counters[0..5] and counters[7].  A load is not a step and not a finished episode.
 * An env with status 2 or 3 is left exactly as it is and counted once in counters[6].
 * A RECORD DOES NOT HOLD ITS EPISODE: the env supplies the start positions (the Move tasks compare with them) and the goal state.  Loading a record that grew
 *   out of another episode is the caller's affair; it is legal after a with_stream == 0 fork (cw_snapshot_load), which gives envs one episode.  The record's
 *   desired mask is taken as it is: if it differs from the episode's, the goal state and frame stay the episode's -- cw_imagine_masked(commit) draws a
 *   matching goal.  A TERMINAL record may be loaded (step_num >= max_steps, or achieved == desired): the next step is then what the reference does with a
 *   finished env (ray.py:367) -- done again, and on auto_reset engines reset.
 * Enqueues ONE kernel (cw_load_records_kernel, dealt out like the snapshot kernels) on `stream` -- no host synchronisation, no allocation -- and can be
 *   captured into a HIP graph with cw_expand / cw_plan / cw_step.  Every obs_mode, with and without auto_reset, host_outputs engines included (the resident
 *   stepper is parked first; host_onehot is rewritten by the next cw_step_resident).  n_records == 0: CW_OK, nothing enqueued.  CW_ERR_STATE before the first
 *   cw_reset / cw_checkpoint_load.  CW_ERR_INVALID: a null engine, hdr or slot_pos, n_records < 0 or above 2^27, src == NULL with n_records != num_envs, a
 *   misaligned hdr / slot_pos (16 bytes) or src (4 bytes), the overlaps above.  (65 536 envs at 21x21: 20 us state-only, 0.33 ms with the dirty-cell frames repainted; 13 us for 219 selected envs:
 *   tools/measure_load_records.py, profiles/r13_load_records.txt.) */
int cw_load_records(cw_engine *e, const int32_t *src, const uint8_t *hdr, const uint16_t *slot_pos, int32_t n_records, uint8_t *status, cw_stream_t stream);

/* --- the learner's side of the record family: a device-resident REPLAY BUFFER of transitions kept as packed records, and minibatches drawn from it with
 * hindsight relabelling (HER), without a host round trip.  A transition is (s, s', the episode's goal) as three 32-byte records plus action, flags, reward and
 * an episode number: 106 bytes, where the three frames of a 21x21 pixel transition are 63 KB; cw_render_records paints the frames of a minibatch when it is drawn.
 * Everything below is exact integer arithmetic and a function of the inputs alone, never of scheduling.  cw_replay_push is called BEFORE cw_step with the same
 * actions; cw_step_many and cw_rollout are NOT recorded (out of scope).
 *
 * THE BUFFER: L = steps slots of N = num_envs transitions, time-major [L][N] (slot t of env i at index t * N + i).  Per slot and env: hdr [16] / slot_pos [8] (the
 *   state s), next_hdr / next_slot_pos (the successor s'), goal_hdr / goal_slot_pos (the goal record), action uint8, flags uint8 (bit 0 changed, bit 1 done),
 *   reward int32, episode uint32.  A control block holds uint64 n, the pushes since the last clear, and per env the episode number of its newest transition.
 *   POSITION k = 0, 1, ... is the k-th push since the last clear; it lives in slot k % L; positions lo .. n - 1 are stored, lo = max(0, n - L).
 * cw_replay_reserve: ONE allocation of cw_replay_bytes() bytes, made as cw_seen_reserve and cw_snapshot_reserve make theirs; synchronous, waits for this engine's own
 *   work only.  The new buffer is zero-filled and cleared (n = 0) before the call returns; steps == 0 frees it; CW_ERR_HIP leaves the engine WITHOUT a buffer.  Freed
 *   by cw_destroy.  Not part of a checkpoint blob or a snapshot row; left alone by cw_reset, cw_checkpoint_load and cw_seed_*.  CW_ERR_INVALID: a null engine, steps
 *   outside 0 .. 2^24, steps * num_envs >= 2^31.  Offsets are 64-bit throughout.
 * cw_replay_buffers: the device arrays, zero-copy, READ-ONLY for callers and valid until the next cw_replay_reserve; CW_ERR_STATE without a buffer.
 * cw_replay_clear: n = 0 and every env's episode number 0 (ONE kernel, capturable); the slots' bytes stay and are unreachable.  CW_ERR_STATE before the first
 *   cw_reset / cw_checkpoint_load and without a buffer.
 *
 * cw_replay_push: one lane per env i (cw_replay_push_kernel).  actions and action_dtype exactly as cw_step takes them, host_actions of a host_outputs engine included.
 *   s = the env's current hdr / slot_pos.  (s', reward, done, changed) = the pure step of s under the action exactly as cw_expand computes it, with the env's own
 *   start positions.  An action id outside 0..5 is cw_step's state-preserving no-op (step_num += 1, reward -1, changed 0); it is stored as 255 and NOT counted
 *   anywhere.  The transition is written to slot n % L.
 *   THE GOAL RECORD of env i: bytes 0-1 the row and column of the goal state's agent cell, byte 2 (hold) 0, byte 3 the env's menu id, bytes 4-5 (achieved) =
 *   bytes 6-7 (desired) = the env's desired mask, bytes 8-11 (step_num, flags) 0, bytes 12-15 the goal state's slot codes; goal_slot_pos the goal state's slot
 *   positions.  Its cw_render_records frame is the env's desired_goal frame.
 *   PURE with respect to the engine: nothing but the buffer is written -- no state, stream, look-ahead ring, counter (counters[3] included), output array or frame.
 *   THE EPISODE RULE is a function of what was pushed, with no hook into any reset, load or restore call.  The transition of push k for env i CONTINUES the episode
 *   of push k - 1 iff that transition was not done AND its next_hdr / next_slot_pos equal this push's hdr / slot_pos in all 32 bytes; otherwise the env's episode
 *   number goes up by one.  The first push after a clear starts episode 0.  The predecessor is read before the slot is written, so steps == 1 is legal.
 *   Consequences: an auto-reset, cw_reset_masked, cw_load_records, cw_snapshot_load or cw_imagine_masked(commit) between two pushes starts a new episode, because
 *   the bytes differ (a load of the very bytes s' continues it); on an engine without auto-reset a finished env that keeps stepping yields episodes of length 1.
 *   Episode numbers never decrease along an env's positions; they are uint32 and only ever compared for equality.
 *   n lives on the device and advances there AFTER the push's stores, by a kernel boundary (a second, one-lane launch) -- never by a lane or workgroup waiting for
 *   another -- so a replayed graph pushes into the next slot each time.  Enqueues TWO kernels; no host synchronisation, no allocation; capturable with cw_step.
 *   CW_ERR_STATE before the first cw_reset / cw_checkpoint_load and without a buffer; otherwise the argument rules of cw_step (CW_ERR_INVALID: a null engine or
 *   actions, a bad dtype).
 *
 * cw_replay_sample: B = n_rows rows, one minibatch (cw_replay_sample_kernel: one lane per row, grid-stride).  s = seed + (seed_dev ? *seed_dev : 0) mod 2^64, as
 *   cw_shoot; draw and mulhi32 are THE DRAW of cw_shoot, draw(s, state, sample, step).  The kernel reads n from the device, so the call is capturable.
 *   lo = max(0, n - L), V = n - lo.  For n == 0 NO row is written.  For row b:
 *     env       i = mulhi32(draw(s, b, 0, 0), N);
 *     position  p = lo + mulhi32(draw(s, b, 1, 0), V)      -- together uniform over the stored transitions;
 *     the row is RELABELLED iff (draw(s, b, 2, 0) >> 16) < her; her is 0 .. 65 536: 0 never, 65 536 always;
 *     e = the last position in [p, n) whose stored episode number for env i equals that of p (a binary search, at most 24 loads, no back-pointers);
 *     strategy 0 (future): f = p + mulhi32(draw(s, b, 3, 0), e - p + 1);  strategy 1 (final): f = e;
 *     the relabelled goal g = the achieved mask of the stored next_hdr at (f, i), bytes 4-5.
 *   Outputs (cw_replay_out; DEVICE pointers [B]; a NULL field is not written, all NULL is CW_ERR_INVALID; the record fields 16-byte, reward / env / slot / future
 *   4-byte, desired 2-byte aligned; no output may overlap another):
 *     hdr, slot_pos            the stored s at (p, i); in a relabelled row bytes 6-7 of hdr are g.
 *     next_hdr, next_slot_pos  the stored s'; the same rule for bytes 6-7.
 *     goal_hdr, goal_slot_pos  not relabelled: the stored goal record.  Relabelled: the stored s' record at (f, i) with bytes 6-7 = g.  Its achieved equals its
 *                              desired equals the row's `desired` in both cases; its frame is the achieved-goal image HER uses.
 *     action                   the stored action (255: outside 0..5).
 *     reward, done             not relabelled: as stored.  Relabelled: reward = -1 unless the stored changed bit is set; if it is set, reward = max_steps iff the
 *                              reward rule holds of a' = the achieved mask of the stored s' (bytes 4-5) and g under the engine's task mask, the rule named by bit 1
 *                              of the stored s' record's flag word (byte 10): clear, EQUAL: a' == g; set, SUBSET: (g & ~a') == 0 and some position equal, i.e.
 *                              (~(g ^ a') & task mask) != 0 -- cw_step's own expressions.  done = (step_num of the stored s', bytes 8-9, >= max_steps) or
 *                              reward == max_steps.
 *     desired                  g, or the stored mask (bytes 6-7 of the stored hdr).
 *     env, slot, future        i, p % L, and f % L (-1 when not relabelled): with these a caller gathers side data of its own kept in [L][N] tensors.
 *   Every other byte of the records is the stored one: the success count in flag bits 2-15 stays the episode's AS PLAYED, step_num and the slot data likewise.
 *   PURE: reads the buffer, writes the outputs, nothing else.  ONE kernel, no atomics, no host synchronisation, no allocation; every obs_mode, host_outputs engines
 *   included.  n_rows == 0: CW_OK, nothing enqueued.  CW_ERR_INVALID, tested in this order: a null engine or out; n_rows < 0 or above 2^27; her above 65 536; a
 *   strategy other than 0 or 1; every field NULL; a misaligned field; two fields sharing a byte.  Then CW_ERR_STATE before the first cw_reset / cw_checkpoint_load
 *   and without a buffer.
 *   (21x21, L = 256, launch included, 4 096 / 65 536 envs: a push 14 / 14 us beside 9 / 10 us for the state-only cw_step it precedes; a sample at her = 52 429 of
 *   4 096 rows 21 us and of 65 536 rows 30 - 34 us, against 620 - 640 us for the same minibatch assembled in torch from the table (randint, index gathers, the
 *   episode end from the episode column, compute_reward_batch); with three cw_render_records calls 75 us against 0.71 ms and 0.83 - 0.85 against 1.46 ms: no shape
 *   measured is slower than the torch route.  tools/measure_replay.py, profiles/r15_replay.txt.) */
typedef struct cw_replay_table {   /* DEVICE pointers into the buffer, [steps][num_envs] unless noted */
    const uint8_t  *hdr;            /* [..][16] */
    const uint16_t *slot_pos;       /* [..][8]  */
    const uint8_t  *next_hdr;
    const uint16_t *next_slot_pos;
    const uint8_t  *goal_hdr;
    const uint16_t *goal_slot_pos;
    const uint8_t  *action;
    const uint8_t  *flags;
    const int32_t  *reward;
    const uint32_t *episode;
    const uint32_t *env_episode;    /* [num_envs] the episode number of each env's newest transition */
    const uint64_t *n;              /* [1] the pushes since the last clear */
    int32_t steps;
    int32_t num_envs;
} cw_replay_table;
typedef struct cw_replay_out {     /* DEVICE pointers [B]; a NULL field is not written; all NULL: CW_ERR_INVALID */
    uint8_t  *hdr;                  /* [B][16], 16-byte aligned like the five record fields below */
    uint16_t *slot_pos;             /* [B][8] */
    uint8_t  *next_hdr;
    uint16_t *next_slot_pos;
    uint8_t  *goal_hdr;
    uint16_t *goal_slot_pos;
    uint8_t  *action;
    int32_t  *reward;
    uint8_t  *done;
    uint16_t *desired;
    int32_t  *env;
    int32_t  *slot;
    int32_t  *future;
} cw_replay_out;
int cw_replay_reserve(cw_engine *e, int32_t steps);
size_t cw_replay_bytes(const cw_engine *e);                      /* 0 without a buffer */
int cw_replay_buffers(cw_engine *e, cw_replay_table *out);
int cw_replay_clear(cw_engine *e, cw_stream_t stream);
int cw_replay_push(cw_engine *e, const void *actions, int action_dtype, cw_stream_t stream);
int cw_replay_sample(cw_engine *e, int32_t n_rows, uint64_t seed, const uint64_t *seed_dev, uint32_t her, int32_t strategy,
                     const cw_replay_out *out, cw_stream_t stream);

/* --- step(action) for every env (ray.py:301-378) + auto-reset of finished envs --------------
 * actions: DEVICE pointer to N actions of dtype CW_ACT_*, values 0..5 = Up,Right,Down,Left,
 * PickUp,Drop (ACTIONS, ray.py:130-131).  Out-of-range values of any dtype (an int64 beyond the int range included) are counted in
 * counters[3] and executed as a state-preserving step (step_num += 1, reward -1).  Enqueues the step kernel -- engines with auto_reset: finished envs take
 * over the record of their next episode, computed ahead of time by a refill kernel that rides on every max_steps/4-th call (8 ... 64; fewer steps apart while
 * envs finish faster than that: the period follows the count of slow resets the card reports, never waited for); every env keeps a queue of four such records,
 * and one that finishes a fifth time between two refills is reset on the spot -- and, in CW_OBS_PIXELS_FULL, the sweep that paints the observation array.
 * With cw_config.host_outputs `actions` may be cw_buffer_table.host_actions. */
int cw_step(cw_engine *e, const void *actions, int action_dtype, cw_stream_t stream);

/* --- n_steps consecutive step()s from a DEVICE action array [n_steps][N] (dtype as cw_step): exactly what n_steps calls of cw_step enqueue,
 * in one call (a host loop in Python costs more per call than a state-only step takes on the card).  The frames and outputs left behind are
 * the last step's.  Capturable into a HIP graph as one piece (a replay re-reads the action array: refill it in place between replays).
 * A captured sequence carries ONE look-ahead refill at its head (plus the regular one every max_steps/4 steps inside it): a replayed graph must
 * refill by itself.  That launch costs ~15 us whatever it finds to do -- capture sequences of a refill period or more (a graph of a single
 * cw_step pays it on every replay: three times a 5-us state-only step).  An env that finds no record is reset on the spot and rejoins the list,
 * so a graph replayed after a re-seed has its records back after one episode. */
int cw_step_many(cw_engine *e, const void *actions, int action_dtype, int32_t n_steps, cw_stream_t stream);

/* --- n_steps consecutive step()s (+ auto-reset) for every env in ONE persistent kernel launch --
 * For scripted / random action streams known up front (BASELINE config 2 style): actions is a DEVICE
 * array [n_steps][N] of uint8 action ids; rewards [n_steps][N] int32 and dones [n_steps][N] uint8 are
 * DEVICE arrays or NULL.  The result (state, RNG streams, counters, the reward/done/achieved buffers of
 * the last step) is bit-identical to n_steps calls of cw_step.  CW_OBS_STATE engines with auto_reset
 * only: no frames are painted (use cw_render afterwards).  A call longer than max_steps steps is issued as several launches of max_steps steps
 * (64 at least) with a look-ahead refill ahead of each, in stream order: every env's time-out then finds its next episode's record waiting. */
int cw_rollout(cw_engine *e, const uint8_t *actions, int32_t n_steps, int32_t *rewards, uint8_t *dones,
               cw_stream_t stream);

/* step(action) of the SINGLE-ENV loop without a kernel launch (ray.py:301-378 called from host code, docs/source/envs/gen_info.rst:62-82).
 * For engines with num_envs == 1, host_outputs, auto_reset == 0 and obs_mode CW_OBS_STATE or CW_OBS_PIXELS_DIRTY: a resident
 * single-wavefront kernel polls a doorbell word in pinned host memory; this call rings it and spins until the step's outputs (reward, done,
 * masks, the <= 2 repainted cells of the host-mapped frame) are visible -- a few microseconds instead of a launch plus a stream
 * synchronisation.  Results are those of cw_step with the same action (0..127; larger ids than 5 are the counted no-op of cw_step).  The kernel is started on demand and leaves by itself: after 0.5 ms
 * without a request, after a 200-ms time slice, or when any other entry point of this engine is called (they park it first; cw_resident_stop
 * does only that).  Synchronous.  A new instance of the kernel waits for the stream of the engine's last cw_reset / cw_step / cw_rollout first, so
 * `cw_reset(e, s); cw_step_resident(e, a, 0);` needs no synchronisation in between. */
int cw_step_resident(cw_engine *e, int32_t action, int32_t want_onehot /* 1: also rewrite cw_buffer_table.host_onehot */);
int cw_resident_stop(cw_engine *e);

/* render(state=None) for every env into a caller-supplied DEVICE buffer [N][P][P][3] (works in
 * every obs_mode; ray.py:442-520).  Any pointer the rasteriser's stores accept (Ray: 4-byte aligned); a 16-byte
 * aligned one is painted by the fastest kernel. */
int cw_render(cw_engine *e, uint8_t *out_frames, cw_stream_t stream);

/* render(state) (ray.py:442-486) for caller-supplied one-hot states of ANY content: onehot is a DEVICE array [n_states][S][S][12]
 * uint8 (S = the engine's size), out_frames a DEVICE array [n_states][4S][4S][3] uint16 -- the reference's image is the SUM of the
 * colours of the objects in a cell (int; up to 8 x 255), the agent is the first cell (row-major) with channel 8 set and must exist,
 * the held item's colour comes from the largest hold channel set anywhere.  Does not touch the engine's own state.
 * Engines with CW_RASTER_ALT render CraftingWorldEnvAltObs.render(state) instead (craftingworld_altobs.py:489-560): out_frames is
 * [n_states][3S+3][3S][3] uint16, pixel k of a cell's tile = CPV_COLORS[k] x (channel k + hold channel 9+k for k < 3), the strip's
 * pixels 3..5 are 255 if any cell has a hold channel set. */
int cw_render_onehot(cw_engine *e, const uint8_t *onehot, int32_t n_states, uint16_t *out_frames, cw_stream_t stream);

/* Dense state views written to caller-supplied DEVICE buffers (observation_vector_space,
 * ray.py:94-110): cw_export_grid -> [N][S][S] uint8 codes; cw_export_onehot -> [N][S][S][12]
 * uint8 0/1 (channels 0-7 objects, 8 agent, 9-11 held item at the agent cell). */
int cw_export_grid(cw_engine *e, uint8_t *out, cw_stream_t stream);
int cw_export_onehot(cw_engine *e, uint8_t *out, cw_stream_t stream);
/* The same one-hot view of the episode's other two states -- what CraftingWorldEnvOneHot returns as desired_goal
 * (imagine_obs' final state, carftingworld_onehot.py:310) and init_observation (the state at reset, :203). */
enum { CW_STATE_CURRENT = 0, CW_STATE_GOAL = 1, CW_STATE_INIT = 2 };
int cw_export_onehot_of(cw_engine *e, int which, uint8_t *out, cw_stream_t stream);

/* --- state injection / checkpoint (synchronous; SURVEY §5 "checkpoint / resume") ------------ */
int cw_get_state(cw_engine *e, cw_state_view *host);
int cw_set_state(cw_engine *e, const cw_state_view *host);

/* --- checkpoint / resume of the whole batch as one opaque host blob (the reference has none: its de-facto
 * state is the attribute set of ray.py:119-141).  The blob holds the engine's raw records -- current state, the
 * episode's goal and start states, every env's RNG stream, the fixed_init_state pool, the last step's outputs, the
 * counters -- and is restored verbatim, so a resumed engine continues bit-identically, state tensors included.
 * cw_checkpoint_load needs an engine created with the same num_envs, size, max_steps, len(task_list),
 * fixed_init_state and task menus (verified; CW_ERR_INVALID otherwise); it repaints the frames in the pixel modes and
 * needs no cw_reset first.  Synchronous host calls. */
size_t cw_checkpoint_bytes(cw_engine *e);
int cw_checkpoint_save(cw_engine *e, void *buf, size_t capacity);
int cw_checkpoint_load(cw_engine *e, const void *buf, size_t length);

/* --- per-kernel timing with HIP events on the caller's stream (bench.py's roofline leg) -----
 * cw_profile_begin: from now on cw_step brackets its kernels with hipEventRecord on the stream it launches on (at most max_steps
 * steps are kept).  cw_profile_end: synchronises the events, returns durations in milliseconds and stops recording.
 * What is bracketed: in CW_OBS_PIXELS_FULL only the sweep of the observation array (cw_render_pieces_kernel; all chunk launches of a large
 * batch together) -- every event record costs the stream a pipeline bubble, and the step kernel in front of the sweep is short; in the
 * other two modes the step kernel (cw_step_fused_kernel / cw_step_kernel), which is the whole step there.  The look-ahead refill
 * (cw_refill_kernel, every max_steps/4-th step) is never bracketed. */
typedef struct cw_profile {
    int32_t steps;           /* cw_step calls recorded */
    float ms_step_kernel;    /* average per launch; 0 in CW_OBS_PIXELS_FULL (not bracketed there) */
    float ms_reset_kernel;   /* always 0 since ABI 4: no reset kernel runs inside a step (finished envs take look-ahead records in the step kernel) */
    float ms_render_kernel;  /* the sweep, average per step; 0 in CW_OBS_STATE and CW_OBS_PIXELS_DIRTY */
    float ms_render_kernel_max;
    float ms_render_kernel_min;
    float ms_render_kernel_median;
} cw_profile;
int cw_profile_begin(cw_engine *e, int max_steps);
int cw_profile_end(cw_engine *e, cw_profile *out);
/* Name of the kernel that paints this engine's frames, as a rocprofv3 kernel trace of the same run lists it (without template arguments):
 * CW_OBS_PIXELS_FULL: "cw_render_pieces_kernel" -- the one painter of whole frame arrays, a clocked sweep of aligned 4-KiB pieces; a trace
 * shows cw_render_pieces_kernel<raster, frames per job> (<0, 2> for Ray frames of 4 KiB and more, <1, 2> AltObs; 4 / 8 / 16 frames per job for
 * smaller frames) -- or "cw_render_gather_kernel" for the smallest Ray frames (grids up to 7x7; <4> / <8> frames per piece in a trace), where
 * every lane computes its own 16-byte chunks; this is what ms_render_kernel brackets.  CW_OBS_PIXELS_DIRTY: the step kernel itself, which repaints the <= 2 changed cells
 * ("cw_step_fused_kernel" with auto_reset, else "cw_step_kernel").  CW_OBS_STATE: "" (nothing is painted).  A static string. */
const char *cw_render_kernel_name(const cw_engine *e);

/* What the engine's tuning holds (full-frame mode): the period of the sweep's clock -- a wave starts a 4-KiB piece every
 * period16 / 16 ticks of the 100-MHz clock, 0: unclocked; period16_head: the period of a launch's first 64 jobs, period16_busy: of those after a
 * step on which envs finished --, and whether the engine
 * keeps look-ahead records (cw_config.auto_reset, device-resident outputs); `resident`: 1 if cw_step_resident can be used on this engine;
 * guard_slowdowns: how often the clock's guard has lowered the rate because sweeps stopped keeping their schedule (-1: no guard; the guard also
 * probes one notch UP when the best rate known has held for ~4 000 steps and keeps it if the sweeps get shorter: period16 may fall below cw_create's).
 * Only performance depends on any of it. */
typedef struct cw_tuner_state {
    int32_t period16, period16_head, period16_busy, lookahead, resident, guard_slowdowns;
} cw_tuner_state;
int cw_tuner(const cw_engine *e, cw_tuner_state *out);

int cw_buffers(cw_engine *e, cw_buffer_table *out);
/* Blocks the calling thread until everything enqueued on `stream` has finished (hipStreamSynchronize): the one host
 * synchronisation of the single-env loop, where step() returns Python scalars (ray.py:376-378). */
int cw_synchronize(cw_engine *e, cw_stream_t stream);
int cw_num_envs(const cw_engine *e);
int cw_abi_version(void);
const char *cw_last_error(void);   /* thread-local text of the last failing call */

#ifdef __cplusplus
}
#endif
#endif
