"""CraftingWorldVecEnv -- N CraftingWorld envs stepped by hand-written HIP kernels on one MI355X.

Mirrors the reference's CraftingWorldEnvRay (gym_craftingworld/envs/craftingworld_ray.py,
"ray.py") batched the gym.vector.VectorEnv way: same ctor kwargs (ray.py:59-60), same action
ids (ray.py:130-131), same rewards/done rule (ray.py:361-367), same four-image Dict observation
(ray.py:194-196), auto-reset of finished envs.  All compute happens in libcraftingworld.so
(include/craftingworld.h); this file is host plumbing: config marshalling, torch views of the
engine's device buffers, stream hand-off.  There is no CPU fallback.
"""
import atexit
import ctypes as C
import sys
import weakref

import numpy as np
import torch

from . import _lib as L
from . import seeding
from ._wrap import tensor_view
from .spaces import Box, Dict, Discrete, MultiDiscrete, batch_space

TASK_LIST = ['MakeBread', 'EatBread', 'BuildHouse', 'ChopTree', 'ChopRock', 'GoToHouse', 'MoveAxe',
             'MoveHammer', 'MoveSticks']                       # ray.py:40-41
OBJECTS = ['sticks', 'axe', 'hammer', 'rock', 'tree', 'bread', 'house', 'wheat']   # ray.py:21
PICKUPABLE = ['sticks', 'axe', 'hammer']                       # ray.py:20
ACTION_NAMES = ['up', 'right', 'down', 'left', 'pickup', 'drop']   # ray.py:130-131
UP, RIGHT, DOWN, LEFT, PICKUP, DROP = range(6)                  # action ids (ray.py:15-18 names the four moves; 4 / 5 are pickup / drop, ray.py:130-131)
# the palette (ray.py:26-31), as data for callers that decode frames: an object's 4x4 tile, the same with index 0 = the empty floor, and what the
# reference SUBTRACTS from the agent's white centre for a held item (255 - its colour).  The kernels carry their own copy (csrc/cw_kernels.hip).
COLORS = [(110, 69, 39), (255, 105, 180), (100, 100, 200), (100, 100, 100), (0, 128, 0), (205, 133, 63), (197, 91, 97), (240, 230, 140)]
COLORS_N = [(0, 0, 0)] + COLORS
COLORS_H = [tuple(255 - c for c in COLORS[k]) for k in range(3)]
STATE_W = STATE_H = 21                                         # ray.py:43-44: the default grid
MAX_STEPS = 300                                                # ray.py:46

_OBS_MODES = {'state': L.CW_OBS_STATE, 'pixels': L.CW_OBS_PIXELS_FULL, 'pixels_dirty': L.CW_OBS_PIXELS_DIRTY}
_ACT_DTYPES = {torch.int32: L.CW_ACT_I32, torch.int64: L.CW_ACT_I64, torch.uint8: L.CW_ACT_U8}


def _menu_struct(task_list, selected_tasks, number_of_tasks, stacking, reward_style):
    m = L.cw_task_menu()
    selected_tasks = list(selected_tasks)
    if not 1 <= len(selected_tasks) <= L.CW_MAX_TASKS:
        raise ValueError('selected_tasks must hold 1..%d tasks' % L.CW_MAX_TASKS)
    m.n_selected = len(selected_tasks)
    n = number_of_tasks if number_of_tasks is not None else len(selected_tasks)      # ray.py:79
    m.number_of_tasks = min(int(n), len(selected_tasks))                             # ray.py:80-81
    if m.number_of_tasks < 1:
        raise ValueError('number_of_tasks must be >= 1')
    m.stacking = 1 if stacking is True else 0                                        # `is True`, ray.py:169
    m.reward_subset = 0 if reward_style is None else 1                               # ray.py:71-74
    tl = list(task_list)
    for i, t in enumerate(selected_tasks):
        m.selected_bits[i] = tl.index(t)                                             # ValueError like ray.py:174
    return m


_NP_OF = {torch.uint8: np.uint8, torch.int8: np.int8, torch.int16: np.int16, torch.int32: np.int32, torch.int64: np.int64, torch.bool: np.bool_}


def as_numpy(a):
    """a tensor (wherever it lives), an array or a list as a numpy array on the host; None stays None"""
    if a is None:
        return None
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _shape_dtype(a):
    """(shape, numpy dtype) of a tensor or an array: what the validators below take in place of the data"""
    return tuple(a.shape), _NP_OF.get(a.dtype, np.float64) if torch.is_tensor(a) else a.dtype


def _vp(t):
    """a tensor's address as the library takes it; None -> NULL"""
    return None if t is None else C.c_void_p(t.data_ptr())


def _out_struct(cls, out):
    """cw_expand_out / cw_simulate_out over the tensors of an out dict ('achieved_mask' is the structs' `achieved`); a field not asked for stays NULL"""
    return cls(**{'achieved' if f == 'achieved_mask' else f: t.data_ptr() for f, t in out.items()})


def _host_view(ptr, shape, dtype):
    """CPU tensor over engine-owned pinned host memory (cw_config.host_outputs); None for a NULL pointer."""
    if not ptr:
        return None
    npdt = np.dtype(_NP_OF[dtype])
    nbytes = int(np.prod(shape)) * npdt.itemsize
    arr = np.frombuffer((C.c_uint8 * nbytes).from_address(int(ptr)), dtype=npdt).reshape(shape)
    return torch.from_numpy(arr)


def reset_mask(num_envs, mask=None, indices=None):
    """The byte mask cw_reset_masked takes, built and validated on the host: -> np.uint8 [num_envs], 1 = reset that env.  Exactly one of
    `mask` (a bool / integer array of shape [num_envs], non-zero = reset) and `indices` (env ids in -num_envs .. num_envs - 1, duplicates allowed,
    an empty list selects nothing).  ValueError for a wrong shape or both / neither argument, IndexError for an index outside the batch."""
    num_envs = int(num_envs)
    if (mask is None) == (indices is None):
        raise ValueError('give exactly one of mask and indices')
    if mask is not None:
        m = np.asarray(mask)
        if m.shape != (num_envs,):
            raise ValueError('mask must have shape (%d,), got %s' % (num_envs, m.shape))
        if m.dtype != np.bool_ and not np.issubdtype(m.dtype, np.integer):
            raise ValueError('mask must be a bool or integer array, got %s' % m.dtype)
        return np.ascontiguousarray(m != 0, dtype=np.uint8)
    idx = np.asarray(indices)
    if idx.size == 0:
        return np.zeros(num_envs, dtype=np.uint8)
    if idx.ndim > 1 or not np.issubdtype(idx.dtype, np.integer):
        raise ValueError('indices must be a flat list of integer env ids')
    idx = idx.reshape(-1).astype(np.int64)
    bad = idx[(idx < -num_envs) | (idx >= num_envs)]
    if bad.size:
        raise IndexError('env index %d outside a batch of %d envs' % (int(bad[0]), num_envs))
    out = np.zeros(num_envs, dtype=np.uint8)
    out[idx] = 1
    return out


def desired_bits(num_envs, desired, n_tasks):
    """The uint16 task masks cw_imagine_masked takes, built and validated on the host: -> np.uint16 [num_envs], bit t = task_list[t].  `desired` is either
    those masks already (an integer array [num_envs], every value below 1 << n_tasks) or the reference's desired_goal_vector layout, one 0/1 row per
    env: [num_envs, n_tasks] (a single row [1, n_tasks] or [n_tasks] is taken for a batch of one).  ValueError for any other shape, dtype or value."""
    num_envs, n_tasks = int(num_envs), int(n_tasks)
    d = np.asarray(desired)
    if d.dtype != np.bool_ and not np.issubdtype(d.dtype, np.integer):
        raise ValueError('desired must be a bool or integer array, got %s' % d.dtype)
    if d.shape == (num_envs,) and not (num_envs == n_tasks == 1 and d.dtype == np.bool_):
        d = d.astype(np.int64)
        if ((d < 0) | (d >= (1 << n_tasks))).any():
            raise ValueError('a desired mask outside 0 .. %d (%d tasks)' % ((1 << n_tasks) - 1, n_tasks))
        return np.ascontiguousarray(d, dtype=np.uint16)
    if num_envs == 1 and d.shape == (n_tasks,):
        d = d.reshape(1, n_tasks)
    if d.shape != (num_envs, n_tasks):
        raise ValueError('desired must have shape (%d,) or (%d, %d), got %s' % (num_envs, num_envs, n_tasks, d.shape))
    d = d.astype(np.int64)
    if ((d != 0) & (d != 1)).any():
        raise ValueError('a desired vector holds 0 and 1 only')
    return np.ascontiguousarray((d << np.arange(n_tasks, dtype=np.int64)).sum(axis=1), dtype=np.uint16)


def snapshot_rows(num_envs, capacity, rows, envs=None, fork=False):
    """The row numbers cw_snapshot_save / cw_snapshot_load take, built and validated on the host: -> np.int32 [num_envs], entry i = the bank row of env i,
    -1 = env i takes no part.  `rows` alone: one entry per env (length num_envs; a negative entry = no part).  With `envs`: envs[j] is paired with
    rows[j] (env ids in -num_envs .. num_envs - 1), every env not listed takes no part.  ValueError for lengths that differ, an env listed twice, a row
    at or above `capacity`, anything that is not a flat integer list and -- unless fork=True (a load: many envs may continue from one row) -- a row listed
    twice; IndexError for an env outside the batch."""
    num_envs, capacity = int(num_envs), int(capacity)
    if rows is None:
        raise ValueError('give rows (one per env), or envs and rows')
    r = np.asarray(rows)
    if r.ndim != 1 or (r.size and not np.issubdtype(r.dtype, np.integer)):
        raise ValueError('rows must be a flat list of integer row numbers')
    r = r.astype(np.int64)
    if envs is None:
        if len(r) != num_envs:
            raise ValueError('rows must hold one entry per env (%d), got %d' % (num_envs, len(r)))
        out = np.where(r < 0, -1, r)
    else:
        e = np.asarray(envs)
        if e.ndim != 1 or (e.size and not np.issubdtype(e.dtype, np.integer)):
            raise ValueError('envs must be a flat list of integer env ids')
        e = e.astype(np.int64)
        if len(e) != len(r):
            raise ValueError('%d envs but %d rows' % (len(e), len(r)))
        bad = e[(e < -num_envs) | (e >= num_envs)]
        if bad.size:
            raise IndexError('env index %d outside a batch of %d envs' % (int(bad[0]), num_envs))
        e = np.where(e < 0, e + num_envs, e)
        if len(np.unique(e)) != len(e):
            raise ValueError('an env is listed twice')
        out = np.full(num_envs, -1, np.int64)
        out[e] = np.where(r < 0, -1, r)
    used = out[out >= 0]
    if used.size and used.max() >= capacity:
        raise ValueError('row %d is outside a bank of %d rows' % (int(used.max()), capacity))
    if not fork and len(np.unique(used)) != len(used):
        raise ValueError('a row is listed twice: two envs cannot be saved into one row')
    return np.ascontiguousarray(out, dtype=np.int32)


LOAD_NO_PART, LOAD_LOADED, LOAD_BAD_INDEX, LOAD_REFUSED = range(4)     # the status bytes of load_records(status=True)


def load_records_src(num_envs, n_records, src=None, envs=None):
    """The record indices cw_load_records takes, built and validated on the host: -> np.int32 [num_envs], entry i = the record env i takes, -1 = env i takes
    no part.  Neither `src` nor `envs`: record i for env i (n_records must be num_envs).  `src` alone: one entry per env (a negative entry = no part).  With
    `envs`: envs[j] is paired with src[j] (env ids in -num_envs .. num_envs - 1; src None: with record j), every env not listed takes no part; any number
    of envs may name one record.  ValueError for lengths that differ, an env listed twice, anything that is not a flat integer list; IndexError for an env
    outside the batch or an index outside the records."""
    num_envs, n_records = int(num_envs), int(n_records)
    if src is None:
        r = np.arange(n_records if envs is None else len(np.asarray(envs).reshape(-1)), dtype=np.int64)
    else:
        r = np.asarray(src)
        if r.ndim != 1 or (r.size and (r.dtype == np.bool_ or not np.issubdtype(r.dtype, np.integer))):
            raise ValueError('src must be a flat list of integer record indices')
        r = r.astype(np.int64)
    if envs is None:
        if len(r) != num_envs:
            raise ValueError('%s must hold one entry per env (%d), got %d' % ('the records' if src is None else 'src', num_envs, len(r)))
        out = np.where(r < 0, -1, r)
    else:
        e = np.asarray(envs)
        if e.ndim != 1 or (e.size and not np.issubdtype(e.dtype, np.integer)):
            raise ValueError('envs must be a flat list of integer env ids')
        e = e.astype(np.int64)
        if len(e) != len(r):
            raise ValueError('%d envs but %d record indices' % (len(e), len(r)))
        bad = e[(e < -num_envs) | (e >= num_envs)]
        if bad.size:
            raise IndexError('env index %d outside a batch of %d envs' % (int(bad[0]), num_envs))
        e = np.where(e < 0, e + num_envs, e)
        if len(np.unique(e)) != len(e):
            raise ValueError('an env is listed twice')
        out = np.full(num_envs, -1, np.int64)
        out[e] = np.where(r < 0, -1, r)
    if out.size and out.max() >= n_records:
        raise IndexError('record index %d outside %d records' % (int(out[out >= n_records][0]), n_records))
    return np.ascontiguousarray(out, dtype=np.int32)


def load_records_args(num_envs, size, hdr, slot_pos, src=None, envs=None, record_ok=None):
    """What cw_load_records is handed, validated and packed on the host (numpy inputs): -> (hdr uint8 [R, 16], slot_pos uint16 [R, 8], src int32 [num_envs]),
    all contiguous.  hdr uint8 [..., 16] and slot_pos int16 / uint16 [..., 8] under expand_args' rules (both required, flattened to R records); src / envs
    as load_records_src takes them.  Every record some env takes is put to THE RULE the kernel applies -- record_ok(size, hdr16, slot_pos8) -> bool, by
    default the library's own cwh_record_ok_of (include/craftingworld.h states the rule) -- and ValueError names the first one that fails it."""
    if hdr is None or slot_pos is None:
        raise ValueError('load_records needs hdr and slot_pos')
    hdr, slot_pos = np.asarray(hdr), np.asarray(slot_pos)
    r = _expand_m(1, (hdr.shape, hdr.dtype), (slot_pos.shape, slot_pos.dtype), None)
    idx = load_records_src(num_envs, r, src, envs)
    hdr = np.ascontiguousarray(hdr).reshape(r, 16)
    slot_pos = np.ascontiguousarray(slot_pos).reshape(r, 8).view(np.uint16)
    if record_ok is None:
        lib = L.load()
        record_ok = lambda s, h, p: lib.cwh_record_ok_of(s, h.ctypes.data, p.ctypes.data) != 0  # noqa: E731
    for j in np.unique(idx[idx >= 0]).tolist():
        if not record_ok(int(size), hdr[j], slot_pos[j]):
            raise ValueError('record %d cannot be loaded into an env of size %d: hdr %s, slot_pos %s (include/craftingworld.h: cw_load_records states the rule)'
                             % (j, int(size), hdr[j].tolist(), slot_pos[j].tolist()))
    return hdr, slot_pos, idx


EXPAND_FIELDS = ('reward', 'done', 'changed', 'achieved_mask', 'hdr', 'slot_pos')


def _expand_m(num_envs, hdr, slot_pos, env_of):
    """expand_args on (shape, numpy dtype) pairs (or None): what both of expand()'s paths share -- a device tensor is checked without being copied"""
    num_envs = int(num_envs)
    if (hdr is None) != (slot_pos is None):
        raise ValueError('hdr and slot_pos go together: %s given without %s' % (('slot_pos', 'hdr') if hdr is None else ('hdr', 'slot_pos')))
    if hdr is None:
        if env_of is not None:
            raise ValueError('env_of needs hdr and slot_pos: the engine\'s own states are env 0 .. num_envs - 1')
        return num_envs
    (hs, hd), (ps, pd) = hdr, slot_pos
    if len(hs) < 1 or hs[-1] != 16 or np.dtype(hd) != np.uint8:
        raise ValueError('hdr must be uint8 [..., 16], got %s %s' % (np.dtype(hd), tuple(hs)))
    if len(ps) < 1 or ps[-1] != 8 or np.dtype(pd) not in (np.dtype(np.int16), np.dtype(np.uint16)):
        raise ValueError('slot_pos must be int16 [..., 8], got %s %s' % (np.dtype(pd), tuple(ps)))
    if tuple(hs[:-1]) != tuple(ps[:-1]):
        raise ValueError('hdr holds %s records, slot_pos %s' % (tuple(hs[:-1]), tuple(ps[:-1])))
    m = int(np.prod(hs[:-1], dtype=np.int64))
    if m > 2 ** 27:
        raise ValueError('%d states: at most 2**27 in one call' % m)
    if env_of is not None:
        es, ed = env_of
        if len(es) != 1 or not np.issubdtype(np.dtype(ed), np.integer) or es[0] != m:
            raise ValueError('env_of must be a flat integer list with one entry per state (%d), got %s %s' % (m, np.dtype(ed), tuple(es)))
    return m


def expand_args(num_envs, hdr, slot_pos, env_of):
    """What cw_expand is handed, validated on the host (numpy inputs): -> M, the number of input states.  hdr uint8 [..., 16] and slot_pos int16 / uint16
    [..., 8] with the same leading shape (flattened to M), or both None: the engine's own states, M = num_envs -- nothing else can be asked of them, so
    env_of must be None too.  env_of: None (state j belongs to env j % num_envs), or a flat integer list of M env ids; a negative entry = the state
    takes no part.  ValueError for one of hdr / slot_pos without the other, env_of without them, leading shapes that differ, a wrong dtype or last
    dimension, an env_of that is not flat, not integer or not of length M; IndexError for an env_of entry >= num_envs (a device tensor handed over in
    place is not read on the host: there the kernel skips such an entry and counts it)."""
    sd = lambda a: None if a is None else (np.shape(a), np.asarray(a).dtype)  # noqa: E731
    e = None if env_of is None else np.asarray(env_of)
    m = _expand_m(num_envs, sd(hdr), sd(slot_pos), None if e is None else (e.shape, e.dtype if e.size else np.dtype(np.int32)))
    if e is not None and e.size and int(e.max()) >= int(num_envs):
        raise IndexError('env index %d outside a batch of %d envs' % (int(e.max()), int(num_envs)))
    return m


SIMULATE_FIELDS = ('ret', 'length', 'done', 'achieved_mask', 'hdr', 'slot_pos', 'rewards', 'dones')
SIMULATE_MAX_STEPS = 32767


def _simulate_tm(num_envs, shape, dtype, m):
    """simulate_args on the actions' (shape, numpy dtype): -> T.  m: the number of records, None for the engine's own states (the broadcast form)"""
    num_envs, shape = int(num_envs), tuple(int(s) for s in shape)
    if not np.issubdtype(np.dtype(dtype), np.integer):
        raise ValueError('actions must be integers (uint8 goes over in place), got %s' % np.dtype(dtype))
    if m is None:
        if len(shape) == 2 and shape[1] > 0 and shape[1] % num_envs == 0:
            m = shape[1]
        elif len(shape) == 3 and shape[1] > 0 and shape[2] == num_envs:
            m = shape[1] * shape[2]
        else:
            raise ValueError('actions must be [T, K * num_envs] or [T, K, num_envs] with K >= 1 and num_envs = %d, got %s' % (num_envs, shape))
        if m > 2 ** 27:
            raise ValueError('%d states: at most 2**27 in one call' % m)
    elif len(shape) < 2 or int(np.prod(shape[1:], dtype=np.int64)) != m:
        raise ValueError('actions must be [T, M] with one column per record (M = %d), got %s' % (m, shape))
    if not 1 <= shape[0] <= SIMULATE_MAX_STEPS:
        raise ValueError('T = %d steps: 1 .. %d in one call' % (shape[0], SIMULATE_MAX_STEPS))
    return shape[0], m


def simulate_actions(a):
    """actions on the host-validated path of simulate(): integers of any width -> contiguous uint8; ValueError for another dtype or a value outside 0 .. 255
    (0..5 act, everything above is the no-op; nothing wraps into range)"""
    a = np.asarray(a)
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError('actions must be integers (uint8 goes over in place), got %s' % a.dtype)
    if a.size and (int(a.min()) < 0 or int(a.max()) > 255):
        raise ValueError('actions must lie in 0 .. 255 (0..5 act, the rest is the no-op), got %d .. %d' % (int(a.min()), int(a.max())))
    return np.ascontiguousarray(a, dtype=np.uint8)


def simulate_args(num_envs, actions_shape_dtype, hdr, slot_pos, env_of):
    """What cw_simulate is handed, validated on the host: -> (T, M).  actions_shape_dtype: the actions' (shape, dtype) -- integers, [T, M], or without
    records [T, K * num_envs] / [T, K, num_envs] (the broadcast form: plan k of env i in column k * num_envs + i); T = 1 .. 32 767.  hdr / slot_pos / env_of:
    numpy inputs under expand_args' rules (both records or neither, env_of only with them, IndexError for an entry >= num_envs); with records M is their
    number and the actions hold one column each.  ValueError for everything else."""
    shape, dtype = actions_shape_dtype
    m = expand_args(num_envs, hdr, slot_pos, env_of)
    return _simulate_tm(num_envs, shape, dtype, None if hdr is None else m)


UNROLL_FIELDS = ('hdr', 'slot_pos', 'reward', 'done', 'changed', 'taken', 'length')
UNROLL_MAX_ROWS = 2 ** 27


def _unroll_rows(T, m):
    """cw_unroll's cap on one launch: the [T + 1, M] record arrays hold at most 2**27 records"""
    if (T + 1) * m > UNROLL_MAX_ROWS:
        raise ValueError('(T + 1) * M = %d * %d records: at most 2**27 in one call' % (T + 1, m))
    return T, m


def unroll_args(num_envs, actions_shape_dtype, hdr, slot_pos, env_of):
    """What cw_unroll is handed, validated on the host: -> (T, M).  simulate_args' rules, and (T + 1) * M <= 2**27: ValueError beyond it."""
    return _unroll_rows(*simulate_args(num_envs, actions_shape_dtype, hdr, slot_pos, env_of))


PLAN_FIELDS = ('q', 'length', 'done', 'achieved_mask', 'hdr', 'slot_pos', 'plan', 'best_action', 'best_q')
PLAN_MAX_DEPTH, PLAN_MAX_LEAVES = 8, 2 ** 32


def _plan_depth(depth, m):
    """plan_args on the depth and the number of states: -> D"""
    if isinstance(depth, (bool, np.bool_)) or not isinstance(depth, (int, np.integer)):
        raise ValueError('depth must be an integer 1 .. %d, got %r' % (PLAN_MAX_DEPTH, depth))
    depth = int(depth)
    if not 1 <= depth <= PLAN_MAX_DEPTH:
        raise ValueError('depth = %d: 1 .. %d in one call' % (depth, PLAN_MAX_DEPTH))
    if m * 6 ** depth > PLAN_MAX_LEAVES:
        raise ValueError('%d states at depth %d are %d plans: at most 2**32 in one call' % (m, depth, m * 6 ** depth))
    return depth


def plan_args(num_envs, depth, hdr, slot_pos, env_of):
    """What cw_plan is handed, validated on the host: -> (D, M).  depth: an integer 1 .. 8 with M * 6**depth <= 2**32 (65 536 states at depth 6, 2 048 at
    depth 8); hdr / slot_pos / env_of: numpy inputs under expand_args' rules (both records or neither, env_of only with them, IndexError for an entry
    >= num_envs).  ValueError for everything else."""
    m = expand_args(num_envs, hdr, slot_pos, env_of)
    return _plan_depth(depth, m), m


SHOOT_FIELDS = ('best_ret', 'best_sample', 'best_action', 'length', 'done', 'achieved_mask', 'hdr', 'slot_pos', 'plan', 'ret')
SHOOT_MAX_SAMPLES, SHOOT_MAX_WORK = 65536, 2 ** 32
SEEN_FIELDS = ('fresh', 'first')
REACH_FIELDS = ('distance', 'plan', 'first_action', 'frontier', 'searched_depth')
REACH_MAX_ROWS = (2 ** 28 - 1) // 6 - 63       # 6 * (max_rows + 63) < 2**28: the row field of the visited set's bids


def _shoot_int(v, what, lo, hi):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError('%s must be an integer %d .. %d, got %r' % (what, lo, hi, v))
    if not lo <= int(v) <= hi:
        raise ValueError('%s = %d: %d .. %d in one call' % (what, int(v), lo, hi))
    return int(v)


def _shoot_tk(horizon, samples, m):
    """shoot_args on the horizon, the number of samples and the number of states: -> (T, K)"""
    T, K = _shoot_int(horizon, 'horizon', 1, SIMULATE_MAX_STEPS), _shoot_int(samples, 'samples', 1, SHOOT_MAX_SAMPLES)
    if m * K * T > SHOOT_MAX_WORK:
        raise ValueError('%d states x %d samples x %d steps are %d steps: at most 2**32 in one call' % (m, K, T, m * K * T))
    return T, K


def shoot_args(num_envs, horizon, samples, hdr, slot_pos, env_of):
    """What cw_shoot is handed, validated on the host: -> (T, K, M).  horizon: an integer 1 .. 32 767, samples: an integer 1 .. 65 536, with
    M * samples * horizon <= 2**32 (65 536 states x 1 024 samples x 64 steps); hdr / slot_pos / env_of: numpy inputs under expand_args' rules (both records
    or neither, env_of only with them, IndexError for an entry >= num_envs).  ValueError for everything else."""
    m = expand_args(num_envs, hdr, slot_pos, env_of)
    return _shoot_tk(horizon, samples, m) + (m,)


def shoot_seed(seed):
    """the scalar seed of shoot() / shoot_actions(): an integer 0 .. 2**64 - 1 (ValueError otherwise)"""
    return _shoot_int(seed, 'seed', 0, 2 ** 64 - 1)


def shoot_weights(weights, horizon, m):
    """The weights of shoot() / shoot_actions() on the host-validated path: integers 0 .. 65 535 of shape [T, 6, M] or [T, 6] (every state alike: BROADCAST
    WITH A COPY to [T, 6, M]) -> contiguous np.uint16 [T, 6, M].  Floats raise TypeError: the draw is integer arithmetic, and how probabilities become
    integers is the caller's choice (np.round(p * 65535).astype(np.uint16) keeps 16 bits; a weight that must stay possible has to stay >= 1).  ValueError
    for another dtype, shape or a value outside 0 .. 65 535."""
    w = np.asarray(weights)
    if np.issubdtype(w.dtype, np.floating):
        raise TypeError('weights are integers 0 .. 65535 (the draw is exact integer arithmetic): quantise probabilities yourself, e.g. '
                        'np.round(p * 65535).astype(np.uint16), got %s' % w.dtype)
    if w.dtype == np.bool_ or not np.issubdtype(w.dtype, np.integer):
        raise ValueError('weights must be integers 0 .. 65535 (uint16 goes over in place), got %s' % w.dtype)
    if w.shape not in ((horizon, 6, m), (horizon, 6)):
        raise ValueError('weights must be [T, 6, M] = %s or [T, 6], got %s' % ((horizon, 6, m), w.shape))
    if w.size and (int(w.min()) < 0 or int(w.max()) > 65535):
        raise ValueError('weights must lie in 0 .. 65535, got %d .. %d' % (int(w.min()), int(w.max())))
    if w.ndim == 2:
        w = np.broadcast_to(w[:, :, None], (horizon, 6, m))
    return np.ascontiguousarray(w, dtype=np.uint16)


REFIT_FIELDS = ('elites', 'weights', 'elite_min')
REPLAY_FIELDS = ('hdr', 'slot_pos', 'next_hdr', 'next_slot_pos', 'goal_hdr', 'goal_slot_pos', 'action', 'reward', 'done', 'desired', 'env', 'slot', 'future')
REPLAY_STRATEGIES = ('future', 'final')


def refit_args(ret, elites, horizon, smooth=1, gain=1, env_of=None, num_envs=None):
    """What cw_shoot_refit is handed, validated on the host: -> (T, K, E, M).  ret: the (shape, numpy dtype) of the returns -- int32 [K, M] with K 1 .. 65 536
    and M <= 2**27; elites: an integer 1 .. K; horizon: an integer 1 .. 32 767 with M * K * horizon <= 2**32 (shoot()'s cap: the refit draws at most that often);
    smooth: an integer 0 .. 65 535; gain: an integer 1 .. 65 535; env_of: None or a flat integer list of M env ids (a negative entry = the state takes no
    part; IndexError for an entry >= num_envs, where num_envs is given).  ValueError for everything else."""
    shape, dtype = ret
    if len(shape) != 2 or np.dtype(dtype) != np.int32:
        raise ValueError('ret must be int32 [K, M] (shoot()\'s \'ret\' field), got %s %s' % (np.dtype(dtype), tuple(shape)))
    K, m = int(shape[0]), int(shape[1])
    if m > 2 ** 27:
        raise ValueError('%d states: at most 2**27 in one call' % m)
    T, K = _shoot_tk(horizon, K, m)
    E = _shoot_int(elites, 'elites', 1, K)
    _shoot_int(smooth, 'smooth', 0, 65535)
    _shoot_int(gain, 'gain', 1, 65535)
    if env_of is not None:
        e = np.asarray(env_of)
        if e.ndim != 1 or e.shape[0] != m or e.size and not np.issubdtype(e.dtype, np.integer):
            raise ValueError('env_of must be a flat integer list with one entry per state (%d), got %s %s' % (m, e.dtype, e.shape))
        if num_envs is not None and e.size and int(e.max()) >= int(num_envs):
            raise IndexError('env index %d outside a batch of %d envs' % (int(e.max()), int(num_envs)))
    return T, K, E, m


def _render_records_m(frame_shape, lead, mask, out):
    """render_records_args on the records' leading shape and the (shape, numpy dtype) of mask and out (None: not given)"""
    lead, frame_shape = tuple(int(x) for x in lead), tuple(int(x) for x in frame_shape)
    if mask is not None:
        ms, md = mask
        if np.dtype(md) not in (np.dtype(np.bool_), np.dtype(np.uint8)):
            raise ValueError('mask must be bool or uint8, got %s' % np.dtype(md))
        if tuple(ms) != lead:
            raise ValueError('mask must have the records\' leading shape %s, got %s' % (lead, tuple(ms)))
    if out is not None:
        os_, od = out
        if np.dtype(od) != np.uint8 or tuple(os_) != lead + frame_shape:
            raise ValueError('out must be a contiguous uint8 tensor %s, got %s %s' % (lead + frame_shape, np.dtype(od), tuple(os_)))


def render_records_args(frame_shape, hdr, slot_pos, mask=None, out=None):
    """What cw_render_records is handed, validated on the host (numpy inputs): -> (M, the records' leading shape).  hdr uint8 [..., 16] and slot_pos int16 /
    uint16 [..., 8] under expand_args' rules, both required; mask: None or bool / uint8 with the records' leading shape; out: None or a C-contiguous uint8
    array of the leading shape plus frame_shape.  ValueError for everything else."""
    if hdr is None or slot_pos is None:
        raise ValueError('render_records needs hdr and slot_pos')
    m = expand_args(1, hdr, slot_pos, None)
    lead = tuple(np.shape(hdr)[:-1])
    if out is not None and not (isinstance(out, np.ndarray) and out.flags['C_CONTIGUOUS']):
        raise ValueError('out must be a contiguous uint8 array %s' % (lead + tuple(frame_shape),))
    _render_records_m(frame_shape, lead, None if mask is None else (np.shape(mask), np.asarray(mask).dtype),
                      None if out is None else (out.shape, out.dtype))
    return m, lead


def _field_names(fields, known, default):
    names = default if fields is None else tuple(fields)
    if not names or any(f not in known for f in names) or len(set(names)) != len(names):
        raise ValueError('fields must be a non-empty subset of %s' % (known,))
    return names


# What _in_place does with a tensor that is NOT on the env's device.  Every call keeps the rule it came with:
#   records, env_of, simulate's actions, render_records' mask   _RAISES: ValueError for another CUDA device, whatever else the tensor is; a CPU tensor is copied
#   reset_envs / imagine_obs / sample_states: the mask          _RAISES_CPU_TOO: the same, and a CPU tensor raises as well -- unless host_outputs, then it is copied
#   snapshot_save / snapshot_load: rows                         _RAISES_IF_ELIGIBLE: ValueError only if it would otherwise go over in place, else copied (CPU: copied)
#   imagine_obs: desired                                        _COPIED: never an error -- copied through the host
_RAISES, _RAISES_CPU_TOO, _RAISES_IF_ELIGIBLE, _COPIED = range(4)

_LIVE = weakref.WeakSet()


@atexit.register
def _close_all():      # destroy engines before the HIP runtime is torn down at interpreter exit
    for env in list(_LIVE):
        try:
            env.close()
        except Exception:  # noqa: BLE001
            pass


class CraftingWorldVecEnv:
    """Batched drop-in for CraftingWorldEnvRay; see module docstring.

    Extra (non-reference) kwargs: num_envs, obs_mode ('pixels' full-frame render every step |
    'pixels_dirty' persistent frame with <=2 repainted cells per step, the reference's own
    render_edit strategy | 'state' no pixel buffers), device, seed, seed_style, auto_reset,
    task_menus + env_menu (heterogeneous ordered task lists: env i uses task_menus[env_menu[i]],
    each menu a dict with any of selected_tasks / number_of_tasks / stacking / reward_style),
    raster ('ray' = CraftingWorldEnvRay's 4x4 colour tiles, 'alt' = CraftingWorldEnvAltObs's 3x3 CPV tiles),
    keep_terminal_obs (pixel modes: info['terminal_observation'] holds the last frame of every episode
    that ended this step, as gym.vector does, at the cost of one extra frame write per finished env),
    host_outputs (small batches driven from host code -- the single-env gym loop: frames, reward, done and masks
    live in pinned host memory the kernels write directly; they come back as CPU tensors, step()/reset() return
    after one stream sync and there is no copy; actions may be plain ints/arrays).
    """

    metadata = {'render.modes': ['Non']}
    is_vector_env = True          # gym.vector.VectorEnv marker (wrappers key on it)
    viewer = None

    def __init__(self, num_envs, size=(21, 21), fixed_init_state=0, max_steps=300, store_gif=False,
                 render_save_rate=1, task_list=TASK_LIST, selected_tasks=TASK_LIST, number_of_tasks=None,
                 stacking=True, reward_style=None, obs_mode='pixels', device=None, seed=None,
                 seed_style='numpy', auto_reset=True, task_menus=None, env_menu=None,
                 keep_terminal_obs=False, raster='ray', host_outputs=False):
        if store_gif:
            raise NotImplementedError('the GIF episode recorder (ray.py:565-597) records ONE env: use the N=1 classes (env.py, recorder.py) or '
                                      'recorder.EpisodeRecorder on a row of this batch')
        w, h = size
        if w != h:
            raise ValueError('non-square grids raise IndexError in the reference (SURVEY.md §8a); rejected')
        if raster not in ('ray', 'alt'):
            raise ValueError("raster must be 'ray' (4x4 colour tiles) or 'alt' (CraftingWorldEnvAltObs 3x3 CPV tiles)")
        if obs_mode not in _OBS_MODES:
            raise ValueError('obs_mode must be one of %s' % sorted(_OBS_MODES))
        if not torch.cuda.is_available():
            raise L.CraftingWorldError('no MI355X visible to torch: the CraftingWorld engine has no CPU fallback')
        self._lib = L.load()
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != 'cuda':
            raise ValueError('device must be a cuda (HIP) device')
        self.device = torch.device('cuda', dev.index if dev.index is not None else torch.cuda.current_device())
        self.num_envs = int(num_envs)
        self.STATE_W = self.STATE_H = self.size = int(w)
        self.MAX_STEPS = int(max_steps)
        self.task_list = list(task_list)
        self.selected_tasks = list(selected_tasks)
        self.stacking = stacking
        self.fixed_init_state = int(fixed_init_state)
        self.obs_mode = obs_mode
        self.auto_reset = bool(auto_reset)
        self.seed_style = seed_style

        defaults = dict(selected_tasks=selected_tasks, number_of_tasks=number_of_tasks, stacking=stacking,
                        reward_style=reward_style)
        menus = [dict(defaults)] if task_menus is None else [dict(defaults, **m) for m in task_menus]
        self._menus = (L.cw_task_menu * len(menus))(*[_menu_struct(self.task_list, **m) for m in menus])
        self.number_of_tasks = self._menus[0].number_of_tasks
        if env_menu is not None:
            env_menu = np.ascontiguousarray(env_menu, dtype=np.uint8)
            if env_menu.shape != (self.num_envs,):
                raise ValueError('env_menu must have shape (num_envs,)')
        self._env_menu = env_menu

        cfg = L.cw_config()
        cfg.abi_version = L.CW_ABI_VERSION
        cfg.num_envs = self.num_envs
        cfg.size = self.size
        cfg.max_steps = self.MAX_STEPS
        cfg.n_task_list = len(self.task_list)
        cfg.fixed_init_state = self.fixed_init_state
        cfg.obs_mode = _OBS_MODES[obs_mode]
        cfg.auto_reset = 1 if self.auto_reset else 0
        cfg.keep_terminal_obs = 1 if (keep_terminal_obs and obs_mode != 'state') else 0
        cfg.raster = L.CW_RASTER_ALT if raster == 'alt' else L.CW_RASTER_RAY
        self.raster = raster
        self.host_outputs = bool(host_outputs)
        cfg.host_outputs = 1 if self.host_outputs else 0
        cfg.n_menus = len(menus)
        cfg.menus = self._menus
        cfg.env_menu = env_menu.ctypes.data_as(C.POINTER(C.c_uint8)) if env_menu is not None else None
        h_ = C.c_void_p()
        L.check(self._lib.cw_create(C.byref(cfg), self.device.index, C.byref(h_)), 'cw_create', self._lib)
        self._h = h_
        _LIVE.add(self)

        # zero-copy views of the engine's buffers
        tab = L.cw_buffer_table()
        L.check(self._lib.cw_buffers(self._h, C.byref(tab)), 'cw_buffers', self._lib)
        N, di = self.num_envs, self.device.index
        # frame geometry: ray.py:84 (4W,4H,3) / craftingworld_altobs.py:115 ((W+1)*3, H*3, 3)
        self.frame_shape = (3 * self.size + 3, 3 * self.size, 3) if raster == 'alt' else (4 * self.size, 4 * self.size, 3)
        fs = (N,) + self.frame_shape
        assert tab.frame_bytes == fs[1] * fs[2] * fs[3]
        dv = lambda p, shape, dt: tensor_view(p, shape, dt, di)  # noqa: E731
        v = (lambda p, shape, dt: _host_view(p, shape, dt)) if self.host_outputs else dv  # noqa: E731
        self._host_actions = _host_view(tab.host_actions, (N,), torch.int32).numpy() if self.host_outputs else None
        self._host_onehot = _host_view(tab.host_onehot, (self.size, self.size, 12), torch.uint8).numpy() if (self.host_outputs and tab.host_onehot) else None
        self._obs = v(tab.obs, fs, torch.uint8)
        self._desired_img = v(tab.desired_goal, fs, torch.uint8)
        self._init_img = v(tab.init_obs, fs, torch.uint8)
        self.terminal_observation = v(tab.terminal_obs, fs, torch.uint8)   # None unless keep_terminal_obs
        self.reward = v(tab.reward, (N,), torch.int32)
        self._done_u8 = v(tab.done, (N,), torch.uint8)
        self.done = self._done_u8.view(torch.bool)
        self.achieved_mask = v(tab.achieved, (N,), torch.int16)      # bit i = task_list[i] (bit pattern of a u16)
        self.desired_mask = v(tab.desired, (N,), torch.int16)
        self.episode_length = v(tab.episode_length, (N,), torch.int32)
        self.episode_return = v(tab.episode_return, (N,), torch.int32)   # sum of the finished episode's rewards (ray.py:361-367), valid where done
        self.hdr = dv(tab.hdr, (N, 16), torch.uint8)                 # packed current state, layout in craftingworld.h
        self.slot_pos = dv(tab.slot_pos, (N, 8), torch.int16)
        self.counters = dv(tab.counters, (4,), torch.int64)
        self._counters_raw = dv(tab.counters, (8,), torch.int64)     # (+ the engine's private words, craftingworld.h: tests only)
        self.agent_rc = self.hdr[:, 0:2]
        self.hold = self.hdr[:, 2]

        pix = self.frame_shape
        self.single_action_space = Discrete(len(ACTION_NAMES))       # ray.py:133
        self.action_space = MultiDiscrete([len(ACTION_NAMES)] * N)
        if obs_mode == 'state':
            self.single_observation_space = Dict(dict(hdr=Box(0, 255, (16,), np.uint8), slot_pos=Box(-2, 32767, (8,), np.int16)))
        else:
            self.single_observation_space = Dict({k: Box(0, 255, pix, np.uint8) for k in
                                                  ('observation', 'desired_goal', 'achieved_goal', 'init_observation')})
        self.observation_space = batch_space(self.single_observation_space, N)   # gym.vector: leading N on every Box
        self.observation_vector_space = Dict(dict(                   # ray.py:94-110
            observation=Box(0, 1, (self.size, self.size, 12), np.uint8),
            desired_goal=Box(0, 1, (1, len(self.task_list)), np.uint8),
            achieved_goal=Box(0, 1, (1, len(self.task_list)), np.uint8),
            init_observation=Box(0, 1, (self.size, self.size, 12), np.uint8)))
        self._pending = False
        self._actions_keepalive = None
        self._keepalive = {}                                         # entry point -> the tensors its last call handed over (_call)
        self._cw_step, self._di = self._lib.cw_step, self.device.index
        self._raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None) or (lambda di: torch.cuda.current_stream(di).cuda_stream)
        self.seed(seed)                                              # ray.py:70 (OS entropy when None)
        if self.fixed_init_state:                                    # ray.py:116-118
            self._call('cw_generate_fixed_states', sync=False)

    # ------------------------------------------------------------------ plumbing
    def _stream(self):
        return C.c_void_p(self._raw_stream(self._di))       # (the raw handle without building a torch.cuda.Stream object)

    def _call(self, name, *args, sync=True, keep=None):
        """The tail of a call that enqueues work: library entry point `name` with the engine, `args` and torch's current stream.  A tensor among `args`
        goes over as its address and is kept alive under `name` until the next call of the same entry point (the kernel may not have run yet, and a
        captured graph replays it), as is `keep`: tensors that go over inside a struct; what the caller alone owns goes in as a pointer (_vp) and is
        not kept.  sync: a host_outputs engine waits for the work, its results being read by host code next."""
        self._keepalive[name] = (args, keep)
        rc = getattr(self._lib, name)(self._h, *[C.c_void_p(a.data_ptr()) if type(a) is torch.Tensor else a for a in args], self._stream())
        if rc:
            L.check(rc, name, self._lib)
        if sync and self.host_outputs:
            self._sync()

    def _in_place(self, t, dtypes, shape=None, elsewhere=_RAISES, what='tensor'):
        """Does `t` go to the kernel as it is -- no copy, no synchronisation?  Yes for a contiguous CUDA tensor on the env's device of one of `dtypes` (and
        of `shape`, where one is given); everything else the caller validates and packs on the host and copies over.  elsewhere: the call's rule for a
        tensor on another device (the table above _RAISES)."""
        if type(t) is not torch.Tensor:
            return False
        here = t.device == self.device
        if not here and (t.is_cuda and (elsewhere == _RAISES or elsewhere == _RAISES_CPU_TOO) or elsewhere == _RAISES_CPU_TOO and not self.host_outputs):
            raise ValueError('the %s is on %s, the envs are on %s' % (what, t.device, self.device))
        if not (t.is_cuda and t.dtype in dtypes and (shape is None or tuple(t.shape) == shape) and t.is_contiguous()):
            return False
        if not here and elsewhere == _RAISES_IF_ELIGIBLE:
            raise ValueError('the %s is on %s, the envs are on %s' % (what, t.device, self.device))
        return here

    def _out(self, out, shape, full=True):
        """The uint8 tensor a call writes: a fresh one, or the caller's once it is found to be a contiguous uint8 tensor of `shape` on the env's device
        (ValueError otherwise; full=False: shape and dtype are left to the caller's own check)."""
        if out is None:
            return torch.empty(shape, dtype=torch.uint8, device=self.device)
        if (type(out) is not torch.Tensor or out.device != self.device or not out.is_contiguous()
                or full and (out.dtype != torch.uint8 or tuple(out.shape) != shape)):
            raise ValueError('out must be a contiguous uint8 tensor %s on %s' % (shape, self.device))
        return out

    def _out_dict(self, out, names, spec):
        """The named tensors a call writes, spec[name] = (shape, dtype): fresh ones for `names` (a bool field is allocated as bytes and viewed: the kernels
        write 0 / 1), or the caller's dict once it holds exactly `names`, each a contiguous tensor of its shape and dtype on the env's device (ValueError
        otherwise)."""
        if out is None:
            out = {f: torch.empty(spec[f][0], dtype=torch.uint8 if spec[f][1] is torch.bool else spec[f][1], device=self.device) for f in names}
            return {f: t.view(torch.bool) if spec[f][1] is torch.bool else t for f, t in out.items()}
        if set(out) != set(names):
            raise ValueError('out holds %s, asked for %s' % (sorted(out), sorted(names)))
        for f in names:
            t = out[f]
            if (type(t) is not torch.Tensor or tuple(t.shape) != spec[f][0] or t.dtype != spec[f][1] or t.device != self.device
                    or not t.is_contiguous()):
                raise ValueError('out[%r] must be a contiguous %s tensor %s on %s' % (f, spec[f][1], spec[f][0], self.device))
        return out

    def close_extras(self, **kwargs):
        """gym.vector hook: nothing besides the engine to release."""

    def close(self, **kwargs):
        if getattr(self, '_h', None):
            self.close_extras(**kwargs)
            self._lib.cw_destroy(self._h)
            self._h = None

    @property
    def closed(self):
        return getattr(self, '_h', None) is None

    @property
    def unwrapped(self):
        return self

    def __repr__(self):
        return 'CraftingWorldVecEnv(%d envs, %dx%d, obs_mode=%r, %s)' % (self.num_envs, self.size, self.size, self.obs_mode, self.device)

    def __del__(self):
        if sys is None or sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    # ------------------------------------------------------------------ RNG (ray.py:145-147)
    def seed(self, seed=None):
        """gym.vector's seed(seeds): an int -> env i gets seed+i; a list/array of num_envs ints -> env i gets seeds[i];
        None -> OS entropy (ray.py:70).  seed_style 'numpy': env stream = numpy RandomState(seed_i);
        'gym': gym<=0.21 np_random(seed_i) hashing (seeding.py, unpinned).  Returns the per-env seeds."""
        if seed is not None and not isinstance(seed, (int, np.integer)):
            seeds = [seeding.create_seed(int(s)) for s in np.asarray(seed).reshape(-1)]
            if len(seeds) != self.num_envs:
                raise ValueError('expected %d seeds, got %d' % (self.num_envs, len(seeds)))
        else:
            base = seeding.create_seed(seed)
            seeds = [(base + i) for i in range(self.num_envs)]
        self._seeds = seeds
        if self.seed_style == 'gym':
            keys = np.empty((self.num_envs, L.CW_MT_N), dtype=np.uint32)
            pos = np.empty(self.num_envs, dtype=np.int32)
            for i, s in enumerate(seeds):
                keys[i], pos[i] = seeding.mt_state_from_seed(s)
            self.set_rng_states(keys, pos)
        else:
            arr = np.array([s & 0xFFFFFFFF for s in seeds], dtype=np.uint32)
            self._settle()
            L.check(self._lib.cw_seed_int(self._h, arr.ctypes.data_as(C.c_void_p)), 'cw_seed_int', self._lib)
        return seeds

    def set_rng_states(self, keys, pos):
        """Inject numpy RandomState states: keys uint32 [N,624], pos [N] (get_state()[1:3])."""
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        if keys.shape != (self.num_envs, L.CW_MT_N) or pos.shape != (self.num_envs,):
            raise ValueError('keys must be [N,624] and pos [N]')
        self._settle()
        L.check(self._lib.cw_seed_mt(self._h, keys.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p)), 'cw_seed_mt', self._lib)

    def get_rng_states(self):
        """-> (keys uint32 [N,624], pos int32 [N]) accepted by RandomState.set_state, same stream."""
        keys = np.empty((self.num_envs, L.CW_MT_N), dtype=np.uint32)
        pos = np.empty(self.num_envs, dtype=np.int32)
        self._settle()
        L.check(self._lib.cw_get_mt(self._h, keys.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p)), 'cw_get_mt', self._lib)
        return keys, pos

    # ------------------------------------------------------------------ gym.vector surface
    def _observation(self):
        if self.obs_mode == 'state':
            return {'hdr': self.hdr, 'slot_pos': self.slot_pos}
        return {'observation': self._obs, 'desired_goal': self._desired_img, 'achieved_goal': self._obs,
                'init_observation': self._init_img}                  # achieved_goal IS observation, ray.py:194-196

    def _sync(self):
        L.check(self._lib.cw_synchronize(self._h, self._stream()), 'cw_synchronize', self._lib)

    def _settle(self):
        """Ahead of a synchronous library call (seeding, state get/set, checkpoints): wait for torch's CURRENT stream.  The library waits for the
        streams the engine was handed by itself -- but a replayed HIP graph runs wherever torch replays it, which the engine never sees."""
        if getattr(self, '_h', None):
            self._lib.cw_synchronize(self._h, self._stream())

    def synchronize(self):
        """Block until everything this env enqueued on the current stream (and on its own side stream) has finished."""
        self._sync()

    def reset_async(self):
        self._call('cw_reset', sync=False)                  # enqueues; nothing waits
        self._has_reset = True
        self._reset_pending = True

    def reset_wait(self):
        if not getattr(self, '_reset_pending', False):
            raise RuntimeError('reset_wait without reset_async')
        self._reset_pending = False
        if self.host_outputs:
            self._sync()
        return self._observation()

    def reset(self):
        self.reset_async()
        return self.reset_wait()

    def reset_envs(self, mask=None, *, indices=None):
        """reset() of SOME envs (cw_reset_masked): those with mask[i] set, or those listed in `indices` -- exactly one of the two; every other env
        is left exactly as it is.  -> the observation dict (live views, as reset() returns).  A contiguous torch.bool / torch.uint8 tensor [num_envs]
        on the env's device is handed to the kernel in place -- no copy, no synchronisation: `env.reset_envs(env.done)` after every step() is the
        manual-reset loop of an auto_reset=False engine (and can be captured into a graph with the steps).  Anything else (numpy, lists, `indices`)
        is validated and packed on the host (reset_mask) and copied over.  A selected row afterwards holds what reset() leaves there; reward, done,
        the episode statistics and the counters are not touched: a forced reset is not a finished episode."""
        m = self._select(mask, indices)
        if m is None:
            reset_mask(self.num_envs)           # (nothing given: its "exactly one of" ValueError)
        self._call('cw_reset_masked', m)
        return self._observation()

    def _select(self, mask, indices):
        """mask / indices as reset_envs takes them -> the byte tensor the masked kernels read; None (every env) when neither is given."""
        if mask is None and indices is None:
            return None
        if self._in_place(mask, (torch.bool, torch.uint8), (self.num_envs,), _RAISES_CPU_TOO, 'mask tensor') and indices is None:
            return mask
        return torch.as_tensor(reset_mask(self.num_envs, as_numpy(mask), indices)).to(self.device)

    def imagine_obs(self, mask=None, *, indices=None, desired=None, commit=False, out=None, one_hot=False):
        """imagine_obs() (ray.py:220-299) of the selected envs against their RUNNING episode (cw_imagine_masked): a goal state drawn from each env's
        start state, its task bits and -- for GoToHouse -- whether the agent stands on its start cell; each selected env's stream advances by its draws.
        mask / indices select as in reset_envs (neither: every env).  desired: the task bits to imagine, a uint16 / int16 device tensor [N] handed over
        in place, or anything desired_bits() packs ([N] masks, [N, len(task_list)] 0/1 rows); None: each env's own desired mask.
        -> the goal frames uint8 [N, ...frame_shape] in the engine's raster (every obs_mode), or with one_hot=True the goal states uint8 [N,S,S,12]
        (CraftingWorldEnvOneHot's return).  Rows of unselected envs are NOT written.  Without `out` the tensor is engine-owned scratch, reused by the next
        call: copy what you keep.
        commit=True is the batch relabel: the drawn goal (and `desired`, when given) becomes the episode's -- desired_mask, get_state()['goal_grid'],
        one_hot(which='goal') and the desired_goal frames show it; achieved, step counts, reward, done and the counters are untouched.
        On an engine that keeps look-ahead records (auto_reset=True on the device) the call rewinds every stream through the host first: correct, but off
        the hot path and not capturable; relabel on an auto_reset=False engine with reset_envs(env.done)."""
        m = self._select(mask, indices)
        d = desired
        if d is not None and not self._in_place(d, (torch.uint16, torch.int16), (self.num_envs,), _COPIED):
            d = torch.as_tensor(desired_bits(self.num_envs, as_numpy(d), len(self.task_list)).view(np.int16)).to(self.device)
        shape = (self.num_envs, self.size, self.size, 12) if one_hot else (self.num_envs,) + self.frame_shape
        if out is None:
            key = '_imagine_oh' if one_hot else '_imagine_frames'
            out = getattr(self, key, None)
            if out is None:
                out = torch.zeros(shape, dtype=torch.uint8, device=self.device)
                setattr(self, key, out)
        else:
            self._out(out, shape)
        self._call('cw_imagine_masked', m, d, 1 if commit else 0, None if one_hot else _vp(out), _vp(out) if one_hot else None)
        return out

    def sample_states(self, mask=None, *, indices=None, pooled=False):
        """sample_state() (ray.py:599-628; pooled=True: generate_fixed_initial_state(), :630-644) from the selected envs' streams
        (cw_sample_state_masked) -> uint16 tensor [N, 9]: the cells (row * S + col) of objects 0..7 and of the agent, fixed_states()' format.
        Engine-owned scratch, reused by the next call; rows of unselected envs are not written.  Nothing of an env but its stream moves.
        ValueError for pooled with fixed_init_state == 0 (the reference's randint(0))."""
        if pooled and not self.fixed_init_state:
            raise ValueError('sample_states(pooled=True) needs fixed_init_state > 0')
        m = self._select(mask, indices)
        out = getattr(self, '_sample_cells', None)
        if out is None:
            out = self._sample_cells = torch.zeros((self.num_envs, 9), dtype=torch.int16, device=self.device).view(torch.uint16)
        self._call('cw_sample_state_masked', m, 1 if pooled else 0, _vp(out))
        return out

    # ------------------------------------------------------------------ device-resident snapshots
    def snapshot_reserve(self, rows):
        """Allocate (or re-allocate: every saved row is dropped; 0 frees it) the engine's snapshot bank of `rows` rows in device memory, each of which
        holds one env completely (cw_snapshot_reserve; synchronises this engine's work).  ValueError for rows < 0."""
        self._settle()
        L.check(self._lib.cw_snapshot_reserve(self._h, int(rows)), 'cw_snapshot_reserve', self._lib)
        self._snapshot_capacity = int(rows)

    @property
    def snapshot_row_bytes(self):
        """bytes one bank row holds (0 without a bank)"""
        return int(self._lib.cw_snapshot_row_bytes(self._h))

    @property
    def snapshot_skipped(self):
        """how many envs snapshot_save / snapshot_load have skipped so far for a bad row number, and load_records for an index outside its records or a
        record an env cannot take (counters[6]; reading it synchronises)"""
        return int(self._counters_raw[6].item())

    def _snapshot_rows(self, rows, envs, fork):
        """rows / envs as snapshot_save and snapshot_load take them -> the int32 tensor [num_envs] the kernels read"""
        if envs is None and self._in_place(rows, (torch.int32,), (self.num_envs,), _RAISES_IF_ELIGIBLE, 'rows tensor'):
            return rows
        cap = getattr(self, '_snapshot_capacity', 0) if self.snapshot_row_bytes else 2 ** 31 - 1      # (no bank: the library reports the call order)
        return torch.as_tensor(snapshot_rows(self.num_envs, cap, as_numpy(rows), as_numpy(envs), fork)).to(self.device)

    def snapshot_save(self, rows=None, *, envs=None):
        """Save envs into rows of the bank (cw_snapshot_save: one kernel, no host round trip, capturable): env i into row rows[i].  A contiguous
        torch.int32 tensor [num_envs] on the env's device is handed over in place -- no copy, no synchronisation; a negative entry = env i takes no
        part, an entry at or above the capacity is skipped and counted (snapshot_skipped).  Anything else is validated and packed on the host
        (snapshot_rows): `rows` alone holds one entry per env, `envs=[3, 5], rows=[0, 1]` pairs envs with rows.  Nothing of the envs changes."""
        self._call('cw_snapshot_save', self._snapshot_rows(rows, envs, False))

    def snapshot_load(self, rows=None, *, envs=None, with_stream=True):
        """Load rows of the bank into envs (cw_snapshot_load): env i from row rows[i], `rows` / `envs` as in snapshot_save; any number of envs may name
        the same row -- the fork.  with_stream=True: the env becomes an exact twin of the saved one, its later resets included.  with_stream=False: the
        saved episode only -- the env keeps its own RNG stream, look-ahead records, pool and task menu, plays the saved episode to its end and goes
        on with episodes of its own.  A row never saved since snapshot_reserve is skipped and counted like a row outside the bank.  reward, done, the
        episode statistics and counters[0..5] are not touched; achieved_mask / desired_mask and, in the pixel modes, the three frames show the
        restored state at once.  -> the observation dict (live views, as reset_envs returns)."""
        self._call('cw_snapshot_load', self._snapshot_rows(rows, envs, True), 1 if with_stream else 0)
        return self._observation()

    def load_records(self, hdr, slot_pos, src=None, *, envs=None, status=False):
        """Put packed records back INTO envs, which go on stepping from them (cw_load_records: one kernel, no host round trip, capturable): env i takes
        record src[i] of hdr [..., 16] / slot_pos [..., 8] (flattened to R records) -- env.hdr / env.slot_pos cloned earlier, a row of expand()'s, simulate()'s,
        plan()'s, shoot()'s or reach's result, an archive cell.  src None: R = num_envs and env i takes record i; a negative entry = env i takes no part; any
        number of envs may name one record; `envs=[3, 5], src=[0, 1]` pairs envs with records.  The records may not be env.hdr / env.slot_pos themselves.
        A loaded env receives the record's header (but keeps its own task menu) and slots; achieved_mask / desired_mask and, in the pixel modes, its
        observation frame show the record at once.  Its episode -- the start and goal states and their frames, the RNG stream, the look-ahead records -- reward,
        done, the episode statistics and counters[0..5] are not touched: the env supplies the episode, a load is not a step.  A terminal record may be loaded:
        the next step is done again (and resets, on an auto_reset engine).
        Contiguous tensors on the env's device (hdr uint8, slot_pos int16, src int32 [num_envs]) go over in place -- no copy, no synchronisation -- and are
        checked on the device: an index >= R or a record an env cannot take (include/craftingworld.h states the rule) is skipped, the env left exactly as it
        is and counted (snapshot_skipped).  Anything else is validated on the host through the same rule and packed (load_records_args: ValueError names the
        first bad record, IndexError an index outside the records).
        -> the observation dict (live views, as snapshot_load returns); with status=True (that, a uint8 tensor [num_envs]): 0 no part, 1 loaded, 2 index
        out of range, 3 record refused."""
        if hdr is None or slot_pos is None:
            raise ValueError('load_records needs hdr and slot_pos')
        h_dev, p_dev = self._in_place(hdr, (torch.uint8,)), self._in_place(slot_pos, (torch.int16,))
        if h_dev and p_dev:
            r = _expand_m(1, _shape_dtype(hdr), _shape_dtype(slot_pos), None)
            if envs is None and (src is None or self._in_place(src, (torch.int32,), (self.num_envs,))):
                if src is None and r != self.num_envs:
                    raise ValueError('the records must hold one entry per env (%d), got %d' % (self.num_envs, r))
            else:
                src = torch.as_tensor(load_records_src(self.num_envs, r, as_numpy(src), as_numpy(envs))).to(self.device)
        else:
            h, p, idx = load_records_args(self.num_envs, self.size, as_numpy(hdr), as_numpy(slot_pos), as_numpy(src), as_numpy(envs))
            r = len(h)
            hdr, slot_pos, src = (torch.as_tensor(a).to(self.device) for a in (h, p.view(np.int16), idx))
        st = torch.empty(self.num_envs, dtype=torch.uint8, device=self.device) if status else None
        if r:
            self._call('cw_load_records', src, hdr, slot_pos, r, st)
        elif status:
            st.zero_()
        obs = self._observation()
        return (obs, st.cpu() if self.host_outputs else st) if status else obs

    # ------------------------------------------------------------------ looking one step ahead
    @property
    def expand_skipped(self):
        """how many states expand(), simulate(), unroll(), plan() and shoot() have skipped so far for an env index >= num_envs (counters[7]; reading it synchronises)"""
        return int(self._counters_raw[7].item())

    def _records(self, hdr, slot_pos, env_of):
        """hdr / slot_pos / env_of as expand() and one_hot_states() take them -> (M, leading shape, device tensors or None)"""
        if hdr is None or slot_pos is None:
            return _expand_m(self.num_envs, None if hdr is None else ((16,), np.uint8), None if slot_pos is None else ((8,), np.int16),
                             None if env_of is None else ((0,), np.int32)), (self.num_envs,), None, None, None
        h_dev, p_dev = self._in_place(hdr, (torch.uint8,)), self._in_place(slot_pos, (torch.int16,))
        e_dev = env_of is None or self._in_place(env_of, (torch.int32,))
        if not h_dev:
            hdr = as_numpy(hdr)
        if not p_dev:
            slot_pos = as_numpy(slot_pos)
        if not e_dev:
            env_of = as_numpy(env_of)
            if not env_of.size:
                env_of = env_of.astype(np.int32)        # (an empty list is an empty list of ints)
        m = _expand_m(self.num_envs, _shape_dtype(hdr), _shape_dtype(slot_pos), None if env_of is None else _shape_dtype(env_of))
        lead = tuple(hdr.shape[:-1])
        if not h_dev:
            hdr = torch.as_tensor(np.ascontiguousarray(hdr)).to(self.device)
        if not p_dev:
            slot_pos = torch.as_tensor(np.ascontiguousarray(slot_pos).view(np.int16)).to(self.device)
        if not e_dev:
            if env_of.size and int(env_of.max()) >= self.num_envs:
                raise IndexError('env index %d outside a batch of %d envs' % (int(env_of.max()), self.num_envs))
            env_of = torch.as_tensor(np.ascontiguousarray(np.maximum(env_of.astype(np.int64), -1), dtype=np.int32)).to(self.device)
        return m, lead, hdr, slot_pos, env_of

    def expand(self, hdr=None, slot_pos=None, env_of=None, *, fields=None, out=None):
        """What would each of the six actions do from here?  (cw_expand: one kernel, no host round trip, capturable; no env is touched.)  -> a dict of
        device tensors, ACTION-MAJOR: entry [a, j] is action a (0..5 = Up, Right, Down, Left, PickUp, Drop) applied to input state j:
        'reward' int32 [6, M] (what step() would return), 'done' and 'changed' bool [6, M] (the action changed the state: the reference's reward gate),
        'achieved_mask' int16 [6, M], 'hdr' uint8 [6, M, 16] and 'slot_pos' int16 [6, M, 8]: the successor as a packed record -- byte for byte what
        step() leaves on an auto_reset=False engine; on an auto-reset engine therefore the terminal state a step would have replaced.
        Without arguments: the envs' current states, M = num_envs.  With hdr [..., 16] / slot_pos [..., 8] (both, same leading shape, flattened to M):
        those states -- env.hdr / env.slot_pos, a pruned frontier, or an earlier result: `expand(hdr=r['hdr'], slot_pos=r['slot_pos'])` is depth 2 with
        shape [6, 6 * N], and so on.  A record supplies agent, hold, both masks, step_num and the reward rule; the env it belongs to supplies its episode's
        start positions: env j % num_envs, or env_of[j] (int32 [M]; negative: the state takes no part and its rows are not written).
        Contiguous tensors on the env's device go over in place -- no copy, no synchronisation; an env_of entry >= num_envs is then skipped by the kernel
        and counted (expand_skipped).  Anything else is validated on the host (expand_args: ValueError, IndexError).
        fields: a subset of EXPAND_FIELDS to compute (default all).  out: a dict returned by an earlier call with the same M and fields, written again."""
        names = _field_names(fields, EXPAND_FIELDS, EXPAND_FIELDS)
        m, _, hdr, slot_pos, env_of = self._records(hdr, slot_pos, env_of)
        spec = {'reward': ((6, m), torch.int32), 'done': ((6, m), torch.bool), 'changed': ((6, m), torch.bool),
                'achieved_mask': ((6, m), self.achieved_mask.dtype), 'hdr': ((6, m, 16), torch.uint8), 'slot_pos': ((6, m, 8), self.slot_pos.dtype)}
        out = self._out_dict(out, names, spec)
        if m:
            self._call('cw_expand', env_of, hdr, slot_pos, m, C.byref(_out_struct(L.cw_expand_out, out)), keep=out)
        return out

    # ------------------------------------------------------------------ trying plans
    def simulate(self, actions, hdr=None, slot_pos=None, env_of=None, *, stop_at_done=True, fields=None, out=None):
        """What would these action sequences do from here?  (cw_simulate: one kernel that keeps every state in registers for all T steps, no host round
        trip, capturable; no env is touched and no RNG stream drawn from.)  actions: uint8 [T, M] -- state j steps through actions[:, j]; an id above 5
        is step()'s state-preserving no-op.  Without records the envs' current states are BROADCAST: actions [T, K * N] or [T, K, N] try K plans per
        env, plan k of env i in column k * N + i, with no copy of the records.  With hdr [..., 16] / slot_pos [..., 8] / env_of (expand()'s rules: env
        j % num_envs or env_of[j], a negative entry takes no part and none of its rows is written, an entry >= num_envs is skipped by the kernel and
        counted in expand_skipped) the states are the caller's and actions hold one column per record.  A contiguous uint8 tensor on the env's device
        goes over in place; other integer inputs are validated and converted on the host (a value outside 0..255: ValueError).
        stop_at_done=True: a state's first done step is its last, as on an auto-reset engine minus the reset; False: every state takes all T steps, as
        the reference keeps stepping a finished env.  -> a dict of device tensors: 'ret' int32 [M] (sum of the rewards of the steps taken), 'length'
        int32 [M] (1 + the first done step, T if none), 'done' bool [M], 'achieved_mask' [M], 'hdr' uint8 [M, 16] / 'slot_pos' int16 [M, 8] (the
        record after the last step taken, byte for byte what step() leaves on an auto_reset=False engine) and, only when named in `fields`, the traces
        'rewards' int32 [T, M] / 'dones' bool [T, M] (rows after a stopped state's end: 0 / False).  fields: a subset of SIMULATE_FIELDS (default: the
        six per-state ones).  out: a dict returned by an earlier call with the same T, M and fields, written again."""
        names = _field_names(fields, SIMULATE_FIELDS, SIMULATE_FIELDS[:6])
        own = hdr is None and slot_pos is None
        m, _, hdr, slot_pos, env_of = self._records(hdr, slot_pos, env_of)
        if self._in_place(actions, (torch.uint8,)):
            T, m = _simulate_tm(self.num_envs, actions.shape, np.uint8, None if own else m)
        else:
            a = as_numpy(actions)
            T, m = _simulate_tm(self.num_envs, a.shape, a.dtype, None if own else m)
            actions = torch.as_tensor(simulate_actions(a)).to(self.device)
        spec = {'ret': ((m,), torch.int32), 'length': ((m,), torch.int32), 'done': ((m,), torch.bool), 'achieved_mask': ((m,), self.achieved_mask.dtype),
                'hdr': ((m, 16), torch.uint8), 'slot_pos': ((m, 8), self.slot_pos.dtype), 'rewards': ((T, m), torch.int32), 'dones': ((T, m), torch.bool)}
        out = self._out_dict(out, names, spec)
        if m:
            self._call('cw_simulate', env_of, hdr, slot_pos, m, actions, T, 1 if stop_at_done else 0, C.byref(_out_struct(L.cw_simulate_out, out)), keep=out)
        return out

    # ------------------------------------------------------------------ whole trajectories
    def unroll(self, actions, hdr=None, slot_pos=None, env_of=None, *, stop_at_done=True, fields=None, out=None):
        """Which states does this plan pass through?  (cw_unroll: simulate()'s kernel with the record after EVERY step written out -- one launch, no host
        round trip, no synchronisation, capturable; no env is touched and no RNG stream drawn from.)  The arguments are simulate()'s, rule for rule:
        actions uint8 [T, M] (an id above 5 is the no-op), without records the envs' current states BROADCAST ([T, K * N] or [T, K, N]: plan k of env i
        in column k * N + i), with hdr [..., 16] / slot_pos [..., 8] / env_of the caller's states, one column per record (a negative env_of entry takes
        no part and NO row of it is written at any step; an entry >= num_envs is skipped by the kernel and counted in expand_skipped).  (T + 1) * M
        <= 2**27 in one call.  -> a dict of device tensors, STEP-MAJOR, the states flattened to M as simulate() returns them:
        'hdr' uint8 [T + 1, M, 16] / 'slot_pos' int16 [T + 1, M, 8]: row 0 is the state as read, row t + 1 the state after step t -- byte for byte
        expand()'s successor of row t for actions[t], and row T simulate()'s final record; 'reward' int32 [T, M], 'done' / 'changed' / 'taken' bool
        [T, M] (simulate()'s traces; expand()'s `changed`; taken: the step was taken); 'length' int32 [M] (simulate()'s).  stop_at_done=True: a step is
        taken iff no earlier step of its state returned done; a step not taken has reward 0, done / changed / taken False, and its row repeats the row
        before it, so the final record repeats to row T.  False: every step is taken.  The achieved mask after step t is bytes 4-5 of hdr[t + 1].
        fields: a subset of UNROLL_FIELDS (default all).  out: a dict returned by an earlier call with the same T, M and fields, written again.
        The slices callers want, with r = env.unroll(actions):
            r['hdr'][:-1] (and r['slot_pos'][:-1]) with actions are the (s_t, a_t) pairs;
            r['hdr'][1:] are the successors;
            env.render_records(r['hdr'][1:].reshape(-1, 16), r['slot_pos'][1:].reshape(-1, 8), mask=r['taken'].reshape(-1)) paints the frames of
            the steps taken."""
        names = _field_names(fields, UNROLL_FIELDS, UNROLL_FIELDS)
        own = hdr is None and slot_pos is None
        m, _, hdr, slot_pos, env_of = self._records(hdr, slot_pos, env_of)
        if self._in_place(actions, (torch.uint8,)):
            T, m = _unroll_rows(*_simulate_tm(self.num_envs, actions.shape, np.uint8, None if own else m))
        else:
            a = as_numpy(actions)
            T, m = _unroll_rows(*_simulate_tm(self.num_envs, a.shape, a.dtype, None if own else m))
            actions = torch.as_tensor(simulate_actions(a)).to(self.device)
        spec = {'hdr': ((T + 1, m, 16), torch.uint8), 'slot_pos': ((T + 1, m, 8), self.slot_pos.dtype), 'reward': ((T, m), torch.int32),
                'done': ((T, m), torch.bool), 'changed': ((T, m), torch.bool), 'taken': ((T, m), torch.bool), 'length': ((m,), torch.int32)}
        out = self._out_dict(out, names, spec)
        if m:
            self._call('cw_unroll', env_of, hdr, slot_pos, m, actions, T, 1 if stop_at_done else 0, C.byref(_out_struct(L.cw_unroll_out, out)), sync=False,
                       keep=out)                                  # (device tensors, nothing a host reads next: no synchronisation, host_outputs engines included)
        return out

    # ------------------------------------------------------------------ searching every plan
    def plan(self, depth, hdr=None, slot_pos=None, env_of=None, *, fields=None, out=None):
        """What is the best that can be done from here within `depth` steps, and which action starts it?  (cw_plan: ONE kernel that walks all 6**depth
        action strings of every state depth-first with its stack in registers -- shared prefixes are stepped once, a plan stops at its first done step;
        no host round trip, capturable; no env is touched.)  depth: 1 .. 8, with M * 6**depth <= 2**32.  The states are expand()'s: without records the
        envs' current ones (M = num_envs), else hdr [..., 16] / slot_pos [..., 8] / env_of under expand()'s rules (env j % num_envs or env_of[j], a
        negative entry takes no part and none of its rows is written, an entry >= num_envs handed over on the device is skipped and counted in
        expand_skipped).  -> a dict of device tensors, ACTION-MAJOR: entry [a, j] belongs to the plans of state j that begin with action a.
        'q' int32 [6, M]: the largest return simulate(stop_at_done=True) gives any of them; the BEST PLAN is the lexicographically smallest one that
        reaches it, zeros behind its end.  'length' int32 [6, M], 'done' bool [6, M], 'achieved_mask' [6, M], 'hdr' uint8 [6, M, 16] and 'slot_pos'
        int16 [6, M, 8]: what simulate() returns for the best plan; 'plan' uint8 [6, depth, M]: the plan itself, plan[a] step-major as simulate() takes
        its actions, plan[a, 0] == a.  'best_q' int32 [M]: the maximum of q over a, and 'best_action' uint8 [M]: the SMALLEST a that reaches it -- both
        derived from q on the device, on the env's stream, without synchronisation (of a state that takes no part they are computed from unwritten rows).
        fields: a subset of PLAN_FIELDS (default: all but 'hdr' and 'slot_pos').  out: a dict returned by an earlier call with the same depth, M and
        fields, written again."""
        names = _field_names(fields, PLAN_FIELDS, tuple(f for f in PLAN_FIELDS if f not in ('hdr', 'slot_pos')))
        m, _, hdr, slot_pos, env_of = self._records(hdr, slot_pos, env_of)
        depth = _plan_depth(depth, m)
        spec = {'q': ((6, m), torch.int32), 'length': ((6, m), torch.int32), 'done': ((6, m), torch.bool), 'achieved_mask': ((6, m), self.achieved_mask.dtype),
                'hdr': ((6, m, 16), torch.uint8), 'slot_pos': ((6, m, 8), self.slot_pos.dtype), 'plan': ((6, depth, m), torch.uint8),
                'best_action': ((m,), torch.uint8), 'best_q': ((m,), torch.int32)}
        out = self._out_dict(out, names, spec)
        derived = [f for f in ('best_action', 'best_q') if f in out]
        kernel = {f: t for f, t in out.items() if f not in derived}
        if derived and 'q' not in kernel:
            kernel['q'] = torch.empty((6, m), dtype=torch.int32, device=self.device)        # (scratch: the caller did not ask for q itself)
        if m:
            self._call('cw_plan', env_of, hdr, slot_pos, m, depth, C.byref(_out_struct(L.cw_plan_out, kernel)), keep=kernel)
        if derived:
            q = kernel['q']
            best = out['best_q'] if 'best_q' in out else torch.empty((m,), dtype=torch.int32, device=self.device)
            torch.amax(q, dim=0, out=best)
            if 'best_action' in out:                                                        # the smallest a with q[a] == best: no argmax, whose ties are not pinned
                first = torch.where(q == best, self._plan_action_ids(), 6)
                torch.amin(first, dim=0, out=out['best_action'])
        return out

    def _plan_action_ids(self):
        ids = getattr(self, '_plan_ids', None)
        if ids is None:
            ids = self._plan_ids = torch.arange(6, dtype=torch.uint8, device=self.device).reshape(6, 1)
        return ids

    # ------------------------------------------------------------------ shooting plans
    def _shoot_seed(self, seed):
        """seed as shoot() takes it -> (the scalar, the device word or None); a pair (int, tensor) is both at once -- the kernel adds them: cem()'s form"""
        if type(seed) is tuple and len(seed) == 2 and type(seed[1]) is torch.Tensor:
            return shoot_seed(seed[0]), self._shoot_seed(seed[1])[1]
        if type(seed) is torch.Tensor:
            if seed.numel() != 1 or seed.dtype not in (torch.int64, torch.uint64) or seed.device != self.device or not seed.is_contiguous():
                raise ValueError('a seed tensor must hold one int64 / uint64 element on %s, got %s %s on %s' % (self.device, seed.dtype, tuple(seed.shape), seed.device))
            return 0, seed
        return shoot_seed(seed), None

    def _shoot_weights(self, weights, T, m):
        """weights as shoot() takes them -> a uint16 [T, 6, M] tensor on the env's device, or None"""
        if weights is None or self._in_place(weights, (torch.uint16,), (T, 6, m)):
            return weights
        if self._in_place(weights, (torch.uint16,), (T, 6)):
            return weights[:, :, None].expand(T, 6, m).contiguous()
        if torch.is_tensor(weights) and weights.dtype.is_floating_point:
            shoot_weights(np.empty(0, np.float32), T, m)                 # (the TypeError, without a copy of the tensor)
        return torch.as_tensor(shoot_weights(as_numpy(weights), T, m)).to(self.device)

    def shoot(self, horizon, samples, seed=0, hdr=None, slot_pos=None, env_of=None, *, weights=None, fields=None, out=None):
        """Which of `samples` random plans of `horizon` steps does best from here?  (cw_shoot: ONE kernel that draws every action where it is used --
        a counter-based integer function of (seed, state, sample, step), stated in include/craftingworld.h and reproduced by shoot_actions() -- so no
        [T, K, M] action tensor exists; no host round trip, capturable; no env is touched.)  horizon: 1 .. 32 767, samples: 1 .. 65 536, with
        M * samples * horizon <= 2**32.  seed: an int 0 .. 2**64 - 1, or a one-element int64 / uint64 tensor on the env's device, which the KERNEL reads:
        a captured graph draws new plans on every replay once the caller has changed the word (a pair (int, tensor) is both: the kernel adds them -- cem()'s
        form).  The states are plan()'s: without records the envs' current
        ones (M = num_envs), else hdr [..., 16] / slot_pos [..., 8] / env_of under expand()'s rules (a negative env_of entry takes no part and none of its
        rows is written, an entry >= num_envs handed over on the device is skipped and counted once in expand_skipped).  weights: None (uniform actions)
        or integers 0 .. 65 535 of shape [T, 6, M] -- weights[t, a, j] is the weight of action a at step t of state j, 0 forbids it, six zeros mean
        uniform -- or [T, 6], every state alike, which is BROADCAST WITH A COPY; a uint16 tensor on the env's device goes over in place, other integers
        are validated and converted on the host, floats raise TypeError (shoot_weights).
        -> a dict of device tensors: 'best_ret' int32 [M], the largest return simulate(stop_at_done=True) gives any sample; 'best_sample' int32 [M], the
        SMALLEST sample that reaches it; 'best_action' uint8 [M], its first action; 'length' int32 [M], 'done' bool [M], 'achieved_mask' [M], 'hdr' uint8
        [M, 16] and 'slot_pos' int16 [M, 8]: what simulate() returns for it; 'plan' uint8 [T, M]: all T actions drawn for it, as simulate() takes them;
        'ret' int32 [K, M]: the return of every sample (CEM's elite selection; shoot_actions(samples=elites) gives their actions).  fields: a subset of
        SHOOT_FIELDS (default: all but 'hdr', 'slot_pos' and 'ret').  out: a dict returned by an earlier call with the same horizon, samples, M and
        fields, written again."""
        names = _field_names(fields, SHOOT_FIELDS, tuple(f for f in SHOOT_FIELDS if f not in ('hdr', 'slot_pos', 'ret')))
        m, _, hdr, slot_pos, env_of = self._records(hdr, slot_pos, env_of)
        T, K = _shoot_tk(horizon, samples, m)
        seed, seed_dev = self._shoot_seed(seed)
        weights = self._shoot_weights(weights, T, m)
        spec = {'best_ret': ((m,), torch.int32), 'best_sample': ((m,), torch.int32), 'best_action': ((m,), torch.uint8), 'length': ((m,), torch.int32),
                'done': ((m,), torch.bool), 'achieved_mask': ((m,), self.achieved_mask.dtype), 'hdr': ((m, 16), torch.uint8),
                'slot_pos': ((m, 8), self.slot_pos.dtype), 'plan': ((T, m), torch.uint8), 'ret': ((K, m), torch.int32)}
        out = self._out_dict(out, names, spec)
        if m:
            self._call('cw_shoot', env_of, hdr, slot_pos, m, T, K, seed, seed_dev, weights, C.byref(_out_struct(L.cw_shoot_out, out)), keep=out)
        return out

    def shoot_actions(self, horizon, seed=0, *, samples=None, rows=None, weights=None, n_states=None, out=None):
        """The actions shoot() draws, themselves (cw_shoot_actions: one kernel, pure) -> uint8 [T, R, M]: entry [t, r, j] is step t of sample
        samples[r, j] of state j -- or, with samples=None, of sample r, rows = R = K giving the whole action tensor in simulate()'s broadcast layout.
        samples: int32 [R, M] (an int32 tensor on the env's device goes over in place); a NEGATIVE entry leaves its column of `out` unwritten.
        horizon, seed and weights as shoot() takes them (the same seed and weights give the same draws); n_states: M (default num_envs).  out: a
        contiguous uint8 tensor [T, R, M] on the env's device, written again."""
        m = self.num_envs if n_states is None else _shoot_int(n_states, 'n_states', 0, 2 ** 27)
        T = _shoot_int(horizon, 'horizon', 1, SIMULATE_MAX_STEPS)
        if samples is None:
            if rows is None:
                raise ValueError('give samples, or rows: how many samples 0 .. rows - 1 to decode')
            R = _shoot_int(rows, 'rows', 0, 2 ** 27)
        else:
            if not self._in_place(samples, (torch.int32,)):
                s = as_numpy(samples)
                if not np.issubdtype(s.dtype, np.integer) or s.dtype == np.bool_:
                    raise ValueError('samples must be integers (int32 goes over in place), got %s' % s.dtype)
                if s.size and int(s.max()) >= 2 ** 31:
                    raise ValueError('samples must fit int32, got %d' % int(s.max()))
                samples = torch.as_tensor(np.ascontiguousarray(np.maximum(s.astype(np.int64), -1), dtype=np.int32)).to(self.device)
            if samples.dim() != 2 or samples.shape[1] != m or rows is not None and rows != samples.shape[0]:
                raise ValueError('samples must be [R, M] with M = %d%s, got %s' % (m, '' if rows is None else ' and R = rows = %r' % (rows,), tuple(samples.shape)))
            R = int(samples.shape[0])
            if R > 2 ** 27:
                raise ValueError('%d rows: at most 2**27 in one call' % R)
        if R * m * T > SHOOT_MAX_WORK:
            raise ValueError('%d rows x %d states x %d steps are %d actions: at most 2**32 in one call' % (R, m, T, R * m * T))
        seed, seed_dev = self._shoot_seed(seed)
        weights = self._shoot_weights(weights, T, m)
        out = self._out(out, (T, R, m))
        if R and m:
            self._call('cw_shoot_actions', m, T, seed, seed_dev, weights, samples, R, out)
        return out

    # ------------------------------------------------------------------ refitting plans
    def shoot_refit(self, ret, elites, horizon, seed=0, *, weights=None, env_of=None, smooth=1, gain=1, fields=None, out=None):
        """The other half of a CEM iteration: from shoot()'s 'ret' to the next weights (cw_shoot_refit: two kernels, exact integer arithmetic, no host round
        trip, capturable; no env is touched).  ret: int32 [K, M], a contiguous tensor on the env's device, which goes over in place -- shoot()'s, or any
        int32 values.  elites: E, 1 .. K.  The ELITES of state j are the first E samples in the order (return descending, sample ascending): ties go to the
        smaller sample, best_sample's rule, so two runs never differ.  horizon, seed and weights as the shoot() call that produced ret took them (the same
        seed and weights give the same draws): the actions of the elites are regenerated from the draw, ALL `horizon` of them -- the steps behind a
        sample's done step included, as 'plan' holds them -- and no [T, E, M] tensor exists.  The new weight of action a at step t of state j is
        min(65535, smooth + gain * (the number of elites that drew a there)): smooth 0 .. 65 535 is a pseudo-count (0: an action no elite drew becomes
        forbidden), gain 1 .. 65 535.  env_of: None, or shoot()'s env_of (int32 [M]; an int32 tensor on the env's device goes over in place): a negative
        entry or one >= num_envs takes no part -- the states whose 'ret' column shoot() did not write -- and nothing of it is written; expand_skipped does
        not move.
        -> a dict of device tensors: 'elites' int32 [E, M], the elite samples in ascending order; 'weights' uint16 [T, 6, M], as shoot() takes them;
        'elite_min' int32 [M], the smallest return among the elites.  fields: a subset of REFIT_FIELDS (default all).  out: a dict returned by an earlier
        call with the same shapes and fields, written again; out={'weights': w, ...} with w the very tensor passed as weights= is the refit IN PLACE (any
        other overlap of the two raises)."""
        names = _field_names(fields, REFIT_FIELDS, REFIT_FIELDS)
        if type(ret) is not torch.Tensor or ret.device != self.device or not ret.is_contiguous():
            raise ValueError('ret must be a contiguous int32 tensor [K, M] on %s (shoot()\'s \'ret\' field)' % (self.device,))
        e_dev = env_of is None or self._in_place(env_of, (torch.int32,))
        if not e_dev:
            env_of = as_numpy(env_of)
            if not env_of.size:
                env_of = env_of.astype(np.int32)        # (an empty list is an empty list of ints)
        T, K, E, m = refit_args(_shape_dtype(ret), elites, horizon, smooth, gain, None if e_dev else env_of, self.num_envs)
        if env_of is not None and e_dev and tuple(env_of.shape) != (m,):
            raise ValueError('env_of must hold one entry per state (%d), got %s' % (m, tuple(env_of.shape)))
        if not e_dev:
            env_of = torch.as_tensor(np.ascontiguousarray(np.maximum(env_of.astype(np.int64), -1), dtype=np.int32)).to(self.device)
        seed, seed_dev = self._shoot_seed(seed)
        spec = {'elites': ((E, m), torch.int32), 'weights': ((T, 6, m), torch.uint16), 'elite_min': ((m,), torch.int32)}
        in_place = weights is not None and out is not None and out.get('weights') is weights
        out = self._out_dict(out, names, spec)
        weights = out['weights'] if in_place else self._shoot_weights(weights, T, m)
        kernel = out if 'elites' in out else dict(out, elites=torch.empty((E, m), dtype=torch.int32, device=self.device))   # (the selection is always written)
        if m:
            self._call('cw_shoot_refit', env_of, m, T, K, E, seed, seed_dev, weights, ret, int(smooth), int(gain),
                       C.byref(_out_struct(L.cw_refit_out, kernel)), keep=kernel)
        return out

    def _cem_scratch(self, K, E, m):
        """what a cem() call needs and does not return, per shape and kept by the env (a captured graph goes on using it): the elites, and the returns
        where the caller did not name 'ret'"""
        held = self.__dict__.setdefault('_cem_held', {})
        if (K, E, m) not in held:
            held[(K, E, m)] = {'elites': torch.empty((E, m), dtype=torch.int32, device=self.device),
                               'ret': torch.empty((K, m), dtype=torch.int32, device=self.device)}
        return held[(K, E, m)]

    def cem(self, horizon, samples, elites, iters, seed=0, hdr=None, slot_pos=None, env_of=None, *, weights=None, smooth=1, gain=1, fields=None, out=None):
        """`iters` iterations of the cross-entropy method on the device: shoot(), then shoot_refit() of its returns into ONE weights buffer, again and
        again -- a plain loop over the two public calls with NO synchronisation and no host round trip.  Iteration i = 0 .. iters - 1 shoots with the
        current weights and the effective seed (seed + i) mod 2**64 -- a seed tensor goes over as the device word with the scalar i, so a captured graph
        draws new plans on every replay once the caller has bumped the word -- and refits with the same seed and weights, in place.  weights=None starts
        uniform and the first refit fills the buffer; other weights are COPIED into the buffer first: a caller's tensor is never written unless it is
        handed in through out= (weights=r['weights'], out=r of an earlier result r is the warm start without a copy).  horizon, samples, hdr / slot_pos /
        env_of and fields as shoot() takes them; elites, smooth and gain as shoot_refit() does.
        -> shoot()'s dict of the LAST iteration plus 'weights' uint16 [T, 6, M] (after the last refit: the warm start of the next MPC step) and
        'elite_min' int32 [M] (of the last refit).  THE RESULT IS THE LAST ITERATION'S BEST, NOT THE BEST OVER ALL ITERATIONS: 'best_ret' may lie below
        what an earlier iteration found.  out: the dict an earlier call with the same shapes and fields returned -- every buffer is used again, the
        env's own scratch included, and nothing is allocated, so the whole call can be captured into a graph together with the steps."""
        iters = _shoot_int(iters, 'iters', 1, 2 ** 31 - 1)
        names = _field_names(fields, SHOOT_FIELDS, tuple(f for f in SHOOT_FIELDS if f not in ('hdr', 'slot_pos', 'ret')))
        m, _, hdr, slot_pos, env_of = self._records(hdr, slot_pos, env_of)
        T, K = _shoot_tk(horizon, samples, m)
        E = _shoot_int(elites, 'elites', 1, K)
        smooth, gain = _shoot_int(smooth, 'smooth', 0, 65535), _shoot_int(gain, 'gain', 1, 65535)
        scalar, word = self._shoot_seed(seed)
        own = ('weights', 'elite_min')
        if out is not None and set(out) != set(names + own):
            raise ValueError('out holds %s, asked for %s' % (sorted(out), sorted(names + own)))
        fit = self._out_dict(None if out is None else {f: out[f] for f in own}, own, {'weights': ((T, 6, m), torch.uint16), 'elite_min': ((m,), torch.int32)})
        scratch = self._cem_scratch(K, E, m)
        fit['elites'] = scratch['elites']
        inner = names if 'ret' in names else names + ('ret',)
        shot = None if out is None else dict({f: out[f] for f in names}, **({} if 'ret' in names else {'ret': scratch['ret']}))
        current = None
        if weights is not None:
            if weights is not fit['weights']:
                fit['weights'].copy_(self._shoot_weights(weights, T, m))
            current = fit['weights']
        for i in range(iters):
            s = (scalar + i) % 2 ** 64 if word is None else (i, word)
            shot = self.shoot(T, K, s, hdr, slot_pos, env_of, weights=current, fields=inner, out=shot)
            self.shoot_refit(shot['ret'], E, T, s, weights=current, env_of=env_of, smooth=smooth, gain=gain, out=fit)
            current = fit['weights']
        return dict({f: shot[f] for f in names}, weights=fit['weights'], elite_min=fit['elite_min'])

    def one_hot_states(self, hdr, slot_pos, out=None):
        """obs_one_hot (ray.py:119) of caller-supplied packed records hdr [..., 16] / slot_pos [..., 8] (as expand() takes and returns them):
        -> uint8 [..., S, S, 12], the held item's channel 9-11 at the agent's cell (cw_export_onehot_states).  render_states() of the result is the
        reference's int image of that state (int16); the uint8 frame a pixel policy would see is render_records().  Does not touch the envs."""
        if hdr is None or slot_pos is None:
            raise ValueError('one_hot_states needs hdr and slot_pos')
        m, lead, hdr, slot_pos, _ = self._records(hdr, slot_pos, None)
        out = self._out(out, lead + (self.size, self.size, 12))
        if m:
            self._call('cw_export_onehot_states', hdr, slot_pos, m, out)
        return out

    def render_records(self, hdr, slot_pos, *, mask=None, out=None):
        """The frames a pixel policy would see of caller-supplied packed records hdr [..., 16] / slot_pos [..., 8] (as expand() and simulate() return them,
        env.hdr / env.slot_pos, a pruned frontier) -> uint8 [..., *frame_shape] on the env's device, in the env's raster, in every obs_mode: byte for byte
        what render() or the observation array shows of an env in that state (cw_render_records: one kernel straight from the records, no one-hot scratch
        tensor, no host round trip, capturable; no env is touched).  Contiguous tensors on the env's device go over in place; anything else is validated on
        the host and copied (render_records_args: ValueError).  mask: bool or uint8 with the records' leading shape -- where it is 0 no byte of that
        state's frame is written; expand()'s 'changed' goes in as it is (an unchanged successor's frame is its parent's).  out: a contiguous uint8 tensor of
        the leading shape plus frame_shape on the env's device (Ray raster: 4-byte aligned), written in place; without it a fresh torch.empty is returned,
        whose masked-out rows are UNINITIALISED memory."""
        if hdr is None or slot_pos is None:
            raise ValueError('render_records needs hdr and slot_pos')
        m, lead, hdr, slot_pos, _ = self._records(hdr, slot_pos, None)
        m_dev = mask is not None and self._in_place(mask, (torch.bool, torch.uint8))
        if not m_dev:
            mask = as_numpy(mask)
        if out is not None:
            self._out(out, lead + tuple(self.frame_shape), full=False)
        _render_records_m(self.frame_shape, lead, None if mask is None else _shape_dtype(mask), None if out is None else _shape_dtype(out))
        if mask is not None and not m_dev:
            mask = torch.as_tensor(np.ascontiguousarray(mask).view(np.uint8)).to(self.device)
        if out is None:
            out = self._out(None, lead + tuple(self.frame_shape))
        if m:
            self._call('cw_render_records', hdr, slot_pos, mask, m, out)
        return out

    # ------------------------------------------------------------------ searching deep
    def seen_reserve(self, capacity, *, tag_bits=0):
        """Allocate (or re-allocate: everything seen is dropped; 0 frees it) the engine's visited set for `capacity` distinct keys: the next power of two
        >= 2 * capacity slots of 48 bytes in device memory (cw_seen_reserve; synchronises this engine's work).  tag_bits: 0, a slot is tagged with the
        key's full 64-bit hash; 1 .. 63 truncates the tag -- results stay exact, only speed and seen_collisions depend on it (tests and
        tools/measure_seen.py drive the same-tag-different-key path with it).  ValueError for capacity < 0 or above 2**28 or tag_bits outside 0 .. 63."""
        capacity, tag_bits = _shoot_int(capacity, 'capacity', 0, 2 ** 28), _shoot_int(tag_bits, 'tag_bits', 0, 63)
        self._settle()
        self._seen_ctl = None
        L.check(self._lib.cw_seen_reserve(self._h, capacity, tag_bits), 'cw_seen_reserve', self._lib)
        if capacity:
            p = C.c_void_p()
            L.check(self._lib.cw_seen_counters(self._h, C.byref(p)), 'cw_seen_counters', self._lib)
            self._seen_ctl = tensor_view(p.value, (3,), torch.int64, self.device.index)

    def seen_clear(self):
        """Empty the visited set and reset its counters (cw_seen_clear: one kernel, capturable)."""
        self._call('cw_seen_clear')

    def _seen_counter(self, k):
        ctl = getattr(self, '_seen_ctl', None)
        return 0 if ctl is None else int(ctl[k].item())

    @property
    def seen_size(self):
        """how many keys the visited set holds (0 without a set; reading it synchronises, like expand_skipped)"""
        return self._seen_counter(0)

    @property
    def seen_overflow(self):
        """how many rows seen_insert() has reported fresh since the last clear because they found no slot within the probe bound -- a set filled beyond its
        capacity (reading it synchronises)"""
        return self._seen_counter(1)

    @property
    def seen_collisions(self):
        """how many rows seen_insert() has reported fresh since the last clear because a slot held their tag under another key (reading it synchronises)"""
        return self._seen_counter(2)

    @property
    def seen_slots(self):
        """slots of the visited set (0 without a set)"""
        return int(self._lib.cw_seen_slots(self._h))

    def seen_insert(self, hdr, slot_pos, group=None, *, fields=None, out=None):
        """Which of these records has the visited set not held before?  (cw_seen_insert: two kernels, no host round trip, capturable with expand(); no
        env is touched.)  hdr [..., 16] / slot_pos [..., 8] as expand() takes and returns them (flattened to M): contiguous tensors on the env's device go
        over in place -- no copy, no synchronisation --, anything else is validated on the host.  Two records are the same state if they are of one GROUP
        and agree in agent, hold, both masks, the reward rule, the slot codes and the slot positions; the menu byte, step_num, flag bit 0 and the success
        count do not count (include/craftingworld.h: THE KEY).  group: None (row j is of group j % num_envs -- its env, as expand() reads it), or an int32
        tensor or integer array with the records' leading shape; a NEGATIVE entry: the row takes no part, nothing of it is written and it is not inserted.
        -> {'fresh': bool [M], 'first': int32 [M]}: first[j] is -1 if the key was in the set before this call, else the smallest participating row of
        this call with the same key (j itself for the row that brings it in); fresh[j] = (first[j] == j).  Afterwards every participating key is in the
        set.  The result does not depend on scheduling.  A row that finds no slot (seen_overflow) or meets its tag under another key (seen_collisions) is
        reported fresh and counted: the set never calls a new key seen.  fields: a subset of SEEN_FIELDS (default both).  out: a dict returned by an
        earlier call with the same M and fields, written again (rows that take no part keep what it held)."""
        names = _field_names(fields, SEEN_FIELDS, SEEN_FIELDS)
        if hdr is None or slot_pos is None:
            raise ValueError('seen_insert needs hdr and slot_pos')
        m, lead, hdr, slot_pos, _ = self._records(hdr, slot_pos, None)
        if group is not None and not self._in_place(group, (torch.int32,), lead, what='group tensor'):
            g = as_numpy(group)
            if g.dtype == np.bool_ or not np.issubdtype(g.dtype, np.integer) or tuple(g.shape) != lead:
                raise ValueError('group must be integers of the records\' leading shape %s (int32 goes over in place), got %s %s' % (lead, g.dtype, g.shape))
            if g.size and int(g.max()) >= 2 ** 31:
                raise ValueError('group must fit int32, got %d' % int(g.max()))
            group = torch.as_tensor(np.ascontiguousarray(np.maximum(g.astype(np.int64), -1), dtype=np.int32)).to(self.device)
        out = self._out_dict(out, names, {'fresh': ((m,), torch.bool), 'first': ((m,), torch.int32)})
        if m:
            self._call('cw_seen_insert', group, hdr, slot_pos, m, C.byref(_out_struct(L.cw_seen_out, out)), keep=out)
        return out

    def reach(self, max_depth, hdr=None, slot_pos=None, env_of=None, *, max_rows=2 ** 22):
        """The SHORTEST plan that ends in success, or "none within max_depth steps" -- exact, at depths plan() cannot reach: a breadth-first search over
        STATES, not action strings (expand() + seen_insert() + torch compaction).  The start states follow plan()'s rules: without records the envs'
        current states, else hdr [..., 16] / slot_pos [..., 8] / env_of (env j % num_envs or env_of[j]; a start row whose entry is negative or >= num_envs
        takes no part and reports -1).  M0 start rows.
        The engine's visited set is cleared (none reserved: seen_reserve(4 * max_rows)) and the start rows go in with group = their row number, so two
        start rows are searched apart whatever they share.  Per level: expand() of the frontier; a successor whose reward is max_steps solves its start
        row, which then leaves the search; a done successor is not expanded further (the time-out ends a branch); the rest go through seen_insert() and
        the fresh ones form the next frontier.  ONE host synchronisation per level, for the frontier's size: the call is NOT capturable.  If the next
        frontier would exceed max_rows the search stops before that level.
        -> dict: 'distance' int32 [M0], the steps of a shortest plan that ends in success, -1 for none within the searched depth; 'plan' uint8
        [max_depth, M0], that plan, zeros behind its end and for -1 rows -- it feeds simulate() as it is; 'first_action' uint8 [M0]; 'searched_depth' (an
        int <= max_depth: every plan of at most that many steps has been considered); 'states' (seen_size afterwards); 'frontier' (a list: how many states each
        level expanded).  Among equally short plans the one
        returned is fixed by the smallest-row rule of seen_insert() and of the level's scan, so two calls agree -- it is NOT promised to be plan()'s
        lexicographically smallest one.  The set is left filled: its keys are the states searched."""
        D = _shoot_int(max_depth, 'max_depth', 1, SIMULATE_MAX_STEPS)
        max_rows = _shoot_int(max_rows, 'max_rows', 1, 2 ** 27 // 6)
        m0, _, hdr, slot_pos, env_of = self._records(hdr, slot_pos, env_of)
        dev, N = self.device, self.num_envs
        if hdr is None:
            hdr, slot_pos = self.hdr, self.slot_pos
        hdr, slot_pos = hdr.reshape(m0, 16), slot_pos.reshape(m0, 8)
        rows0 = torch.arange(m0, dtype=torch.int32, device=dev)
        env0 = rows0 % N if env_of is None else env_of
        part = (env0 >= 0) & (env0 < N)
        if not self.seen_slots:
            self.seen_reserve(4 * max_rows)
        self.seen_clear()
        dist = torch.full((m0,), -1, dtype=torch.int32, device=dev)
        sol_action = torch.zeros((m0,), dtype=torch.int64, device=dev)
        sol_parent = torch.zeros((m0,), dtype=torch.int64, device=dev)
        plan = torch.zeros((D, m0), dtype=torch.uint8, device=dev)
        active = part.clone()
        if m0:
            self.seen_insert(hdr, slot_pos, torch.where(part, rows0, -1), fields=('fresh',))
        keep = torch.nonzero(part).reshape(-1)
        f_hdr, f_pos, f_env, f_start = hdr[keep].contiguous(), slot_pos[keep].contiguous(), env0[keep].contiguous(), keep
        links, sizes, searched = [], [], D
        for d in range(1, D + 1):
            F = int(f_start.numel())
            if F == 0:                              # every branch has ended: nothing deeper exists
                break
            sizes.append(F)
            r = self.expand(f_hdr, f_pos, f_env, fields=('reward', 'done', 'hdr', 'slot_pos'))
            row = torch.arange(6 * F, dtype=torch.int64, device=dev)
            parent = row % F
            start = f_start[parent]
            hit = (r['reward'].reshape(-1) == self.MAX_STEPS) & active[start]
            best = torch.full((m0,), 6 * F, dtype=torch.int64, device=dev).scatter_reduce(0, start, torch.where(hit, row, 6 * F), 'amin')
            new = best < 6 * F
            dist = torch.where(new, d, dist)
            sol_action, sol_parent = torch.where(new, best // F, sol_action), torch.where(new, best % F, sol_parent)
            active = active & ~new
            if d == D:
                break
            go = ~r['done'].reshape(-1) & active[start]
            fresh = torch.zeros((6 * F,), dtype=torch.bool, device=dev)
            s_hdr, s_pos = r['hdr'].reshape(6 * F, 16), r['slot_pos'].reshape(6 * F, 8)
            self.seen_insert(s_hdr, s_pos, torch.where(go, start, -1).to(torch.int32), fields=('fresh',), out={'fresh': fresh})
            nxt = torch.nonzero(fresh & go).reshape(-1)
            if int(nxt.numel()) > max_rows:         # (the level's one synchronisation)
                searched = d
                break
            par = parent[nxt]
            links.append((par, nxt // F))
            f_hdr, f_pos, f_env, f_start = s_hdr[nxt].contiguous(), s_pos[nxt].contiguous(), f_env[par].contiguous(), start[nxt]
        # the plans, walked back level by level: cur is a solved row's state in the frontier of the level in hand
        cur = torch.zeros((m0,), dtype=torch.int64, device=dev)
        for lvl in range(len(links) + 1, 0, -1):
            ends = dist == lvl
            a, cur = torch.where(ends, sol_action, 0), torch.where(ends, sol_parent, cur)
            if lvl <= len(links) and int(links[lvl - 1][0].numel()):
                par, act = links[lvl - 1]
                via = dist > lvl
                at = torch.where(via, cur, 0)
                a, cur = torch.where(via, act[at], a), torch.where(via, par[at], cur)
            plan[lvl - 1] = a.to(torch.uint8)
        return {'distance': dist, 'plan': plan, 'first_action': plan[0].clone(), 'searched_depth': searched, 'states': self.seen_size, 'frontier': sizes}

    def reach_reserve(self, max_rows, max_depth):
        """Allocate (or re-allocate; max_rows = 0 frees it) the workspace of reach_async() for frontiers of at most `max_rows` states -- the cap on the
        start rows of a call too -- and searches of at most `max_depth` levels (cw_reach_reserve; synchronises this engine's work): about
        315 + 4 * (max_depth - 1) bytes a row in device memory (reach_bytes).  ValueError for max_rows outside 0 .. REACH_MAX_ROWS or max_depth outside
        1 .. 32 767."""
        max_rows, max_depth = _shoot_int(max_rows, 'max_rows', 0, REACH_MAX_ROWS), _shoot_int(max_depth, 'max_depth', 1, SIMULATE_MAX_STEPS)
        self._settle()
        self._reach_ws = None
        L.check(self._lib.cw_reach_reserve(self._h, max_rows, max_depth), 'cw_reach_reserve', self._lib)
        if max_rows:
            self._reach_ws = (max_rows, max_depth)

    @property
    def reach_bytes(self):
        """bytes of reach_async()'s workspace (0 without one)"""
        return int(self._lib.cw_reach_bytes(self._h))

    def reach_async(self, max_depth, hdr=None, slot_pos=None, env_of=None, *, max_rows=None, out=None):
        """reach() as ONE library call that only enqueues kernels (cw_reach): no host round trip -- the frontier's size lives in device memory --, no
        synchronisation, capturable with the steps.  Arguments and rules are reach()'s, and with the same start rows, the same max_rows and a set that
        neither overflows nor collides every result equals reach()'s byte for byte, the choice among equally short plans included.
        -> a dict of DEVICE tensors: 'distance' int32 [M0], 'plan' uint8 [max_depth, M0], 'first_action' uint8 [M0], 'frontier' int32 [max_depth] (the
        states each level expanded, 0 for levels not run), 'searched_depth' int32 [1] and 'states' int64 [1] (a copy of seen_size made on the env's
        stream).  out: a dict returned by an earlier call with the same max_depth and M0, written again ('states' is replaced).
        The search needs the engine's visited set and a workspace (reach_reserve).  max_rows: the cap on a frontier; None: the workspace's, or 2**22
        without one.  Without a set seen_reserve(4 * max_rows) is called; without a workspace, with one of ANOTHER max_rows or with one of fewer levels
        reach_reserve(max_rows, max_depth) is.  Both reserves synchronise and allocate: RESERVE BEFORE CAPTURING, then call with max_rows=None."""
        D = _shoot_int(max_depth, 'max_depth', 1, SIMULATE_MAX_STEPS)
        ws = getattr(self, '_reach_ws', None)
        if max_rows is None:
            max_rows = ws[0] if ws else 2 ** 22
        max_rows = _shoot_int(max_rows, 'max_rows', 1, REACH_MAX_ROWS)
        m0, _, hdr, slot_pos, env_of = self._records(hdr, slot_pos, env_of)
        if m0 > max_rows:
            raise ValueError('%d start rows: at most max_rows = %d' % (m0, max_rows))
        if not self.seen_slots:
            self.seen_reserve(4 * max_rows)
        if ws is None or ws[0] != max_rows or ws[1] < D:
            self.reach_reserve(max_rows, D)
        spec = {'distance': ((m0,), torch.int32), 'plan': ((D, m0), torch.uint8), 'first_action': ((m0,), torch.uint8), 'frontier': ((D,), torch.int32),
                'searched_depth': ((1,), torch.int32)}
        if out is not None:
            out = {f: t for f, t in out.items() if f != 'states'}
        out = self._out_dict(out, REACH_FIELDS, spec)
        if m0:
            self._call('cw_reach', env_of, hdr, slot_pos, m0, D, C.byref(_out_struct(L.cw_reach_out, out)), keep=out)
        else:                                       # (no start rows, and no address to hand over: what the call would leave)
            self.seen_clear()
            out['frontier'].zero_()
            out['searched_depth'].fill_(D)
        return dict(out, states=self._seen_ctl[0:1].clone())

    # ------------------------------------------------------------------ replay of packed records
    def replay_reserve(self, steps):
        """Allocate (or re-allocate: everything stored is dropped; 0 frees it) the engine's replay buffer of `steps` slots of num_envs transitions, 106
        bytes a transition, in device memory (cw_replay_reserve; synchronises this engine's work).  steps: 0 .. 2**24 with steps * num_envs < 2**31
        (ValueError otherwise)."""
        steps = _shoot_int(steps, 'steps', 0, 2 ** 24)
        if steps * self.num_envs >= 2 ** 31:
            raise ValueError('steps * num_envs = %d must stay below 2**31' % (steps * self.num_envs))
        self._settle()
        self._replay = None
        L.check(self._lib.cw_replay_reserve(self._h, steps), 'cw_replay_reserve', self._lib)
        if steps:
            tab = L.cw_replay_table()
            L.check(self._lib.cw_replay_buffers(self._h, C.byref(tab)), 'cw_replay_buffers', self._lib)
            di, ln = self.device.index, (tab.steps, tab.num_envs)
            rec = {f: tensor_view(getattr(tab, f), ln + ((16,) if f.endswith('hdr') else (8,)), torch.uint8 if f.endswith('hdr') else torch.int16, di)
                   for f in ('hdr', 'slot_pos', 'next_hdr', 'next_slot_pos', 'goal_hdr', 'goal_slot_pos')}
            self._replay = dict(rec, action=tensor_view(tab.action, ln, torch.uint8, di), flags=tensor_view(tab.flags, ln, torch.uint8, di),
                                reward=tensor_view(tab.reward, ln, torch.int32, di), episode=tensor_view(tab.episode, ln, torch.int32, di),
                                env_episode=tensor_view(tab.env_episode, ln[1:], torch.int32, di), n=tensor_view(tab.n, (1,), torch.int64, di))

    def replay_bytes(self):
        """bytes of the replay buffer (0 without one)"""
        return int(self._lib.cw_replay_bytes(self._h))

    def replay_clear(self):
        """Forget every stored transition: n = 0, every env's episode number 0 (cw_replay_clear: one kernel, capturable)."""
        self._call('cw_replay_clear', sync=False)

    def replay_size(self):
        """n, the pushes since the last clear (0 without a buffer; reading it synchronises).  min(n, steps) positions are stored."""
        view = getattr(self, '_replay', None)
        return 0 if view is None else int(view['n'].item())

    def replay_view(self):
        """The buffer as zero-copy device tensors, READ-ONLY and valid until the next replay_reserve(): 'hdr' uint8 [L, N, 16] / 'slot_pos' int16 [L, N, 8]
        (the state s), 'next_hdr' / 'next_slot_pos' (s'), 'goal_hdr' / 'goal_slot_pos' (the goal record), 'action' uint8 [L, N] (255: outside 0..5),
        'flags' uint8 [L, N] (bit 0 changed, bit 1 done), 'reward' int32 [L, N], 'episode' int32 [L, N] (the bit pattern of a uint32), 'env_episode'
        int32 [N] and 'n' int64 [1].  Position k lives in slot k % L.  CraftingWorldError without a buffer."""
        view = getattr(self, '_replay', None)
        if view is None:
            raise L.CraftingWorldError('no replay buffer reserved (replay_reserve)')
        return dict(view)

    def replay_push(self, actions):
        """Store the transition every env is ABOUT to make: call it BEFORE step() / step_async() with the same actions (the same argument handling).  One
        lane per env reads its state, applies the pure step as expand() does, and writes (s, s', the goal record, action, flags, reward, episode) into
        slot n % L; n advances on the device (cw_replay_push: two kernels, no host round trip, capturable with the step; nothing of the engine but the
        buffer is written).  An action outside 0..5 is stored as 255.  The episode number goes up whenever the previous transition of the env was done or
        its s' is not this push's s byte for byte -- an auto-reset, reset_envs, load_records, snapshot_load, imagine_obs(commit=True) in between.
        step_many() and rollout() are not recorded."""
        a, dt = self._actions(actions)
        self._call('cw_replay_push', a, dt, sync=False)

    def replay_sample(self, batch, seed=0, *, her=0.0, strategy='future', fields=None, out=None):
        """A minibatch of `batch` rows drawn uniformly from the stored transitions, a fraction of them relabelled in hindsight (cw_replay_sample: one
        kernel, exact integer arithmetic, no host round trip, capturable; nothing but the outputs is written; include/craftingworld.h states every rule).
        seed: an int 0 .. 2**64 - 1 or a device word, as shoot() takes it.  her: a float in [0, 1], the probability that a row is relabelled; it goes
        over as round(her * 65536) and a row is relabelled iff a 16-bit draw lies below that (0.0 never, 1.0 always).  strategy: 'future' -- the new goal
        is the achieved mask after a uniformly drawn step of the same episode from the row's own on -- or 'final', after the episode's last stored step.
        -> a dict of device tensors, rows [B]: 'hdr' uint8 [B, 16] / 'slot_pos' int16 [B, 8] (s), 'next_hdr' / 'next_slot_pos' (s'), 'goal_hdr' /
        'goal_slot_pos' (the goal as a record), 'action' uint8, 'reward' int32, 'done' bool, 'desired' int16 (the goal mask the row is judged by), 'env',
        'slot' and 'future' int32 (-1: not relabelled) for gathering side data kept in [L, N] tensors.  In a relabelled row the desired bytes of the
        records, reward and done are those under the new goal.  fields: a subset of REPLAY_FIELDS (default all).  out: a dict returned by an earlier call
        with the same batch and fields, written again.  With an empty buffer no row is written.  The frames of a sample:
            obs      = env.render_records(r['hdr'], r['slot_pos'])
            next_obs = env.render_records(r['next_hdr'], r['next_slot_pos'])
            goal     = env.render_records(r['goal_hdr'], r['goal_slot_pos'])"""
        names = _field_names(fields, REPLAY_FIELDS, REPLAY_FIELDS)
        b = _shoot_int(batch, 'batch', 0, 2 ** 27)
        if type(her) is bool or not isinstance(her, (int, float, np.integer, np.floating)) or not 0.0 <= her <= 1.0:
            raise ValueError('her must be a number in [0, 1], got %r' % (her,))
        if strategy not in REPLAY_STRATEGIES:
            raise ValueError('strategy must be one of %s, got %r' % (REPLAY_STRATEGIES, strategy))
        seed, seed_dev = self._shoot_seed(seed)
        spec = {f: ((b, 16), torch.uint8) if f.endswith('hdr') else ((b, 8), torch.int16) if f.endswith('slot_pos') else
                ((b,), {'action': torch.uint8, 'done': torch.bool, 'desired': torch.int16}.get(f, torch.int32)) for f in REPLAY_FIELDS}
        out = self._out_dict(out, names, spec)
        if b:
            self._call('cw_replay_sample', b, seed, seed_dev, int(round(float(her) * 65536)), REPLAY_STRATEGIES.index(strategy),
                       C.byref(_out_struct(L.cw_replay_out, out)), sync=False, keep=out)
        return out

    def step_async(self, actions):
        # the per-step path: a device tensor of the right shape goes to cw_step with nothing built on the way (pointer and stream as plain ints)
        if type(actions) is torch.Tensor and actions.is_cuda:
            dt = _ACT_DTYPES.get(actions.dtype)
            if dt is not None and actions.numel() == self.num_envs and actions.is_contiguous() and actions.device == self.device:
                self._actions_keepalive = actions
                rc = self._cw_step(self._h, actions.data_ptr(), dt, self._raw_stream(self._di))
                if rc:
                    L.check(rc, 'cw_step', self._lib)
                self._pending = True
                return
        actions, dt = self._actions(actions)
        if type(actions) is torch.Tensor:
            self._actions_keepalive = actions
            actions = C.c_void_p(actions.data_ptr())
        L.check(self._lib.cw_step(self._h, actions, dt, self._stream()), 'cw_step', self._lib)
        self._pending = True

    def _actions(self, actions):
        """actions as step_async takes them -> (what cw_step / cw_replay_push is handed, its CW_ACT_* dtype): a contiguous tensor of num_envs actions on the
        env's device, or -- a host_outputs engine given host actions -- the engine's mapped buffer, filled, as a pointer"""
        if self.host_outputs and not (torch.is_tensor(actions) and actions.is_cuda):
            a = np.asarray(actions).reshape(-1)             # host actions go through the engine's mapped buffer
            if a.size != self.num_envs:
                raise ValueError('expected %d actions, got %d' % (self.num_envs, a.size))
            self._host_actions[:] = a
            if a.dtype != np.int32:                          # (a wider value must not wrap into 0..5: every one outside it is the counted no-op)
                self._host_actions[(a < 0) | (a > 5)] = -1
            return C.c_void_p(self._host_actions.ctypes.data), L.CW_ACT_I32
        if not torch.is_tensor(actions):
            actions = torch.as_tensor(np.asarray(actions), device=self.device)
        if actions.device != self.device:
            actions = actions.to(self.device)
        if actions.dtype not in _ACT_DTYPES:
            actions = actions.to(torch.int32)
        actions = actions.contiguous()
        if actions.numel() != self.num_envs:
            raise ValueError('expected %d actions, got %d' % (self.num_envs, actions.numel()))
        return actions, _ACT_DTYPES[actions.dtype]

    def step_wait(self):
        if not self._pending:
            raise RuntimeError('step_wait without step_async')
        self._pending = False
        if self.host_outputs:
            self._sync()
        # 'episode': the finished episode's statistics the way gym's RecordEpisodeStatistics reports them (r: return = the sum of its rewards,
        # ray.py:361-367; l: length), as device tensors, rows valid where done (SURVEY 5 "metrics")
        info = {'task_success': self.achieved_mask, 'desired_goal': self.desired_mask,
                'achieved_goal': self.achieved_mask, 'episode_length': self.episode_length,
                'episode': {'r': self.episode_return, 'l': self.episode_length}}
        if self.terminal_observation is not None:
            info['terminal_observation'] = self.terminal_observation     # rows valid where done
        return self._observation(), self.reward, self.done, info

    def step(self, actions):
        """-> (obs, reward int32[N], done bool[N], info); all device tensors, results are ordered on the
        current torch stream (no host sync).  Finished envs are already reset: obs rows of done
        envs show the first frame of the new episode; info masks are the terminal ones."""
        self.step_async(actions)
        return self.step_wait()

    def step_many(self, actions):
        """K consecutive steps from a device tensor `actions` [K, N] (uint8 / int32 / int64): exactly what K calls of step_async enqueue, in ONE
        library call -- a Python loop costs more per step than a state-only step takes on the card.  Nothing is returned: read the usual
        views (reward, done, the observation tensors: the last step's) afterwards.  Auto-reset as in step()."""
        if not (type(actions) is torch.Tensor and actions.dtype in _ACT_DTYPES and actions.device == self.device and actions.is_contiguous()
                and actions.dim() == 2 and actions.shape[1] == self.num_envs):
            raise ValueError('actions must be a contiguous [K, num_envs] tensor of dtype uint8 / int32 / int64 on %s' % (self.device,))
        self._call('cw_step_many', actions, _ACT_DTYPES[actions.dtype], int(actions.shape[0]), sync=False)

    def capture_steps(self, actions):
        """-> a torch.cuda.CUDAGraph that takes K = actions.shape[0] steps per replay(), reading row t of the device tensor `actions` [K, N] on
        step t: fill the tensor IN PLACE (the ring a policy or an action sampler writes into), call graph.replay(), read the views.  One graph
        launch per K steps instead of K library calls: the way to run the launch-bound modes (state-only, dirty-cell frames) at the card's pace
        rather than the host's.  The envs' episode bookkeeping needs nothing from the host, so replays can be queued back to back.
        Capturing takes NO step: nothing runs until the first replay() (cw_step_many allocates nothing and launches nothing lazily, so torch's
        eager warm-up pass is not needed -- it would advance every env by K steps on whatever the tensor holds at that moment)."""
        self.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self.step_many(actions)
        return graph

    def rollout(self, actions, record=True):
        """T consecutive steps (auto-reset included) in ONE persistent kernel launch, for action streams
        known up front: actions uint8 [T, N] on the device (any other dtype is converted: values outside 0..5 become 255, the counted no-op
        they are in step()).  Bit-identical to T calls of step().
        State-only observation mode.  -> (rewards int32 [T,N], dones bool [T,N]) if record."""
        if not torch.is_tensor(actions):
            actions = torch.as_tensor(np.asarray(actions), device=self.device)
        actions = actions.to(device=self.device)
        if actions.dtype != torch.uint8:
            if actions.dtype not in _ACT_DTYPES:
                actions = actions.to(torch.int32)            # (as step_async converts it)
            invalid = (actions < 0) | (actions > 5)          # (a plain cast wraps modulo 256: 258 would run as Down)
            actions = actions.to(torch.uint8).masked_fill_(invalid, 255)
        actions = actions.contiguous()
        if actions.dim() != 2 or actions.shape[1] != self.num_envs:
            raise ValueError('actions must have shape [T, num_envs]')
        T = actions.shape[0]
        rew = torch.empty((T, self.num_envs), dtype=torch.int32, device=self.device) if record else None
        don = torch.empty((T, self.num_envs), dtype=torch.uint8, device=self.device) if record else None
        self._call('cw_rollout', actions, T, _vp(rew), _vp(don), sync=False)      # (the results are the caller's alone)
        return (rew, don.view(torch.bool)) if record else None

    # ------------------------------------------------------------------ views / checkpoints
    def render(self, out=None):
        """render() of ray.py:442-520 for every env -> uint8 [N,4S,4S,3] (works in every obs_mode)."""
        if out is None:
            out = torch.empty((self.num_envs,) + self.frame_shape, dtype=torch.uint8, device=self.device)
        self._call('cw_render', _vp(out), sync=False)
        return out

    def render_exact(self):
        """The reference's INT image of every env's current state, exactly: int16 [N, ...frame_shape].  The uint8 frames of the engine hold it
        modulo 256, which differs in ONE reachable pixel of the AltObs raster (sticks held over a sticks cell: (90, 164, 320),
        craftingworld_altobs.py:527-543) and nowhere in the Ray raster; this is the batch counterpart of the N=1 classes' reference_dtypes=True.
        Two kernels (cw_export_onehot, cw_render_onehot): a side view for checks and logging, not a per-step observation."""
        return self.render_states(self.one_hot())

    def render_states(self, one_hot):
        """render(state) of ray.py:442-486 for caller-supplied one-hot states [M,S,S,12] of any content (several objects in a
        cell, any number of objects): -> int16 tensor [M,4S,4S,3] holding the reference's int image (sums of colours; the
        agent is the first cell with channel 8 set and must exist).  raster='alt': CraftingWorldEnvAltObs.render(state)
        (craftingworld_altobs.py:489-560), [M,3S+3,3S,3].  Does not touch the envs."""
        oh = torch.as_tensor(np.asarray(one_hot) if not torch.is_tensor(one_hot) else one_hot)
        oh = oh.to(device=self.device, dtype=torch.uint8).contiguous()
        if oh.dim() != 4 or tuple(oh.shape[1:]) != (self.size, self.size, 12):
            raise ValueError('states must have shape [M, %d, %d, 12]' % (self.size, self.size))
        out = torch.empty((oh.shape[0],) + self.frame_shape, dtype=torch.int16, device=self.device)
        self._call('cw_render_onehot', oh, oh.shape[0], _vp(out), sync=False)
        return out

    def grid(self, out=None):
        """Dense cell codes uint8 [N,S,S] (0 empty, k+1 = OBJECTS[k])."""
        if out is None:
            out = torch.empty((self.num_envs, self.size, self.size), dtype=torch.uint8, device=self.device)
        self._call('cw_export_grid', _vp(out), sync=False)
        return out

    def one_hot(self, out=None, which='current'):
        """obs_one_hot of ray.py:119 for every env: uint8 [N,S,S,12].  which='goal' / 'init' give the episode's goal state
        and its state at reset -- CraftingWorldEnvOneHot's desired_goal and init_observation (onehot.py:310, :203)."""
        if out is None:
            out = torch.empty((self.num_envs, self.size, self.size, 12), dtype=torch.uint8, device=self.device)
        w = {'current': 0, 'goal': 1, 'init': 2}[which]
        self._call('cw_export_onehot_of', w, _vp(out), sync=False)
        return out

    def mask_to_vector(self, mask):
        """int16 bit mask [N] -> 0/1 tensor [N, len(task_list)] (achieved_goal_vector layout, ray.py:114)."""
        bits = torch.arange(len(self.task_list), device=mask.device, dtype=torch.int32)
        return ((mask.to(torch.int32).unsqueeze(1) >> bits) & 1).to(torch.uint8)

    def fixed_states(self):
        """generate_fixed_states' pool (ray.py:116-118, 149-154: fixed_state_list) as cell indices: uint16 [N, K, 9] = the cells (row * S + col)
        of objects 0..7 (OBJECTS order) and of the agent in each of the K pooled placements of every env.  ValueError when fixed_init_state == 0."""
        out = np.empty((self.num_envs, max(self.fixed_init_state, 1), 9), dtype=np.uint16)
        self._settle()
        L.check(self._lib.cw_get_fixed_states(self._h, out.ctypes.data_as(C.c_void_p)), 'cw_get_fixed_states', self._lib)
        return out

    def get_state(self):
        """Host snapshot (numpy) of every env: the de-facto checkpoint."""
        N, S = self.num_envs, self.size
        out = dict(grid=np.empty((N, S, S), np.uint8), init_grid=np.empty((N, S, S), np.uint8),
                   goal_grid=np.empty((N, S, S), np.uint8), agent_rc=np.empty((N, 2), np.uint8),
                   init_agent_rc=np.empty((N, 2), np.uint8), goal_agent_rc=np.empty((N, 2), np.uint8),
                   hold=np.empty(N, np.uint8), achieved=np.empty(N, np.uint16), desired=np.empty(N, np.uint16),
                   step_num=np.empty(N, np.int32), ep_no=np.empty(N, np.int32))
        view = L.cw_state_view(**{k: a.ctypes.data_as(C.c_void_p) for k, a in out.items()})
        self._settle()
        L.check(self._lib.cw_get_state(self._h, C.byref(view)), 'cw_get_state', self._lib)
        return out

    def set_state(self, **fields):
        """Overwrite state from numpy arrays: any subset of get_state()'s fields (grid, init_grid, goal_grid, agent_rc,
        init_agent_rc, goal_agent_rc, hold, achieved, desired, step_num, ep_no); with a goal / init-agent field given,
        all three frames are repainted from the restored states."""
        dt = dict(grid=np.uint8, init_grid=np.uint8, goal_grid=np.uint8, agent_rc=np.uint8, init_agent_rc=np.uint8,
                  goal_agent_rc=np.uint8, hold=np.uint8, achieved=np.uint16, desired=np.uint16, step_num=np.int32,
                  ep_no=np.int32)
        keep = {}
        view = L.cw_state_view()
        for k, a in fields.items():
            if k not in dt:
                raise ValueError('cannot set %r' % k)
            keep[k] = np.ascontiguousarray(a, dtype=dt[k])
            if keep[k].shape[0] != self.num_envs:
                raise ValueError('%s must have num_envs rows' % k)
            setattr(view, k, keep[k].ctypes.data_as(C.c_void_p))
        self._settle()
        L.check(self._lib.cw_set_state(self._h, C.byref(view)), 'cw_set_state', self._lib)

    # ------------------------------------------------------------------ checkpoint / resume
    def save_checkpoint(self, path):
        """Everything the env batch needs to continue bit-identically, as one file written exactly at `path`: the engine's
        raw records (current state, the episode's goal and start states, RNG streams, fixed_init_state pools, the last
        step's outputs, counters) behind a header that pins the configuration (cw_checkpoint_save; synchronises)."""
        n = int(self._lib.cw_checkpoint_bytes(self._h))
        buf = np.empty(n, dtype=np.uint8)
        self._settle()
        L.check(self._lib.cw_checkpoint_save(self._h, buf.ctypes.data_as(C.c_void_p), n), 'cw_checkpoint_save', self._lib)
        with open(path, 'wb') as f:
            buf.tofile(f)

    def load_checkpoint(self, path):
        """Restore a save_checkpoint() file into an engine built with the same configuration (num_envs, size, max_steps,
        task_list, fixed_init_state and task menus are verified: ValueError otherwise).  Records are restored verbatim, so
        the state-mode observation tensors (hdr, slot_pos) equal the uninterrupted run's too; frames are repainted.  Per-env
        menu ids, reward rules, pools and counters come from the file."""
        buf = np.fromfile(path, dtype=np.uint8)
        self._settle()
        L.check(self._lib.cw_checkpoint_load(self._h, buf.ctypes.data_as(C.c_void_p), buf.size), 'cw_checkpoint_load', self._lib)
        self._has_reset = True

    def profile_begin(self, max_steps):
        """Bracket each kernel of the following step() calls with HIP events on the launch stream."""
        L.check(self._lib.cw_profile_begin(self._h, int(max_steps)), 'cw_profile_begin', self._lib)

    def render_kernel_name(self):
        """Name of the kernel `profile_end()['ms_render_kernel']` brackets (as a rocprofv3 kernel trace lists it)."""
        return (self._lib.cw_render_kernel_name(self._h) or b'').decode()

    def profile_end(self):
        """-> dict of average per-launch kernel durations (ms) since profile_begin."""
        p = L.cw_profile()
        L.check(self._lib.cw_profile_end(self._h, C.byref(p)), 'cw_profile_end', self._lib)
        return {k: getattr(p, k) for k, _ in p._fields_}

    def tuner_state(self):
        """What the engine's tuning holds right now (full-frame mode; performance only): dict with `period16` (the period of the sweep's clock in
        1/16 of a 10-ns tick, 0: unclocked; `period16_head`: of a launch's first 64 jobs, `period16_busy`: of those after a step on which envs finished), `lookahead` (1: the outcome of every env's next reset() is computed ahead of time), `resident` (1: the
        N=1 doorbell stepper is available) and `guard_slowdowns` (how often the clock's guard has lowered the rate; -1: no guard)."""
        t = L.cw_tuner_state()
        L.check(self._lib.cw_tuner(self._h, C.byref(t)), 'cw_tuner', self._lib)
        return {k: int(getattr(t, k)) for k, _ in t._fields_}

    def compute_reward_batch(self, achieved_mask, desired_mask, subset=None):
        """Vectorised compute_reward_equal / compute_reward_subset (ray.py:757-767) on bit masks, for
        HER-style relabelling on the device: int tensors of any shape -> int32 rewards (MAX_STEPS or -1).
        subset=None uses menu 0's reward_style."""
        full = (1 << len(self.task_list)) - 1
        a = achieved_mask.to(torch.int32) & full
        d = desired_mask.to(torch.int32) & full
        if subset is None:
            subset = bool(self._menus[0].reward_subset)
        if subset:      # np.max(desired - achieved) == 0: nothing missing and at least one position equal
            hit = ((d & ~a) == 0) & (((~(d ^ a)) & full) != 0)
        else:
            hit = a == d
        return torch.where(hit, torch.full_like(a, self.MAX_STEPS), torch.full_like(a, -1))

    def compute_reward(self, achieved_goal, desired_goal, info=None):
        """compute_reward_equal / compute_reward_subset of ray.py:757-767 on 0/1 goal vectors
        (host convenience for HER-style relabelling; the per-step reward comes from the kernel)."""
        a = np.asarray(achieved_goal).reshape(-1)
        d = np.asarray(desired_goal).reshape(-1)
        if self._menus[0].reward_subset:
            return self.MAX_STEPS if np.max(d.astype(np.int64) - a.astype(np.int64)) == 0 else -1
        return self.MAX_STEPS if np.array_equal(a, d) else -1
