"""What "a seen_insert call did exactly what it should" means for cw_seen_insert, and what reach() must find, said once.  key_of() is the key of a packed
record in numpy (include/craftingworld.h: THE KEY); SeenModel is the visited set as a Python set of those keys; check_seen_call() compares what a call wrote
with the model: every participating row, every row that must not be written against the sentinel the test pre-filled, the set's counters, and the engine
before and after the call (masked_check.take() snapshots: nothing may have changed).  A row may deviate from the model ONLY in the safe direction -- reported
fresh where the model knows its key -- and only as often as the overflow and collision counters grew; a key the model has never seen is never reported as seen
or as a duplicate, whatever the counters did.  reference_reach() is the breadth-first search over records_check.oracle_simulate with T = 1 and a Python set on
key_of, brute_reach() the best of all 6^D action strings; oracle_starts() the start states the reach tests share.  Pure CPU: numpy arrays in, no GPU.  A plain
module, not a fixture; tests/test_seen_logic.py tests the comparison itself."""
import functools

import numpy as np

from oracle_replay import same
from records_check import DENSE, encode, oracle_simulate

KEY_WORDS = 9
SIZE, OVERFLOW, COLLISIONS = 0, 1, 2


def key_of(hdr, slot_pos, group):
    """the keys of M packed records hdr uint8 [M, 16] / slot_pos (u)int16 [M, 8] in the groups `group` [M] -> uint32 [M, 9]: group, hdr bytes 0-2, hdr bytes
    4-7, bit 1 of hdr byte 10, hdr bytes 12-15, the four dwords of slot_pos.  Not in it: hdr byte 3 (menu), bytes 8-9 (step_num), flag bit 0, flag bits 2-15."""
    h = np.ascontiguousarray(hdr, dtype=np.uint8).reshape(-1, 16).astype(np.uint32)
    p = np.ascontiguousarray(np.ascontiguousarray(slot_pos).reshape(-1, 8).view(np.uint16)).view(np.uint32).reshape(-1, 4)
    g = np.asarray(group).reshape(-1).astype(np.int64)
    if not (len(h) == len(p) == len(g)):
        raise ValueError('%d headers, %d slot records, %d groups' % (len(h), len(p), len(g)))
    le = lambda b: h[:, b] | (h[:, b + 1] << 8) | (h[:, b + 2] << 16) | (h[:, b + 3] << 24)  # noqa: E731
    key = np.empty((len(h), KEY_WORDS), np.uint32)
    key[:, 0] = (g & 0xFFFFFFFF).astype(np.uint32)
    key[:, 1] = h[:, 0] | (h[:, 1] << 8) | (h[:, 2] << 16)
    key[:, 2] = le(4)
    key[:, 3] = (h[:, 10] >> 1) & 1
    key[:, 4] = le(12)
    key[:, 5:9] = p
    return key


def groups_of(group, M, N):
    """the group of every row as the call reads it: `group` [M], or row j % N without one -> int64 [M] (negative: the row takes no part)"""
    if group is None:
        return np.arange(M, dtype=np.int64) % N
    g = np.asarray(group).reshape(-1).astype(np.int64)
    if len(g) != M:
        raise ValueError('%d group entries for %d rows' % (len(g), M))
    return g


class SeenModel:
    """the visited set as a Python set of key bytes"""

    def __init__(self):
        self.keys = set()

    def clear(self):
        self.keys.clear()

    def __len__(self):
        return len(self.keys)

    def insert(self, keys, part):
        """keys uint32 [M, 9], part bool [M] -> (fresh bool [M], first int64 [M]) of the participating rows (the others: False, -2); every participating
        key is in the set afterwards"""
        M = len(keys)
        fresh, first = np.zeros(M, bool), np.full(M, -2, np.int64)
        mine = {}
        for j in np.flatnonzero(part):
            k = keys[j].tobytes()
            if k in self.keys:
                first[j] = -1
            else:
                first[j] = mine.setdefault(k, j)
                fresh[j] = first[j] == j
        self.keys.update(mine)
        return fresh, first


def check_seen_call(model, inputs, outputs, sentinel, counters_before, counters_after, engine_before, engine_after, *, exact=False):
    """Pure CPU.  cw_seen_insert ran once.  model: the SeenModel of every call since the last clear, this one not yet in it -- it is inserted here.
    inputs: dict(hdr [M, 16], slot_pos [M, 8], group [M] or None, num_envs); outputs: {'fresh': [M], 'first': [M]} (either or both) as the call left the
    buffers it was given, every byte of which held `sentinel` before; counters_before / counters_after: the set's three counters (keys held, overflow,
    collisions) around the call; engine_before / engine_after: masked_check.take() snapshots (None, None: not compared).
    Every row that takes no part still holds the sentinel.  Every participating row equals the model, or DEVIATES as (fresh = 1, first = j) where the model
    says otherwise; the number of deviating rows is at most the growth of overflow + collisions (a condition, not a tolerance), neither counter shrinks, and
    keys held lies between the model's size minus overflow + collisions (since the last clear) and the model's size.  exact=True (64-bit tags, enough capacity): both counters stay 0 and
    nothing deviates.  The engine is unchanged, its counters included.  ValueError when no row takes part.  -> the number of deviating rows."""
    if not outputs or set(outputs) - {'fresh', 'first'}:
        raise ValueError('outputs must hold fresh, first or both')
    hdr = np.asarray(inputs['hdr']).reshape(-1, 16)
    M = len(hdr)
    g = groups_of(inputs.get('group'), M, int(inputs['num_envs']))
    part = g >= 0
    if not part.any():
        raise ValueError('no row takes part: nothing would be compared with the model')
    want_fresh, want_first = model.insert(key_of(hdr, inputs['slot_pos'], np.where(part, g, 0)), part)
    rows, rest = np.flatnonzero(part), np.flatnonzero(~part)
    outputs = {f: np.asarray(a).reshape(-1) for f, a in outputs.items()}
    for f, a in outputs.items():
        if len(a) != M:
            raise ValueError('%s holds %d rows, the call read %d' % (f, len(a), M))
        raw = np.ascontiguousarray(a[rest]).view(np.uint8)
        same('%s of the rows that must not be written' % f, rest, raw.reshape(len(rest), a.itemsize), np.full((len(rest), a.itemsize), sentinel, np.uint8))
    off = np.zeros(M, bool)
    if 'first' in outputs:
        got = outputs['first'].astype(np.int64)
        off |= part & (got != want_first)
        bad = np.flatnonzero(off & (got != np.arange(M)))
        assert len(bad) == 0, 'first differs from the model other than as "fresh" at %d rows, first %s: got %s, the model %s' % (
            len(bad), bad[:8].tolist(), got[bad[:8]].tolist(), want_first[bad[:8]].tolist())
    if 'fresh' in outputs:
        got = outputs['fresh'].astype(np.uint8)
        assert set(np.unique(got[rows]).tolist()) <= {0, 1}, 'fresh holds other bytes than 0 / 1'
        diff = part & (got != want_fresh.astype(np.uint8))
        bad = np.flatnonzero(diff & (got != 1))
        assert len(bad) == 0, 'a key the model has never seen is reported as seen at %d rows, first %s' % (len(bad), bad[:8].tolist())
        off |= diff
    if 'first' in outputs and 'fresh' in outputs:
        same('fresh == (first == row)', rows, outputs['fresh'][rows].astype(np.int64), (outputs['first'][rows].astype(np.int64) == rows).astype(np.int64))
    c0, c1 = np.asarray(counters_before).astype(np.int64), np.asarray(counters_after).astype(np.int64)
    grown = (c1[OVERFLOW] - c0[OVERFLOW]) + (c1[COLLISIONS] - c0[COLLISIONS])
    assert c1[OVERFLOW] >= c0[OVERFLOW] and c1[COLLISIONS] >= c0[COLLISIONS], 'a counter shrank: %s -> %s' % (c0.tolist(), c1.tolist())
    n_off = int(off.sum())
    assert n_off <= grown, '%d rows deviate from the model, overflow + collisions grew by %d (first rows %s)' % (n_off, grown, np.flatnonzero(off)[:8].tolist())
    lost = c1[OVERFLOW] + c1[COLLISIONS]                # (since the last clear: each such row is one key the set may not hold)
    assert len(model) - lost <= c1[SIZE] <= len(model), 'the set holds %d keys, the model %d (overflow + collisions since the clear: %d)' % (c1[SIZE], len(model), lost)
    if exact:
        assert c1[OVERFLOW] == 0 and c1[COLLISIONS] == 0 and n_off == 0, 'overflow %d, collisions %d, %d rows deviate' % (c1[OVERFLOW], c1[COLLISIONS], n_off)
        assert c1[SIZE] == len(model), (c1[SIZE], len(model))
    if engine_before is not None or engine_after is not None:
        if set(engine_before) != set(engine_after):
            raise ValueError('the snapshots hold different entries: %s' % sorted(set(engine_before) ^ set(engine_after)))
        for k in sorted(engine_before):
            same('after cw_seen_insert: %s' % k, 0, engine_after[k], engine_before[k])
    return n_off


# ------------------------------------------------------------------------------------------------------------------------------ reach
def _tile6(states, init_grids):
    """every state six times, action-major like cw_expand: row a * F + i is action a on state i"""
    tiled = {k: np.tile(np.asarray(states[k]), (6,) + (1,) * (np.asarray(states[k]).ndim - 1)) for k in DENSE}
    return tiled, np.tile(np.asarray(init_grids), (6, 1, 1))


def reference_reach(states, init_grids, max_depth, oracle_kw, max_rows=None):
    """M0 dense start states (records_check.decode()'s fields; init_grids uint8 [M0, S, S]) -> dict: distance int64 [M0] (the steps of a shortest action
    string that ends in success, -1: none within the searched depth), searched_depth, frontier (the sizes of the frontiers expanded, level by level) and
    states (distinct keys met).  Breadth-first over oracle_simulate with T = 1: a successor that pays max_steps solves its start row, which then leaves the
    search; a done successor is not expanded; the rest are merged by key_of of their canonical encoding (records_check.encode) in the group of their start
    row.  max_rows: stop before a level whose frontier would exceed it, as reach() does."""
    M0 = len(states['hold'])
    max_steps = int(oracle_kw['max_steps'])
    dist = np.full(M0, -1, np.int64)
    front = {k: np.asarray(states[k]) for k in DENSE}
    start = np.arange(M0, dtype=np.int64)
    h, p = encode(front)
    seen = set(k.tobytes() for k in key_of(h, p, start))
    sizes, searched = [], max_depth
    for d in range(1, max_depth + 1):
        F = len(start)
        if F == 0:
            break
        sizes.append(F)
        tiled, inits = _tile6(front, np.asarray(init_grids)[start])
        r = oracle_simulate(tiled, inits, np.repeat(np.arange(6), F)[None, :], True, oracle_kw)
        st6 = np.tile(start, 6)
        for j in np.flatnonzero(r['rewards'][0] == max_steps):
            if dist[st6[j]] < 0:
                dist[st6[j]] = d
        if d == max_depth:
            break
        go = np.flatnonzero(~r['dones'][0] & (dist[st6] < 0))
        h, p = encode({k: r[k][go] for k in DENSE})
        keys = key_of(h, p, st6[go])
        nxt = []
        for i, j in enumerate(go):
            k = keys[i].tobytes()
            if k not in seen:
                seen.add(k)
                nxt.append(j)
        if max_rows is not None and len(nxt) > max_rows:
            searched = d
            break
        nxt = np.array(nxt, np.int64)
        front, start = {k: r[k][nxt] for k in DENSE}, st6[nxt]
    return dict(distance=dist, searched_depth=searched, frontier=sizes, states=len(seen))


def brute_reach(states, init_grids, max_depth, oracle_kw):
    """distance [M0] by brute force: every one of the 6^D action strings of every start state through oracle_simulate(stop_at_done=True); a string that ends
    by success after L steps returns max_steps - (L - 1), so the best return names the shortest one.  -1: none within max_depth."""
    from plan_check import strings
    M0 = len(states['hold'])
    max_steps = int(oracle_kw['max_steps'])
    n = 6 ** max_depth
    tiled = {k: np.tile(np.asarray(states[k]), (n,) + (1,) * (np.asarray(states[k]).ndim - 1)) for k in DENSE}
    r = oracle_simulate(tiled, np.tile(np.asarray(init_grids), (n, 1, 1)), np.repeat(strings(max_depth), M0, axis=1), True, oracle_kw)
    ok = (r['n_success'] > 0).reshape(n, M0)
    length = np.where(ok, r['length'].reshape(n, M0), max_depth + 1).min(axis=0)
    assert ((r['ret'].reshape(n, M0)[ok]) == (max_steps - (r['length'].reshape(n, M0)[ok] - 1))).all()
    return np.where(length <= max_depth, length, -1)


REACH_SEEDS = {5: (4004, 4000, 4005, 4001, 4017, 4002, 4020, 4003, 4029, 4006, 4117, 4007),       # grid size -> the RandomState seeds of the start rows
               8: (4013, 4000, 4017, 4001, 4029, 4002, 4044, 4003, 4117, 4006, 4007, 4008)}       # (tests/test_seen_logic.py holds what the oracle says of them)
REACH_N = 12
REACH_MAX_STEPS = 40


def seed_states(seeds):
    """numpy RandomState(seed)'s (key, pos) for every seed: what oracle_replay.make_env injects"""
    sts = [np.random.RandomState(int(s)).get_state() for s in seeds]
    return np.stack([s[1] for s in sts]).astype(np.uint32), np.array([s[2] for s in sts], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def oracle_starts(seeds, size, max_steps):
    """one oracle env per seed, RandomState(seed), after reset() -> (dense states [n], init grids [n, S, S]): what an engine whose streams are
    seed_states(seeds) holds after reset().  flags: bit 0, no step taken yet."""
    from oracle import OracleEnv
    st = []
    for seed in seeds:
        s0 = np.random.RandomState(int(seed)).get_state()
        o = OracleEnv(rng_state=(s0[1].astype(np.uint32), int(s0[2])), size=(size, size), max_steps=max_steps)
        o.reset()
        st.append(o.state())
    n = len(st)
    dense = dict(grid=np.stack([s['grid'] for s in st]), agent=np.array([s['agent'] for s in st], np.int64), hold=np.array([s['hold'] for s in st], np.int64),
                 achieved=np.array([s['achieved'] for s in st], np.int64), desired=np.array([s['desired'] for s in st], np.int64),
                 step_num=np.array([s['step_num'] for s in st], np.int64), flags=np.full(n, 1, np.int64))
    return dense, np.stack([s['init_grid'] for s in st])


@functools.lru_cache(maxsize=None)
def reach_reference(size, depth):
    """(dense start states, init grids, reference_reach of them) of the REACH_N start rows at `size`: computed once, shared, left unchanged"""
    dense, inits = oracle_starts(REACH_SEEDS[size], size, REACH_MAX_STEPS)
    return dense, inits, reference_reach(dense, inits, depth, dict(size=(size, size), max_steps=REACH_MAX_STEPS))
