"""What "an expand call did exactly what it should" means for cw_expand, in one place.  decode() turns packed records into dense numpy, oracle_successors()
gives the six successors of dense states by OracleEnv.set_state + step and nothing else, and check_expand() compares what a call wrote with them: EVERY
written row against the oracle, every row that must not be written against the sentinel the test pre-filled, and the engine before and after the call
(masked_check.take() snapshots): nothing may have changed but counters[7], which counts the skipped states.  Pure CPU: numpy arrays in, no GPU.  A plain
module, not a fixture; tests/test_expand_logic.py tests the comparison itself.  encode() is the test-side inverse of decode()."""
import numpy as np

from oracle_replay import same

FIELDS = ('reward', 'done', 'changed', 'achieved_mask', 'hdr', 'slot_pos')
SKIPPED = 7                                     # counters[7]: states skipped for an env index at or above num_envs
POS_GONE, POS_HELD = 0xFFFF, 0xFFFE
DENSE = ('grid', 'agent', 'hold', 'achieved', 'desired', 'step_num', 'flags')


def decode(hdr, slot_pos, S):
    """packed records hdr uint8 [M, 16] / slot_pos (u)int16 [M, 8] (craftingworld.h: cw_buffer_table.hdr / .slot_pos) -> dense numpy: grid uint8 [M, S, S],
    agent [M, 2], hold, achieved, desired, step_num, flags (the 16-bit word: bit 0 no step yet, bit 1 subset rule, bits 2-15 the success count), menu [M];
    held_code [M]: the code of the slot marked held (0: none is, 255: more than one)."""
    hdr = np.ascontiguousarray(hdr, dtype=np.uint8).reshape(-1, 16)
    pos = np.ascontiguousarray(slot_pos).reshape(-1, 8).view(np.uint16).astype(np.int64)
    if len(hdr) != len(pos):
        raise ValueError('%d headers, %d slot records' % (len(hdr), len(pos)))
    M = len(hdr)
    u16 = lambda lo: hdr[:, lo].astype(np.int64) | (hdr[:, lo + 1].astype(np.int64) << 8)  # noqa: E731
    codes = np.stack([(hdr[:, 12 + k // 2] >> (4 * (k % 2))) & 15 for k in range(8)], axis=1).astype(np.uint8)
    grid = np.zeros((M, S * S), np.uint8)
    for k in range(8):
        on = pos[:, k] < S * S
        grid[np.flatnonzero(on), pos[on, k]] = codes[on, k]
    held = pos == POS_HELD
    held_code = np.where(held.sum(axis=1) == 1, (codes * held).sum(axis=1), np.where(held.any(axis=1), 255, 0))
    return dict(grid=grid.reshape(M, S, S), agent=hdr[:, 0:2].astype(np.int64), hold=hdr[:, 2].astype(np.int64), menu=hdr[:, 3].astype(np.int64),
                achieved=u16(4), desired=u16(6), step_num=u16(8), flags=u16(10), held_code=held_code.astype(np.int64))


def encode(dense, menu=0):
    """dense states (decode()'s fields grid, agent, hold, achieved, desired, step_num, flags) -> (hdr uint8 [M, 16], slot_pos uint16 [M, 8]): the objects of
    the grid take the slots in row-major order, the held item the next one, the rest are gone.  ValueError for a state of more than 8 objects."""
    grid = np.asarray(dense['grid'])
    M, S = grid.shape[0], grid.shape[1]
    hdr = np.zeros((M, 16), np.uint8)
    pos = np.full((M, 8), POS_GONE, np.uint16)
    for j in range(M):
        cells = np.flatnonzero(grid[j].reshape(-1))
        items = [(int(c), int(grid[j].reshape(-1)[c])) for c in cells] + ([(POS_HELD, int(dense['hold'][j]))] if dense['hold'][j] else [])
        if len(items) > 8:
            raise ValueError('state %d holds %d objects' % (j, len(items)))
        for k, (c, code) in enumerate(items):
            pos[j, k] = c
            hdr[j, 12 + k // 2] |= code << (4 * (k % 2))
    hdr[:, 0], hdr[:, 1], hdr[:, 2], hdr[:, 3] = np.asarray(dense['agent'])[:, 0], np.asarray(dense['agent'])[:, 1], dense['hold'], menu
    for lo, k in ((4, 'achieved'), (6, 'desired'), (8, 'step_num'), (10, 'flags')):
        v = np.asarray(dense[k]).astype(np.int64)
        hdr[:, lo], hdr[:, lo + 1] = v & 0xFF, v >> 8
    return hdr, pos


def oracle_successors(states, init_grids, oracle_kw):
    """The six successors of each of M dense states (decode()'s fields; init_grids uint8 [M, S, S]: the start state of the episode the state belongs to) by
    the oracle's set_state + step (the two C calls behind OracleEnv.set_state / .step), and nothing else -> dict of arrays [6, M, ...]: reward, done, changed (the oracle's state before and after differs in grid,
    agent or hold), grid, agent, hold, achieved, desired, step_num and flags -- bit 0 cleared, bit 1 kept, the count in bits 2-15 one up (saturating) where
    the oracle's reward is max_steps.  The reward rule is each state's own (flags bit 1); oracle_kw: size and max_steps (reward_style in it is ignored)."""
    from oracle import OracleEnv
    kw = {k: v for k, v in oracle_kw.items() if k != 'reward_style'}
    envs = (OracleEnv(reward_style=None, **kw), OracleEnv(reward_style='subset', **kw))
    S, max_steps = envs[0].size, envs[0].MAX_STEPS
    M = len(states['hold'])
    out = dict(reward=np.zeros((6, M), np.int64), done=np.zeros((6, M), bool), changed=np.zeros((6, M), bool), grid=np.zeros((6, M, S, S), np.uint8),
               agent=np.zeros((6, M, 2), np.int64), hold=np.zeros((6, M), np.int64), achieved=np.zeros((6, M), np.int64), desired=np.zeros((6, M), np.int64),
               step_num=np.zeros((6, M), np.int64), flags=np.zeros((6, M), np.int64))
    grids = np.ascontiguousarray(states['grid'], dtype=np.uint8)
    inits = np.ascontiguousarray(init_grids, dtype=np.uint8)
    import ctypes as C
    lib, u8p = envs[0]._lib, C.POINTER(C.c_uint8)
    ags, holds = np.asarray(states['agent']).astype(np.int64).tolist(), np.asarray(states['hold']).astype(np.int64).tolist()
    achs, dess, sns = (np.asarray(states[k]).astype(np.int64).tolist() for k in ('achieved', 'desired', 'step_num'))
    fls = np.asarray(states['flags']).astype(np.int64).tolist()
    r, d, v = C.c_int32(), C.c_int32(), type(envs[0].view())()
    num = np.zeros((6, M, 8), np.int64)
    for j in range(M):                          # (OracleEnv.set_state / .step without their Python wrapping: the same two C calls, 10^5 times a test)
        h = envs[(fls[j] >> 1) & 1]._h
        gp, ip = grids[j].ctypes.data_as(u8p), inits[j].ctypes.data_as(u8p)
        (ar, ac), hold = ags[j], holds[j]
        for a in range(6):
            lib.cwo_set_state(h, gp, ip, ar, ac, hold, achs[j], dess[j], sns[j])
            if lib.cwo_step(h, a, C.byref(r), C.byref(d)) != 0:
                raise IndexError('action out of range')
            lib.cwo_get_view(h, C.byref(v))
            C.memmove(out['grid'][a, j].ctypes.data, v.grid, S * S)
            num[a, j] = (r.value, d.value, v.agent_r, v.agent_c, v.hold, v.achieved, v.desired, v.step_num)
    out['reward'], out['done'], out['agent'], out['hold'] = num[..., 0], num[..., 1] != 0, num[..., 2:4], num[..., 4]
    out['achieved'], out['desired'], out['step_num'] = num[..., 5], num[..., 6], num[..., 7]
    out['changed'] = ((out['agent'] != np.asarray(states['agent'])[None]).any(axis=-1) | (out['hold'] != np.asarray(states['hold'])[None])
                      | (out['grid'] != grids[None]).any(axis=(-1, -2)))
    fl = np.asarray(states['flags']).astype(np.int64)[None]
    out['flags'] = (fl & 2) | (np.minimum((fl >> 2) + (out['reward'] == max_steps), 0x3FFF) << 2)
    return out


def participation(env_of, M, N):
    """-> (env [M]: the env state j belongs to, -1 where its rows must not be written; the number of skipped states: entries >= N)"""
    if env_of is None:
        return np.arange(M, dtype=np.int64) % N, 0
    e = np.asarray(env_of).reshape(-1).astype(np.int64)
    if len(e) != M:
        raise ValueError('%d env_of entries for %d states' % (len(e), M))
    return np.where((e >= 0) & (e < N), e, -1), int((e >= N).sum())


def check_expand(before, after, inputs, env_of, outputs, sentinel, *, oracle_kw, successors=None):
    """Pure CPU.  cw_expand ran between the snapshots `before` and `after` (masked_check.take()).  inputs: None (the engine's own states: before['hdr'] /
    before['slot_pos']) or dict(hdr=[M, 16], slot_pos=[M, 8]), the records it read; env_of: None or the M entries it read; outputs: {field of FIELDS:
    [6, M, ...]} what the call left in the buffers it was given; sentinel: the byte every one of them was filled with before the call.
    EVERY row (a, j) of a state that takes part: reward, done, changed, achieved_mask and the decoded successor record (grid, agent, hold, both masks,
    step_num, flags, the slot marked held; the menu byte as in the input) equal the oracle's successor of action a from input state j with the start state
    of its env.  Every row of a state that takes no part (negative entry) or is skipped (entry >= num_envs): sentinel bytes.  The engine: `after` equals
    `before` everywhere, counters[7] == before + the skipped states, once each.  ValueError when no row would be compared with the oracle.
    successors: (dense states, oracle_successors of them) a test has computed already from the oracle's OWN values for the states that take part, in
    order: the records the call read must then decode to exactly these states, and the oracle is not run again.
    -> (states that took part, states skipped)."""
    if set(before) != set(after):
        raise ValueError('the snapshots hold different entries: %s' % sorted(set(before) ^ set(after)))
    if not outputs or set(outputs) - set(FIELDS):
        raise ValueError('outputs must hold some of %s' % (FIELDS,))
    N, S = len(before['rng_pos']), before['state_grid'].shape[1]
    if inputs is None:
        if env_of is not None:
            raise ValueError('env_of goes with caller-supplied records')
        inputs = dict(hdr=before['hdr'], slot_pos=before['slot_pos'])
    states = decode(inputs['hdr'], inputs['slot_pos'], S)
    M = len(states['hold'])
    env, skipped = participation(env_of, M, N)
    part = np.flatnonzero(env >= 0)
    if len(part) == 0:
        raise ValueError('no state takes part: nothing would be compared with the oracle')
    for f, got in outputs.items():
        if np.shape(got)[:2] != (6, M):
            raise ValueError('%s has shape %s, expected [6, %d, ...]' % (f, np.shape(got), M))
    sub = {k: v[part] for k, v in states.items()}
    if successors is None:
        want = oracle_successors(sub, before['state_init_grid'][env[part]], oracle_kw)
    else:
        mine, want = successors
        for k in DENSE:
            same('the records the call read: ' + k, part, sub[k], np.asarray(mine[k]))
    rest = np.flatnonzero(env < 0)
    for a in range(6):
        tag = 'action %d: ' % a
        for f, k in (('reward', 'reward'), ('done', 'done'), ('changed', 'changed'), ('achieved_mask', 'achieved')):
            if f in outputs:
                got = np.asarray(outputs[f])[a, part]
                got = got.view(np.uint16) if f == 'achieved_mask' and got.dtype == np.int16 else got
                same(tag + f, part, got.astype(np.int64), want[k][a].astype(np.int64))
        if 'hdr' in outputs and 'slot_pos' in outputs:
            got = decode(np.asarray(outputs['hdr'])[a, part], np.asarray(outputs['slot_pos'])[a, part], S)
            for k in DENSE:
                same(tag + 'successor ' + k, part, got[k], want[k][a])
            same(tag + 'successor: the slot marked held', part, got['held_code'], want['hold'][a])
            same(tag + 'successor menu byte', part, got['menu'], sub['menu'])
        elif 'hdr' in outputs:                  # (without the slots: the header's own fields)
            h = np.asarray(outputs['hdr'])[a, part]
            got = decode(h, np.full((len(part), 8), POS_GONE, np.uint16), S)
            for k in ('agent', 'hold', 'achieved', 'desired', 'step_num', 'flags'):
                same(tag + 'successor ' + k, part, got[k], want[k][a])
            same(tag + 'successor menu byte', part, got['menu'], sub['menu'])
        elif 'slot_pos' in outputs:             # (without the codes: where the objects are)
            p = np.asarray(outputs['slot_pos'])[a, part].reshape(len(part), 8).view(np.uint16)
            occ = np.zeros((len(part), S * S + 1), bool)
            occ[np.arange(len(part))[:, None], np.minimum(p.astype(np.int64), S * S)] = True
            same(tag + 'successor occupied cells', part, occ[:, :S * S].reshape(-1, S, S), want['grid'][a] != 0)
        for f, got in outputs.items():
            g = np.asarray(got)
            raw = np.ascontiguousarray(g[a, rest]).view(np.uint8).reshape(len(rest), g[0, 0].nbytes)
            same(tag + f + ' of the rows that must not be written', rest, raw, np.full_like(raw, sentinel))
    for k in sorted(before):
        if k == 'counters':
            w = before[k].copy()
            w[SKIPPED] += skipped
            assert np.array_equal(after[k], w), 'counters after an expand with %d skipped states: %s, expected %s' % (skipped, after[k].tolist(), w.tolist())
        else:
            same('after an expand: ' + k, 0, after[k], before[k])
    return len(part), skipped
