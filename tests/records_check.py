"""What "a records call did exactly what it should" means for cw_expand, cw_simulate, cw_plan and cw_shoot, said once.  These calls read packed state
records, with or without env_of, touch no env and write rows only for the states that take part.  Three layers: decode() / encode() turn packed records
into dense numpy and back; oracle_simulate() steps dense states by OracleEnv.set_state + step (the two C calls behind them) and nothing else -- the only
loop over the oracle's C calls, every other oracle of these tests is a reduction of it; check_records_call() compares what a call wrote with what its
`expect` says: EVERY written row against the oracle, every row that must not be written against the sentinel the test pre-filled, and the engine before and
after the call (masked_check.take() snapshots): nothing may have changed but counters[7], which counts the skipped states.  check_expand, check_simulate,
check_plan and check_shoot (tests/{expand,simulate,plan,shoot}_check.py) are this function with a layout and an `expect` each.  Pure CPU: numpy arrays in,
no GPU.  A plain module, not a fixture; the four tests/test_*_logic.py test the comparison itself through each wrapper."""
import ctypes as C

import numpy as np

from oracle_replay import same

SKIPPED = 7                                     # counters[7]: states skipped for an env index at or above num_envs
POS_GONE, POS_HELD = 0xFFFF, 0xFFFE
DENSE = ('grid', 'agent', 'hold', 'achieved', 'desired', 'step_num', 'flags')
RECORD = ('hdr', 'slot_pos')


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


def participation(env_of, M, N):
    """-> (env [M]: the env state j belongs to, -1 where its rows must not be written; the number of skipped states: entries >= N)"""
    if env_of is None:
        return np.arange(M, dtype=np.int64) % N, 0
    e = np.asarray(env_of).reshape(-1).astype(np.int64)
    if len(e) != M:
        raise ValueError('%d env_of entries for %d states' % (len(e), M))
    return np.where((e >= 0) & (e < N), e, -1), int((e >= N).sum())


def oracle_simulate(states, init_grids, actions, stop_at_done, oracle_kw):
    """M dense states (decode()'s fields; init_grids uint8 [M, S, S]: the start state of the episode a state belongs to) stepped through actions [T, M] by
    the oracle's set_state + step and nothing else -> dict: ret, length, done [M]; rewards, dones [T, M]; taken [M] (steps taken); n_success [M] (steps
    taken that paid max_steps) and the dense final state grid, agent, hold, achieved, desired, step_num, flags [M, ...] -- flags: bit 0 cleared, bit 1
    kept, the count in bits 2-15 up by the successes (saturating).  An action above 5 is the engine's state-preserving no-op, which the oracle refuses:
    the state goes back in with step_num + 1, reward -1, done at the time-out.  stop_at_done: a state's first done step is its last, the trace rows after
    it are (0, 0); else every state takes all T steps, length is still 1 + the first done step.  The reward rule is each state's own (flags bit 1);
    oracle_kw: size and max_steps (reward_style in it is ignored)."""
    from oracle import OracleEnv
    kw = {k: v for k, v in oracle_kw.items() if k != 'reward_style'}
    envs = (OracleEnv(reward_style=None, **kw), OracleEnv(reward_style='subset', **kw))
    S, max_steps = envs[0].size, envs[0].MAX_STEPS
    acts = np.asarray(actions).astype(np.int64)
    M = len(states['hold'])
    acts = acts.reshape(acts.shape[0], -1)
    T = acts.shape[0]
    if acts.shape[1] != M or T < 1:
        raise ValueError('actions %s for %d states' % (acts.shape, M))
    grids = np.ascontiguousarray(states['grid'], dtype=np.uint8)
    inits = np.ascontiguousarray(init_grids, dtype=np.uint8)
    if grids.shape != (M, S, S) or inits.shape != (M, S, S):
        raise ValueError('grids %s, init grids %s for %d states of size %d' % (grids.shape, inits.shape, M, S))
    lib, u8p = envs[0]._lib, C.POINTER(C.c_uint8)
    ags, holds = np.asarray(states['agent']).astype(np.int64).tolist(), np.asarray(states['hold']).astype(np.int64).tolist()
    achs, dess, sns, fls = (np.asarray(states[k]).astype(np.int64).tolist() for k in ('achieved', 'desired', 'step_num', 'flags'))
    out = dict(ret=np.zeros(M, np.int64), length=np.full(M, T, np.int64), done=np.zeros(M, bool), rewards=np.zeros((T, M), np.int64),
               dones=np.zeros((T, M), bool), taken=np.zeros(M, np.int64), n_success=np.zeros(M, np.int64), grid=np.zeros((M, S, S), np.uint8))
    num = np.zeros((M, 7), np.int64)
    r, d, v = C.c_int32(), C.c_int32(), type(envs[0].view())()
    cols = acts.T.tolist()
    g0, i0, o0 = grids.ctypes.data, inits.ctypes.data, out['grid'].ctypes.data  # (a row's address by arithmetic: .ctypes on a row costs more than the C calls)
    for j in range(M):
        h = envs[(fls[j] >> 1) & 1]._h
        ip = C.cast(i0 + j * S * S, u8p)
        lib.cwo_set_state(h, C.cast(g0 + j * S * S, u8p), ip, ags[j][0], ags[j][1], holds[j], achs[j], dess[j], sns[j])
        for t, a in enumerate(cols[j]):
            if a <= 5:
                if lib.cwo_step(h, a, C.byref(r), C.byref(d)) != 0:
                    raise IndexError('action out of range')
                rew, dn = r.value, d.value != 0
            else:
                lib.cwo_get_view(h, C.byref(v))
                lib.cwo_set_state(h, v.grid, ip, v.agent_r, v.agent_c, v.hold, v.achieved, v.desired, v.step_num + 1)
                rew, dn = -1, v.step_num + 1 >= max_steps
            out['rewards'][t, j], out['dones'][t, j] = rew, dn
            out['ret'][j] += rew
            out['taken'][j] += 1
            out['n_success'][j] += rew == max_steps
            if dn and not out['done'][j]:
                out['done'][j], out['length'][j] = True, t + 1
            if dn and stop_at_done:
                break
        lib.cwo_get_view(h, C.byref(v))
        C.memmove(o0 + j * S * S, v.grid, S * S)
        num[j] = (v.agent_r, v.agent_c, v.hold, v.achieved, v.desired, v.step_num, 0)
    out['agent'], out['hold'], out['achieved'], out['desired'], out['step_num'] = num[:, 0:2], num[:, 2], num[:, 3], num[:, 4], num[:, 5]
    fl = np.asarray(states['flags']).astype(np.int64)
    out['flags'] = (fl & 2) | (np.minimum((fl >> 2) + out['n_success'], 0x3FFF) << 2)
    return out


def rows(dense, pick):
    """the states `pick` of a dict of per-state arrays"""
    return {k: np.asarray(v)[pick] for k, v in dense.items()}


def check_records_call(before, after, inputs, env_of, outputs, sentinel, *, name, layout, expect, M=None):
    """Pure CPU.  The call `name` ran between the snapshots `before` and `after` (masked_check.take()).  inputs: None (the engine's own states, state j
    being before['hdr'][j % N]: M of them, N unless given) or dict(hdr=[M, 16], slot_pos=[M, 8]), the records it read; env_of: None or the M entries it
    read; outputs: {field of layout: array} what the call left in the buffers it was given; sentinel: the byte every one of them was filled with before.
    layout: {field: prefix shape} -- an output's leading shape is prefix + (M,): () a row per state, (6,) a row per first action and state, (T,) a trace.
    expect(states, env, part) says what the call should have written, from the M decoded input states, the env of each (-1: it takes no part) and the
    rows that take part -> (None or the dense states, in the order of `part`, that a test computed `want` from beforehand; want): want[f] in the layout
    of field f over the len(part) states (`achieved` for achieved_mask), want[k] for k of DENSE the final states in the layout of hdr.
    EVERY row of a state that takes part, at every index of its field's prefix, equals want; the records decode to want's final state (grid, agent, hold,
    both masks, step_num, flags, the slot marked held; the menu byte as in the input; hdr or slot_pos alone: what that array alone pins).  Every row of a
    state that takes no part (negative entry) or is skipped (entry >= num_envs), at every index of the prefix: sentinel bytes.  The records the call read
    decode to the states `want` was computed from.  The engine: `after` equals `before` everywhere, counters[7] == before + the skipped states, once
    each.  ValueError when no row would be compared with the oracle.  -> (states that took part, states skipped)."""
    if set(before) != set(after):
        raise ValueError('the snapshots hold different entries: %s' % sorted(set(before) ^ set(after)))
    if not outputs or set(outputs) - set(layout):
        raise ValueError('outputs must hold some of %s' % (tuple(layout),))
    N, S = len(before['rng_pos']), before['state_grid'].shape[1]
    if inputs is None:
        if env_of is not None:
            raise ValueError('env_of goes with caller-supplied records')
        M = N if M is None else M
        if M == 0 or M % N:
            raise ValueError('%d states for %d envs' % (M, N))
        inputs = dict(hdr=np.tile(before['hdr'], (M // N, 1)), slot_pos=np.tile(before['slot_pos'], (M // N, 1)))
    states = decode(inputs['hdr'], inputs['slot_pos'], S)
    if M is not None and len(states['hold']) != M:
        raise ValueError('%d records for %d states' % (len(states['hold']), M))
    M = len(states['hold'])
    env, skipped = participation(env_of, M, N)
    part, rest = np.flatnonzero(env >= 0), np.flatnonzero(env < 0)
    if len(part) == 0:
        raise ValueError('no state takes part: nothing would be compared with the oracle')
    outputs = {f: np.asarray(g) for f, g in outputs.items()}
    for f, g in outputs.items():
        if g.shape[:len(layout[f]) + 1] != tuple(layout[f]) + (M,):
            raise ValueError('%s has shape %s, expected %s + [%d, ...]' % (f, g.shape, list(layout[f]), M))
    mine, want = expect(states, env, part)
    sub = rows(states, part)
    if mine is not None:
        for k in DENSE:
            same('%s: the records the call read: %s' % (name, k), part, sub[k], np.asarray(mine[k]))
    at = lambda f, i: '%s: %s%s' % (name, f, list(i) if i else '')  # noqa: E731
    for f, g in outputs.items():
        for i in np.ndindex(*layout[f]):
            raw = np.ascontiguousarray(g[i][rest]).view(np.uint8).reshape(len(rest), g[i][0].nbytes)
            same(at(f, i) + ' of the rows that must not be written', rest, raw, np.full_like(raw, sentinel))
            if f not in RECORD:
                got = g[i][part]
                got = got.view(np.uint16) if f == 'achieved_mask' and got.dtype == np.int16 else got
                same(at(f, i), part, got.astype(np.int64), np.asarray(want['achieved' if f == 'achieved_mask' else f])[i].astype(np.int64))
    for i in np.ndindex(*layout['hdr']) if set(RECORD) & set(outputs) else ():
        tag = at('final record', i) + ': '
        if 'hdr' in outputs and 'slot_pos' in outputs:
            got = decode(outputs['hdr'][i][part], outputs['slot_pos'][i][part], S)
            for k in DENSE:
                same(tag + k, part, got[k], want[k][i])
            same(tag + 'the slot marked held', part, got['held_code'], want['hold'][i])
            same(tag + 'menu byte', part, got['menu'], sub['menu'])
        elif 'hdr' in outputs:                  # (without the slots: the header's own fields)
            got = decode(outputs['hdr'][i][part], np.full((len(part), 8), POS_GONE, np.uint16), S)
            for k in ('agent', 'hold', 'achieved', 'desired', 'step_num', 'flags'):
                same(tag + k, part, got[k], want[k][i])
            same(tag + 'menu byte', part, got['menu'], sub['menu'])
        else:                                   # (without the codes: where the objects are)
            p = np.ascontiguousarray(outputs['slot_pos'][i][part]).reshape(len(part), 8).view(np.uint16)
            occ = np.zeros((len(part), S * S + 1), bool)
            occ[np.arange(len(part))[:, None], np.minimum(p.astype(np.int64), S * S)] = True
            same(tag + 'occupied cells', part, occ[:, :S * S].reshape(-1, S, S), want['grid'][i] != 0)
    for k in sorted(before):
        if k == 'counters':
            w = before[k].copy()
            w[SKIPPED] += skipped
            assert np.array_equal(after[k], w), 'counters after %s with %d skipped states: %s, expected %s' % (name, skipped, after[k].tolist(), w.tolist())
        else:
            same('after %s: %s' % (name, k), 0, after[k], before[k])
    return len(part), skipped
