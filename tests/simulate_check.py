"""What "a simulate call did exactly what it should" means for cw_simulate, in one place.  oracle_simulate() steps dense states through action sequences by
OracleEnv.set_state + step (the two C calls behind them) and nothing else; check_simulate() compares what a call wrote with that: EVERY written row against
the oracle, every row that must not be written -- trace rows included -- against the sentinel the test pre-filled, and the engine before and after the
call (masked_check.take() snapshots): nothing may have changed but counters[7], which counts the skipped states.  recipe() is the batch of states and plans
the tests share, built from the oracle alone, and coverage() counts what it exercises.  Pure CPU: numpy arrays in, no GPU.  A plain module, not a
fixture; tests/test_simulate_logic.py tests the comparison itself.  The packed records are expand_check's (decode, the flags rule)."""
import ctypes as C
import functools

import numpy as np

from expand_check import DENSE, POS_GONE, SKIPPED, decode, participation
from oracle_replay import same

FIELDS = ('ret', 'length', 'done', 'achieved_mask', 'hdr', 'slot_pos', 'rewards', 'dones')
PER_STATE, TRACES = FIELDS[:6], FIELDS[6:]


def oracle_simulate(states, init_grids, actions, stop_at_done, oracle_kw):
    """M dense states (expand_check.decode()'s fields; init_grids uint8 [M, S, S]: the start state of the episode a state belongs to) stepped through
    actions [T, M] by the oracle's set_state + step and nothing else -> dict: ret, length, done [M]; rewards, dones [T, M]; taken [M] (steps taken);
    n_success [M] (steps taken that paid max_steps) and the dense final state grid, agent, hold, achieved, desired, step_num, flags [M, ...] -- flags as
    expand_check.oracle_successors counts them: bit 0 cleared, bit 1 kept, bits 2-15 up by the successes (saturating).  An action above 5 is the engine's
    state-preserving no-op, which the oracle refuses: the state goes back in with step_num + 1, reward -1, done at the time-out.  stop_at_done: a state's
    first done step is its last, the trace rows after it are (0, 0); else every state takes all T steps, length is still 1 + the first done step.  The
    reward rule is each state's own (flags bit 1); oracle_kw: size and max_steps (reward_style in it is ignored)."""
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
    lib, u8p = envs[0]._lib, C.POINTER(C.c_uint8)
    ags, holds = np.asarray(states['agent']).astype(np.int64).tolist(), np.asarray(states['hold']).astype(np.int64).tolist()
    achs, dess, sns, fls = (np.asarray(states[k]).astype(np.int64).tolist() for k in ('achieved', 'desired', 'step_num', 'flags'))
    out = dict(ret=np.zeros(M, np.int64), length=np.full(M, T, np.int64), done=np.zeros(M, bool), rewards=np.zeros((T, M), np.int64),
               dones=np.zeros((T, M), bool), taken=np.zeros(M, np.int64), n_success=np.zeros(M, np.int64), grid=np.zeros((M, S, S), np.uint8))
    num = np.zeros((M, 7), np.int64)
    r, d, v = C.c_int32(), C.c_int32(), type(envs[0].view())()
    cols = acts.T.tolist()
    for j in range(M):
        h = envs[(fls[j] >> 1) & 1]._h
        ip = inits[j].ctypes.data_as(u8p)
        lib.cwo_set_state(h, grids[j].ctypes.data_as(u8p), ip, ags[j][0], ags[j][1], holds[j], achs[j], dess[j], sns[j])
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
        C.memmove(out['grid'][j].ctypes.data, v.grid, S * S)
        num[j] = (v.agent_r, v.agent_c, v.hold, v.achieved, v.desired, v.step_num, 0)
    out['agent'], out['hold'], out['achieved'], out['desired'], out['step_num'] = num[:, 0:2], num[:, 2], num[:, 3], num[:, 4], num[:, 5]
    fl = np.asarray(states['flags']).astype(np.int64)
    out['flags'] = (fl & 2) | (np.minimum((fl >> 2) + out['n_success'], 0x3FFF) << 2)
    return out


def check_simulate(before, after, inputs, env_of, actions, stop_at_done, outputs, sentinel, *, oracle_kw, expected=None):
    """Pure CPU.  cw_simulate ran between the snapshots `before` and `after` (masked_check.take()).  inputs: None (the engine's own states, broadcast:
    state j is before['hdr'][j % N], M = the actions' columns) or dict(hdr=[M, 16], slot_pos=[M, 8]), the records it read; env_of: None or the M entries
    it read; actions [T, M] (any trailing shape of M columns); outputs: {field of FIELDS: [M, ...] or [T, M]} what the call left in the buffers it was
    given; sentinel: the byte every one of them was filled with before the call.
    EVERY row of a state that takes part: ret, length, done, achieved_mask, the decoded final record (grid, agent, hold, both masks, step_num, flags, the
    slot marked held; the menu byte as in the input) and every trace row equal oracle_simulate of input state j with the start state of its env.  Every
    row of a state that takes no part (negative entry) or is skipped (entry >= num_envs), trace rows included: sentinel bytes.  The engine: `after`
    equals `before` everywhere, counters[7] == before + the skipped states.  ValueError when no row would be compared with the oracle.
    expected: (dense states, oracle_simulate of them) a test has computed already for the states that take part, in order: the records the call read must
    then decode to exactly these states, and the oracle is not run again.  -> (states that took part, states skipped)."""
    if set(before) != set(after):
        raise ValueError('the snapshots hold different entries: %s' % sorted(set(before) ^ set(after)))
    if not outputs or set(outputs) - set(FIELDS):
        raise ValueError('outputs must hold some of %s' % (FIELDS,))
    N, S = len(before['rng_pos']), before['state_grid'].shape[1]
    acts = np.asarray(actions)
    if acts.ndim < 2:
        raise ValueError('actions must be [T, M], got %s' % (acts.shape,))
    acts = acts.reshape(acts.shape[0], -1)
    T, M = acts.shape
    if inputs is None:
        if env_of is not None:
            raise ValueError('env_of goes with caller-supplied records')
        if M == 0 or M % N:
            raise ValueError('%d plans for %d envs' % (M, N))
        inputs = dict(hdr=np.tile(before['hdr'], (M // N, 1)), slot_pos=np.tile(before['slot_pos'], (M // N, 1)))
    states = decode(inputs['hdr'], inputs['slot_pos'], S)
    if len(states['hold']) != M:
        raise ValueError('%d records, %d action columns' % (len(states['hold']), M))
    env, skipped = participation(env_of, M, N)
    part, rest = np.flatnonzero(env >= 0), np.flatnonzero(env < 0)
    if len(part) == 0:
        raise ValueError('no state takes part: nothing would be compared with the oracle')
    for f, got in outputs.items():
        if np.shape(got)[:2 if f in TRACES else 1] != ((T, M) if f in TRACES else (M,)):
            raise ValueError('%s has shape %s for T = %d, M = %d' % (f, np.shape(got), T, M))
    sub = {k: v[part] for k, v in states.items()}
    if expected is None:
        want = oracle_simulate(sub, before['state_init_grid'][env[part]], acts[:, part], stop_at_done, oracle_kw)
    else:
        mine, want = expected
        for k in DENSE:
            same('the records the call read: ' + k, part, sub[k], np.asarray(mine[k]))
    for f, k in (('ret', 'ret'), ('length', 'length'), ('done', 'done'), ('achieved_mask', 'achieved')):
        if f in outputs:
            got = np.asarray(outputs[f])[part]
            got = got.view(np.uint16) if f == 'achieved_mask' and got.dtype == np.int16 else got
            same(f, part, got.astype(np.int64), want[k].astype(np.int64))
    for f in TRACES:
        if f in outputs:
            got = np.asarray(outputs[f])
            for t in range(T):
                same('%s of step %d' % (f, t), part, got[t, part].astype(np.int64), want[f][t].astype(np.int64))
    if 'hdr' in outputs and 'slot_pos' in outputs:
        got = decode(np.asarray(outputs['hdr'])[part], np.asarray(outputs['slot_pos'])[part], S)
        for k in DENSE:
            same('final ' + k, part, got[k], want[k])
        same('final record: the slot marked held', part, got['held_code'], want['hold'])
        same('final menu byte', part, got['menu'], sub['menu'])
    elif 'hdr' in outputs:                      # (without the slots: the header's own fields)
        got = decode(np.asarray(outputs['hdr'])[part], np.full((len(part), 8), POS_GONE, np.uint16), S)
        for k in ('agent', 'hold', 'achieved', 'desired', 'step_num', 'flags'):
            same('final ' + k, part, got[k], want[k])
        same('final menu byte', part, got['menu'], sub['menu'])
    elif 'slot_pos' in outputs:                 # (without the codes: where the objects are)
        p = np.asarray(outputs['slot_pos'])[part].reshape(len(part), 8).view(np.uint16)
        occ = np.zeros((len(part), S * S + 1), bool)
        occ[np.arange(len(part))[:, None], np.minimum(p.astype(np.int64), S * S)] = True
        same('final occupied cells', part, occ[:, :S * S].reshape(-1, S, S), want['grid'] != 0)
    for f, got in outputs.items():
        g = np.asarray(got)
        for t in (range(T) if f in TRACES else (None,)):
            rows = g[rest] if t is None else g[t, rest]
            raw = np.ascontiguousarray(rows).view(np.uint8).reshape(len(rest), g.dtype.itemsize * int(np.prod(rows.shape[1:], dtype=np.int64)))
            same(f + (' of the rows' if t is None else ' of step %d of the rows' % t) + ' that must not be written', rest, raw, np.full_like(raw, sentinel))
    for k in sorted(before):
        if k == 'counters':
            w = before[k].copy()
            w[SKIPPED] += skipped
            assert np.array_equal(after[k], w), 'counters after a simulate with %d skipped states: %s, expected %s' % (skipped, after[k].tolist(), w.tolist())
        else:
            same('after a simulate: ' + k, 0, after[k], before[k])
    return len(part), skipped


# ------------------------------------------------------------------------------------------------------------------------------ the shared batch of plans
RECIPE_N, RECIPE_KW = 600, dict(size=(5, 5), max_steps=17)


@functools.lru_cache(maxsize=None)
def recipe(T, style=None):
    """600 states on a 5 x 5 grid, max_steps 17: oracle envs seeded RandomState(900 + j) after reset(); actions RandomState(7).randint(0, 6, (T, 600)); for
    even j `desired` is replaced by the achieved mask the oracle itself reaches after 2 + (j // 2) % 9 steps of its own column (without the relabel 2-3
    of 600 ever succeed).  -> (dense states, init grids [600, 5, 5], actions int64 [T, 600]); flags: the reward rule `style`, no step taken yet."""
    from oracle import OracleEnv
    acts = np.random.RandomState(7).randint(0, 6, (T, RECIPE_N))
    st = []
    for j in range(RECIPE_N):
        s0 = np.random.RandomState(900 + j).get_state()
        o = OracleEnv(rng_state=(s0[1].astype(np.uint32), int(s0[2])), reward_style=style, **RECIPE_KW)
        o.reset()
        s = o.state()
        if j % 2 == 0:
            for t in range(2 + (j // 2) % 9):
                o.step(int(acts[t, j]))
            s['desired'] = o.view().achieved
        st.append(s)
    dense = dict(grid=np.stack([s['grid'] for s in st]), agent=np.array([s['agent'] for s in st], np.int64), hold=np.array([s['hold'] for s in st], np.int64),
                 achieved=np.array([s['achieved'] for s in st], np.int64), desired=np.array([s['desired'] for s in st], np.int64),
                 step_num=np.array([s['step_num'] for s in st], np.int64), flags=np.full(RECIPE_N, 1 | (2 if style else 0), np.int64))
    return dense, np.stack([s['init_grid'] for s in st]), acts


def coverage(stepped_on, max_steps):
    """what a batch of plans exercises, counted from oracle_simulate(..., stop_at_done=False) alone -> dict: never (no step done), success_first /
    timeout_first (the first done step paid max_steps / did not), success_steps (the distinct step indices that paid), paid_after_done (success rewards
    behind a state's first done step)"""
    rew, T = stepped_on['rewards'], stepped_on['rewards'].shape[0]
    first = stepped_on['length'] - 1
    cols = np.arange(rew.shape[1])
    paid_first = stepped_on['done'] & (rew[np.minimum(first, T - 1), cols] == max_steps)
    behind = np.arange(T)[:, None] > first[None, :]
    return dict(never=int((~stepped_on['done']).sum()), success_first=int(paid_first.sum()), timeout_first=int((stepped_on['done'] & ~paid_first).sum()),
                success_steps=sorted(set(np.nonzero(rew == max_steps)[0].tolist())),
                paid_after_done=int(((rew == max_steps) & behind & stepped_on['done'][None, :]).sum()))


def assert_recipe_coverage(cov12, cov24):
    """the conditions every test of the recipe asserts before anything is compared: each of the three classes 200 times across the two horizons, successes
    at 8 distinct step indices, 500 success rewards behind a first done"""
    assert cov12['never'] >= 200 and cov12['success_first'] >= 200 and cov24['success_first'] >= 200 and cov24['timeout_first'] >= 200, (cov12, cov24)
    assert len(cov12['success_steps']) >= 8 and cov12['paid_after_done'] >= 500, cov12
