"""What "an unroll call did exactly what it should" means for cw_unroll: records_check.check_records_call with a record row per (t, state) for t = 0 .. T, a
trace row per step and state and a length per state, and oracle_unroll() as what to expect -- a chain of T ONE-step records_check.oracle_simulate calls, the
chain frozen by selection.  Pure CPU: numpy arrays in, no GPU.  A plain module, not a fixture; tests/test_unroll_logic.py tests the comparison itself."""
import numpy as np

from oracle_replay import same
from records_check import DENSE, RECORD, check_records_call, oracle_simulate, participation, rows

FIELDS = ('hdr', 'slot_pos', 'reward', 'done', 'changed', 'taken', 'length')
TRACES = ('reward', 'done', 'changed', 'taken')


def layout(T):
    """{field: the shape in front of the M states}: the records a row per t = 0 .. T and state, the traces a row per step and state, length a row per state"""
    return {f: (T + 1,) if f in RECORD else (T,) if f in TRACES else () for f in FIELDS}


def oracle_unroll(states, init_grids, actions, stop_at_done, oracle_kw):
    """M dense states (records_check.decode()'s fields; init_grids uint8 [M, S, S]) stepped through actions [T, M], ONE step of oracle_simulate at a time,
    every state in between kept -> dict: grid, agent, hold, achieved, desired, step_num, flags [T + 1, M, ...] (row 0: the states as given, row t + 1: after
    step t); reward, done, changed, taken [T, M]; length [M].  stop_at_done: step t of a state is taken iff no earlier step of it returned done; a step not
    taken has reward 0, done / changed / taken False and row t + 1 = row t (selection: the oracle still steps, its result is dropped).  Else every step is
    taken.  changed: expand_check's definition -- grid, agent or hold differs.  length: 1 + the first done step, T if none."""
    acts = np.asarray(actions).astype(np.int64)
    acts = acts.reshape(acts.shape[0], -1)
    T, M = acts.shape[0], len(states['hold'])
    if acts.shape[1] != M or T < 1:
        raise ValueError('actions %s for %d states' % (acts.shape, M))
    cur = {k: np.asarray(states[k]).astype(np.uint8 if k == 'grid' else np.int64) for k in DENSE}
    path = {k: [cur[k]] for k in DENSE}
    out = dict(reward=np.zeros((T, M), np.int64), done=np.zeros((T, M), bool), changed=np.zeros((T, M), bool), taken=np.zeros((T, M), bool),
               length=np.full(M, T, np.int64))
    active, any_done = np.ones(M, bool), np.zeros(M, bool)
    for t in range(T):
        s = oracle_simulate(cur, init_grids, acts[t:t + 1], False, oracle_kw)
        moved = ((s['agent'] != cur['agent']).any(axis=-1) | (s['hold'] != cur['hold']) | (s['grid'] != cur['grid']).any(axis=(-1, -2)))
        done_now = active & s['dones'][0]
        out['reward'][t], out['done'][t], out['changed'][t], out['taken'][t] = np.where(active, s['rewards'][0], 0), done_now, active & moved, active
        out['length'] = np.where(done_now & ~any_done, t + 1, out['length'])
        any_done = any_done | done_now
        cur = {k: np.where(active.reshape((M,) + (1,) * (cur[k].ndim - 1)), np.asarray(s[k]).astype(cur[k].dtype), cur[k]) for k in DENSE}
        for k in DENSE:
            path[k].append(cur[k])
        if stop_at_done:
            active = active & ~s['dones'][0]
    out.update({k: np.stack(v) for k, v in path.items()})
    return out


def check_unroll(before, after, inputs, env_of, actions, stop_at_done, outputs, sentinel, *, oracle_kw, expected=None):
    """Pure CPU.  cw_unroll ran between the snapshots `before` and `after` (masked_check.take()); inputs (None: the engine's own states, broadcast: state j
    is before['hdr'][j % N], M = the actions' columns), env_of, outputs ({field of FIELDS: [T + 1, M, ...], [T, M] or [M]}), sentinel and what is compared:
    records_check.check_records_call -- every row of a state that takes part, at every t, equals oracle_unroll of input state j with the start state of its
    env; every row of a state that does not, at every t, holds the sentinel; the engine is untouched but for counters[7].  On top of it, on packed bytes
    (decode() does not pin slot order): row 0 of the records is the record read, and row t + 1 of a step not taken is row t.
    expected: (dense states, oracle_unroll of them) a test has computed already for the states that take part, in order.
    -> (states that took part, states skipped)."""
    acts = np.asarray(actions)
    if acts.ndim < 2:
        raise ValueError('actions must be [T, M], got %s' % (acts.shape,))
    acts = acts.reshape(acts.shape[0], -1)
    T, M = acts.shape
    seen = {}

    def expect(states, env, part):
        mine, want = expected or (None, oracle_unroll(rows(states, part), before['state_init_grid'][env[part]], acts[:, part], stop_at_done, oracle_kw))
        seen['taken'] = np.asarray(want['taken'])
        return mine, want
    got = check_records_call(before, after, inputs, env_of, outputs, sentinel, name='cw_unroll', layout=layout(T), expect=expect, M=M)
    N = len(before['rng_pos'])
    part = np.flatnonzero(participation(env_of, M, N)[0] >= 0)
    for f in RECORD:
        if f not in outputs:
            continue
        g = np.ascontiguousarray(outputs[f]).view(np.uint8).reshape(T + 1, M, 16)[:, part]
        read = before[f][np.arange(M) % N] if inputs is None else inputs[f]
        same('cw_unroll: %s[0] is the record read, byte for byte' % f, part, g[0], np.ascontiguousarray(read).view(np.uint8).reshape(M, 16)[part])
        for t in range(T):
            idle = ~seen['taken'][t]
            same('cw_unroll: %s[%d] of a step not taken repeats the row before it' % (f, t + 1), part[idle], g[t + 1][idle], g[t][idle])
    return got
