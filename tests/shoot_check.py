"""What "a shoot call did exactly what it should" means for cw_shoot, in one place.  draw() / action() are the numpy model of the draw function, written
from the text of include/craftingworld.h (uint64 arithmetic masked to 32 bits); model_actions() is the action tensor the kernel never materialises;
expected_shoot() sends those actions through simulate_check.oracle_simulate(..., stop_at_done=True) and reduces by the header's rule: the largest return,
the SMALLEST sample that reaches it.  check_shoot() compares what a call wrote with that: EVERY written row against the oracle, `plan` against the model,
every row that must not be written against the sentinel the test pre-filled, and the engine before and after the call (masked_check.take() snapshots):
nothing may have changed but counters[7], up by the skipped states.  coverage() counts what a batch exercises.  Pure CPU: numpy arrays in, no GPU.  A plain
module, not a fixture; tests/test_shoot_logic.py tests the model and the comparison themselves."""
import functools

import numpy as np

from expand_check import DENSE, POS_GONE, SKIPPED, decode, participation
from oracle_replay import same
from simulate_check import RECIPE_KW, oracle_simulate, recipe

FIELDS = ('best_ret', 'best_sample', 'best_action', 'length', 'done', 'achieved_mask', 'hdr', 'slot_pos', 'plan', 'ret')
M32 = np.uint64(0xFFFFFFFF)
_U = np.uint64


def mix(x):
    """mix(x) of the header on uint64 arrays that hold uint32 values"""
    x = np.asarray(x, np.uint64)
    x = x ^ (x >> _U(16))
    x = (x * _U(0x7FEB352D)) & M32
    x = x ^ (x >> _U(15))
    x = (x * _U(0x846CA68B)) & M32
    return x ^ (x >> _U(16))


def draw(seed, state, sample, step):
    """draw(seed, state, sample, step) of the header: seed a Python int 0 .. 2**64 - 1 (or an array of them), the rest integer arrays (broadcast) of uint32 values -> uint64"""
    seed = np.asarray(seed, dtype=np.uint64)                         # (a negative seed or one of 2**64 and more: OverflowError)
    lo, hi = seed & M32, seed >> _U(32)
    state, sample, step = (np.asarray(v).astype(np.uint64) for v in (state, sample, step))
    x = mix(lo ^ ((state * _U(0x9E3779B1)) & M32))
    x = mix(x ^ ((hi + ((sample * _U(0x85EBCA77)) & M32)) & M32))
    return mix(x ^ ((step * _U(0xC2B2AE3D)) & M32))


def action(r, w=None):
    """action(r, w) of the header: r uint64 [...] of uint32 values, w None or integers [..., 6] in 0 .. 65 535 -> int64 [...] in 0 .. 5"""
    r = np.asarray(r, np.uint64)
    uniform = ((r * _U(6)) >> _U(32)).astype(np.int64)
    if w is None:
        return uniform
    c = np.cumsum(np.asarray(w).astype(np.uint64), axis=-1)
    W = c[..., 5]
    x = (r * W) >> _U(32)
    return np.where(W == 0, uniform, (c[..., :5] <= x[..., None]).sum(axis=-1).astype(np.int64))


def model_actions(seed, M, K, T, weights=None, samples=None):
    """the actions cw_shoot draws -> int64 [T, K, M]: entry [t, k, j] = action(draw(seed, j, k, t), weights[t, :, j]); weights None or integers [T, 6, M].
    samples: None, or integers [R, M] -> [T, R, M], row r of state j being sample samples[r, j] (a negative entry: the column holds -1)."""
    t = np.arange(T)[:, None, None]
    j = np.arange(M)[None, None, :]
    if samples is None:
        k, dead = np.arange(K)[None, :, None], None
    else:
        s = np.asarray(samples).astype(np.int64).reshape(-1, M)
        k, dead = np.maximum(s, 0)[None], np.broadcast_to((s < 0)[None], (T,) + s.shape)
    r = draw(seed, j, k, t)
    w = None if weights is None else np.broadcast_to(np.moveaxis(np.asarray(weights).reshape(T, 6, M), 1, 2)[:, None], r.shape + (6,))
    a = action(r, w)
    return a if dead is None else np.where(dead, -1, a)


def expected_shoot(dense, init_grids, T, K, seed, oracle_kw, weights=None):
    """M dense states (expand_check.decode()'s fields; init_grids uint8 [M, S, S]) -> dict: actions [T, K, M] (the model's), ret [K, M] (oracle_simulate's
    `ret` of every sample with stop_at_done=True), best_ret, best_sample (numpy's argmax returns the FIRST maximum: the smallest sample), best_action, length,
    done, n_success (1: the best sample ends by success), ties (how many samples reach best_ret) [M], plan [T, M] (all T drawn actions of the best sample)
    and the dense final state of the best sample (grid, agent, hold, achieved, desired, step_num, flags)."""
    M = len(dense['hold'])
    acts = model_actions(seed, M, K, T, weights)
    tiled = {k: np.tile(np.asarray(dense[k]), (K,) + (1,) * (np.asarray(dense[k]).ndim - 1)) for k in DENSE}
    r = oracle_simulate(tiled, np.tile(np.asarray(init_grids), (K, 1, 1)), acts.reshape(T, K * M), True, oracle_kw)
    ret = r['ret'].reshape(K, M)
    best = ret.argmax(axis=0)
    flat = best * M + np.arange(M)
    out = dict(actions=acts, ret=ret, best_ret=ret.max(axis=0), best_sample=best, best_action=acts[0, best, np.arange(M)], length=r['length'][flat],
               done=r['done'][flat], n_success=r['n_success'][flat], ties=(ret == ret.max(axis=0)[None]).sum(axis=0), plan=acts[:, best, np.arange(M)],
               any_success=(r['n_success'].reshape(K, M) > 0).any(axis=0))
    for k in DENSE:
        out[k] = r[k][flat]
    return out


def check_shoot(before, after, inputs, env_of, T, K, seed, weights, outputs, sentinel, *, oracle_kw, expected=None):
    """Pure CPU.  cw_shoot ran between the snapshots `before` and `after` (masked_check.take()).  inputs: None (the engine's own states: before['hdr'] /
    before['slot_pos']) or dict(hdr=[M, 16], slot_pos=[M, 8]), the records it read; env_of: None or the M entries it read; T, K, seed (the EFFECTIVE seed, a
    Python int) and weights (None or [T, 6, M]) as the call had them; outputs: {field of FIELDS: [M, ...], plan [T, M], ret [K, M]} what the call left in the
    buffers it was given; sentinel: the byte every one of them was filled with before the call.
    EVERY row of a state j that takes part: best_ret, best_sample, best_action, length, done, achieved_mask, ret[:, j] and the decoded final record (grid,
    agent, hold, both masks, step_num, flags, the slot marked held; the menu byte as in the input) equal expected_shoot of input state j -- ROW j, whatever
    its env -- with the start state of its env; plan[:, j] equals the model's actions of sample best_sample, all T of them.  Every row of a state that takes
    no part (negative entry) or is skipped (entry >= num_envs), ret and plan columns included: sentinel bytes.  The engine: `after` equals `before` everywhere,
    counters[7] == before + the skipped states.  ValueError when no row would be compared with the oracle.
    expected: (dense states, expected_shoot of them) a test has computed already for ALL M input states in order (the draw is keyed by the row): the records
    the call read must then decode to exactly these states, and the oracle is not run again.  -> (states that took part, states skipped)."""
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
    part, rest = np.flatnonzero(env >= 0), np.flatnonzero(env < 0)
    if len(part) == 0:
        raise ValueError('no state takes part: nothing would be compared with the oracle')
    lead = {'plan': (T, M), 'ret': (K, M)}
    for f, got in outputs.items():
        if np.shape(got)[:len(lead.get(f, (M,)))] != lead.get(f, (M,)):
            raise ValueError('%s has shape %s for T = %d, K = %d, M = %d' % (f, np.shape(got), T, K, M))
    if expected is None:
        # the draw is keyed by the ROW: the states that take no part are simulated too (with env 0's start state) and never compared
        want = expected_shoot(states, before['state_init_grid'][np.maximum(env, 0)], T, K, seed, oracle_kw, weights)
    else:
        mine, want = expected
        for k in DENSE:
            same('the records the call read: ' + k, part, states[k][part], np.asarray(mine[k])[part])
    sub = {k: v[part] for k, v in states.items()}
    for f, k in (('best_ret', 'best_ret'), ('best_sample', 'best_sample'), ('best_action', 'best_action'), ('length', 'length'), ('done', 'done'),
                 ('achieved_mask', 'achieved')):
        if f in outputs:
            got = np.asarray(outputs[f])[part]
            got = got.view(np.uint16) if f == 'achieved_mask' and got.dtype == np.int16 else got
            same(f, part, got.astype(np.int64), want[k][part].astype(np.int64))
    if 'ret' in outputs:
        got = np.asarray(outputs['ret'])
        for k in range(K):
            same('ret of sample %d' % k, part, got[k, part].astype(np.int64), want['ret'][k, part])
    if 'plan' in outputs:
        got = np.asarray(outputs['plan'])
        model = model_actions(seed, M, K, T, weights, samples=want['best_sample'][None])[:, 0]
        for t in range(T):
            same('plan, step %d' % t, part, got[t, part].astype(np.int64), model[t, part])
    if 'hdr' in outputs and 'slot_pos' in outputs:
        got = decode(np.asarray(outputs['hdr'])[part], np.asarray(outputs['slot_pos'])[part], S)
        for k in DENSE:
            same('final ' + k, part, got[k], want[k][part])
        same('final record: the slot marked held', part, got['held_code'], want['hold'][part])
        same('final menu byte', part, got['menu'], sub['menu'])
    elif 'hdr' in outputs:                      # (without the slots: the header's own fields)
        got = decode(np.asarray(outputs['hdr'])[part], np.full((len(part), 8), POS_GONE, np.uint16), S)
        for k in ('agent', 'hold', 'achieved', 'desired', 'step_num', 'flags'):
            same('final ' + k, part, got[k], want[k][part])
        same('final menu byte', part, got['menu'], sub['menu'])
    elif 'slot_pos' in outputs:                 # (without the codes: where the objects are)
        p = np.asarray(outputs['slot_pos'])[part].reshape(len(part), 8).view(np.uint16)
        occ = np.zeros((len(part), S * S + 1), bool)
        occ[np.arange(len(part))[:, None], np.minimum(p.astype(np.int64), S * S)] = True
        same('final occupied cells', part, occ[:, :S * S].reshape(-1, S, S), want['grid'][part] != 0)
    for f, got in outputs.items():
        g = np.asarray(got)
        for t in (range(g.shape[0]) if f in lead else (None,)):
            rows = g[rest] if t is None else g[t, rest]
            raw = np.ascontiguousarray(rows).view(np.uint8).reshape(len(rest), g.dtype.itemsize * int(np.prod(rows.shape[1:], dtype=np.int64)))
            same(f + (' of the rows' if t is None else ', row %d, of the columns' % t) + ' that must not be written', rest, raw, np.full_like(raw, sentinel))
    for k in sorted(before):
        if k == 'counters':
            w = before[k].copy()
            w[SKIPPED] += skipped
            assert np.array_equal(after[k], w), 'counters after a shoot with %d skipped states: %s, expected %s' % (skipped, after[k].tolist(), w.tolist())
        else:
            same('after a shoot: ' + k, 0, after[k], before[k])
    return len(part), skipped


# ------------------------------------------------------------------------------------------------------------------------------ the shared batch of states
SHAPES = ((6, 5, 1), (6, 8, 1), (12, 33, 1), (12, 100, 2))      # (T, K, seed) on simulate_check.recipe(12)'s states
LONG = (24, 64, 3)                                              # ... and on recipe(24)'s: the horizon passes max_steps = 17


@functools.lru_cache(maxsize=None)
def recipe_shots(T, K, seed, style=None, states=12):
    """(the 600 dense states of simulate_check.recipe(states, style), their init grids, expected_shoot of them): computed once, shared by every test of the
    recipe and left unchanged"""
    dense, init_grids, _ = recipe(states, style)
    return dense, init_grids, expected_shoot(dense, init_grids, T, K, seed, RECIPE_KW, None)


def coverage(want, T, max_steps):
    """what a batch exercises, counted from expected_shoot alone -> dict: succeed (the best sample ends by success), none (no sample succeeds: every sample
    ties unless time-outs differ), later (best_sample != 0), later_tied (of those, a later sample reaches best_ret too), lengths (the distinct lengths of
    best samples that succeed), timeout (the best sample ends by time-out: done, no success)"""
    ok = want['done'] & (want['n_success'] > 0)
    later = want['best_sample'] != 0
    return dict(succeed=int(ok.sum()), none=int((~want['any_success']).sum()), later=int(later.sum()), later_tied=int((later & (want['ties'] >= 2)).sum()),
                lengths=sorted(set(want['length'][ok].tolist())), timeout=int((want['done'] & ~ok).sum()))


def assert_coverage(cov):
    """the bounds every test of a recipe shape asserts, from the oracle alone, before anything is compared"""
    assert cov['succeed'] >= 200 and cov['none'] >= 200 and cov['later'] >= 150 and cov['later_tied'] >= 80, cov
