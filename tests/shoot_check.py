"""What "a shoot call did exactly what it should" means for cw_shoot: records_check.check_records_call with a row per state, plan a row per step, ret a
row per sample, and expected_shoot() as what to expect.  draw() / action() are the numpy model of the draw function, written from the text of
include/craftingworld.h (uint64 arithmetic masked to 32 bits); model_actions() is the action tensor the kernel never materialises; expected_shoot() sends
those actions through records_check.oracle_simulate(..., stop_at_done=True) and reduces by the header's rule: the largest return, the SMALLEST sample that
reaches it.  `plan` is compared against the model.  coverage() counts what a batch exercises.  Pure CPU: numpy arrays in, no GPU.  A plain module, not a
fixture; tests/test_shoot_logic.py tests the model and the comparison themselves."""
import functools

import numpy as np

from records_check import DENSE, check_records_call, oracle_simulate, rows
from simulate_check import RECIPE_KW, recipe

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
    """M dense states (records_check.decode()'s fields; init_grids uint8 [M, S, S]) -> dict: actions [T, K, M] (the model's), ret [K, M] (oracle_simulate's
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


def layout(T, K):
    """{field: the shape in front of the M states}: a row per state, plan a row per (step, state), ret a row per (sample, state)"""
    return dict({f: () for f in FIELDS}, plan=(T,), ret=(K,))


def check_shoot(before, after, inputs, env_of, T, K, seed, weights, outputs, sentinel, *, oracle_kw, expected=None):
    """Pure CPU.  cw_shoot ran between the snapshots `before` and `after` (masked_check.take()); inputs, env_of, outputs ({field of FIELDS: [M, ...], plan
    [T, M], ret [K, M]}), sentinel and what is compared: records_check.check_records_call.  T, K, seed (the EFFECTIVE seed, a Python int) and weights
    (None or [T, 6, M]) as the call had them.  Every row of a state j that takes part, ret[:, j] included, equals expected_shoot of input state j -- ROW j,
    whatever its env -- with the start state of its env; plan[:, j] equals the model's actions of sample best_sample, all T of them.
    expected: (dense states, expected_shoot of them) a test has computed already for ALL M input states in order (the draw is keyed by the row): the records
    the call read must then decode to exactly these states, and the oracle is not run again.  -> (states that took part, states skipped)."""
    def expect(states, env, part):
        # the draw is keyed by the ROW: the states that take no part are simulated too (with env 0's start state) and never compared
        mine, want = expected or (None, expected_shoot(states, before['state_init_grid'][np.maximum(env, 0)], T, K, seed, oracle_kw, weights))
        want = dict(want, plan=model_actions(seed, len(env), K, T, weights, samples=want['best_sample'][None])[:, 0])
        cut = {f: want[f][..., part] for f in ('best_ret', 'best_sample', 'best_action', 'length', 'done', 'plan', 'ret')}
        return mine and rows({k: mine[k] for k in DENSE}, part), dict(cut, **rows({k: want[k] for k in DENSE}, part))
    return check_records_call(before, after, inputs, env_of, outputs, sentinel, name='cw_shoot', layout=layout(T, K), expect=expect)


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
