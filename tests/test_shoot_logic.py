"""CPU tier: the draw function of cw_shoot and the checker of the shoot tests (tests/shoot_check.py over records_check.py).  The numpy model, written from the header's
text, against the library's own function bit for bit; the statistics the header's function was chosen on; then the outputs a correct cw_shoot would leave,
synthesised on the CPU -- the model's actions through the oracle, reduced, encoded into packed records by the test-side encoder -- which must pass, and each
planted fault, which must be caught.  Also here: what the shared batch of states exercises, counted from the oracle alone."""
import ctypes as C

import numpy as np
import pytest

from gym_craftingworld_amd.vec_env import SHOOT_FIELDS
from hostlib import host_lib
from plan_check import far_goals
from records_check import DENSE, encode, oracle_simulate
from records_fixtures import ENV_OF, M, N, S, SENT, snap, world as _world
from shoot_check import (FIELDS, LONG, RECIPE_KW, SHAPES, action, assert_coverage, check_shoot, coverage, draw, expected_shoot, mix, model_actions,
                         recipe_shots)

MAX_STEPS, T, K, SEED = 9, 4, 12, 0x123456789ABCDEF
OKW = dict(size=(S, S), max_steps=MAX_STEPS)
GRID_SEEDS = (0, 1, 2, 0xDEADBEEF12345678, 2 ** 64 - 1)


@pytest.fixture(scope='module')
def lib():
    return host_lib()


def test_the_checker_knows_the_ten_fields_the_kernel_writes():
    assert FIELDS == SHOOT_FIELDS and len(FIELDS) == 10


# ------------------------------------------------------------------------------------------------------------------------------ the draw
def _lib_actions(lib, seeds, states, samples, steps, weights=None):
    f = lib.cwh_shoot_action_of
    out = np.empty(len(states), np.int64)
    for i in range(len(states)):
        w = None if weights is None else np.ascontiguousarray(weights[i], np.uint16).ctypes.data_as(C.c_void_p)
        out[i] = f(int(seeds[i]), int(states[i]), int(samples[i]), int(steps[i]), w)
    return out


def _model(seeds, states, samples, steps, weights=None):
    return action(draw(np.array(seeds, dtype=np.uint64), states, samples, steps), weights)


def test_mix_by_hand():
    """one value worked in Python integers, line by line as the header writes it"""
    x = 0x9E3779B9
    y = x ^ (x >> 16)
    y = (y * 0x7FEB352D) & 0xFFFFFFFF
    y ^= y >> 15
    y = (y * 0x846CA68B) & 0xFFFFFFFF
    y ^= y >> 16
    assert int(mix(np.uint64(x))) == y and int(mix(np.uint64(0))) == 0
    assert int(draw(0, 0, 0, 0)) == 0                               # (every term vanishes: the all-zero draw is 0, action 0)
    assert int(draw(0, 0, 0, 1)) == int(mix(np.uint64(0xC2B2AE3D)))


def test_the_model_equals_the_library_bit_for_bit(lib):
    _, lib = lib
    rng = np.random.RandomState(11)
    n = 100000
    seeds = [int(a) << 32 | int(b) for a, b in zip(rng.randint(0, 2 ** 32, n, dtype=np.uint64), rng.randint(0, 2 ** 32, n, dtype=np.uint64))]
    states, samples, steps = rng.randint(0, 2 ** 27, n), rng.randint(0, 65536, n), rng.randint(0, 32767, n)
    states[:4], samples[:4], steps[:4] = (0, 2 ** 27 - 1, 0, 2 ** 27 - 1), (0, 65535, 65535, 0), (0, 32766, 0, 32766)
    draws = np.array([lib.cwh_shoot_draw_of(s, int(j), int(k), int(t)) for s, j, k, t in zip(seeds[:2000], states, samples, steps)], np.uint64)
    assert np.array_equal(draws, draw(np.array(seeds[:2000], dtype=np.uint64), states[:2000], samples[:2000], steps[:2000]))
    assert np.array_equal(_lib_actions(lib, seeds, states, samples, steps), _model(seeds, states, samples, steps))
    # the seeds at the ends, and ones that differ only in the high word: the high word matters
    for base in (0, 2 ** 64 - 1, 5, 5 | 1 << 32, 5 | 1 << 63, 0xFFFFFFFF, 1 << 32):
        s = [base] * 3000
        got = _lib_actions(lib, s, states[:3000], samples[:3000], steps[:3000])
        assert np.array_equal(got, _model(s, states[:3000], samples[:3000], steps[:3000])), base
    a5, a5h = _lib_actions(lib, [5] * 3000, states[:3000], samples[:3000], steps[:3000]), _lib_actions(lib, [5 | 1 << 32] * 3000, states[:3000], samples[:3000], steps[:3000])
    assert (a5 != a5h).mean() > 0.7
    # weights: uniform, random, with zero entries, W == 0, all 65 535
    m = 20000
    for name, w in (('uniform', np.full((m, 6), 7)), ('random', rng.randint(0, 65536, (m, 6))), ('zero entries', rng.randint(0, 65536, (m, 6)) * rng.randint(0, 2, (m, 6))),
                    ('W == 0', np.zeros((m, 6), np.int64)), ('all 65535', np.full((m, 6), 65535)), ('one action', np.eye(6, dtype=np.int64)[rng.randint(0, 6, m)] * 9)):
        got = _lib_actions(lib, seeds[:m], states[:m], samples[:m], steps[:m], w)
        assert np.array_equal(got, _model(seeds[:m], states[:m], samples[:m], steps[:m], w)), name
        assert got.min() >= 0 and got.max() <= 5
        if name in ('W == 0', 'uniform', 'all 65535'):
            plain = _lib_actions(lib, seeds[:m], states[:m], samples[:m], steps[:m])
            assert np.array_equal(got, plain)                                     # equal weights ARE the uniform draw: mulhi(r, 6 w) // w == mulhi(r, 6)
        if name == 'one action':
            assert np.array_equal(got, w.argmax(axis=1))


def _chi2(counts):
    e = counts.sum() / counts.size
    return float(((counts - e) ** 2 / e).sum())


@pytest.mark.parametrize('seed', GRID_SEEDS)
def test_the_draw_is_uniform_and_its_neighbours_are_independent(seed):
    """64^3 triples (state, sample, step): the six actions against 5 degrees of freedom (35.9 is the 1e-6 critical value), and the 36 pairs of neighbours
    along each of the three axes against 35 (89.9) -- the bounds the function was chosen on"""
    a = model_actions(seed, 64, 64, 64)                              # [t, k, j]
    assert _chi2(np.bincount(a.ravel(), minlength=6).astype(np.float64)) < 35.9
    for axis in range(3):
        lo, hi = np.take(a, np.arange(63), axis=axis), np.take(a, np.arange(1, 64), axis=axis)
        assert _chi2(np.bincount((lo * 6 + hi).ravel(), minlength=36).astype(np.float64)) < 89.9, axis


@pytest.mark.parametrize('seed', GRID_SEEDS[:2])
def test_single_rows_along_each_axis(seed):
    n = 6000
    for j, k, t in ((np.arange(n), 3, 5), (7, np.arange(n), 5), (7, 3, np.arange(n))):
        a = action(draw(seed, j, k, t))
        assert _chi2(np.bincount(a, minlength=6).astype(np.float64)) < 35.9
        assert _chi2(np.bincount(a[:-1] * 6 + a[1:], minlength=36).astype(np.float64)) < 89.9


def test_a_zero_weight_is_never_drawn():
    n = 100000
    r = draw(3, np.arange(n) % 1000, np.arange(n) // 1000, 9)
    a = action(r, np.broadcast_to(np.array([1, 0, 3, 0, 0, 4]), (n, 6)))
    share = np.bincount(a, minlength=6) / n
    assert share[1] == share[3] == share[4] == 0
    assert abs(share[0] - 1 / 8) < 0.01 and abs(share[2] - 3 / 8) < 0.01 and abs(share[5] - 4 / 8) < 0.01
    assert (action(np.array([0, 2 ** 32 - 1], np.uint64), np.array([[0, 0, 0, 0, 0, 9], [9, 0, 0, 0, 0, 0]])) == [5, 0]).all()      # the ends of the range


def test_model_actions_layout():
    w = np.random.RandomState(1).randint(0, 9, (3, 6, 4))
    a = model_actions(77, 4, 5, 3, w)
    assert a.shape == (3, 5, 4)
    for t, k, j in ((0, 0, 0), (2, 4, 3), (1, 2, 3)):
        assert a[t, k, j] == action(draw(77, j, k, t), w[t, :, j])
    s = np.array([[4, 0, -1, 2], [1, 1, 1, -5]])
    b = model_actions(77, 4, 5, 3, w, samples=s)
    assert b.shape == (3, 2, 4) and (b[:, 0, 2] == -1).all() and (b[:, 1, 3] == -1).all()
    assert np.array_equal(b[:, 0, 0], a[:, 4, 0]) and np.array_equal(b[:, 1, 2], a[:, 1, 2]) and np.array_equal(b[:, 0, 3], a[:, 2, 3])


# ------------------------------------------------------------------------------------------------------------------------------ the checker
@pytest.fixture(scope='module')
def world():
    """the N oracle envs of records_fixtures, with a goal two steps away where there is one, else one step away, else as they are"""
    dense, init_grids = _world()
    two, one = far_goals(dense, init_grids, np.full(N, 2), OKW), far_goals(dense, init_grids, np.full(N, 1), OKW)
    goal = np.where(two >= 0, two, one)
    return dict(dense, desired=np.where(goal >= 0, goal, dense['desired'])), init_grids


def _rows(want, menu):
    """expected_shoot's result as the ten arrays a call writes"""
    h, p = encode({k: want[k] for k in DENSE}, menu=menu)
    return dict(best_ret=want['best_ret'].astype(np.int32), best_sample=want['best_sample'].astype(np.int32), best_action=want['best_action'].astype(np.uint8),
                length=want['length'].astype(np.int32), done=want['done'].astype(np.uint8), achieved_mask=want['achieved'].astype(np.int16), hdr=h,
                slot_pos=p.view(np.int16), plan=want['plan'].astype(np.uint8), ret=want['ret'].astype(np.int32))


def _correct(dense, init_grids, env_of, weights=None):
    """what a correct call leaves: (before, after, inputs, outputs, expected_shoot, the input states and their init grids)"""
    before = snap(dense, init_grids)
    if env_of is None:
        env, inputs, sub, menu = np.arange(N), None, dense, np.full(N, 3)
    else:
        env = np.where((env_of >= 0) & (env_of < N), env_of, 0)
        sub = {k: v[env] for k, v in dense.items()}
        sub['step_num'] = (sub['step_num'] + np.arange(M)) % MAX_STEPS            # records of the caller's: not the envs' own; some time out inside the horizon
        menu = np.arange(M) % 4
        h, p = encode(sub, menu=menu)
        inputs = dict(hdr=h, slot_pos=p)
    want = expected_shoot(sub, init_grids[env], T, K, SEED, OKW, weights)
    out = _rows(want, menu)
    after = {k: v.copy() for k, v in before.items()}
    if env_of is not None:
        dead = np.flatnonzero((env_of < 0) | (env_of >= N))
        for f, v in out.items():
            if f in ('plan', 'ret'):
                v.view(np.uint8).reshape(v.shape[0], len(env), -1)[:, dead] = SENT
            else:
                v.view(np.uint8).reshape(len(env), -1)[dead] = SENT
        after['counters'][7] += int((env_of >= N).sum())
    return before, after, inputs, out, want, sub, init_grids[env]


def test_expected_shoot_is_the_reduction_of_oracle_simulate(world):
    """by hand: every sample of every state through oracle_simulate one at a time, the maximum and the smallest sample that reaches it in a Python loop"""
    dense, init_grids = world
    want = expected_shoot(dense, init_grids, T, K, SEED, OKW)
    assert want['actions'].shape == (T, K, N) and want['ret'].shape == (K, N) and want['plan'].shape == (T, N)
    for j in range(N):
        best = None
        for k in range(K):
            acts = np.array([[int(action(draw(SEED, j, k, t)))] for t in range(T)])
            r = oracle_simulate({f: v[j:j + 1] for f, v in dense.items()}, init_grids[j:j + 1], acts, True, OKW)
            assert r['ret'][0] == want['ret'][k, j]
            if best is None or r['ret'][0] > best[1]['ret'][0]:
                best = (k, r, acts)
        k, r, acts = best
        assert (want['best_sample'][j], want['best_ret'][j], want['length'][j], want['done'][j]) == (k, r['ret'][0], r['length'][0], r['done'][0])
        assert want['plan'][:, j].tolist() == acts[:, 0].tolist() and want['best_action'][j] == acts[0, 0]
        for f in DENSE:
            assert np.array_equal(want[f][j], r[f][0]), f
    with_w = expected_shoot(dense, init_grids, T, K, SEED, OKW, np.tile(np.array([0, 0, 0, 0, 1, 1])[None, :, None], (T, 1, N)))
    assert set(np.unique(with_w['actions'])) == {4, 5}


@pytest.mark.parametrize('own', [True, False])
def test_a_correct_call_passes(world, own):
    before, after, inputs, out, want, _, _ = _correct(*world, None if own else ENV_OF)
    part, skipped = check_shoot(before, after, inputs, None if own else ENV_OF, T, K, SEED, None, out, SENT, oracle_kw=OKW)
    assert (part, skipped) == ((N, 0) if own else (7, 3))
    for f in out:                                                                 # every single field, and the two records one without the other
        check_shoot(before, after, inputs, None if own else ENV_OF, T, K, SEED, None, {f: out[f]}, SENT, oracle_kw=OKW)
    if not own:
        live = (ENV_OF >= 0) & (ENV_OF < N)
        ok = want['done'] & (want['n_success'] > 0)
        assert (ok & live).any() and (~want['any_success'] & live).any() and ((want['ties'] >= 2) & (want['best_sample'] > 0) & live).any()
        assert ((want['length'] < T) & live).any()
        check_shoot(before, after, inputs, ENV_OF, T, K, SEED, None, out, SENT, oracle_kw=OKW, expected=(_correct(*world, ENV_OF)[5], want))


def test_a_correct_weighted_call_passes(world):
    w = np.random.RandomState(3).randint(0, 5, (T, 6, M)) * 1000
    w[1, :, 3] = 0
    before, after, inputs, out, want, _, _ = _correct(*world, ENV_OF, w)
    check_shoot(before, after, inputs, ENV_OF, T, K, SEED, w, out, SENT, oracle_kw=OKW)
    with pytest.raises(AssertionError):                                           # the same outputs are not those of the uniform draw
        check_shoot(before, after, inputs, ENV_OF, T, K, SEED, None, out, SENT, oracle_kw=OKW)
    with pytest.raises(AssertionError):                                           # ... nor of another seed
        check_shoot(before, after, inputs, ENV_OF, T, K, SEED + 1, w, out, SENT, oracle_kw=OKW)


def _rows_of_sample(sub, inits, want, j, k, menu):
    """the rows a call would write for state j had sample k won"""
    r = oracle_simulate({f: np.asarray(sub[f])[j:j + 1] for f in DENSE}, inits[j:j + 1], want['actions'][:, k, j:j + 1], True, OKW)
    one = dict({f: r[f] for f in DENSE}, best_ret=r['ret'], best_sample=np.array([k]), best_action=want['actions'][0, k, j:j + 1], length=r['length'], done=r['done'],
               plan=want['actions'][:, k, j:j + 1], ret=want['ret'][:, j:j + 1])
    return _rows(one, menu)


def _plant(name, before, after, inputs, out, want, sub, inits):
    live = np.flatnonzero((ENV_OF >= 0) & (ENV_OF < N))
    j0 = int(live[0])
    if name in ('a later maximiser chosen', 'a later maximiser chosen, its sample alone'):
        j = int([j for j in live if want['ties'][j] >= 2 and want['any_success'][j]][0])
        k = int(np.flatnonzero(want['ret'][:, j] == want['best_ret'][j])[1])
        alt = _rows_of_sample(sub, inits, want, j, k, int(inputs['hdr'][j, 3]))
        assert alt['best_ret'][0] == out['best_ret'][j] and k > out['best_sample'][j]
        for f in (FIELDS[:9] if name == 'a later maximiser chosen' else ('best_sample',)):
            if f == 'plan':
                out[f][:, j] = alt[f][:, 0]
            else:
                out[f][j] = alt[f][0]
    elif name == 'a tie broken upward':
        j = int([j for j in live if not want['any_success'][j] and want['ties'][j] == K][0])     # every sample ties: the answer is sample 0
        alt = _rows_of_sample(sub, inits, want, j, K - 1, int(inputs['hdr'][j, 3]))
        for f in FIELDS[:9]:
            if f == 'plan':
                out[f][:, j] = alt[f][:, 0]
            else:
                out[f][j] = alt[f][0]
    elif name == 'one wrong ret[k][j]':
        out['ret'][K - 2, int(live[-1])] -= 1
    elif name == 'one wrong plan byte behind length':
        j = int([j for j in live if want['length'][j] < T][0])
        out['plan'][T - 1, j] = (out['plan'][T - 1, j] + 1) % 6
    elif name == 'plan zeroed behind length':
        j = int([j for j in live if want['length'][j] < T and want['plan'][want['length'][j]:, j].any()][0])
        out['plan'][want['length'][j]:, j] = 0
    elif name == 'best_ret off by one':
        out['best_ret'][j0] += 1
    elif name == 'best_action of another sample':
        out['best_action'][j0] = (out['best_action'][j0] + 1) % 6
    elif name == 'length one short':
        out['length'][j0] -= 1
    elif name == 'done inverted':
        out['done'][j0] ^= 1
    elif name == 'an achieved bit dropped':
        out['achieved_mask'][j0] ^= 1 << 6
    elif name == 'step_num of the final record':
        out['hdr'][j0, 8] += 1
    elif name == 'a slot moved':
        out['slot_pos'][j0, 0] = (out['slot_pos'][j0, 0] + 1) % (S * S) if 0 <= out['slot_pos'][j0, 0] < S * S else 0
    elif name == 'the draw keyed by the env, not the row':
        j = int(live[-2])                                                         # (row 10 is env 0's: row 0's draws)
        out['plan'][:, j] = out['plan'][:, 0]
    elif name == 'a written row of a negative entry':
        out['best_ret'][2] = -T
    elif name == 'a written ret column of a negative entry':
        out['ret'][K - 1, 7] = -T
    elif name == 'a written plan column of a skipped state':
        out['plan'][T - 1, 5] = 0
    elif name == 'an unwritten row':
        out['best_sample'].view(np.uint8).reshape(M, 4)[j0] = SENT
    elif name == 'an unwritten ret row':
        out['ret'].view(np.uint8).reshape(K, M, 4)[K - 1, j0] = SENT
    elif name == 'counters[7] up by G instead of 1':
        after['counters'][7] += 3 * 3                                             # (three skipped states, each counted by its four lanes)
    elif name == 'a skipped state not counted':
        after['counters'][7] -= 1
    elif name == 'counters[0] moved':
        after['counters'][0] += 1
    elif name == 'a changed engine byte':
        after['hdr'][2, 0] ^= 1
    elif name == 'a stream moved':
        after['rng_pos'][4] += 1
    else:
        raise KeyError(name)


FAULTS = ['a later maximiser chosen', 'a later maximiser chosen, its sample alone', 'a tie broken upward', 'one wrong ret[k][j]', 'one wrong plan byte behind length',
          'plan zeroed behind length', 'best_ret off by one', 'best_action of another sample', 'length one short', 'done inverted', 'an achieved bit dropped',
          'step_num of the final record', 'a slot moved', 'the draw keyed by the env, not the row', 'a written row of a negative entry',
          'a written ret column of a negative entry', 'a written plan column of a skipped state', 'an unwritten row', 'an unwritten ret row',
          'counters[7] up by G instead of 1', 'a skipped state not counted', 'counters[0] moved', 'a changed engine byte', 'a stream moved']


@pytest.mark.parametrize('fault', FAULTS)
def test_every_planted_fault_is_caught(world, fault):
    before, after, inputs, out, want, sub, inits = _correct(*world, ENV_OF)
    check_shoot(before, after, inputs, ENV_OF, T, K, SEED, None, out, SENT, oracle_kw=OKW)
    _plant(fault, before, after, inputs, out, want, sub, inits)
    with pytest.raises(AssertionError):
        check_shoot(before, after, inputs, ENV_OF, T, K, SEED, None, out, SENT, oracle_kw=OKW)


def test_nothing_to_compare_is_an_error(world):
    before, after, inputs, out, _, _, _ = _correct(*world, ENV_OF)
    for bad in (dict(env_of=np.full(M, -1)), dict(env_of=np.full(M, N)), dict(outputs={}), dict(env_of=ENV_OF[:-1]),
                dict(after={k: v for k, v in after.items() if k != 'reward'}), dict(T=T + 1), dict(K=K + 1), dict(outputs={'plan': out['plan'][:, :-1]}),
                dict(outputs={'best_ret': out['best_ret'][:-1]}), dict(outputs={'q': out['best_ret']}), dict(inputs=None)):
        kw = dict(dict(before=before, after=after, inputs=inputs, env_of=ENV_OF, T=T, K=K, outputs=out), **bad)
        with pytest.raises(ValueError):
            check_shoot(kw['before'], kw['after'], kw['inputs'], kw['env_of'], kw['T'], kw['K'], SEED, None, kw['outputs'], SENT, oracle_kw=OKW)


# ------------------------------------------------------------------------------------------------------------------------------ what the shared states exercise
@pytest.mark.parametrize('style', [None, 'subset'])
def test_the_recipe_covers_what_it_should(style):
    """counted from the oracle alone, BEFORE anything is compared (the GPU test asserts the same conditions): for each shape at least 200 states whose best
    sample succeeds, 200 with no success at all, 150 whose best sample is not sample 0, 80 of those tied by a later sample; every winning length 1 .. T - 1
    across the shapes; and on the long horizon the class that ends by time-out at step 17"""
    lengths = {6: set(), 12: set()}
    for T_, K_, seed in SHAPES:
        _, _, want = recipe_shots(T_, K_, seed, style, 12)
        cov = coverage(want, T_, RECIPE_KW['max_steps'])
        print(style, T_, K_, seed, cov)
        assert_coverage(cov)
        none = ~want['any_success']
        assert (want['best_sample'][none] == 0).all() and (want['best_ret'][none] == -T_).all()          # every sample ties
        lengths[T_] |= set(cov['lengths'])
        if style is None:                                                         # the figures of the issue that asked for the kernel
            assert (cov['succeed'], cov['none'], cov['later'], cov['later_tied']) == {(6, 5): (276, 324, 157, 83), (6, 8): (282, 318, 169, 124),
                                                                                      (12, 33): (311, 289, 204, 171), (12, 100): (323, 277, 222, 187)}[(T_, K_)]
    assert lengths[6] >= set(range(1, 6)) and lengths[12] >= set(range(1, 12))
    _, _, want = recipe_shots(*LONG, style, 24)
    cov = coverage(want, LONG[0], RECIPE_KW['max_steps'])
    none = ~want['any_success']
    assert cov['timeout'] >= 200 and none.sum() == cov['timeout']
    assert (want['done'][none]).all() and (want['length'][none] == 17).all() and (want['best_ret'][none] == -17).all()
