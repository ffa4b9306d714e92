"""CPU tier: the checker of the plan tests (tests/plan_check.py over records_check.py) itself.  The outputs a correct cw_plan would leave are synthesised on the CPU -- the
oracle's enumeration, reduced, encoded into packed records by the test-side encoder -- and must pass; each planted fault must be caught.  Also here: what
the shared batch of states (plan_check.recipe) exercises, counted from the oracle alone."""
import numpy as np
import pytest

from gym_craftingworld_amd.vec_env import PLAN_FIELDS
from plan_check import (COVERAGE_MIN, FIELDS, RECIPE_KW, RECIPE_N, RECIPE_PART, assert_recipe_coverage, check_plan, coverage, far_goals, oracle_plan,
                        recipe, recipe_env_of, recipe_plans, strings)
from records_check import DENSE, encode, oracle_simulate
from records_fixtures import ENV_OF, M, N, S, SENT, snap, world as _world

MAX_STEPS, D = 9, 3
OKW = dict(size=(S, S), max_steps=MAX_STEPS)


def test_the_checker_knows_the_seven_fields_the_kernel_writes():
    """plan()'s fields are these seven, in the order of cw_plan_out's members, and the two derived from q on top"""
    assert FIELDS == PLAN_FIELDS[:7] and PLAN_FIELDS[7:] == ('best_action', 'best_q')


@pytest.fixture(scope='module')
def world():
    """the N oracle envs of records_fixtures, with a goal two steps away where there is one, else one step away, else as they are"""
    dense, init_grids = _world()
    two, one = far_goals(dense, init_grids, np.full(N, 2), OKW), far_goals(dense, init_grids, np.full(N, 1), OKW)
    goal = np.where(two >= 0, two, one)
    assert (two >= 0).sum() >= 2 and (goal >= 0).sum() >= 3 and (goal < 0).any()
    return dict(dense, desired=np.where(goal >= 0, goal, dense['desired'])), init_grids


def _rows(want, menu):
    """oracle_plan's result as the seven arrays a call writes"""
    m = want['q'].shape[1]
    out = dict(q=want['q'].astype(np.int32), length=want['length'].astype(np.int32), done=want['done'].astype(np.uint8),
               achieved_mask=want['achieved'].astype(np.int16), hdr=np.zeros((len(want['q']), m, 16), np.uint8), slot_pos=np.zeros((len(want['q']), m, 8), np.int16),
               plan=want['plan'].astype(np.uint8))
    for a in range(len(want['q'])):
        h, p = encode({k: want[k][a] for k in DENSE}, menu=menu)
        out['hdr'][a], out['slot_pos'][a] = h, p.view(np.int16)
    return out


def _correct(dense, init_grids, env_of):
    """what a correct call leaves: (before, after, inputs, outputs, the oracle's plans, the states that take part and their init grids)"""
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
    want = oracle_plan(sub, init_grids[env], D, OKW)
    out = _rows(want, menu)
    after = {k: v.copy() for k, v in before.items()}
    if env_of is not None:
        dead = np.flatnonzero((env_of < 0) | (env_of >= N))
        for f, v in out.items():
            if f == 'plan':
                v[:, :, dead] = SENT
            else:
                v.view(np.uint8).reshape(6, len(env), -1)[:, dead] = SENT
        after['counters'][7] += int((env_of >= N).sum())
    return before, after, inputs, out, want, sub, init_grids[env]


def test_oracle_plan_is_the_reduction_of_oracle_simulate(world):
    """by hand: every string of every state through oracle_simulate one at a time, the maximum and the smallest string that reaches it in a Python loop"""
    dense, init_grids = world
    want = oracle_plan(dense, init_grids, D, OKW)
    digits = strings(D)
    assert digits.shape == (D, 6 ** D) and digits[:, 0].tolist() == [0] * D and digits[:, 7].tolist() == [0, 1, 1] and digits[:, -1].tolist() == [5] * D
    for j in range(N):
        one = {k: np.repeat(v[j:j + 1], 6 ** D, axis=0) for k, v in dense.items()}
        r = oracle_simulate(one, np.repeat(init_grids[j:j + 1], 6 ** D, axis=0), digits, True, OKW)
        for a in range(6):
            best = None
            for s in range(a * 6 ** (D - 1), (a + 1) * 6 ** (D - 1)):              # (ascending: the first strict maximum is the smallest maximiser)
                if best is None or r['ret'][s] > r['ret'][best]:
                    best = s
            plan = [x if t < r['length'][best] else 0 for t, x in enumerate(digits[:, best].tolist())]
            assert plan == digits[:, best].tolist()                               # (it is in canonical form already)
            assert (want['q'][a, j], want['length'][a, j], want['done'][a, j]) == (r['ret'][best], r['length'][best], r['done'][best])
            assert want['plan'][a, :, j].tolist() == plan
            for k in DENSE:
                assert np.array_equal(want[k][a, j], r[k][best]), k
            prefixes = {tuple(digits[:r['length'][s], s].tolist()) for s in range(a * 6 ** (D - 1), (a + 1) * 6 ** (D - 1)) if r['ret'][s] == r['ret'][best]}
            assert want['ties'][a, j] == len(prefixes)
    ok = want['done'] & (want['n_success'] > 0)
    assert ok.any() and (~want['done']).any() and (want['q'][~want['done']] == -D).all() and (want['q'][ok] == MAX_STEPS + 1 - want['length'][ok]).all()
    with pytest.raises(ValueError):
        oracle_plan(dense, init_grids, 0, OKW)


@pytest.mark.parametrize('own', [True, False])
def test_a_correct_call_passes(world, own):
    before, after, inputs, out, want, _, _ = _correct(*world, None if own else ENV_OF)
    ok = want['done'] & (want['n_success'] > 0)
    assert ok.any() and (~want['done']).any() and (want['ties'] >= 2).any()
    if not own:
        assert (want['done'] & ~ok).any()                                         # (records near the time-out)
    part, skipped = check_plan(before, after, inputs, None if own else ENV_OF, D, out, SENT, oracle_kw=OKW)
    assert (part, skipped) == ((N, 0) if own else (7, 3))
    for f in out:                                                                 # every single field, and the two records one without the other
        check_plan(before, after, inputs, None if own else ENV_OF, D, {f: out[f]}, SENT, oracle_kw=OKW)


def _second_maximiser(sub, inits, want):
    """-> (a, j, oracle_plan-shaped rows of the SECOND smallest maximiser of that pair) for the first pair of a state that takes part whose maximum two or more
    taken prefixes reach"""
    part = np.flatnonzero((ENV_OF >= 0) & (ENV_OF < N))
    a, j = [(a, j) for a in range(6) for j in part if want['ties'][a, j] >= 2][0]                    # (want holds a column for each of the M records)
    digits, n = strings(D), 6 ** D
    one = {k: np.repeat(np.asarray(sub[k])[j:j + 1], n, axis=0) for k in DENSE}
    r = oracle_simulate(one, np.repeat(inits[j:j + 1], n, axis=0), digits, True, OKW)
    best = [s for s in range(a * n // 6, (a + 1) * n // 6) if r['ret'][s] == want['q'][a, j] and s % 6 ** (D - r['length'][s]) == 0]
    assert len(best) == want['ties'][a, j] and digits[:, best[0]].tolist() == want['plan'][a, :, j].tolist()
    s = best[1]
    return a, j, dict({k: r[k][[s]][None] for k in DENSE}, achieved=r['achieved'][[s]][None], q=r['ret'][[s]][None], length=r['length'][[s]][None], done=r['done'][[s]][None],
                      plan=digits[:, [s]][None])


def _plant(name, before, after, inputs, out, want, sub, inits):
    live = 0                                                                      # (state 0 takes part)
    if name == 'q off by one':
        out['q'][2, live] += 1
    elif name == 'the second-smallest maximiser':
        a, j, rows = _second_maximiser(sub, inits, want)
        alt = _rows(rows, int(inputs['hdr'][j, 3]))
        assert alt['q'][0, 0] == out['q'][a, j] and alt['plan'][0, :, 0].tolist() != out['plan'][a, :, j].tolist()
        for f in FIELDS:
            if f == 'plan':
                out[f][a, :, j] = alt[f][0, :, 0]
            else:
                out[f][a, j] = alt[f][0, 0]
    elif name == 'the second-smallest maximiser, its plan alone':
        a, j, rows = _second_maximiser(sub, inits, want)
        out['plan'][a, :, j] = rows['plan'][0, :, 0]
    elif name == 'plan bytes behind the end':
        part = np.flatnonzero((ENV_OF >= 0) & (ENV_OF < N))
        a, j = [(a, j) for a in range(6) for j in part if want['length'][a, j] < D][0]
        out['plan'][a, D - 1, j] = 3
    elif name == 'length one short':
        out['length'][0, live] -= 1
    elif name == 'done inverted':
        out['done'][5, live] ^= 1
    elif name == 'an achieved bit dropped':
        out['achieved_mask'][1, live] ^= 1 << 6
    elif name == 'step_num of the final record':
        out['hdr'][3, live, 8] += 1
    elif name == 'a slot moved':
        out['slot_pos'][4, live, 0] = (out['slot_pos'][4, live, 0] + 1) % (S * S) if 0 <= out['slot_pos'][4, live, 0] < S * S else 0
    elif name == 'plan[a][0] is not a':
        out['plan'][2, 0, live] = 1
    elif name == 'a written row of a negative entry':
        out['q'][0, 2] = -D                                                       # (state 2: a negative entry)
    elif name == 'a written plan row of a skipped state':
        out['plan'][5, D - 1, 5] = 0                                              # (state 5: env 7 of 5)
    elif name == 'an unwritten row':
        out['q'].view(np.uint8).reshape(6, M, 4)[3, live] = SENT
    elif name == 'an unwritten plan row':
        out['plan'][1, :, live] = SENT
    elif name == 'counters[0] moved':
        after['counters'][0] += 1
    elif name == 'a skipped state not counted':
        after['counters'][7] -= 1
    elif name == 'a changed engine byte':
        after['hdr'][2, 0] ^= 1
    elif name == 'a stream moved':
        after['rng_pos'][4] += 1
    else:
        raise KeyError(name)


FAULTS = ['q off by one', 'the second-smallest maximiser', 'the second-smallest maximiser, its plan alone', 'plan bytes behind the end', 'length one short',
          'done inverted', 'an achieved bit dropped', 'step_num of the final record', 'a slot moved', 'plan[a][0] is not a', 'a written row of a negative entry',
          'a written plan row of a skipped state', 'an unwritten row', 'an unwritten plan row', 'counters[0] moved', 'a skipped state not counted',
          'a changed engine byte', 'a stream moved']


@pytest.mark.parametrize('fault', FAULTS)
def test_every_planted_fault_is_caught(world, fault):
    before, after, inputs, out, want, sub, inits = _correct(*world, ENV_OF)
    check_plan(before, after, inputs, ENV_OF, D, out, SENT, oracle_kw=OKW)
    _plant(fault, before, after, inputs, out, want, sub, inits)
    with pytest.raises(AssertionError):
        check_plan(before, after, inputs, ENV_OF, D, out, SENT, oracle_kw=OKW)


def test_nothing_to_compare_is_an_error(world):
    before, after, inputs, out, _, _, _ = _correct(*world, ENV_OF)
    for bad in (dict(env_of=np.full(M, -1)), dict(env_of=np.full(M, N)), dict(outputs={}), dict(env_of=ENV_OF[:-1]),
                dict(after={k: v for k, v in after.items() if k != 'reward'}), dict(depth=D + 1), dict(outputs={'plan': out['plan'][:, :-1]}),
                dict(outputs={'q': out['q'][:, :-1]}), dict(outputs={'best_q': out['q'][0]}), dict(inputs=None)):
        kw = dict(dict(before=before, after=after, inputs=inputs, env_of=ENV_OF, depth=D, outputs=out), **bad)
        with pytest.raises(ValueError):
            check_plan(kw['before'], kw['after'], kw['inputs'], kw['env_of'], kw['depth'], kw['outputs'], SENT, oracle_kw=OKW)


# ------------------------------------------------------------------------------------------------------------------------------ what the shared states exercise
@pytest.mark.parametrize('style', [None, 'subset'])
def test_the_recipe_covers_what_it_should(style):
    """counted from the oracle alone, BEFORE anything is compared (the GPU test asserts the same conditions): over the (first action, state) pairs of the
    five depths at least 20 best plans that succeed at each length 1 .. 5, 20 that end by time-out, 20 states no plan ends, 20 ties resolved, 20 best plans
    with a pick-up and 20 with a drop -- under each reward rule"""
    covs = {}
    for depth in range(1, 6):
        dense, init_grids, env_of = recipe(depth, style)
        assert len(dense['hold']) == RECIPE_N == len(env_of) and (env_of >= 0).sum() == RECIPE_PART[depth] and np.array_equal(env_of, recipe_env_of(depth))
        assert (env_of[env_of >= 0] == np.flatnonzero(env_of >= 0)).all() and (dense['flags'] == (2 if style else 0)).all()
        sub, want = recipe_plans(depth, style)
        assert len(sub['hold']) == RECIPE_PART[depth] and want['q'].shape == (6, RECIPE_PART[depth]) and want['plan'].shape == (6, depth, RECIPE_PART[depth])
        covs[depth] = coverage(want, depth)
        assert sum(covs[depth]['success'].values()) + covs[depth]['timeout'] + covs[depth]['never'] == 6 * RECIPE_PART[depth]
    print(covs)
    assert COVERAGE_MIN == 20
    assert_recipe_coverage(covs)
    assert covs[5]['success'][5] >= COVERAGE_MIN and covs[4]['success'][4] >= COVERAGE_MIN         # (the full length, at the depths only they reach)
    if style is None:                                                             # the figures the recipe was designed on
        assert (covs[5]['success'][5], covs[5]['success'][4], covs[4]['success'][4], covs[3]['success'][3]) == (38, 14, 82, 157)
    assert RECIPE_KW == dict(size=(5, 5), max_steps=17)
