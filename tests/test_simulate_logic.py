"""CPU tier: the checker of the simulate tests (simulate_check.py, records_check.py) itself.  The outputs a correct cw_simulate would leave are synthesised on the CPU --
the oracle's rollouts, encoded into packed records by the test-side encoder -- and must pass; each planted fault must be caught.  Also here: what the shared
batch of plans (simulate_check.recipe) exercises, counted from the oracle alone."""
import numpy as np
import pytest

from records_check import decode, encode, oracle_simulate
from records_fixtures import ENV_OF, M, N, S, SENT, snap, world as _world
from simulate_check import RECIPE_KW, RECIPE_N, assert_recipe_coverage, check_simulate, coverage, recipe

MAX_STEPS, T = 17, 7
OKW = dict(size=(S, S), max_steps=MAX_STEPS)


@pytest.fixture(scope='module')
def world():
    """the N oracle envs of records_fixtures"""
    return _world()


def _plans(m):
    return np.random.RandomState(3).randint(0, 6, (T, m))


def _correct(dense, init_grids, env_of, stop):
    """what a correct call leaves: (before, after, inputs, actions, outputs) for the M states ENV_OF picks (env_of None: the engine's own states, 2 plans each)"""
    before = snap(dense, init_grids)
    if env_of is None:
        env = np.arange(2 * N) % N
        sub, inputs, menu = {k: v[env] for k, v in dense.items()}, None, np.full(2 * N, 3)
    else:
        env = np.where((env_of >= 0) & (env_of < N), env_of, 0)
        sub = {k: v[env] for k, v in dense.items()}
        sub['step_num'] = (sub['step_num'] + np.arange(M)) % (MAX_STEPS - 3)       # records of the caller's: not the envs' own
        menu = np.arange(M) % 4
    m = len(env)
    acts = _plans(m)
    if env_of is None:                      # every other env wants what its first plan has achieved after two steps: plans that end early
        two = oracle_simulate(dense, init_grids, acts[:2, :N], False, OKW)
        dense = dict(dense, desired=np.where(np.arange(N) % 2 == 0, two['achieved'], dense['desired']))
        sub = {k: v[env] for k, v in dense.items()}
        before = snap(dense, init_grids)
    else:
        two = oracle_simulate(sub, init_grids[env], acts[:2], False, OKW)
        sub['desired'] = np.where(np.arange(m) % 2 == 0, two['achieved'], sub['desired'])
        h, p = encode(sub, menu=menu)
        inputs = dict(hdr=h, slot_pos=p)
    want = oracle_simulate(sub, init_grids[env], acts, stop, OKW)
    h, p = encode({k: want[k] for k in ('grid', 'agent', 'hold', 'achieved', 'desired', 'step_num', 'flags')}, menu=menu)
    out = dict(ret=want['ret'].astype(np.int32), length=want['length'].astype(np.int32), done=want['done'].astype(np.uint8),
               achieved_mask=want['achieved'].astype(np.int16), hdr=h, slot_pos=p.view(np.int16), rewards=want['rewards'].astype(np.int32),
               dones=want['dones'].astype(np.uint8))
    after = {k: v.copy() for k, v in before.items()}
    if env_of is not None:
        dead = np.flatnonzero((env_of < 0) | (env_of >= N))
        for f, v in out.items():
            if f in ('rewards', 'dones'):
                v.view(np.uint8).reshape(T, m, -1)[:, dead] = SENT
            else:
                v.view(np.uint8).reshape(m, -1)[dead] = SENT
        after['counters'][7] += int((env_of >= N).sum())
    return before, after, inputs, acts, out, want


def test_oracle_simulate_is_steps_of_the_oracle(world):
    """one step at a time by OracleEnv.step, the no-op and both stop rules by hand"""
    from oracle import OracleEnv
    dense, init_grids = world
    acts = _plans(N)
    acts[2, 1], acts[4, 3] = 6, 255                                               # the engine's no-op
    for stop in (False, True):
        got = oracle_simulate(dense, init_grids, acts, stop, OKW)
        for j in range(N):
            o = OracleEnv(reward_style='subset' if dense['flags'][j] & 2 else None, **OKW)
            o.set_state(dense['grid'][j], init_grids[j], dense['agent'][j], dense['hold'][j], dense['achieved'][j], dense['desired'][j], dense['step_num'][j])
            ret, ended, taken = 0, None, 0
            for t in range(T):
                if stop and ended is not None:
                    assert got['rewards'][t, j] == 0 and not got['dones'][t, j]
                    continue
                if acts[t, j] > 5:
                    s = o.state()
                    o.set_state(s['grid'], init_grids[j], s['agent'], s['hold'], s['achieved'], s['desired'], s['step_num'] + 1)
                    r, d = -1, s['step_num'] + 1 >= MAX_STEPS
                else:
                    _, r, d, _ = o.step(int(acts[t, j]))
                ret, taken = ret + r, taken + 1
                assert (got['rewards'][t, j], got['dones'][t, j]) == (r, d)
                if d and ended is None:
                    ended = t
            s = o.state()
            assert (got['ret'][j], got['length'][j], got['done'][j], got['taken'][j]) == (ret, T if ended is None else ended + 1, ended is not None, taken)
            assert np.array_equal(got['grid'][j], s['grid']) and tuple(got['agent'][j]) == tuple(s['agent'])
            assert (got['hold'][j], got['achieved'][j], got['desired'][j], got['step_num'][j]) == (s['hold'], s['achieved'], s['desired'], s['step_num'])
            assert got['step_num'][j] == dense['step_num'][j] + taken and got['flags'][j] & 1 == 0 and got['flags'][j] & 2 == dense['flags'][j] & 2
            assert got['flags'][j] >> 2 == (got['rewards'][:, j] == MAX_STEPS).sum()
    with pytest.raises(ValueError):
        oracle_simulate(dense, init_grids, acts[:, :-1], True, OKW)


@pytest.mark.parametrize('stop', [True, False])
@pytest.mark.parametrize('own', [True, False])
def test_a_correct_call_passes(world, own, stop):
    before, after, inputs, acts, out, want = _correct(*world, None if own else ENV_OF, stop)
    assert want['done'].any() and not want['done'].all() and (want['taken'] < T).any() == stop      # (plans that end early, plans that never end)
    part, skipped = check_simulate(before, after, inputs, None if own else ENV_OF, acts, stop, out, SENT, oracle_kw=OKW)
    assert (part, skipped) == ((2 * N, 0) if own else (7, 3))
    for f in out:                                                              # every single field, and the two records one without the other
        check_simulate(before, after, inputs, None if own else ENV_OF, acts, stop, {f: out[f]}, SENT, oracle_kw=OKW)
    if own:                                                                    # the broadcast form as [T, K, N]
        check_simulate(before, after, None, None, acts.reshape(T, 2, N), stop, out, SENT, oracle_kw=OKW)


def _plant(name, before, after, inputs, acts, out, want):
    live = 0                                                                   # (state 0 takes part)
    part = np.flatnonzero((ENV_OF >= 0) & (ENV_OF < N))
    ended = part[want['taken'][part] < T - 1]                                  # (states that take part and end before the last step)
    if name == 'ret off by one reward':
        out['ret'][live] += MAX_STEPS + 1
    elif name == 'length one short':
        out['length'][live] -= 1
    elif name == 'done inverted':
        out['done'][live] ^= 1
    elif name == 'an achieved bit dropped':
        out['achieved_mask'][live] ^= 1 << 6
    elif name == 'step_num of the final record':
        out['hdr'][live, 8] += 1
    elif name == 'a slot moved':
        out['slot_pos'][live, 0] = (out['slot_pos'][live, 0] + 1) % (S * S) if 0 <= out['slot_pos'][live, 0] < S * S else 0
    elif name == 'one traced reward flipped':
        out['rewards'][3, live] = MAX_STEPS if out['rewards'][3, live] != MAX_STEPS else -1
    elif name == 'one traced done flipped':
        out['dones'][0, live] ^= 1
    elif name == 'a must-not-write row written':
        out['ret'][2] = 0                                                      # (state 2: a negative entry)
    elif name == 'a trace row of a skipped state written':
        out['dones'][T - 1, 5] = 0                                             # (state 5: env 7 of 5)
    elif name == 'a frozen state kept stepping':
        j = ended[0]
        sub = {k: v[[j]] for k, v in _decode_inputs(inputs).items()}
        on = oracle_simulate(sub, before['state_init_grid'][[ENV_OF[j]]], acts[:, [j]], False, OKW)
        h, p = encode({k: on[k] for k in ('grid', 'agent', 'hold', 'achieved', 'desired', 'step_num', 'flags')}, menu=int(inputs['hdr'][j, 3]))
        assert not np.array_equal(h[0], out['hdr'][j])
        out['hdr'][j], out['slot_pos'][j] = h[0], p.view(np.int16)[0]
    elif name == 'a trace row after the end not (0, 0)':
        j = ended[0]
        out['rewards'][T - 1, j] = -1
    elif name == 'a trace done after the end':
        j = ended[0]
        out['dones'][T - 1, j] = 1
    elif name == 'counters[0] moved':
        after['counters'][0] += 1
    elif name == 'a skipped state not counted':
        after['counters'][7] -= 1
    elif name == 'an env state moved':
        after['hdr'][2, 0] ^= 1
    elif name == 'a stream moved':
        after['rng_pos'][4] += 1
    else:
        raise KeyError(name)


def _decode_inputs(inputs):
    return {k: v for k, v in decode(inputs['hdr'], inputs['slot_pos'], S).items() if k not in ('menu', 'held_code')}


FAULTS = ['ret off by one reward', 'length one short', 'done inverted', 'an achieved bit dropped', 'step_num of the final record', 'a slot moved',
          'one traced reward flipped', 'one traced done flipped', 'a must-not-write row written', 'a trace row of a skipped state written',
          'a frozen state kept stepping', 'a trace row after the end not (0, 0)', 'a trace done after the end', 'counters[0] moved',
          'a skipped state not counted', 'an env state moved', 'a stream moved']


@pytest.mark.parametrize('fault', FAULTS)
def test_every_planted_fault_is_caught(world, fault):
    before, after, inputs, acts, out, want = _correct(*world, ENV_OF, True)
    check_simulate(before, after, inputs, ENV_OF, acts, True, out, SENT, oracle_kw=OKW)
    _plant(fault, before, after, inputs, acts, out, want)
    with pytest.raises(AssertionError):
        check_simulate(before, after, inputs, ENV_OF, acts, True, out, SENT, oracle_kw=OKW)


def test_nothing_to_compare_is_an_error(world):
    before, after, inputs, acts, out, _ = _correct(*world, ENV_OF, True)
    for bad in (dict(env_of=np.full(M, -1)), dict(env_of=np.full(M, N)), dict(outputs={}), dict(env_of=ENV_OF[:-1]), dict(inputs=None),
                dict(after={k: v for k, v in after.items() if k != 'reward'}), dict(actions=acts[:, :-1]), dict(actions=acts[0]),
                dict(outputs={'rewards': out['rewards'][:-1]}), dict(outputs={'frames': out['ret']})):
        kw = dict(dict(before=before, after=after, inputs=inputs, env_of=ENV_OF, actions=acts, stop_at_done=True, outputs=out), **bad)
        with pytest.raises(ValueError):
            check_simulate(kw['before'], kw['after'], kw['inputs'], kw['env_of'], kw['actions'], kw['stop_at_done'], kw['outputs'], SENT, oracle_kw=OKW)
    with pytest.raises(ValueError):                                            # the broadcast form: a number of plans that is no multiple of the envs
        check_simulate(before, after, None, None, acts[:, :N + 1], True, {'ret': out['ret'][:N + 1]}, SENT, oracle_kw=OKW)


# ------------------------------------------------------------------------------------------------------------------------------ what the shared plans exercise
@pytest.mark.parametrize('style', [None, 'subset'])
def test_the_recipe_covers_what_it_should(style):
    """counted from the oracle alone (the GPU tests assert the same conditions): at T = 12 about half of the 600 states never end and half end by success,
    the successes spread over the step indices; at T = 24 every state has ended, by success or by time-out first; stepped on, a satisfied goal pays again"""
    covs = []
    for horizon in (12, 24):
        dense, init_grids, acts = recipe(horizon, style)
        assert len(dense['hold']) == RECIPE_N and acts.shape == (horizon, RECIPE_N) and np.array_equal(acts[:12], recipe(12, style)[2])
        on = oracle_simulate(dense, init_grids, acts, False, RECIPE_KW)
        covs.append(coverage(on, RECIPE_KW['max_steps']))
        stopped = oracle_simulate(dense, init_grids, acts, True, RECIPE_KW)
        assert np.array_equal(stopped['length'], on['length']) and np.array_equal(stopped['done'], on['done'])
        assert np.array_equal(stopped['taken'], on['length']) and (on['taken'] == horizon).all()
        assert (stopped['rewards'].sum(axis=0) == stopped['ret']).all() and (stopped['ret'] != on['ret']).sum() >= 200
    print(covs)
    assert_recipe_coverage(*covs)
    if style is None:                                                          # the figures the recipe was designed on
        assert (covs[0]['never'], covs[0]['success_first'], covs[0]['paid_after_done']) == (305, 295, 1258)
        assert (covs[1]['success_first'], covs[1]['timeout_first'], covs[1]['never']) == (298, 302, 0)
