"""CPU tests of the comparator the GPU parity tests rest on (tests/oracle_replay.py).  A second OracleBatch plays the engine: its arrays, under the
names snapshot() gives the engine's, must pass compare_with_oracle / same_states; with ONE element of any compared quantity changed they must fail and
name the quantity and the env; a call that would compare nothing (no rows, an unknown array, mismatched shapes) is an error.  And OracleBatch.step
with details=True, which the lock-step tests use, is the same run as OracleBatch.rollout."""
import types

import numpy as np
import pytest

from oracle import OracleBatch
from oracle_replay import FRAMES, STATE, compare_with_oracle, np_states, one_hot_of, oracle_arrays, same_states, set_phase, snapshot

N, T = 24, 40
MENUS = [dict(), dict(selected_tasks=['GoToHouse', 'EatBread'], number_of_tasks=1, reward_style='subset'), dict(selected_tasks=['ChopTree'], stacking=False)]
CONFIGS = {'ray': (dict(size=(5, 5), max_steps=9), None),
           'alt': (dict(size=(6, 6), max_steps=9, alt_obs=True), None),
           'pool': (dict(size=(5, 5), max_steps=9, fixed_init_state=3), None),
           'menus': (dict(size=(5, 5), max_steps=9), [MENUS[i % 3] for i in range(N)])}
PHASE = (np.arange(N) % 8).astype(np.int32)                  # (three envs time out on every step, the last one included)


def _engine_run(name):
    """an OracleBatch in the engine's place: T recorded steps -> (snap, the other arguments of compare_with_oracle, the batch itself)"""
    kw, per_env = CONFIGS[name]
    keys, pos = np_states(N, 900)
    ora = OracleBatch(N, rng_states=list(zip(keys, pos)), per_env_kwargs=per_env, **kw)
    ora.reset()
    set_phase(ora, PHASE)
    acts = np.random.RandomState(3).randint(0, 6, size=(T, N))
    rew, don = np.empty((T, N), np.int32), np.empty((T, N), bool)
    for t in range(T):
        rew[t], don[t], _, term = ora.step(acts[t], details=True)
    snap = oracle_arrays(ora.envs, list(FRAMES) + ['rng_key'] + ['pool'] * (name == 'pool'))
    snap['idx'] = np.arange(N)
    snap['terminal_observation'] = np.zeros_like(snap['observation'])
    for j, frame in term.items():
        snap['terminal_observation'][j] = frame
    assert term and don.sum() > N
    return snap, (keys, pos, kw, acts, rew, don, PHASE, per_env), ora


@pytest.mark.parametrize('name', list(CONFIGS))
def test_a_second_oracle_passes_and_the_run_is_counted(name):
    snap, args, _ = _engine_run(name)
    assert set(STATE) < set(snap) and ('pool' in snap) == (name == 'pool')
    res = compare_with_oracle(snap, *args)
    rew, don = args[4], args[5]
    assert res['finished'] == int(don.sum()) and res['successes'] == int((rew == 9).sum()) and np.array_equal(res['done_per_env'], don.sum(axis=0))
    if name == 'menus':                                      # (the menus matter: without them the replay is another run)
        with pytest.raises(AssertionError):
            compare_with_oracle(snap, *args[:-1])


def test_a_sample_of_rows_is_replayed_and_named_by_its_engine_index():
    snap, args, _ = _engine_run('menus')
    idx = np.array([3, 10, 17])
    part = {k: v[idx] for k, v in snap.items()}
    res = compare_with_oracle(part, *args)
    assert np.array_equal(res['done_per_env'], args[5].sum(axis=0)[idx]) and res['finished'] == int(args[5][:, idx].sum())
    part['hold'][1] += 1
    with pytest.raises(AssertionError, match=r'hold differs from the oracle at 1 envs, first \[10\]'):
        compare_with_oracle(part, *args)


QUANTITIES = ['reward', 'done'] + list(STATE) + list(FRAMES) + ['terminal_observation', 'rng_key', 'rng_pos', 'pool']


@pytest.mark.parametrize('what', QUANTITIES)
def test_one_changed_element_fails_and_is_named(what):
    snap, args, _ = _engine_run('pool')
    keys, pos, kw, acts, rew, don, phase, per_env = args
    e = 5
    if what == 'reward':
        rew[T // 2, e] += 1
    elif what == 'done':
        don[T // 2, e] ^= True
    elif what == 'terminal_observation':
        e = int(np.nonzero(don[T - 1])[0][-1])               # (a frame that is compared: of an env that finished on the last step)
        snap[what][e, 0, 0, 0] ^= 1
    else:
        snap[what][(e,) + (-1,) * (snap[what].ndim - 1)] ^= 1
    with pytest.raises(AssertionError, match=r'%s.* differs from the oracle at 1 envs, first \[%d\]' % (what, e)):
        compare_with_oracle(snap, keys, pos, kw, acts, rew, don, phase, per_env)


def test_a_terminal_frame_of_an_env_that_did_not_finish_is_not_looked_at():
    snap, args, _ = _engine_run('ray')
    snap['terminal_observation'][int(np.nonzero(~args[5][T - 1])[0][0])] ^= 1      # (rows are valid where done: craftingworld.h)
    compare_with_oracle(snap, *args)


def test_same_states_against_a_batch_stepped_alongside():
    snap, _, _ = _engine_run('alt')
    _, _, ora = _engine_run('alt')
    same_states(snap, ora, frames=tuple(FRAMES))
    same_states({k: v[[4, 9]] for k, v in snap.items()}, types.SimpleNamespace(envs=[ora.envs[4], ora.envs[9]]), frames=tuple(FRAMES))
    snap['render'], snap['grid_export'], snap['one_hot'] = snap['observation'], snap['grid'], one_hot_of(snap['grid'], snap['agent_rc'], snap['hold'])
    same_states(snap, ora, frames=('render', 'grid_export', 'one_hot'))
    snap['one_hot'][7, 0, 0, 11] ^= 1
    with pytest.raises(AssertionError, match=r'one_hot differs from the oracle at 1 envs, first \[7\]'):
        same_states(snap, ora, frames=('one_hot',))
    snap['desired'][2] ^= 4
    with pytest.raises(AssertionError, match=r'step 3: desired differs from the oracle at 1 envs, first \[2\]'):
        same_states(snap, ora, tag='step 3: ')
    snap['desired'][2] ^= 4
    snap['desired_goal'][23, -1, -1, 2] ^= 1
    same_states(snap, ora, frames=('observation',))          # (only what was asked for ...)
    with pytest.raises(AssertionError, match=r'desired_goal differs from the oracle at 1 envs, first \[23\]'):
        same_states(snap, ora, frames=tuple(FRAMES))
    snap['rng_pos'][0] += 1
    same_states(snap, ora, rng=False)                        # (... and the RNG state unless it is switched off)
    with pytest.raises(AssertionError, match=r'rng_pos differs from the oracle at 1 envs, first \[0\]'):
        same_states(snap, ora)


def test_calls_that_would_compare_nothing_are_errors():
    snap, args, ora = _engine_run('ray')
    keys, pos, kw, acts, rew, don, phase, _ = args
    engine = types.SimpleNamespace(num_envs=N)               # (refused before anything is read from it)
    for idx in ([], [N], [-1], [[0, 1]]):
        with pytest.raises(ValueError):
            snapshot(engine, idx=idx)
    with pytest.raises(ValueError, match='obs'):
        snapshot(engine, frames=('observation', 'obs'))
    with pytest.raises(ValueError, match='render'):
        same_states(snap, ora, frames=('render',))           # an array the snapshot does not hold
    with pytest.raises(ValueError, match='rng'):
        same_states({k: v for k, v in snap.items() if not k.startswith('rng')}, ora)
    with pytest.raises(ValueError):
        same_states({k: v[:5] for k, v in snap.items()}, ora)                   # 5 rows against 24 oracle envs
    with pytest.raises(ValueError, match='frame0'):
        compare_with_oracle(dict(snap, frame0=snap['observation']), *args)     # an entry nobody compares
    for a, r, d in ((acts[:-1], rew, don), (acts, rew[:, :-1], don), (acts, rew, don[1:]), (acts[0], rew[0], don[0])):
        with pytest.raises(ValueError):
            compare_with_oracle(snap, keys, pos, kw, a, r, d, phase)


@pytest.mark.parametrize('name', ['ray', 'menus'])
def test_lock_step_oracle_equals_its_rollout(name):
    snap, (keys, pos, kw, acts, rew, don, phase, per_env), _ = _engine_run(name)
    ora = OracleBatch(N, rng_states=list(zip(keys, pos)), per_env_kwargs=per_env, **kw)
    ora.reset()
    set_phase(ora, phase)
    total, o_rew, o_don = ora.rollout(acts, nthreads=2, record=True)
    assert total == N * T and np.array_equal(o_rew, rew) and np.array_equal(o_don.astype(bool), don)
    same_states(snap, ora, frames=tuple(FRAMES))
    plain = OracleBatch(N, rng_states=list(zip(keys, pos)), per_env_kwargs=per_env, **kw)      # (without details: the same steps)
    plain.reset()
    set_phase(plain, phase)
    for t in range(T):
        r, d = plain.step(acts[t])
        assert np.array_equal(r, rew[t]) and np.array_equal(d, don[t]), t
    same_states(snap, plain, frames=tuple(FRAMES))


def test_lock_step_oracle_details_and_no_auto_reset():
    keys, pos = np_states(N, 900)
    kw = CONFIGS['ray'][0]
    a, b = (OracleBatch(N, rng_states=list(zip(keys, pos)), **kw) for _ in range(2))
    a.reset(), b.reset()
    acts = np.random.RandomState(3).randint(0, 6, size=(T, N))
    same_run = True
    for t in range(T):
        before = oracle_arrays(a.envs, ('observation',))
        r, d, ach, term = a.step(acts[t], details=True)
        assert sorted(term) == np.nonzero(d)[0].tolist()
        after = oracle_arrays(a.envs, ('observation',))
        for j in range(N):
            if d[j]:                                         # reset: a new episode; the mask returned is the finished one's
                assert after['ep_no'][j] == before['ep_no'][j] + 1 and after['step_num'][j] == 0 and term[j].shape == after['observation'][j].shape
                assert (ach[j] == before['desired'][j]) == (r[j] == 9)
            else:
                assert ach[j] == after['achieved'][j] and after['step_num'][j] == before['step_num'][j] + 1
        rb, db = b.step(acts[t], auto_reset=False)
        if same_run:                                         # (up to the step on which the first env is done)
            assert np.array_equal(r, rb) and np.array_equal(d, db), t
            same_run = not d.any()
    end = oracle_arrays(b.envs, ())
    assert (end['ep_no'] == 0).all() and (end['step_num'] == T).all()             # stepped past done, never reset
