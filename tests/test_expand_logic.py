"""CPU tier: the checker of the expand tests (expand_check.py over records_check.py) itself.  The outputs a correct cw_expand would leave are synthesised on the CPU -- the
oracle's successors, encoded into packed records by the test-side encoder -- and must pass; each planted fault must be caught."""
import numpy as np
import pytest

from expand_check import check_expand, oracle_successors
from records_check import POS_GONE, POS_HELD, decode, encode
from records_fixtures import ENV_OF, M, N, S, SENT, snap, world as _world

MAX_STEPS = 9
OKW = dict(size=(S, S), max_steps=MAX_STEPS)


@pytest.fixture(scope='module')
def world():
    return _world()


def _correct(dense, init_grids, env_of):
    """what a correct call leaves: (inputs, outputs, after-snapshot) for the M states ENV_OF picks (env_of None: the engine's own states)"""
    before = snap(dense, init_grids)
    if env_of is None:
        env, inputs, sub = np.arange(N), None, dense
        menu = np.full(N, 3)
    else:
        env = np.where((env_of >= 0) & (env_of < N), env_of, 0)                # (a state that takes no part still is a record)
        sub = {k: v[env] for k, v in dense.items()}
        sub['step_num'] = (sub['step_num'] + np.arange(M)) % MAX_STEPS            # records of the caller's: not the envs' own
        menu = np.arange(M) % 4
        h, p = encode(sub, menu=menu)
        inputs = dict(hdr=h, slot_pos=p)
    m = len(env)
    suc = oracle_successors(sub, init_grids[env], OKW)
    out = dict(reward=np.full((6, m), 0, np.int32), done=np.zeros((6, m), np.uint8), changed=np.zeros((6, m), np.uint8), achieved_mask=np.zeros((6, m), np.int16),
               hdr=np.zeros((6, m, 16), np.uint8), slot_pos=np.zeros((6, m, 8), np.int16))
    for a in range(6):
        h, p = encode({k: suc[k][a] for k in ('grid', 'agent', 'hold', 'achieved', 'desired', 'step_num', 'flags')}, menu=menu)
        out['hdr'][a], out['slot_pos'][a] = h, p.view(np.int16)
        out['reward'][a], out['done'][a], out['changed'][a], out['achieved_mask'][a] = suc['reward'][a], suc['done'][a], suc['changed'][a], suc['achieved'][a]
    after = {k: v.copy() for k, v in before.items()}
    if env_of is not None:
        dead = np.flatnonzero((env_of < 0) | (env_of >= N))
        for v in out.values():
            v.view(np.uint8).reshape(6, m, -1)[:, dead] = SENT
        after['counters'][7] += int((env_of >= N).sum())
    return before, after, inputs, out


def test_decode_inverts_encode(world):
    dense, _ = world
    hdr, pos = encode(dense, menu=2)
    got = decode(hdr, pos, S)
    for k in ('grid', 'agent', 'hold', 'achieved', 'desired', 'step_num', 'flags'):
        assert np.array_equal(got[k], dense[k]), k
    assert (got['menu'] == 2).all() and np.array_equal(got['held_code'], dense['hold'])
    assert ((pos == POS_HELD).sum(axis=1) == (dense['hold'] > 0)).all() and (pos == POS_GONE).any()
    with pytest.raises(ValueError):
        encode(dict(dense, grid=np.ones_like(dense['grid'])))
    with pytest.raises(ValueError):
        decode(hdr, pos[:-1], S)


def test_oracle_successors_are_steps_of_the_oracle(world):
    """up / right / down / left move the agent one cell or not at all; a successor's step_num is one up; changed is what the name says"""
    dense, init_grids = world
    suc = oracle_successors(dense, init_grids, OKW)
    assert np.array_equal(suc['step_num'], np.broadcast_to(dense['step_num'] + 1, (6, N)))
    assert np.array_equal(suc['desired'], np.broadcast_to(dense['desired'], (6, N))) and (suc['flags'] & 1 == 0).all()
    for a, (dr, dc) in enumerate([(-1, 0), (0, 1), (1, 0), (0, -1)]):
        d = suc['agent'][a] - dense['agent']
        assert (((d == (dr, dc)).all(axis=1)) | ((d == 0).all(axis=1))).all()
        assert np.array_equal(suc['changed'][a], (d != 0).any(axis=1))
    assert np.array_equal(suc['changed'][4], suc['hold'][4] != dense['hold']) and np.array_equal(suc['changed'][5], suc['hold'][5] != dense['hold'])
    assert suc['changed'].any() and not suc['changed'].all() and set(np.unique(suc['reward'])) <= {-1, MAX_STEPS}


def test_oracle_successors_against_the_oracles_own_wrappers(world):
    """one action at a time by OracleEnv.set_state + .step, under each state's own reward rule: every field, `changed` and the flags word worked by hand --
    oracle_successors is pinned to the oracle, not to oracle_simulate"""
    from oracle import OracleEnv
    dense, init_grids = world
    dense = dict(dense, flags=dense['flags'] | 1 | (np.arange(N) * 4), desired=np.where(np.arange(N) % 2, dense['desired'], 0))   # (an empty goal pays at once)
    suc = oracle_successors(dense, init_grids, OKW)
    assert (suc['reward'] == MAX_STEPS).any() and (suc['reward'] == -1).any()
    for j in range(N):
        o = OracleEnv(reward_style='subset' if dense['flags'][j] & 2 else None, **OKW)
        for a in range(6):
            o.set_state(dense['grid'][j], init_grids[j], dense['agent'][j], dense['hold'][j], dense['achieved'][j], dense['desired'][j], dense['step_num'][j])
            _, r, d, _ = o.step(a)
            s = o.state()
            assert (suc['reward'][a, j], suc['done'][a, j]) == (r, d)
            assert np.array_equal(suc['grid'][a, j], s['grid']) and tuple(suc['agent'][a, j]) == tuple(s['agent'])
            assert (suc['hold'][a, j], suc['achieved'][a, j], suc['desired'][a, j], suc['step_num'][a, j]) == (s['hold'], s['achieved'], s['desired'], s['step_num'])
            moved = not np.array_equal(s['grid'], dense['grid'][j]) or tuple(s['agent']) != tuple(dense['agent'][j]) or s['hold'] != dense['hold'][j]
            assert suc['changed'][a, j] == moved
            assert suc['flags'][a, j] == (dense['flags'][j] & 2) | (((dense['flags'][j] >> 2) + (r == MAX_STEPS)) << 2)
    assert {k: (v.shape, v.dtype) for k, v in suc.items()} == dict(
        reward=((6, N), np.int64), done=((6, N), bool), changed=((6, N), bool), grid=((6, N, S, S), np.uint8), agent=((6, N, 2), np.int64),
        hold=((6, N), np.int64), achieved=((6, N), np.int64), desired=((6, N), np.int64), step_num=((6, N), np.int64), flags=((6, N), np.int64))
    top = oracle_successors(dict(dense, flags=np.full(N, 0x3FFF << 2)), init_grids, OKW)['flags']      # (the count saturates)
    assert (top == 0x3FFF << 2).all()


@pytest.mark.parametrize('own', [True, False])
def test_a_correct_call_passes(world, own):
    before, after, inputs, out = _correct(*world, None if own else ENV_OF)
    part, skipped = check_expand(before, after, inputs, None if own else ENV_OF, out, SENT, oracle_kw=OKW)
    assert (part, skipped) == ((N, 0) if own else (7, 3))
    for f in out:                                                              # every single field, and the two records one without the other
        check_expand(before, after, inputs, None if own else ENV_OF, {f: out[f]}, SENT, oracle_kw=OKW)


def _plant(name, before, after, inputs, out):
    live = 0                                                                   # (state 0 takes part)
    if name == 'one reward flipped':
        out['reward'][3, live] = MAX_STEPS if out['reward'][3, live] == -1 else -1
    elif name == 'row (a, j) holds action a + 1':
        a, j = [(a, j) for a in range(5) for j in (0, 1, 3, 4) if not np.array_equal(out['hdr'][a, j], out['hdr'][a + 1, j])][0]
        for v in out.values():
            v[a, j] = v[a + 1, j]
    elif name == 'a must-not-write row written':
        out['done'][2, 2] = 0                                                  # (state 2: a negative entry)
    elif name == 'a skipped row written':
        out['slot_pos'][5, 5, 7] = 3                                           # (state 5: env 7 of 5)
    elif name == 'counters[0] moved':
        after['counters'][0] += 1
    elif name == 'a skipped state not counted':
        after['counters'][7] -= 1
    elif name == 'skipped states counted once per action':
        after['counters'][7] += 5 * 3
    elif name == 'step_num not incremented':
        out['hdr'][1, live, 8] -= 1
    elif name == 'flag bit 0 left set':
        out['hdr'][0, live, 10] |= 1
    elif name == 'the success count not kept':
        out['hdr'][4, live, 10] ^= 4
    elif name == 'the menu byte lost':
        out['hdr'][2, 1, 3] = 0                                                # (state 1: menu 1)
    elif name == 'changed inverted':
        out['changed'][5, live] ^= 1
    elif name == 'an achieved bit dropped':
        out['achieved_mask'][0, live] ^= 1 << 6
    elif name == 'an env state moved':
        after['hdr'][2, 0] ^= 1
    elif name == 'a stream moved':
        after['rng_pos'][4] += 1
    else:
        raise KeyError(name)


FAULTS = ['one reward flipped', 'row (a, j) holds action a + 1', 'a must-not-write row written', 'a skipped row written', 'counters[0] moved',
          'a skipped state not counted', 'skipped states counted once per action', 'step_num not incremented', 'flag bit 0 left set',
          'the success count not kept', 'the menu byte lost', 'changed inverted', 'an achieved bit dropped', 'an env state moved', 'a stream moved']


@pytest.mark.parametrize('fault', FAULTS)
def test_every_planted_fault_is_caught(world, fault):
    before, after, inputs, out = _correct(*world, ENV_OF)
    _plant(fault, before, after, inputs, out)
    with pytest.raises(AssertionError):
        check_expand(before, after, inputs, ENV_OF, out, SENT, oracle_kw=OKW)


def test_nothing_to_compare_is_an_error(world):
    before, after, inputs, out = _correct(*world, ENV_OF)
    with pytest.raises(ValueError):
        check_expand(before, after, inputs, np.full(M, -1), out, SENT, oracle_kw=OKW)
    with pytest.raises(ValueError):
        check_expand(before, after, inputs, np.full(M, N), out, SENT, oracle_kw=OKW)
    with pytest.raises(ValueError):
        check_expand(before, after, inputs, ENV_OF, {}, SENT, oracle_kw=OKW)
    with pytest.raises(ValueError):
        check_expand(before, after, inputs, ENV_OF[:-1], out, SENT, oracle_kw=OKW)
    with pytest.raises(ValueError):
        check_expand(before, after, None, ENV_OF, out, SENT, oracle_kw=OKW)
    with pytest.raises(ValueError):
        check_expand(before, {k: v for k, v in after.items() if k != 'reward'}, inputs, ENV_OF, out, SENT, oracle_kw=OKW)
