"""CPU tier: the checker of the expand tests (tests/expand_check.py) itself.  The outputs a correct cw_expand would leave are synthesised on the CPU -- the
oracle's successors, encoded into packed records by the test-side encoder -- and must pass; each planted fault must be caught."""
import numpy as np
import pytest

from expand_check import POS_GONE, POS_HELD, check_expand, decode, encode, oracle_successors

N, S, MAX_STEPS, SENT = 5, 5, 9, 0xA5
OKW = dict(size=(S, S), max_steps=MAX_STEPS)
ENV_OF = np.array([0, 4, -1, 2, 2, 7, 1, -7, 3, 5 + 31, 0, 2 ** 31 - 1], np.int64)       # 12 states: 7 take part (env 2 and 0 twice), 2 take none, 3 are skipped
M = len(ENV_OF)


def _world():
    """N oracle envs some steps into their episodes -> (dense states [N], their init grids)"""
    from oracle import OracleEnv
    rng = np.random.RandomState(5)
    st = []
    for i in range(N):
        o = OracleEnv(**OKW)
        o.seed_int(100 + i)
        o.reset()
        for a in rng.randint(0, 6, 4 + i):
            o.step(int(a))
        st.append(o.state())
    dense = dict(grid=np.stack([s['grid'] for s in st]), agent=np.array([s['agent'] for s in st]), hold=np.array([s['hold'] for s in st]),
                 achieved=np.array([s['achieved'] for s in st]), desired=np.array([s['desired'] for s in st]),
                 step_num=np.array([min(s['step_num'], MAX_STEPS - 2) for s in st]), flags=np.array([2 * (i % 2) for i in range(N)]))
    return dense, np.stack([s['init_grid'] for s in st])


@pytest.fixture(scope='module')
def world():
    return _world()


def _snap(dense, init_grids):
    """a take()-shaped snapshot of the N envs (what check_expand reads of it, and some buffers it must find unchanged)"""
    hdr, pos = encode(dense, menu=3)
    r = np.random.RandomState(2)
    return dict(state_grid=dense['grid'].copy(), state_init_grid=init_grids.copy(), rng_pos=r.randint(1, 625, N).astype(np.int32),
                rng_key=r.randint(0, 2 ** 31, (N, 624)).astype(np.uint32), hdr=hdr, slot_pos=pos.view(np.int16), reward=np.full(N, -1, np.int32),
                done=np.zeros(N, bool), counters=np.arange(8, dtype=np.int64) * 11)


def _correct(dense, init_grids, env_of):
    """what a correct call leaves: (inputs, outputs, after-snapshot) for the M states ENV_OF picks (env_of None: the engine's own states)"""
    before = _snap(dense, init_grids)
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
