"""CPU tier: the checker of the unroll tests (unroll_check.py) itself.  oracle_unroll -- a chain of one-step oracle calls -- is compared with the T-step
oracle_simulate on the shared batch of plans; the outputs a correct cw_unroll would leave are synthesised on the CPU and must pass; each planted fault must be
caught at its field."""
import numpy as np
import pytest

from records_check import DENSE, encode, oracle_simulate
from records_fixtures import ENV_OF, M, N, S, SENT, snap, world as _world
from simulate_check import RECIPE_KW, RECIPE_N, recipe
from unroll_check import FIELDS, TRACES, check_unroll, layout, oracle_unroll

MAX_STEPS, T = 17, 7
OKW = dict(size=(S, S), max_steps=MAX_STEPS)


@pytest.fixture(scope='module')
def world():
    """the N oracle envs of records_fixtures"""
    return _world()


# ------------------------------------------------------------------------------------------------------------------------------ the chain against the T-step call
@pytest.mark.parametrize('stop', [True, False])
@pytest.mark.parametrize('style', [None, 'subset'])
@pytest.mark.parametrize('horizon', [12, 24])
def test_the_chain_equals_the_T_step_call(horizon, style, stop):
    """row T, the traces and length are oracle_simulate's for the same arguments; row 0 is the input; every row in between is one step of the row before
    it; what is not taken is zero and repeats"""
    dense, init_grids, acts = recipe(horizon, style)
    u = oracle_unroll(dense, init_grids, acts, stop, RECIPE_KW)
    s = oracle_simulate(dense, init_grids, acts, stop, RECIPE_KW)
    assert u['reward'].shape == (horizon, RECIPE_N) and u['grid'].shape == (horizon + 1, RECIPE_N, 5, 5)
    for k in DENSE:                                                            # every dense field and the flags
        assert np.array_equal(u[k][horizon], s[k]), k
        assert np.array_equal(u[k][0], dense[k]), k
    assert np.array_equal(u['reward'], s['rewards']) and np.array_equal(u['done'], s['dones']) and np.array_equal(u['length'], s['length'])
    assert np.array_equal(u['taken'].sum(axis=0), s['taken'])
    assert np.array_equal(u['taken'], np.arange(horizon)[:, None] < s['taken'][None, :])      # (the steps taken are the first ones)
    idle = ~u['taken']
    assert not (u['reward'][idle].any() or u['done'][idle].any() or u['changed'][idle].any())
    for k in DENSE:
        assert np.array_equal(u[k][1:][idle], u[k][:-1][idle]), k
    assert idle.any() == stop and ((~idle).all() or stop)
    if stop:
        assert (s['taken'] < horizon).sum() >= 200
    if horizon == 12:                                                          # counted: 3 666 of 7 200 steps change the state when every step is taken
        n = int(u['changed'].sum())
        assert n >= 1000 and u['changed'].size - n >= 1000
        if not stop and style is None:
            assert n == 3666
    t = horizon // 2                                                           # a row in between: one more one-step call from the row before it
    one = oracle_simulate({k: u[k][t] for k in DENSE}, init_grids, acts[t:t + 1], False, RECIPE_KW)
    on = u['taken'][t]
    for k in DENSE:
        assert np.array_equal(u[k][t + 1][on], one[k][on]), k


def test_the_no_op_changes_nothing_but_the_step_count(world):
    dense, init_grids = world
    acts = np.random.RandomState(4).randint(0, 6, (T, N))
    acts[1], acts[3, 2], acts[5, 4] = 6, 200, 255
    u = oracle_unroll(dense, init_grids, acts, False, OKW)
    for t, j in [(1, j) for j in range(N)] + [(3, 2), (5, 4)]:
        assert not u['changed'][t, j] and u['reward'][t, j] == -1 and u['step_num'][t + 1, j] == u['step_num'][t, j] + 1
        assert np.array_equal(u['grid'][t + 1, j], u['grid'][t, j]) and u['achieved'][t + 1, j] == u['achieved'][t, j]
    assert u['changed'].any()
    with pytest.raises(ValueError):
        oracle_unroll(dense, init_grids, acts[:, :-1], True, OKW)


# ------------------------------------------------------------------------------------------------------------------------------ a correct call, and planted faults
def _plans(m):
    a = np.random.RandomState(3).randint(0, 6, (T, m))
    a[0, 0], a[4, min(3, m - 1)] = 6, 255                                      # the no-op among them
    return a


def _correct(dense, init_grids, env_of, stop):
    """what a correct call leaves: (before, after, inputs, actions, outputs, want) for the M states ENV_OF picks (env_of None: the engine's own states, 2
    plans each)"""
    if env_of is None:
        env = np.arange(2 * N) % N
        acts = _plans(2 * N)
        two = oracle_simulate(dense, init_grids, acts[:2, :N], False, OKW)     # every other env wants what its first plan has achieved after two steps
        dense = dict(dense, desired=np.where(np.arange(N) % 2 == 0, two['achieved'], dense['desired']))
        before = snap(dense, init_grids)
        sub, inputs, menu = {k: v[env] for k, v in dense.items()}, None, np.full(2 * N, 3)
        read = dict(hdr=before['hdr'][env], slot_pos=before['slot_pos'][env])
    else:
        before = snap(dense, init_grids)
        env = np.where((env_of >= 0) & (env_of < N), env_of, 0)
        acts = _plans(M)
        sub = {k: v[env] for k, v in dense.items()}
        sub['step_num'] = (sub['step_num'] + np.arange(M)) % (MAX_STEPS - 3)   # records of the caller's: not the envs' own
        menu = np.arange(M) % 4
        two = oracle_simulate(sub, init_grids[env], acts[:2], False, OKW)
        sub['desired'] = np.where(np.arange(M) % 2 == 0, two['achieved'], sub['desired'])
        h, p = encode(sub, menu=menu)
        inputs = read = dict(hdr=h, slot_pos=p.view(np.int16))
    m = len(env)
    want = oracle_unroll(sub, init_grids[env], acts, stop, OKW)
    hdr, pos = np.zeros((T + 1, m, 16), np.uint8), np.zeros((T + 1, m, 8), np.int16)
    hdr[0], pos[0] = read['hdr'], read['slot_pos']
    for t in range(1, T + 1):
        h, p = encode({k: want[k][t] for k in DENSE}, menu=menu)
        hdr[t], pos[t] = h, p.view(np.int16)
    out = dict(hdr=hdr, slot_pos=pos, reward=want['reward'].astype(np.int32), done=want['done'].astype(np.uint8), changed=want['changed'].astype(np.uint8),
               taken=want['taken'].astype(np.uint8), length=want['length'].astype(np.int32))
    after = {k: v.copy() for k, v in before.items()}
    if env_of is not None:
        dead = np.flatnonzero((env_of < 0) | (env_of >= N))
        for f, v in out.items():
            v.view(np.uint8).reshape(layout(T)[f] + (m, -1))[..., dead, :] = SENT
        after['counters'][7] += int((env_of >= N).sum())
    return before, after, inputs, acts, out, want


@pytest.mark.parametrize('stop', [True, False])
@pytest.mark.parametrize('own', [True, False])
def test_a_correct_call_passes(world, own, stop):
    before, after, inputs, acts, out, want = _correct(*world, None if own else ENV_OF, stop)
    assert want['done'].any() and not want['done'].any(axis=0).all() and (~want['taken']).any() == stop
    assert want['changed'].any() and not want['changed'][want['taken']].all()
    e = None if own else ENV_OF
    part, skipped = check_unroll(before, after, inputs, e, acts, stop, out, SENT, oracle_kw=OKW)
    assert (part, skipped) == ((2 * N, 0) if own else (7, 3))
    for f in out:                                                              # every single field, and the two records one without the other
        check_unroll(before, after, inputs, e, acts, stop, {f: out[f]}, SENT, oracle_kw=OKW)
    if own:                                                                    # the broadcast form as [T, K, N]
        check_unroll(before, after, None, None, acts.reshape(T, 2, N), stop, out, SENT, oracle_kw=OKW)
    else:                                                                      # what a test computed beforehand
        pick = np.flatnonzero((ENV_OF >= 0) & (ENV_OF < N))
        mine = {k: want[k][0][pick] for k in DENSE}
        sub = {k: (v[:, pick] if k != 'length' else v[pick]) for k, v in want.items()}
        check_unroll(before, after, inputs, e, acts, stop, out, SENT, oracle_kw=OKW, expected=(mine, sub))


def _plant(name, before, after, inputs, acts, out, want):
    part = np.flatnonzero((ENV_OF >= 0) & (ENV_OF < N))
    if name == 'row 0 is not the input':                                       # (the record after the first step stored from row 0 on)
        j = part[np.flatnonzero(want['changed'][0, part])[0]]
        out['hdr'][0, j], out['slot_pos'][0, j] = out['hdr'][1, j], out['slot_pos'][1, j]
        return 'final record[0]'
    if name == 'row 0 with another slot order':                                # (the same state, not the same bytes)
        j = part[0]
        p, h = out['slot_pos'][0, j], out['hdr'][0, j]
        assert p[0] != p[1]
        p[0], p[1] = p[1], p[0]
        h[12] = (h[12] >> 4) | ((h[12] & 15) << 4)
        return 'byte for byte'
    if name == 'a frozen row keeps stepping':
        j = part[np.flatnonzero(want['length'][part] < T - 1)[0]]
        t = int(want['length'][j])                                             # (step t is the first one not taken)
        on = oracle_simulate({k: want[k][t][[j]] for k in DENSE}, before['state_init_grid'][[ENV_OF[j]]], acts[t:t + 1, [j]], False, OKW)
        h, p = encode({k: on[k] for k in DENSE}, menu=int(inputs['hdr'][j, 3]))
        assert not np.array_equal(h[0], out['hdr'][t + 1, j])
        out['hdr'][t + 1, j], out['slot_pos'][t + 1, j] = h[0], p.view(np.int16)[0]
        return 'final record[%d]' % (t + 1)
    if name == 'taken off by one step':                                        # (the mask of the step AFTER the ending one still set)
        j = part[np.flatnonzero(want['length'][part] < T)[0]]
        out['taken'][int(want['length'][j]), j] = 1
        return 'taken'
    if name == 'changed set for a no-op id':
        assert acts[0, 0] == 6 and want['taken'][0, 0] and not want['changed'][0, 0]
        out['changed'][0, 0] = 1
        return 'changed'
    if name == 'a row of a negative env_of entry written':
        assert ENV_OF[2] < 0
        out['hdr'][T, 2] = out['hdr'][T, 0]
        return 'hdr[%d] of the rows that must not be written' % T
    if name == 'a trace row of a skipped state written':
        assert ENV_OF[5] >= N
        out['taken'][3, 5] = 0
        return 'taken[3] of the rows that must not be written'
    if name == 'length one short':
        out['length'][0] -= 1
        return 'length'
    if name == 'a reward behind the end':
        j = part[np.flatnonzero(want['length'][part] < T)[0]]
        out['reward'][T - 1, j] = -1
        return 'reward[%d]' % (T - 1)
    if name == 'a skipped state not counted':
        after['counters'][7] -= 1
        return 'counters'
    if name == 'an env state moved':
        after['hdr'][2, 0] ^= 1
        return 'after cw_unroll: hdr'
    raise KeyError(name)


FAULTS = ['row 0 is not the input', 'row 0 with another slot order', 'a frozen row keeps stepping', 'taken off by one step', 'changed set for a no-op id',
          'a row of a negative env_of entry written', 'a trace row of a skipped state written', 'length one short', 'a reward behind the end',
          'a skipped state not counted', 'an env state moved']


@pytest.mark.parametrize('fault', FAULTS)
def test_every_planted_fault_is_caught_at_its_field(world, fault):
    before, after, inputs, acts, out, want = _correct(*world, ENV_OF, True)
    check_unroll(before, after, inputs, ENV_OF, acts, True, out, SENT, oracle_kw=OKW)
    where = _plant(fault, before, after, inputs, acts, out, want)
    with pytest.raises(AssertionError) as err:
        check_unroll(before, after, inputs, ENV_OF, acts, True, out, SENT, oracle_kw=OKW)
    assert where in str(err.value), (where, str(err.value))


def test_nothing_to_compare_is_an_error(world):
    before, after, inputs, acts, out, _ = _correct(*world, ENV_OF, True)
    for bad in (dict(env_of=np.full(M, -1)), dict(outputs={}), dict(env_of=ENV_OF[:-1]), dict(inputs=None), dict(actions=acts[:, :-1]), dict(actions=acts[0]),
                dict(outputs={'reward': out['reward'][:-1]}), dict(outputs={'hdr': out['hdr'][:-1]}), dict(outputs={'rewards': out['reward']})):
        kw = dict(dict(before=before, after=after, inputs=inputs, env_of=ENV_OF, actions=acts, outputs=out), **bad)
        with pytest.raises(ValueError):
            check_unroll(kw['before'], kw['after'], kw['inputs'], kw['env_of'], kw['actions'], True, kw['outputs'], SENT, oracle_kw=OKW)
    assert set(layout(T)) == set(FIELDS) and all(layout(T)[f] == (T,) for f in TRACES) and layout(T)['hdr'] == (T + 1,) and layout(T)['length'] == ()
