"""CPU tier: what CraftingWorldVecEnv.shoot_refit and .cem hand to the library -- entry point, scalars, which pointer sits in which slot, the NULL members
of fields not named, the in-place form (one address twice), the calls and seeds of a cem() loop, what an empty batch does and what raises before any call
(tests/recording_engine.py: the env without an engine, a library that takes notes), after tests/test_shoot_calls.py."""
import numpy as np
import pytest
import torch

from gym_craftingworld_amd.vec_env import REFIT_FIELDS, SHOOT_FIELDS
from recording_engine import make_env, release
from test_vec_env_calls import M, N, S, at, packed, raises_before_any_call, records, the_call

MEMBERS = ['elites', 'weights', 'elite_min']
K, E, T = 9, 4, 5


@pytest.fixture(params=[False, True], ids=['device_outputs', 'host_outputs'])
def env(request):
    e = make_env(N, S, host_outputs=request.param)
    yield e
    release(e)


def shapes(T, E, m, names=REFIT_FIELDS):
    spec = {'elites': ((E, m), torch.int32), 'weights': ((T, 6, m), torch.uint16), 'elite_min': ((m,), torch.int32)}
    return {f: spec[f] for f in names}


def check_out(out, want, struct, hidden_elites=False):
    """the returned dict against the spec, and the struct the library got: a field's member holds its tensor's pointer, every other member is NULL --
    but elites, which the entry point requires: a field not named still gets a buffer of the env's own"""
    assert list(out) == list(want) and {f: (tuple(t.shape), t.dtype) for f, t in out.items()} == want
    assert list(struct) == MEMBERS
    for f in REFIT_FIELDS:
        if f == 'elites' and hidden_elites:
            assert struct[f] is not None and all(struct[f] != t.data_ptr() for t in out.values())
        else:
            assert struct[f] == (out[f].data_ptr() if f in out else None), f


def a_ret(k=K, m=M):
    return torch.zeros((k, m), dtype=torch.int32)


def test_shoot_refit(env):
    ret = a_ret()
    r = env.shoot_refit(ret, E, T, 5)
    e, m, t, k, n_e, seed, seed_dev, w, rp, smooth, gain, struct = the_call(env, 'cw_shoot_refit')
    assert (e, m, t, k, n_e, seed, seed_dev, w, smooth, gain) == (None, M, T, K, E, 5, None, None, 1, 1)
    assert rp == ret.data_ptr()                                  # ret goes over in place: no copy
    check_out(r, shapes(T, E, M), struct)                        # the default: all three
    assert env.shoot_refit(ret, E, T, 5, out=r) is r             # an earlier call's dict, written again
    check_out(r, shapes(T, E, M), the_call(env, 'cw_shoot_refit')[-1])
    env.shoot_refit(ret, np.int64(K), np.int32(T), 2 ** 64 - 1, smooth=0, gain=65535, env_of=[0, 3, -7, 1, 2, 0])
    e, m, t, k, n_e, seed, seed_dev, w, rp, smooth, gain, struct = the_call(env, 'cw_shoot_refit')
    assert (m, t, k, n_e, seed, smooth, gain) == (M, T, K, K, 2 ** 64 - 1, 0, 65535)
    packed(env, e, torch.int32, [0, 3, -1, 1, 2, 0])             # env_of packed as the records calls pack it
    assert at(env, rp) is ret                                    # kept alive: the kernel may not have run yet


def test_fields_not_named_are_null(env):
    ret = a_ret()
    r = env.shoot_refit(ret, E, T, fields=('elites',))
    struct = the_call(env, 'cw_shoot_refit')[-1]
    check_out(r, shapes(T, E, M, ('elites',)), struct)
    assert [f for f, v in struct.items() if v is not None] == ['elites']
    r = env.shoot_refit(ret, E, T, fields=('weights',))          # elites is required by the entry point: a buffer of the env's own, kept alive
    struct = the_call(env, 'cw_shoot_refit')[-1]
    check_out(r, shapes(T, E, M, ('weights',)), struct, hidden_elites=True)
    assert struct['elite_min'] is None and tuple(at(env, struct['elites']).shape) == (E, M)
    r = env.shoot_refit(ret, E, T, fields=('elite_min', 'elites'))
    struct = the_call(env, 'cw_shoot_refit')[-1]
    assert struct['weights'] is None and struct['elites'] == r['elites'].data_ptr() and struct['elite_min'] == r['elite_min'].data_ptr()


def test_the_weights_and_the_in_place_form(env):
    ret = a_ret()
    w = np.arange(T * 6 * M).reshape(T, 6, M)
    r = env.shoot_refit(ret, E, T, weights=w)
    args = the_call(env, 'cw_shoot_refit')
    t = at(env, args[7])
    assert t.dtype == torch.uint16 and t.is_contiguous() and np.array_equal(t.numpy(), w) and args[-1]['weights'] == r['weights'].data_ptr() != args[7]
    row = [[1, 0, 3, 0, 0, 65535]] * T
    env.shoot_refit(ret, E, T, weights=row)                      # [T, 6]: every state alike, broadcast with a copy
    t = at(env, the_call(env, 'cw_shoot_refit')[7])
    assert tuple(t.shape) == (T, 6, M) and np.array_equal(t.numpy(), np.repeat(np.array(row)[:, :, None], M, axis=2))
    buf = torch.ones((T, 6, M), dtype=torch.uint16)
    out = dict(r, weights=buf)
    assert env.shoot_refit(ret, E, T, weights=buf, out=out) is out
    args = the_call(env, 'cw_shoot_refit')
    assert args[7] == args[-1]['weights'] == buf.data_ptr()      # IN PLACE: one address, twice
    env.shoot_refit(ret, E, T, weights=buf, fields=('weights',), out={'weights': buf})
    args = the_call(env, 'cw_shoot_refit')
    assert args[7] == args[-1]['weights'] == buf.data_ptr()
    env.shoot_refit(ret, E, T, weights=buf.clone(), out=out)     # another tensor: its own address
    args = the_call(env, 'cw_shoot_refit')
    assert args[-1]['weights'] == buf.data_ptr() != args[7]
    for bad in (w.astype(np.float32), torch.ones((T, 6, M)), np.array(row) / 3):
        raises_before_any_call(env, TypeError, env.shoot_refit, ret, E, T, weights=bad)
    for bad in (w[:4], w[:, :5], w[:, :, :5], w - 1, w + 65535):
        raises_before_any_call(env, ValueError, env.shoot_refit, ret, E, T, weights=bad)


@pytest.mark.parametrize('dtype', [torch.int64, torch.uint64])
def test_the_seed_as_a_tensor_goes_over_as_the_device_word(env, dtype):
    word = torch.tensor([41], dtype=dtype)
    env.shoot_refit(a_ret(), E, T, word)
    args = the_call(env, 'cw_shoot_refit')
    assert args[5] == 0 and args[6] == word.data_ptr()
    del word
    assert at(env, args[6]).tolist() == [41]                     # kept alive: a captured graph reads it on every replay


def work_calls(env):
    """the calls of the library that enqueue work, in order (a host_outputs engine synchronises behind each)"""
    calls = [c for c in env._lib.calls if c[0] != 'cw_synchronize']
    if env.host_outputs:
        assert env._lib.names() == [n for c in calls for n in (c[0], 'cw_synchronize')]
    else:
        assert len(calls) == len(env._lib.calls)
    env._lib.clear()
    return calls


@pytest.mark.parametrize('seed, want', [(7, [7, 8, 9]), (2 ** 64 - 2, [2 ** 64 - 2, 2 ** 64 - 1, 0]), (0, [0, 1, 2])])
def test_cem_is_a_loop_over_the_two_calls(env, seed, want):
    h, p = records()
    r = env.cem(T, K, E, 3, seed, h, p, [0, 1, 2, 3, -5, 0], smooth=2, gain=3)
    calls = work_calls(env)
    assert [c[0] for c in calls] == ['cw_shoot', 'cw_shoot_refit'] * 3           # exactly iters x (shoot, refit), nothing between them
    assert list(r) == [f for f in SHOOT_FIELDS if f not in ('hdr', 'slot_pos', 'ret')] + ['weights', 'elite_min']
    assert (tuple(r['weights'].shape), r['weights'].dtype, tuple(r['elite_min'].shape), r['elite_min'].dtype) == ((T, 6, M), torch.uint16, (M,), torch.int32)
    for i in range(3):
        (_, shoot), (_, refit) = calls[2 * i], calls[2 * i + 1]
        e, hp, pp, m, t, k, s, s_dev, w, struct = shoot[:-1]
        e2, m2, t2, k2, n_e, s2, s_dev2, w2, rp, smooth, gain, fit = refit[:-1]
        assert (m, t, k, s, s_dev) == (M, T, K, want[i], None) and (m2, t2, k2, n_e, s2, s_dev2, smooth, gain) == (M, T, K, E, want[i], None, 2, 3)
        assert rp == struct['ret'] is not None                                   # the refit reads the returns that shoot wrote
        assert w == w2 == (None if i == 0 else r['weights'].data_ptr())          # uniform first, then the one buffer: shoot reads it, the refit reads
        assert fit['weights'] == r['weights'].data_ptr() and fit['elite_min'] == r['elite_min'].data_ptr() and fit['elites'] is not None    # ... and writes it
        for f in ('best_ret', 'plan', 'done'):
            assert struct[f] == r[f].data_ptr()                                  # every iteration writes the buffers that are returned
    again = env.cem(T, K, E, 2, seed, h, p, [0, 1, 2, 3, -5, 0], weights=r['weights'], out=r)      # the warm start, every buffer used again
    calls = work_calls(env)
    assert [c[0] for c in calls] == ['cw_shoot', 'cw_shoot_refit'] * 2
    assert all(again[f] is r[f] for f in r)
    assert [c[1][8] for c in calls[::2]] == [r['weights'].data_ptr()] * 2 and [c[1][7] for c in calls[1::2]] == [r['weights'].data_ptr()] * 2


def test_cem_with_a_seed_tensor(env):
    word = torch.tensor([5], dtype=torch.int64)
    env.cem(T, K, E, 3, word)
    calls = work_calls(env)
    assert [c[0] for c in calls] == ['cw_shoot', 'cw_shoot_refit'] * 3
    assert [(c[1][6], c[1][7]) for c in calls[::2]] == [(i, word.data_ptr()) for i in range(3)]       # the scalar i, the device word
    assert [(c[1][5], c[1][6]) for c in calls[1::2]] == [(i, word.data_ptr()) for i in range(3)]
    assert [c[1][3] for c in calls[::2]] == [N] * 3                                                    # the engine's own states


def test_cem_never_writes_the_callers_weights(env):
    mine = torch.full((T, 6, N), 9, dtype=torch.uint16)
    r = env.cem(T, K, E, 2, weights=mine, fields=('best_ret', 'ret'))
    calls = work_calls(env)
    assert list(r) == ['best_ret', 'ret', 'weights', 'elite_min'] and r['weights'] is not mine and (r['weights'].numpy() == 9).all()      # copied in
    assert all(c[1][8] == r['weights'].data_ptr() for c in calls[::2]) and all(c[1][-2]['weights'] == r['weights'].data_ptr() for c in calls[1::2])
    assert all(c[1][8] == r['ret'].data_ptr() for c in calls[1::2])
    assert mine.data_ptr() not in [a for c in calls for a in c[1] if isinstance(a, int)]


@pytest.mark.parametrize('lead', [(0,), (0, 3)])
def test_no_states_no_call(env, lead):
    r = env.shoot_refit(a_ret(K, 0), E, T)
    assert {f: (tuple(t.shape), t.dtype) for f, t in r.items()} == shapes(T, E, 0)
    assert env.shoot_refit(a_ret(K, 0), E, T, env_of=[], out=r) is r
    h, p = records(lead)
    c = env.cem(T, K, E, 3, 1, h, p)
    assert tuple(c['weights'].shape) == (T, 6, 0) and tuple(c['best_ret'].shape) == (0,) and tuple(c['plan'].shape) == (T, 0)
    assert env._lib.calls == []


def test_errors_before_any_call(env):
    ret = a_ret()
    r = env.shoot_refit(ret, E, T)
    env._lib.clear()
    for bad in (ret.to(torch.int64), ret.to(torch.float32), ret[0], ret[None], ret.numpy(), ret.tolist(), None, torch.zeros((K, 2 * M), dtype=torch.int32)[:, ::2]):
        raises_before_any_call(env, ValueError, env.shoot_refit, bad, E, T)      # the dtype, the rank, not a tensor, not contiguous
    for bad in (K + 1, 0, -1, 2.0, None, True, '3'):
        raises_before_any_call(env, ValueError, env.shoot_refit, ret, bad, T)    # E > K and its kin
        raises_before_any_call(env, ValueError, env.cem, T, K, bad, 2)
    for bad in (0, 32768, -1, 2.0, None, True):
        raises_before_any_call(env, ValueError, env.shoot_refit, ret, E, bad)
    for bad in (-1, 2 ** 64, 1.0, None, torch.tensor([1, 2]), torch.tensor([1], dtype=torch.int32)):
        raises_before_any_call(env, ValueError, env.shoot_refit, ret, E, T, bad)
    for kw in (dict(smooth=-1), dict(smooth=65536), dict(smooth=1.0), dict(gain=0), dict(gain=65536), dict(gain=None), dict(fields=()), dict(fields=('ret',)),
               dict(fields=('elites', 'elites')), dict(env_of=[0, 1, 2]), dict(env_of=[[0, 1, 2, 3, 0, 1]]), dict(env_of=[0., 1., 2., 3., 0., 1.]),
               dict(out={'elites': r['elites']}), dict(out=dict(r, extra=r['elites'])), dict(out=dict(r, weights=torch.empty((T, 6, M), dtype=torch.int16))),
               dict(out=dict(r, elites=torch.empty((E + 1, M), dtype=torch.int32))), dict(out=dict(r, elite_min=torch.empty((M,), dtype=torch.int64)))):
        raises_before_any_call(env, ValueError, env.shoot_refit, ret, E, T, **kw)
        if 'smooth' in kw or 'gain' in kw:
            raises_before_any_call(env, ValueError, env.cem, T, K, E, 2, **kw)
    raises_before_any_call(env, IndexError, env.shoot_refit, ret, E, T, env_of=[0, 1, 2, 3, 4, 0])
    raises_before_any_call(env, ValueError, env.shoot_refit, ret, E, T + 1, out=r)                    # the horizon is part of the weights' shape
    raises_before_any_call(env, TypeError, env.cem, T, K, E, 2, weights=torch.ones((T, 6, N)))        # float weights
    for bad in (0, -1, 2.0, None, True):
        raises_before_any_call(env, ValueError, env.cem, T, K, E, bad)
    c = env.cem(T, K, E, 1)
    env._lib.clear()
    raises_before_any_call(env, ValueError, env.cem, T, K, E, 1, out={f: c[f] for f in ('weights', 'elite_min')})
    raises_before_any_call(env, ValueError, env.cem, T, K, E, 1, out=dict(c, ret=c['best_ret']))
    raises_before_any_call(env, ValueError, env.cem, T + 1, K, E, 1, out=c)
