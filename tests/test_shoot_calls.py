"""CPU tier: what CraftingWorldVecEnv.shoot and .shoot_actions hand to the library -- entry point, scalars, which pointer sits in which slot, the NULL
members of fields not named, the seed as an int and as a tensor, the weights' broadcast, what an empty batch does, what raises before any call and what is
kept alive (tests/recording_engine.py: the env without an engine, a library that takes notes), after tests/test_plan_calls.py."""
import numpy as np
import pytest
import torch

from gym_craftingworld_amd.vec_env import SHOOT_FIELDS
from recording_engine import make_env, release
from test_vec_env_calls import LEAD, M, N, S, at, packed, raises_before_any_call, records, the_call

DEFAULT = ('best_ret', 'best_sample', 'best_action', 'length', 'done', 'achieved_mask', 'plan')
MEMBER = {'achieved_mask': 'achieved'}          # the out dict's key -> the member of cw_shoot_out
MEMBERS = ['best_ret', 'best_sample', 'best_action', 'length', 'done', 'achieved', 'hdr', 'slot_pos', 'plan', 'ret']


@pytest.fixture(params=[False, True], ids=['device_outputs', 'host_outputs'])
def env(request):
    e = make_env(N, S, host_outputs=request.param)
    yield e
    release(e)


def shapes(T, K, m, names):
    spec = {'best_ret': ((m,), torch.int32), 'best_sample': ((m,), torch.int32), 'best_action': ((m,), torch.uint8), 'length': ((m,), torch.int32),
            'done': ((m,), torch.bool), 'achieved_mask': ((m,), torch.int16), 'hdr': ((m, 16), torch.uint8), 'slot_pos': ((m, 8), torch.int16),
            'plan': ((T, m), torch.uint8), 'ret': ((K, m), torch.int32)}
    return {f: spec[f] for f in names}


def check_out(out, want, struct):
    """the returned dict against the spec, and the struct the library got: a field's member holds its tensor's pointer, every other member is NULL"""
    assert list(out) == list(want) and {f: (tuple(t.shape), t.dtype) for f, t in out.items()} == want
    assert list(struct) == MEMBERS
    for f in SHOOT_FIELDS:
        assert struct[MEMBER.get(f, f)] == (out[f].data_ptr() if f in out else None), f


def test_shoot_with_records(env):
    h, p = records()
    r = env.shoot(7, 33, 5, h, p, [0, 1, 2, 3, -5, 0])
    e, hp, pp, m, T, K, seed, seed_dev, w, struct = the_call(env, 'cw_shoot')
    assert (m, T, K, seed, seed_dev, w) == (M, 7, 33, 5, None, None)
    packed(env, e, torch.int32, [0, 1, 2, 3, -1, 0])
    assert at(env, hp).dtype == torch.uint8 and tuple(at(env, hp).shape) == LEAD + (16,)
    assert at(env, pp).dtype == torch.int16 and tuple(at(env, pp).shape) == LEAD + (8,)
    check_out(r, shapes(7, 33, M, DEFAULT), struct)              # the default: everything but the records and ret
    assert struct['hdr'] is None and struct['slot_pos'] is None and struct['ret'] is None
    assert env.shoot(7, 33, 5, h, p, fields=DEFAULT, out=r) is r     # an earlier call's dict, written again
    e, hp, pp, m, T, K, seed, seed_dev, w, struct = the_call(env, 'cw_shoot')
    assert e is None and (m, T, K) == (M, 7, 33)
    check_out(r, shapes(7, 33, M, DEFAULT), struct)
    full = env.shoot(np.int64(64), np.int32(1024), 2 ** 64 - 1, h, p.view(np.uint16), fields=SHOOT_FIELDS)
    args = the_call(env, 'cw_shoot')
    assert args[3:7] == (M, 64, 1024, 2 ** 64 - 1)
    check_out(full, shapes(64, 1024, M, SHOOT_FIELDS), args[9])
    assert all(v is not None for v in args[9].values())


def test_shoot_of_the_engines_own_states(env):
    own = env.shoot(3, 1)
    e, hp, pp, m, T, K, seed, seed_dev, w, struct = the_call(env, 'cw_shoot')
    assert (e, hp, pp, m, T, K, seed, seed_dev, w) == (None, None, None, N, 3, 1, 0, None, None)
    check_out(own, shapes(3, 1, N, DEFAULT), struct)


def test_fields_not_named_are_null(env):
    h, p = records()
    r = env.shoot(4, 2, 0, h, p, fields=('ret', 'hdr'))
    struct = the_call(env, 'cw_shoot')[9]
    check_out(r, shapes(4, 2, M, ('ret', 'hdr')), struct)
    assert [k for k, v in struct.items() if v is not None] == ['hdr', 'ret']
    r = env.shoot(4, 2, 0, h, p, fields=('plan',))
    struct = the_call(env, 'cw_shoot')[9]
    assert [k for k, v in struct.items() if v is not None] == ['plan']


@pytest.mark.parametrize('dtype', [torch.int64, torch.uint64])
def test_the_seed_as_a_tensor_goes_over_as_the_device_word(env, dtype):
    word = torch.tensor([41], dtype=dtype)
    env.shoot(3, 2, word)
    args = the_call(env, 'cw_shoot')
    assert args[6] == 0 and args[7] == word.data_ptr()           # scalar 0, the word's address
    del word
    assert at(env, args[7]).tolist() == [41]                     # kept alive: a captured graph reads it on every replay
    word = torch.tensor(7, dtype=dtype)                          # (zero dimensions: one element)
    a = env.shoot_actions(3, word, rows=2)
    m, T, seed, seed_dev, w, samples, R, out = the_call(env, 'cw_shoot_actions')
    assert (m, T, seed, w, samples, R) == (N, 3, 0, None, None, 2) and seed_dev == word.data_ptr() and out == a.data_ptr()


def test_the_weights(env):
    h, p = records()
    w = np.arange(5 * 6 * M).reshape(5, 6, M)
    env.shoot(5, 3, 0, h, p, weights=w)
    wp = the_call(env, 'cw_shoot')[8]
    t = at(env, wp)
    assert t.dtype == torch.uint16 and t.is_contiguous() and tuple(t.shape) == (5, 6, M) and np.array_equal(t.numpy(), w)
    row = np.array([[1, 0, 3, 0, 0, 65535]] * 5) + np.arange(5)[:, None] * np.array([1, 1, 1, 1, 1, 0])
    env.shoot(5, 3, 0, h, p, weights=row.tolist())               # [T, 6]: every state alike, broadcast with a copy
    t = at(env, the_call(env, 'cw_shoot')[8])
    assert t.dtype == torch.uint16 and t.is_contiguous() and tuple(t.shape) == (5, 6, M) and np.array_equal(t.numpy(), np.repeat(row[:, :, None], M, axis=2))
    env.shoot(5, 3, 0, weights=torch.full((5, 6, N), 9, dtype=torch.uint16))      # the engine's own states: M = N
    t = at(env, the_call(env, 'cw_shoot')[8])
    assert tuple(t.shape) == (5, 6, N) and (t.numpy() == 9).all()
    env.shoot_actions(5, rows=2, weights=row, n_states=3)
    m, T, seed, seed_dev, wp, samples, R, out = the_call(env, 'cw_shoot_actions')
    assert tuple(at(env, wp).shape) == (5, 6, 3) and (m, R) == (3, 2)
    for bad in (w.astype(np.float32), torch.ones((5, 6, M)), row / 3):
        raises_before_any_call(env, TypeError, env.shoot, 5, 3, 0, h, p, weights=bad)
    with pytest.raises(TypeError, match='65535'):                # the message names the quantisation to choose
        env.shoot(5, 3, 0, h, p, weights=w * 0.5)
    for bad in (w[:4], w[:, :5], w[:, :, :5], w - 1, w + 65535, w != 0, row[None], np.zeros((5, 6, M), 'U1')):
        raises_before_any_call(env, ValueError, env.shoot, 5, 3, 0, h, p, weights=bad)


def test_shoot_actions(env):
    a = env.shoot_actions(6, 9, rows=4)
    m, T, seed, seed_dev, w, samples, R, out = the_call(env, 'cw_shoot_actions')
    assert (m, T, seed, seed_dev, w, samples, R) == (N, 6, 9, None, None, None, 4) and out == a.data_ptr()
    assert a.dtype == torch.uint8 and tuple(a.shape) == (6, 4, N) and a.is_contiguous()
    assert env.shoot_actions(6, 9, rows=4, out=a) is a
    assert the_call(env, 'cw_shoot_actions')[7] == a.data_ptr()
    b = env.shoot_actions(2, samples=[[0, 5, -3, 65535], [1, 1, 1, 1], [-1, -1, -1, -1]])
    m, T, seed, seed_dev, w, samples, R, out = the_call(env, 'cw_shoot_actions')
    assert (m, T, R) == (N, 2, 3) and tuple(b.shape) == (2, 3, N)
    packed(env, samples, torch.int32, [[0, 5, -1, 65535], [1, 1, 1, 1], [-1, -1, -1, -1]])
    env.shoot_actions(2, samples=torch.zeros((1, 9), dtype=torch.int32), n_states=9, rows=1)
    assert the_call(env, 'cw_shoot_actions')[0] == 9
    for kw in (dict(), dict(rows=-1), dict(rows=2.0), dict(rows=2, samples=[[0] * N]), dict(samples=[0] * N), dict(samples=[[0] * (N + 1)]),
               dict(samples=[[0.5] * N]), dict(samples=[[2 ** 31] * N]), dict(rows=2, n_states=-1), dict(rows=2 ** 27 + 1), dict(rows=2, n_states=2 ** 27 + 1),
               dict(rows=2 ** 20, n_states=2 ** 20), dict(rows=2, out=torch.empty((2, 2, N), dtype=torch.uint8)), dict(rows=2, out=torch.empty((6, 2, N), dtype=torch.int8))):
        raises_before_any_call(env, ValueError, env.shoot_actions, 6, **kw)
    for T in (0, -1, 32768, 2.0, None, True):
        raises_before_any_call(env, ValueError, env.shoot_actions, T, rows=2)


@pytest.mark.parametrize('lead', [(0,), (0, 3)])
def test_no_records_no_call(env, lead):
    h, p = records(lead)
    r = env.shoot(5, 9, 1, h, p, fields=SHOOT_FIELDS)
    assert {f: (tuple(t.shape), t.dtype) for f, t in r.items()} == shapes(5, 9, 0, SHOOT_FIELDS)
    assert env.shoot(5, 9, 1, h, p, [], fields=SHOOT_FIELDS, out=r) is r
    assert tuple(env.shoot_actions(5, rows=0).shape) == (5, 0, N) and tuple(env.shoot_actions(5, rows=3, n_states=0).shape) == (5, 3, 0)
    assert tuple(env.shoot_actions(5, samples=np.zeros((0, N), np.int32)).shape) == (5, 0, N)
    assert env._lib.calls == []


def test_errors_before_any_call(env):
    h, p = records()
    r = env.shoot(3, 4, 0, h, p, fields=SHOOT_FIELDS)
    env._lib.clear()
    for bad in (0, 32768, -1, 2.0, '3', None, True):
        raises_before_any_call(env, ValueError, env.shoot, bad, 4, 0, h, p)
        raises_before_any_call(env, ValueError, env.shoot, bad, 4)
    for bad in (0, 65537, -1, 2.0, '3', None, False):
        raises_before_any_call(env, ValueError, env.shoot, 3, bad, 0, h, p)
    for bad in (-1, 2 ** 64, 1.0, None, '0', True, torch.tensor([1, 2]), torch.tensor([1], dtype=torch.int32), torch.tensor([1.0]), np.array([1])):
        raises_before_any_call(env, ValueError, env.shoot, 3, 4, bad, h, p)
        raises_before_any_call(env, ValueError, env.shoot_actions, 3, bad, rows=1)
    assert 65536 * 1024 * 64 == 2 ** 32
    raises_before_any_call(env, ValueError, env.shoot, 64, 1024, 0, *records((65537,)))          # the work cap, at its edge
    raises_before_any_call(env, ValueError, env.shoot, 65, 1024, 0, *records((65536,)))
    raises_before_any_call(env, ValueError, env.shoot, 64, 1025, 0, *records((65536,)))
    for fields in ((), ('ret', 'nope'), ('ret', 'ret'), ('q',), ('best_q',)):
        raises_before_any_call(env, ValueError, env.shoot, 3, 4, 0, h, p, fields=fields)
    raises_before_any_call(env, ValueError, env.shoot, 3, 4, 0, h)                                # hdr without slot_pos
    raises_before_any_call(env, ValueError, env.shoot, 3, 4, 0, None, p)
    raises_before_any_call(env, ValueError, env.shoot, 3, 4, 0, env_of=[0, 1, 2, 3])              # env_of without records
    raises_before_any_call(env, ValueError, env.shoot, 3, 4, 0, h, p[:1])
    raises_before_any_call(env, ValueError, env.shoot, 3, 4, 0, h.astype(np.int8), p)
    raises_before_any_call(env, ValueError, env.shoot, 3, 4, 0, h, p, [0, 1, 2])
    raises_before_any_call(env, IndexError, env.shoot, 3, 4, 0, h, p, [0, 1, 2, 3, 4, 0])
    raises_before_any_call(env, ValueError, env.shoot, 3, 4, 0, h, p, fields=SHOOT_FIELDS, out={f: r[f] for f in ('ret', 'done')})
    raises_before_any_call(env, ValueError, env.shoot, 3, 4, 0, h, p, fields=SHOOT_FIELDS, out=dict(r, extra=r['ret']))
    raises_before_any_call(env, ValueError, env.shoot, 3, 4, 0, h, p, out=r)                      # (the default fields are not the dict's)
    raises_before_any_call(env, ValueError, env.shoot, 4, 4, 0, h, p, fields=SHOOT_FIELDS, out=r) # the horizon is part of plan's shape
    raises_before_any_call(env, ValueError, env.shoot, 3, 5, 0, h, p, fields=SHOOT_FIELDS, out=r) # ... the samples of ret's
    for f, bad in (('ret', torch.empty((4, M + 1), dtype=torch.int32)), ('ret', torch.empty((4, M), dtype=torch.int64)), ('done', torch.empty((M,), dtype=torch.uint8)),
                   ('hdr', torch.empty((M, 32), dtype=torch.uint8)[:, ::2]), ('slot_pos', np.empty((M, 8), np.int16)), ('plan', torch.empty((M, 3), dtype=torch.uint8)),
                   ('best_action', torch.empty((M,), dtype=torch.int64)), ('best_sample', torch.empty((M,), dtype=torch.int64))):
        raises_before_any_call(env, ValueError, env.shoot, 3, 4, 0, h, p, fields=SHOOT_FIELDS, out=dict(r, **{f: bad}))
