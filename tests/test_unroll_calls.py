"""CPU tier: what CraftingWorldVecEnv.unroll hands to the library -- the entry point and the scalars, which pointer sits in which slot, NULL members for
the fields not named, out= identity, that no call synchronises (host_outputs engines included), and what raises before any call
(tests/recording_engine.py: the env without an engine, a library that takes notes)."""
import numpy as np
import pytest
import torch

from gym_craftingworld_amd.vec_env import UNROLL_FIELDS
from recording_engine import kept_tensors, make_env, release

N, S = 4, 5
LEAD, M = (2, 3), 6
MEMBERS = ['hdr', 'slot_pos', 'reward', 'done', 'changed', 'taken', 'length']


@pytest.fixture(params=[False, True], ids=['device_outputs', 'host_outputs'])
def env(request):
    e = make_env(N, S, host_outputs=request.param)
    yield e
    release(e)


def records(lead=LEAD):
    return np.zeros(lead + (16,), np.uint8), np.zeros(lead + (8,), np.int16)


def the_call(env):
    """the one library call unroll() made: cw_unroll and nothing else -- no cw_synchronize, on a host_outputs engine either -> its arguments between the
    engine handle and the stream"""
    assert env._lib.names() == ['cw_unroll']
    args = env._lib.calls[0][1]
    assert args[-1] is None                      # the stream the harness hands out: c_void_p(0)
    env._lib.clear()
    return args[:-1]


def at(env, ptr):
    """the tensor behind a pointer the library was handed: the env must still hold it"""
    assert ptr is not None
    kept = kept_tensors(env)
    assert ptr in kept, 'a pointer went to the library whose tensor the env does not keep'
    return kept[ptr]


def packed(env, ptr, dtype, values):
    t = at(env, ptr)
    assert t.dtype == dtype and t.is_contiguous() and t.tolist() == values, (t.dtype, t.tolist())


def shapes(T, m, names=UNROLL_FIELDS):
    spec = {'hdr': ((T + 1, m, 16), torch.uint8), 'slot_pos': ((T + 1, m, 8), torch.int16), 'reward': ((T, m), torch.int32), 'done': ((T, m), torch.bool),
            'changed': ((T, m), torch.bool), 'taken': ((T, m), torch.bool), 'length': ((m,), torch.int32)}
    return {f: spec[f] for f in names}


def check_out(out, want, struct):
    """the returned dict against the spec, and the struct the library got: a field's member holds its tensor's pointer, every other member is NULL"""
    assert list(out) == list(want) and {f: (tuple(t.shape), t.dtype) for f, t in out.items()} == want
    assert all(t.is_contiguous() and t.device.type == 'cpu' for t in out.values())
    assert list(struct) == MEMBERS
    for f in UNROLL_FIELDS:
        assert struct[f] == (out[f].data_ptr() if f in out else None), f


def raises_before_any_call(env, exc, fn, *a, **kw):
    with pytest.raises(exc):
        fn(*a, **kw)
    assert env._lib.calls == []


def test_unroll_of_the_envs_own_states(env):
    a = np.arange(7 * 8, dtype=np.int64).reshape(7, 8) % 9       # the broadcast form: K = 2 plans per env
    r = env.unroll(a)
    e, hp, pp, m, ap, T, stop, struct = the_call(env)
    assert (e, hp, pp, m, T, stop) == (None, None, None, 8, 7, 1)
    packed(env, ap, torch.uint8, a.tolist())                     # int64 actions arrive as uint8
    check_out(r, shapes(7, 8), struct)                           # the default: all seven, the states flat as simulate() returns them
    r2 = env.unroll(torch.as_tensor(a).view(7, 2, N), stop_at_done=False)       # [T, K, N]
    m, _, T, stop, struct = the_call(env)[3:8]
    assert (m, T, stop) == (8, 7, 0)
    check_out(r2, shapes(7, 8), struct)
    assert all(r2[f] is not r[f] for f in r)                     # (fresh tensors each call)


def test_unroll_with_records(env):
    h, p = records()
    a = [[t % 6] * M for t in range(3)]                          # [3, 6] with records
    r = env.unroll(a, h, p, [0, 1, 2, 3, -5, 0], stop_at_done=False, fields=('taken', 'hdr', 'reward'))
    e, hp, pp, m, ap, T, stop, struct = the_call(env)
    assert (m, T, stop) == (M, 3, 0)
    packed(env, e, torch.int32, [0, 1, 2, 3, -1, 0])
    packed(env, ap, torch.uint8, a)
    assert at(env, hp).dtype == torch.uint8 and tuple(at(env, hp).shape) == LEAD + (16,)
    assert at(env, pp).dtype == torch.int16 and tuple(at(env, pp).shape) == LEAD + (8,)
    check_out(r, shapes(3, M, ('taken', 'hdr', 'reward')), struct)
    assert [k for k, v in struct.items() if v is None] == ['slot_pos', 'done', 'changed', 'length']
    assert env.unroll(np.asarray(a, np.uint8).reshape((3,) + LEAD), h, p, fields=('taken', 'hdr', 'reward'), out=r) is r      # an earlier call's dict, written again
    check_out(r, shapes(3, M, ('taken', 'hdr', 'reward')), the_call(env)[7])
    for f in UNROLL_FIELDS:                                      # each field alone
        one = env.unroll(a, h, p, fields=(f,))
        struct = the_call(env)[7]
        check_out(one, shapes(3, M, (f,)), struct)
        assert sum(v is not None for v in struct.values()) == 1
    assert all(one[f].data_ptr() in kept_tensors(env) for f in one)       # what went over inside the struct is kept alive


def test_no_states_is_no_call(env):
    r = env.unroll(np.zeros((5, 0), np.uint8), *records((0,)))
    assert env._lib.calls == []
    assert {f: tuple(t.shape) for f, t in r.items()} == {f: s for f, (s, _) in shapes(5, 0).items()}


def test_unroll_errors(env):
    h, p = records()
    a = np.zeros((3, M), np.uint8)
    r = env.unroll(a, h, p)
    env._lib.clear()
    for fields in ((), ('hdr', 'nope'), ('hdr', 'hdr'), ('rewards',), ('ret',), ('achieved_mask',)):
        raises_before_any_call(env, ValueError, env.unroll, a, h, p, fields=fields)
    raises_before_any_call(env, ValueError, env.unroll, a, h)
    raises_before_any_call(env, ValueError, env.unroll, a, None, p)
    raises_before_any_call(env, ValueError, env.unroll, a, env_of=[0] * M)
    raises_before_any_call(env, IndexError, env.unroll, a, h, p, [0, 1, 2, 3, 4, 0])
    raises_before_any_call(env, ValueError, env.unroll, a[:, :5], h, p)
    raises_before_any_call(env, ValueError, env.unroll, a)                                        # 6 columns: no multiple of 4 envs
    raises_before_any_call(env, ValueError, env.unroll, a.astype(np.float32), h, p)
    raises_before_any_call(env, ValueError, env.unroll, a.astype(np.int32) + 256, h, p)
    raises_before_any_call(env, ValueError, env.unroll, a[:0], h, p)                              # T = 0
    raises_before_any_call(env, ValueError, env.unroll, a, h, p, out={f: r[f] for f in ('hdr', 'done')})
    raises_before_any_call(env, ValueError, env.unroll, a, h, p, out=dict(r, reward=r['length']))
    for f, bad in (('hdr', torch.empty((3, M, 16), dtype=torch.uint8)), ('slot_pos', torch.empty((4, M, 8), dtype=torch.uint8)),          # T rows, not T + 1
                   ('reward', torch.empty((4, M), dtype=torch.int32)), ('done', torch.empty((3, M), dtype=torch.uint8)),
                   ('taken', torch.empty((3, 2 * M), dtype=torch.bool)[:, ::2]), ('length', [0] * M)):
        raises_before_any_call(env, ValueError, env.unroll, a, h, p, out=dict(r, **{f: bad}))
    raises_before_any_call(env, ValueError, env.unroll, np.zeros((4, M), np.uint8), h, p, fields=('reward',),
                           out={'reward': torch.empty((3, M), dtype=torch.int32)})               # T is part of the shape


def test_the_cap_raises_before_any_call():
    """(T + 1) * M above 2**27 records: refused from the shapes alone -- a strided view of one byte stands in for 2**26 plans"""
    e = make_env(1, S)
    big = torch.zeros(1, dtype=torch.uint8).expand(2, 2 ** 26)
    raises_before_any_call(e, ValueError, e.unroll, big.numpy())
    release(e)
